"""The rule of the morph streams (include/world_class_stream.h, wc_morph_stream) restated in plain Python: positions, counts per
push and backlog per voice from the push sizes and the settings per push.  A helper of tests/test_morph_stream_rule.py and
tests/test_gpu_morph_stream.py, not a test module.

Per stream: Fa, Fb source frames received; formed; last_a, last_b.  A push of n_a and n_b frames: Fa += n_a, Fb += n_b, then
  pa = last_a + speed_a, pb = last_b + speed_b   (0.0, 0.0 for the first frame)
while pa <= Fa - 1 and pb <= Fb - 1.  Voice x keeps rows floor(last_x) .. Fx - 1 (all of them before the first frame)."""
import math


class Stream:
    def __init__(self):
        self.F = [0, 0]
        self.formed = False
        self.last = [0.0, 0.0]
        self.speed = [1.0, 1.0]
        self.frames = 0

    def copy(self):
        s = Stream()
        s.F, s.formed, s.last, s.speed, s.frames = list(self.F), self.formed, list(self.last), list(self.speed), self.frames
        return s

    def push(self, n_a, n_b, limit=None):
        """the positions (pa, pb) of the frames the push forms; with a limit, None as soon as there would be more (the stream is
        then half way: callers work on a copy)"""
        self.F[0] += n_a
        self.F[1] += n_b
        out = []
        while True:
            p = [self.last[x] + self.speed[x] if self.formed else 0.0 for x in (0, 1)]
            if not (p[0] <= self.F[0] - 1 and p[1] <= self.F[1] - 1):
                return out
            if limit is not None and len(out) == limit:
                return None
            out.append((p[0], p[1]))
            self.last, self.formed = p, True
            self.frames += 1

    def count(self, n_a, n_b, limit):
        """what wc_morph_stream_frames_for_push returns: capped at limit + 1"""
        got = self.copy().push(n_a, n_b, limit)
        return limit + 1 if got is None else len(got)

    def keep(self, x):
        return int(math.floor(self.last[x])) if self.formed else 0

    def backlog(self, x):
        return self.F[x] - self.keep(x)

    def position(self, x):
        return self.last[x] if self.formed else float("nan")


def pushes_of(frames_a, frames_b, pattern_a, pattern_b):
    """the push sizes (n_a, n_b) that feed frames_a / frames_b source frames along the two cycled patterns, until both are in"""
    out, left, k = [], [frames_a, frames_b], 0
    while left[0] or left[1]:
        n = [min(pat[k % len(pat)], left[x]) for x, pat in enumerate((pattern_a, pattern_b))]
        out.append(tuple(n))
        left = [left[0] - n[0], left[1] - n[1]]
        k += 1
    return out


# the cases of the tests: frames of A and B, the two push patterns, the speeds as (first push they hold from, speed_a, speed_b)
CASES = {
    "a": dict(frames=(33, 97), patterns=([1], [3]), speeds=[(0, 0.5, 1.5)]),
    "b": dict(frames=(97, 74), patterns=([4, 0, 4], [0, 4, 2]), speeds=[(0, 1.37, 1.0), (15, 0.73, 0.55)]),
    "c": dict(frames=(61, 61), patterns=([6, 0], [0, 6]), speeds=[(0, 1.0, 1.0)]),
    "d": dict(frames=(12, 12), patterns=([12, 0, 0, 0], [0, 4, 4, 4]), speeds=[(0, 1.0, 1.0)]),
}


def speeds_at(case, k):
    """the speeds in effect at push k"""
    return [s[1:] for s in CASES[case]["speeds"] if s[0] <= k][-1]


def run(case, max_backlog=None):
    """the case push by push: a list of dict(n=(n_a, n_b), speeds, pos=[(pa, pb), ...], backlog=(a, b), position=(a, b),
    received=(a, b), formed) per push; with max_backlog, the list ends with None at the first push over the bound"""
    c = CASES[case]
    s, out = Stream(), []
    for k, n in enumerate(pushes_of(*c["frames"], *c["patterns"])):
        s.speed = list(speeds_at(case, k))
        t = s.copy()
        pos = t.push(*n)
        if max_backlog is not None and max(t.backlog(0), t.backlog(1)) > max_backlog:
            out.append(None)
            return out
        s = t
        out.append(dict(n=n, speeds=tuple(s.speed), pos=pos, backlog=(s.backlog(0), s.backlog(1)), position=(s.position(0), s.position(1)),
                        received=tuple(s.F), formed=s.frames))
    return out
