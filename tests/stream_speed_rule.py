"""The rule of a synthesis stream's speed (include/world_class_stream.h, wc_synth_stream_set_speed) restated in Python.  A helper of
tests/test_gpu_synth_stream_speed.py, not a test module.

A stream has received F source frames; `last` is the position of the newest synthesis frame formed.  A push gives n frames, F += n,
and forms the frames at p = last + speed (0.0 for the first; one double addition with the speed in effect at that push) while
p <= F - 1.  Nothing is formed at a flush, nothing is revised."""


def positions(pushes, speeds, limit=None):
    """pushes[k] source frames arrive in push k while the speed is speeds[k] (a number: the same for every push).  Returns the
    positions of all synthesis frames and their count per push; limit: stop a push's count at limit + 1 (a refused push)"""
    if not hasattr(speeds, "__len__"):
        speeds = [speeds] * len(pushes)
    pos, counts, F, last = [], [], 0, None
    for n, speed in zip(pushes, speeds):
        F += n
        c = 0
        while True:
            p = 0.0 if last is None else last + float(speed)
            if not p <= F - 1 or (limit is not None and c > limit):
                break
            pos.append(p)
            last = p
            c += 1
        counts.append(c)
    return pos, counts
