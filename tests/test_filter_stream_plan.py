"""The filter streams' host half (world_class_amd/csrc/wc_filter_stream_plan.hpp) compiled alone by the host compiler -- once plain, once
under the address and undefined-behaviour sanitizers -- and driven by tests/cpp/filter_stream_plan_check.cpp over seeded random scripts
of calls.  Every line it prints is compared with the rule on counts (tests/filter_stream_rule.py: Counts): which segments are done,
what is committed, what is pending, every refusal, and that a refused push leaves every stream as it was."""
import math
import os
import random
import subprocess

import pytest

import filter_rule as fr
import filter_stream_rule as fsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
# (fs, frame_period_ms, fft_size): hops 40, 1, 1.5, the tie hop and the largest
SETTINGS = ((8000, 5.0, 512), (8000, 0.125, 512), (8000, 0.1875, 512), (22050, 64.5 / 22.05, 1024), (48000, 512 / 48.0, 2048))
U = 3


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_stream_plan") / request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-o", exe, os.path.join(ROOT, "tests", "cpp", "filter_stream_plan_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()

    return run


class Model:
    def __init__(self, fs, fp, cap_s, cap_r):
        self.args = (fs, fp, cap_s, cap_r)
        self.st = [fsr.Counts(*self.args) for _ in range(U)]

    def state(self):
        return "".join(" | %d %d %d %d %d %d %d" % (c.n, c.F, c.T, c.C, c.ended, c.pending_samples, c.pending_rows) for c in self.st)

    def reset(self, u):
        if not 0 <= u < U:
            return "reset: bad stream index /" + self.state()
        self.st[u] = fsr.Counts(*self.args)
        return "ok /" + self.state()

    def push(self, ns, nr, fl):
        for u, c in enumerate(self.st):          # the refusals in the order of the streams, each stream's in the rule's order
            why = c.refusal(ns[u], nr[u], fl[u])
            if why:
                return why + " /" + self.state()
        out, seg, act = [], 0, 0
        for u, c in enumerate(self.st):
            act += int(ns[u] > 0 or nr[u] > 0 or (fl[u] and not c.ended))
            T0, T1, C0, C1 = c.step(ns[u], nr[u], fl[u])
            out.append(C1 - C0)
            seg += T1 - T0
        return "ok" + "".join(" %d" % o for o in out) + " / %d %d %d %d %d" % (sum(ns), sum(nr), sum(out), seg, act) + self.state()


def script(setting, seed, calls=500):
    fs, fp, N = setting
    rng = random.Random(seed)
    h = fr.hop(fp, fs)
    cap_s, cap_r = fsr.min_pending_samples(fp, fs) + rng.choice([0, 0, 5]), rng.choice([1, 2, 3])
    m = Model(fs, fp, cap_s, cap_r)
    lines, want, seen = ["init %d %r %d %d %d %d" % (fs, fp, N, U, cap_s, cap_r)], ["ok /" + m.state()], set()
    for _ in range(calls):
        r = rng.random()
        if r < 0.08:
            u = rng.choice([-1, U]) if rng.random() < 0.1 else rng.randrange(U)
            if 0 <= u < U and m.st[u].n and not m.st[u].ended:
                seen.add("reset in mid-stream")
            lines.append("reset %d" % u)
            want.append(m.reset(u))
            continue
        ns = [rng.choice([0, 0, 1, int(h), int(h) + 1, rng.randrange(0, cap_s + 1)]) for _ in range(U)]
        nr = [rng.choice([0, 0, 1, 1, 2]) for _ in range(U)]
        fl = [int(rng.random() < 0.06) for _ in range(U)]
        if rng.random() < 0.6:      # mostly pushes that fit, so that the streams move
            for u, c in enumerate(m.st):
                ns[u] = min(ns[u], cap_s - c.pending_samples) if not c.ended else 0
                nr[u] = min(nr[u], cap_r - c.pending_rows) if not c.ended else 0
        fresh = [u for u, c in enumerate(m.st) if c.n == 0 and c.F == 0 and not c.ended]
        if fresh and rng.random() < 0.15:      # a fresh stream flushed at once: nothing to write, or samples without a row
            u = rng.choice(fresh)
            ns[u], nr[u], fl[u] = rng.choice([0, 1]), 0, 1
        if rng.random() < 0.05:
            ns[rng.randrange(U)] = rng.choice([-1, -9])
        for u, c in enumerate(m.st):
            why = c.refusal(ns[u], nr[u], fl[u])
            seen.add(why or "ok")
            if not why and fl[u] and not c.ended:
                seen.add("flush with n == 0" if c.n + ns[u] == 0 else "held rows at the flush" if c.F + nr[u] < fr.segments(c.n + ns[u], fp, fs) else "flush")
            if not why and c.ended and fl[u]:
                seen.add("flush flag on an ended stream")
            if not why and nr[u] and not ns[u] and c.pending_samples == cap_s:
                seen.add("rows into a full sample window")
            if why:
                break
        lines.append("push " + " ".join(map(str, ns + nr + fl)))
        want.append(m.push(ns, nr, fl))
    return lines, want, seen


ALL_CASES = {"ok", fsr.NEGATIVE, fsr.ENDED, fsr.NO_FIT, fsr.NO_ROW, "reset in mid-stream", "flush with n == 0", "held rows at the flush",
             "flush flag on an ended stream"}


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "hop%g" % fr.hop(s[1], s[0]))
def test_random_scripts_follow_the_rule(program, setting, seed):
    lines, want, seen = script(setting, seed)
    assert ALL_CASES <= seen, ALL_CASES - seen
    got = program(lines)
    assert len(got) == len(want)
    for call, g, w in zip(lines, got, want):
        assert g == w, (call, g, w)


def test_counts_far_out_and_the_31_bit_limit(program):
    """T, C and S at counts near 2^31 agree with the rule in Python's integers, and a stream is refused its 2^31-th sample"""
    lines, want = [], []
    for fs, fp, _ in SETTINGS:
        for n in (0, 1, 2 ** 31 - 1000, 2 ** 31 - 1):
            h = fr.hop(fp, fs)
            for F in (0, int(n / h) - 1, int(n / h) + 3):
                if F < 0:
                    continue
                lo = max(int(min(F, n / h)) - 3, 0)      # T by a walk from just below it
                T = lo
                while T < F and fr.centre(T + 1, fp, fs) <= n:
                    T += 1
                assert fr.centre(lo, fp, fs) <= n
                S = 0 if n == 0 else max(math.ceil((n - 1) / h) - 3, 0) + 1
                while S > 1 and fr.centre(S - 2, fp, fs) >= n - 1:
                    S -= 1
                while n and fr.centre(S - 1, fp, fs) < n - 1:
                    S += 1
                lines.append("count %d %r %d %d" % (fs, fp, n, F))
                want.append("%d %d %d" % (T, fsr.committed(T, fp, fs), S))
    assert program(lines) == want
    top = 2 ** 31 - 1
    got = program(["init 8000 5.0 512 3 100 2", "seek 1 %d %d" % (top - 5, (top - 5) // 40 + 1), "push 0 6 0 0 0 0 0 0 0", "push 0 5 0 0 0 0 0 0 0"])
    c = fsr.Counts(8000, 5.0, 100, 2)
    c.n, c.F = top - 5, (top - 5) // 40 + 1
    c.T = int((top - 5) // 40)
    c.C = fsr.committed(c.T, 5.0, 8000)
    idle = " | 0 0 0 0 0 0 0"
    assert got[1] == "ok /" + idle + " | %d %d %d %d 0 %d %d" % (c.n, c.F, c.T, c.C, c.pending_samples, c.pending_rows) + idle
    assert got[2] == got[1].replace("ok", fsr.TOO_LONG)      # refused, and nothing moved
    assert got[3].startswith("ok 0 ") and " | %d " % top in got[3]


def test_a_written_script(program):
    """hop 40, capacities 100 and 2: a flush with a row per segment, rows ahead, samples ahead, a refusal in between, a reset"""
    lines = ["init 8000 5.0 512 2 100 2", "push 41 0 2 0 1 0", "push 0 0 0 2 0 0", "push 0 80 0 0 0 0", "push 0 62 0 1 0 0", "push 0 1 0 0 0 0",
             "push 1 0 0 0 0 0", "push 0 39 0 1 0 1", "reset 0", "push 40 0 1 0 0 0", "push 0 0 0 0 0 1"]
    assert program(lines) == [
        "ok / | 0 0 0 0 0 0 0 | 0 0 0 0 0 0 0",
        "ok 41 0 / 41 2 41 2 1 | 41 2 2 41 1 0 0 | 0 0 0 0 0 0 0",            # S = 2 at n = 41: both rows are read, none is held
        "ok 0 0 / 0 2 0 0 1 | 41 2 2 41 1 0 0 | 0 2 0 0 0 0 2",               # rows ahead of the samples
        "ok 0 41 / 80 0 41 2 1 | 41 2 2 41 1 0 0 | 80 2 2 41 0 39 0",         # c_2 = 80 <= n: segments 0 and 1
        fsr.NO_FIT + " / | 41 2 2 41 1 0 0 | 80 2 2 41 0 39 0",                # 39 + 62 do not fit 100
        "ok 0 0" + " / 1 0 0 0 1 | 41 2 2 41 1 0 0 | 81 2 2 41 0 40 0",
        fsr.ENDED + " / | 41 2 2 41 1 0 0 | 81 2 2 41 0 40 0",
        "ok 0 79 / 39 1 79 2 1 | 41 2 2 41 1 0 0 | 120 3 4 120 1 0 0",        # the flush: segments 2 and 3, the last row held
        "ok / | 0 0 0 0 0 0 0 | 120 3 4 120 1 0 0",
        "ok 1 0 / 40 1 1 1 1 | 40 1 1 1 0 39 0 | 120 3 4 120 1 0 0",           # c_1 = 40 <= 40: segment 0, one output
        "ok 0 0 / 0 0 0 0 0 | 40 1 1 1 0 39 0 | 120 3 4 120 1 0 0",            # a flush flag for an ended stream does nothing
    ]


def create_rule(fs, N, fp, kind, n_streams, cap_s, cap_r):
    if not fr.accepts(fs, N, fp):
        return None      # (one of the setting's own refusals: held by tests/test_gpu_filter.py for the batch)
    if kind not in (0, 1):
        return "kind is 0 (power gains) or 1 (log amplitude gains)"
    if n_streams < 1:
        return "n_streams must be at least 1"
    if cap_s < 2 * math.ceil(fr.hop(fp, fs)):
        return "max_pending_samples must be at least 2 * ceil(hop)"
    if cap_r < 1:
        return "max_pending_rows must be at least 1"
    return "ok"


def test_create(program):
    cases = [(8000, 512, 5.0, 0, 1, 80, 1), (8000, 512, 5.0, 1, 7, 79, 1), (8000, 512, 5.0, 2, 1, 80, 1), (8000, 512, 5.0, -1, 1, 80, 1),
             (8000, 512, 5.0, 0, 0, 80, 1), (8000, 512, 5.0, 0, 1, 80, 0), (8000, 512, 0.125, 0, 1, 2, 1), (8000, 512, 0.125, 0, 1, 1, 1),
             (22050, 1024, 64.5 / 22.05, 0, 1, 130, 1), (22050, 1024, 64.5 / 22.05, 0, 1, 129, 1), (8000, 512, 0.1875, 1, 1, 4, 1),
             (8000, 512, 0.1875, 1, 1, 3, 1), (8000, 500, 5.0, 0, 1, 80, 1), (0, 512, 5.0, 0, 1, 80, 1), (8000, 512, 0.1, 0, 1, 80, 1),
             (16000, 1024, 16.0625, 0, 1, 600, 1), (16000, 1024, 16.0, 0, 1, 512, 1)]
    got = program(["create %d %d %r %d %d %d %d" % c for c in cases])
    for c, g in zip(cases, got):
        w = create_rule(*c)
        assert g == w if w else g != "ok", (c, g, w)
    assert got.count("ok") == 5
    # far outside: what 32-bit arguments can reach stays in 64 bits
    big = 2 ** 31 - 1
    assert program(["create 8000 512 5.0 0 %d %d %d" % (big, big, big), "create 8000 512 5.0 0 %d 80 1" % big]) == \
        ["a byte count leaves 63 bits", "a launch grid leaves 31 bits"]
