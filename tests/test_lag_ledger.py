"""The lagged ledger (world_class_amd/csrc/wc_lag_stream.hpp), the host half that the MLPG streams and the feature streams share,
compiled alone by the host compiler -- once plain, once under the address and undefined-behaviour sanitizers -- and driven by
tests/cpp/lag_ledger_check.cpp over seeded random scripts of calls.  Every line it prints is compared with the rule of
include/world_class_mlpg_stream.h and include/world_class_feature_stream.h, restated below in a few lines:

    E(T) = max(T - L, 0); a push of k rows gives E(rows + k) - emitted; a flush gives rows - emitted and the stream has ended;
    a refused call leaves every stream as it was.
"""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
N, MAX_ROWS, MAX_LAG, LAGS = 3, 3, 4, (0, 1, 4)

BAD_STREAM = " reset: bad stream index"
BAD_LAG = " reset: a lag outside 0 .. max_lag"
BAD_COUNT = " push: a count outside 0 .. max_rows_per_push"
NOT_OPEN = " push: rows for a stream that was never reset or has ended (reset it first)"
NOT_OPEN_FLUSH = " flush: a wanted stream was never reset or has ended"


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lag_ledger") / request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-o", exe, os.path.join(ROOT, "tests", "cpp", "lag_ledger_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()

    return run


class Model:
    """the rule on counts: a stream is [rows, emitted, lag, ended], lag -1 before its first reset"""

    def __init__(self):
        self.st = [[0, 0, -1, 0] for _ in range(N)]

    def state(self):
        return "".join(" | %d %d %d %d" % tuple(s) for s in self.st)

    def line(self, why, out=(), totals=()):
        head = why if why else "ok" + "".join(" %d" % v for v in out)
        return head + " /" + "".join(" %d" % t for t in totals) + self.state()

    def reset(self, u, lag):
        why = BAD_STREAM if not 0 <= u < N else BAD_LAG if not 0 <= lag <= MAX_LAG else None
        if not why:
            self.st[u] = [0, 0, lag, 0]
        return self.line(why)

    def push(self, k):
        for u, s in enumerate(self.st):  # the refusals in the order of the streams, the count first
            if not 0 <= k[u] <= MAX_ROWS:
                return self.line(BAD_COUNT)
            if k[u] > 0 and (s[2] < 0 or s[3]):
                return self.line(NOT_OPEN)
        out = [max(s[0] + k[u] - s[2], 0) - s[1] if k[u] else 0 for u, s in enumerate(self.st)]
        for u, s in enumerate(self.st):
            s[0] += k[u]
            s[1] += out[u]
        return self.line(None, out, [sum(k), sum(out)])

    def flush(self, want):
        if any(w and (s[2] < 0 or s[3]) for w, s in zip(want, self.st)):
            return self.line(NOT_OPEN_FLUSH)
        out = [s[0] - s[1] if w else 0 for w, s in zip(want, self.st)]
        for w, s, o in zip(want, self.st, out):
            if w:
                s[1] += o
                s[3] = 1
        return self.line(None, out, [sum(out)])


def script(seed, calls=400):
    """calls and the lines the rule expects, with a tally of the cases the script met"""
    rng = random.Random(seed)
    m = Model()
    lines, want, seen = ["init %d %d %d" % (N, MAX_ROWS, MAX_LAG)], ["ok /" + m.state()], set()
    for _ in range(calls):
        r = rng.random()
        if r < 0.22:
            u, lag = rng.randrange(N), rng.choice(LAGS)
            if rng.random() < 0.1:
                u, lag = rng.choice([(-1, 0), (N, 1), (u, -1), (u, MAX_LAG + 1)])
            if 0 <= u < N and 0 <= lag <= MAX_LAG and m.st[u][0] > 0 and not m.st[u][3]:
                seen.add("reset in mid-stream")
            lines.append("reset %d %d" % (u, lag))
            want.append(m.reset(u, lag))
        elif r < 0.82:
            k = [rng.choice([0, 0, 1, 2, 3]) for _ in range(N)]
            if rng.random() < 0.08:
                k[rng.randrange(N)] = rng.choice([MAX_ROWS + 1, -1, -7])
            for u, s in enumerate(m.st):
                if k[u] == MAX_ROWS + 1:
                    seen.add("max + 1")
                elif k[u] < 0:
                    seen.add("negative count")
                elif k[u] > 0 and s[2] < 0:
                    seen.add("push without reset")
                elif k[u] > 0 and s[3]:
                    seen.add("push after flush")
                elif k[u] > 0 and s[0] < s[2] < s[0] + k[u]:
                    seen.add("push straddles the lag")
            if not any(k):
                seen.add("push of 0 rows")
            lines.append("push " + " ".join(map(str, k)))
            want.append(m.push(k))
        else:
            w = [rng.choice([0, 1]) for _ in range(N)]
            if any(x and s[2] >= 0 and not s[3] and s[0] == 0 for x, s in zip(w, m.st)):
                seen.add("flush with no rows")
            lines.append("flush " + " ".join(map(str, w)))
            want.append(m.flush(w))
    return lines, want, seen


ALL_CASES = {"reset in mid-stream", "max + 1", "negative count", "push without reset", "push after flush", "push straddles the lag",
             "push of 0 rows", "flush with no rows"}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_scripts_follow_the_rule(program, seed):
    lines, want, seen = script(seed)
    assert seen == ALL_CASES, ALL_CASES - seen
    got = program(lines)
    assert len(got) == len(want)
    for call, g, w in zip(lines, got, want):
        assert g == w, (call, g, w)


def test_a_written_script(program):
    """one stream per lag, by hand: lag 0 emits with the push, lag 1 a row behind, lag 4 straddled by the second push"""
    lines = ["init 3 3 4", "push 1 0 0", "reset 0 0", "reset 1 1", "reset 2 4", "push 2 1 3", "push 0 0 0", "push 3 3 3", "flush 0 1 1",
             "push 1 1 0", "flush 0 1 0", "reset 1 4", "flush 1 1 0", "push 4 0 0", "push 0 -1 0"]
    assert program(lines) == [
        "ok / | 0 0 -1 0 | 0 0 -1 0 | 0 0 -1 0",
        NOT_OPEN + " / | 0 0 -1 0 | 0 0 -1 0 | 0 0 -1 0",
        "ok / | 0 0 0 0 | 0 0 -1 0 | 0 0 -1 0",
        "ok / | 0 0 0 0 | 0 0 1 0 | 0 0 -1 0",
        "ok / | 0 0 0 0 | 0 0 1 0 | 0 0 4 0",
        "ok 2 0 0 / 6 2 | 2 2 0 0 | 1 0 1 0 | 3 0 4 0",
        "ok 0 0 0 / 0 0 | 2 2 0 0 | 1 0 1 0 | 3 0 4 0",
        "ok 3 3 2 / 9 8 | 5 5 0 0 | 4 3 1 0 | 6 2 4 0",
        "ok 0 1 4 / 5 | 5 5 0 0 | 4 4 1 1 | 6 6 4 1",
        NOT_OPEN + " / | 5 5 0 0 | 4 4 1 1 | 6 6 4 1",
        NOT_OPEN_FLUSH + " / | 5 5 0 0 | 4 4 1 1 | 6 6 4 1",
        "ok / | 5 5 0 0 | 0 0 4 0 | 6 6 4 1",
        "ok 0 0 0 / 0 | 5 5 0 1 | 0 0 4 1 | 6 6 4 1",
        BAD_COUNT + " / | 5 5 0 1 | 0 0 4 1 | 6 6 4 1",
        BAD_COUNT + " / | 5 5 0 1 | 0 0 4 1 | 6 6 4 1",
    ]


def create_rule(width, n_streams, max_rows, max_lag, row_doubles):
    """create's shared checks in Python's integers: the ring of cap = max_lag + max_rows_per_push + 1 rows per stream within 2^30 bytes"""
    if width < 0:
        return ": the row width leaves 31 bits"
    if n_streams < 1 or max_rows < 1:
        return ": n_streams and max_rows_per_push must be at least 1"
    if max_lag < 0:
        return ": max_lag must not be negative"
    return "ok" if 8 * row_doubles * (max_lag + max_rows + 1) * n_streams <= 2 ** 30 else ": the ring exceeds 2^30 bytes"


@pytest.mark.parametrize("row", ["4S+1", "S"])
def test_the_create_bound(program, row):
    """the largest (nd + n_ap, max_lag + max_rows_per_push, n_streams) that passes and the smallest that is refused, each of the three
    taken to its edge with the other two held, for both ring rows: 4 S + 1 doubles (MLPG) and S doubles (features), S = nd + 1 + n_ap"""
    doubles, most = ((lambda S: 4 * S + 1), (lambda d: (d - 1) // 4)) if row == "4S+1" else ((lambda S: S), (lambda d: d))
    budget = 2 ** 27  # doubles of all rings
    cases = []
    for S, n in ((2, 1), (61, 3), (1000, 7), (2 ** 20, 1)):  # the edge in max_lag + max_rows_per_push
        rows = budget // (doubles(S) * n) - 1  # cap = rows + 1
        for lag in (0, rows // 2):
            cases += [(S, n, rows - lag, lag), (S, n, rows - lag + 1, lag)]
    for S, rows in ((2, 5), (61, 100), (513, 4096)):  # the edge in n_streams
        n = budget // (doubles(S) * (rows + 1))
        cases += [(S, n, rows - 2, 2), (S, n + 1, rows - 2, 2)]
    for n, rows in ((1, 1), (3, 64), (16, 1000)):  # the edge in nd + n_ap: the largest S with doubles(S) * cap * n within the budget
        S = most(budget // ((rows + 1) * n))
        cases += [(S, n, rows, 0), (S + 1, n, rows, 0)]
    # far outside: what 32-bit arguments can reach stays in 64 bits, and the leading checks come first
    cases += [(2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 27 + 1, 1, 1, 0), (2, 1, 2 ** 27, 0), (2, 0, 1, 0), (2, 1, 0, 0), (2, 1, 1, -1)]
    lines = ["create 7 %d %d %d %d" % (n, r, lag, doubles(S)) for S, n, r, lag in cases] + ["create -1 0 0 -1 1"]
    want = [create_rule(7, n, r, lag, doubles(S)) for S, n, r, lag in cases] + [": the row width leaves 31 bits"]
    got = program(lines)
    assert got == want, [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]
    assert want[:4] == ["ok", ": the ring exceeds 2^30 bytes"] * 2 and want.count("ok") >= 14  # the edges are edges
