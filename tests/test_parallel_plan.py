"""The host half of include/world_class_parallel.h (world_class_amd/csrc/wc_parallel_plan.hpp) compiled alone by the host compiler -- once
plain, once under the address and undefined-behaviour sanitizers -- and driven by tests/cpp/parallel_plan_check.cpp over seeded
argument sets: the offsets and counts against a restatement in Python's integers, and every refusal by its text."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
MAX_SLOTS, MAX_FRAMES = 2 ** 31 - 1, 2 ** 32 - 1


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("parallel_plan") / request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-o", exe, os.path.join(ROOT, "tests", "cpp", "parallel_plan_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()

    return run


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
class No(Exception):
    pass


def rows_ok(what, fmt, ld, col, width):
    if fmt not in (0, 1):
        raise No(what + ": the format is 0 (double) or 1 (float)")
    if col < 0:
        raise No(what + ": a negative column")
    if width < 1:
        raise No(what + ": fewer than 1 column")
    if ld < col + width:
        raise No(what + ": ld is smaller than col plus the width")


def pairs_of(n, null, ab):
    if n < 0:
        raise No("a negative pair count")
    if n > 0 and null:
        raise No("null length array")
    out, fa, fb, p = [], 0, 0, 0
    for u, (a, b) in enumerate(ab):
        if a < 1 or b < 1:
            raise No("pair %d: a length below 1" % u)
        out.append((fa, fb, p, a, b))
        fa, fb, p = fa + a, fb + b, p + a + b - 1
        if p > MAX_SLOTS:
            raise No("more than 2^31 - 1 path slots in one call")
        if fa > MAX_FRAMES or fb > MAX_FRAMES:
            raise No("more than 2^32 - 1 frames in one call")
    return (p, fa, fb), out


def esz(fmt):
    return 4 if fmt == 1 else 8


def span(rows, fmt, ld, width):
    return 0 if rows < 1 else ((rows - 1) * ld + width) * esz(fmt)


def first(p, fmt, col):
    return p + col * esz(fmt) if p else 0


def overlap(a, na, b, nb):
    return bool(a and b and na and nb and a < b + nb and b < a + na)


def said(counts, pairs):
    return "ok %d %d %d" % counts + "".join(" / %d %d %d %d %d" % p for p in pairs)


def joint_rule(n, null, ab, ra, rb, ro, ptrs):
    try:
        if n < 0:
            raise No("a negative pair count")
        rows_ok("A", *ra)
        rows_ok("B", *rb)
        if ra[3] + rb[3] > 384:
            raise No("dx + dy is larger than 384")
        ro = ro + (ra[3] + rb[3],)
        rows_ok("the joint rows", *ro)
        counts, pairs = pairs_of(n, null, ab)
        if n == 0:
            return said(counts, pairs)
        pa, pb, pl, pp, ma, mb, pj, pm = ptrs
        if not (pa and pb and pl and pp and pj):
            raise No("null array")
        slots, fa, fb = counts
        out0, out_bytes = first(pj, ro[0], ro[2]), span(slots, ro[0], ro[1], ro[3])
        if overlap(out0, out_bytes, pm, slots):
            raise No("the two outputs overlap")
        ins = [(first(pa, ra[0], ra[2]), span(fa, ra[0], ra[1], ra[3])), (first(pb, rb[0], rb[2]), span(fb, rb[0], rb[1], rb[3])), (pl, 4 * n),
               (pp, 8 * slots), (ma, fa), (mb, fb)]
        if any(overlap(out0, out_bytes, p, k) or overlap(pm, slots, p, k) for p, k in ins):
            raise No("an output overlaps an input")
        return said(counts, pairs)
    except No as e:
        return "no: " + str(e)


def dist_rule(n, null, ab, ra, rb, dims, ptrs):
    try:
        if n < 0:
            raise No("a negative pair count")
        rows_ok("A", *ra, dims)
        rows_ok("B", *rb, dims)
        counts, pairs = pairs_of(n, null, ab)
        if n == 0:
            return said(counts, pairs)
        pa, pb, pl, pp, ma, mb, ps, pc_, pe = ptrs
        if not (pa and pb and pl and pp):
            raise No("null array")
        if not (ps or pc_ or pe):
            raise No("all three outputs are NULL")
        slots, fa, fb = counts
        outs = [(ps, 8 * n), (pc_, 8 * n), (pe, 8 * slots)]
        ins = [(first(pa, ra[0], ra[2]), span(fa, ra[0], ra[1], dims)), (first(pb, rb[0], rb[2]), span(fb, rb[0], rb[1], dims)), (pl, 4 * n),
               (pp, 8 * slots), (ma, fa), (mb, fb)]
        for x in range(3):
            if any(overlap(*outs[x], *outs[y]) for y in range(x + 1, 3)):
                raise No("two outputs overlap")
            if any(overlap(*outs[x], p, k) for p, k in ins):
                raise No("an output overlaps an input")
        return said(counts, pairs)
    except No as e:
        return "no: " + str(e)


def mask_rule(n, null, lengths, fmt, ld, col, margin, floor, rows, mask):
    try:
        if n < 0:
            raise No("a negative utterance count")
        rows_ok("the rows", fmt, ld, col, 1)
        if margin != margin or floor != floor:
            raise No("margin or floor is NaN")
        if margin < 0:
            raise No("margin is negative")
        if n > 0 and null:
            raise No("null length array")
        utts, total = [], 0
        for u, k in enumerate(lengths):
            if k < 0:
                raise No("utterance %d: a negative length" % u)
            utts.append((total, k))
            total += k
            if total > MAX_FRAMES:
                raise No("more than 2^32 - 1 frames in one call")
        if total:
            if not (rows and mask):
                raise No("null array")
            if overlap(mask, total, first(rows, fmt, col), span(total, fmt, ld, 1)):
                raise No("the mask overlaps the rows")
        return "ok %d" % total + "".join(" / %d %d" % u for u in utts)
    except No as e:
        return "no: " + str(e)


# ---- seeded argument sets -----------------------------------------------------------------------------------------------------------
def some_pairs(rng):
    r = rng.random()
    if r < 0.04:
        return -rng.randrange(1, 4), []
    if r < 0.08:
        return 0, []
    if r < 0.11:
        return 2, [(2 ** 30, 2 ** 30), (2 ** 30, 2 ** 30)]          # 2^32 - 2 slots
    n = rng.randrange(1, 6)
    ab = [(rng.randrange(1, 300), rng.randrange(1, 300)) for _ in range(n)]
    if rng.random() < 0.08:
        ab[rng.randrange(n)] = rng.choice([(0, 5), (5, 0), (-3, 2)])
    return n, ab


def some_rows(rng, width):
    fmt = rng.choice([0, 0, 1, 1, 1, 2, -1]) if rng.random() < 0.15 else rng.choice([0, 1])
    col = -1 if rng.random() < 0.03 else rng.randrange(0, 4)
    ld = col + width + rng.choice([0, 0, 1, 5]) - (1 if rng.random() < 0.05 else 0)
    return fmt, ld, col


def place(rng, sizes, null_at=(), clash=None):
    """disjoint device ranges of the given sizes (bytes), far apart; null_at: indices that are NULL; clash: (x, y) puts y inside x"""
    base, out = 1 << 20, []
    for k, size in enumerate(sizes):
        out.append(0 if k in null_at else base)
        base += (max(size, 1) + 4095) // 4096 * 4096 + 4096
    if clash:
        x, y = clash
        if out[x] and out[y] and sizes[x] > 0 and sizes[y] > 0:
            out[y] = out[x] + rng.randrange(0, sizes[x])
    return out


def flat(ab):
    return " ".join("%d %d" % p for p in ab)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_joint_and_distortion_arguments(program, seed):
    rng = random.Random(seed)
    lines, want = [], []
    for _ in range(600):
        n, ab = some_pairs(rng)
        null = int(rng.random() < 0.03)
        slots, fa, fb = (sum(a + b - 1 for a, b in ab), sum(a for a, _ in ab), sum(b for _, b in ab)) if ab else (0, 0, 0)
        if rng.random() < 0.5:
            dx, dy = rng.choice([(1, 1), (5, 7), (192, 192), (193, 192), (0, 3), (3, -1), (120, 3)])
            ra, rb, ro = some_rows(rng, dx) + (dx,), some_rows(rng, dy) + (dy,), some_rows(rng, max(dx, 0) + max(dy, 0))
            sizes = [span(fa, ra[0] & 1, max(ra[1], 1), max(dx, 1)) + 64, span(fb, rb[0] & 1, max(rb[1], 1), max(dy, 1)) + 64, 4 * max(n, 1), 8 * slots,
                     fa, fb, span(slots, ro[0] & 1, max(ro[1], 1), max(dx + dy, 1)) + 64, slots]
            nulls = {rng.randrange(8)} if rng.random() < 0.15 else set()
            clash = (rng.choice([6, 7]), rng.randrange(8)) if rng.random() < 0.15 else None
            ptrs = place(rng, sizes, nulls, clash if clash and clash[0] != clash[1] else None)
            lines.append("joint %d %d %s  %d %d %d %d  %d %d %d %d  %d %d %d  %s" % ((n, null, flat(ab)) + ra + rb + ro + (" ".join(map(str, ptrs)),)))
            want.append(joint_rule(n, null, ab, ra, rb, ro, ptrs))
        else:
            dims = rng.choice([1, 4, 24, 0, -2]) if rng.random() < 0.1 else rng.choice([1, 4, 24])
            ra, rb = some_rows(rng, dims), some_rows(rng, dims)
            sizes = [span(fa, ra[0] & 1, max(ra[1], 1), max(dims, 1)) + 64, span(fb, rb[0] & 1, max(rb[1], 1), max(dims, 1)) + 64, 4 * max(n, 1),
                     8 * slots, fa, fb, 8 * max(n, 1), 8 * max(n, 1), 8 * slots]
            nulls = {rng.randrange(9)} if rng.random() < 0.2 else ({6, 7, 8} if rng.random() < 0.05 else set())
            clash = (rng.choice([6, 7, 8]), rng.randrange(9)) if rng.random() < 0.15 else None
            ptrs = place(rng, sizes, nulls, clash if clash and clash[0] != clash[1] else None)
            lines.append("dist %d %d %s  %d %d %d  %d %d %d %d  %s" % ((n, null, flat(ab)) + ra + rb + (dims, " ".join(map(str, ptrs)))))
            want.append(dist_rule(n, null, ab, ra, rb, dims, ptrs))
    got = program(lines)
    assert len(got) == len(want)
    for call, g, w in zip(lines, got, want):
        assert g == w, (call, g, w)
    texts = {w.split(": ", 1)[1].split(": ")[-1] for w in want if w.startswith("no")}
    for text in ("a negative pair count", "null length array", "a length below 1", "the format is 0 (double) or 1 (float)", "a negative column",
                 "fewer than 1 column", "ld is smaller than col plus the width", "dx + dy is larger than 384", "null array",
                 "more than 2^31 - 1 path slots in one call", "the two outputs overlap", "two outputs overlap", "an output overlaps an input",
                 "all three outputs are NULL"):
        assert text in texts, text          # every refusal was met
    assert sum(w.startswith("ok") for w in want) > 150


@pytest.mark.parametrize("seed", [1, 2])
def test_seeded_speech_mask_arguments(program, seed):
    rng = random.Random(seed)
    lines, want = [], []
    for _ in range(400):
        r = rng.random()
        n = -1 if r < 0.04 else 0 if r < 0.08 else rng.randrange(1, 6)
        lengths = [rng.choice([0, 1, 63, 64, 65, 1000]) for _ in range(max(n, 0))]
        if lengths and rng.random() < 0.06:
            lengths[rng.randrange(n)] = -1
        if rng.random() < 0.04:
            n, lengths = 3, [2 ** 31 - 1] * 3
        null = int(rng.random() < 0.03)
        fmt, ld, col = some_rows(rng, 1)
        margin = rng.choice(["0", "3.5", "inf", "inf", "nan", "-1", "-inf"]) if rng.random() < 0.3 else "9.2"
        floor = rng.choice(["-inf", "inf", "nan", "-3"]) if rng.random() < 0.3 else "0"
        total = sum(k for k in lengths if k > 0)
        sizes = [span(total, fmt & 1, max(ld, 1), 1) + 64, total]
        nulls = {rng.randrange(2)} if rng.random() < 0.1 else set()
        ptrs = place(rng, sizes, nulls, (0, 1) if rng.random() < 0.1 else None)
        lines.append("mask %d %d %s  %d %d %d  %s %s  %d %d" % (n, null, " ".join(map(str, lengths)), fmt, ld, col, margin, floor, ptrs[0], ptrs[1]))
        want.append(mask_rule(n, null, lengths, fmt, ld, col, float(margin), float(floor), ptrs[0], ptrs[1]))
    got = program(lines)
    for call, g, w in zip(lines, got, want):
        assert g == w, (call, g, w)
    texts = {w.split(": ", 1)[1].split(": ")[-1] for w in want if w.startswith("no")}
    for text in ("a negative utterance count", "null length array", "a negative length", "the format is 0 (double) or 1 (float)",
                 "a negative column", "ld is smaller than col plus the width", "margin or floor is NaN", "margin is negative", "null array",
                 "more than 2^32 - 1 frames in one call", "the mask overlaps the rows"):
        assert text in texts, text
    assert sum(w.startswith("ok") for w in want) > 100


def test_limits_and_the_lanes_of_a_row(program):
    big = 2 ** 30
    ok = "1 4 0 1  1 4 0 1  0 2 0  4096 8192 12288 16384 0 0 20480 0"
    got = program(["joint 1 0 %d %d  %s" % (big, big, ok),          # 2^31 - 1 slots: the most
                   "joint 2 0 %d %d 1 1  %s" % (big, big, ok),      # one more
                   "mask 3 0 %d %d 1  0 1 0  1 0  0 0" % (2 ** 31 - 1, 2 ** 31 - 1),
                   "mask 3 0 %d %d 2  0 1 0  1 0  4096 0" % (2 ** 31 - 1, 2 ** 31 - 1)] + ["lanes %d" % d for d in (1, 2, 3, 12, 33, 64, 65, 384)])
    assert got[0].startswith("no: an output overlaps an input") or got[0].startswith("ok %d %d %d" % (2 ** 31 - 1, big, big))
    assert got[1] == "no: more than 2^31 - 1 path slots in one call"
    assert got[2] == "no: null array" and got[3] == "no: more than 2^32 - 1 frames in one call"
    assert got[4:] == ["1", "2", "4", "16", "64", "64", "64", "64"]
