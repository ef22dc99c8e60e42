"""CPU: the front-half tables of tests/harvest_front.py reach what they are named for; the CPU restatement (oracle/port.harvest_debug:
decimation, DC removal, FFT band-pass, detectors, raw candidates) keeps the rule's zero pattern on them outside the near-threshold
set and its y and raw tables measure K_ref, the restatement's largest error in the rule's units, per stage; the real reference's
own member functions (oracle/ref.harvest_taps, in a child process) are held beside it where the reference survives; every
near-threshold set is under 1 % with the rule and the restatement alone; and the rule is sharp: each of the six single changes
listed in harvest_front.MUTANTS breaks the device's bound or the zero pattern on the table built for it.  A seventh, `>= 1.1 b`
for `> 1.1 b`, changes the rule only at equality, which no device can be held to: it has a test of its own that says so.

Measured on one x86-64 / glibc host: K_ref(y) = 78.3 (ratio_12), K_ref(raw) = 46.1 (runs_36) -- the tables are written with the
host's sin and cos, so the figures move with its libm (71.3 and 60.7 on another); per table see DESIGN.md, "Harvest's front
half on written signals".
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import harvest_front as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_ref(port):
    """the restatement's largest error against the long double rule, per stage, in the rule's units: something, and not absurd
    (a float64 recursion whose state is up to 1 / (1 - sum a) times its output; a transform of a dozen stages)"""
    k = F.k_ref(port)
    print("harvest front: K_ref(y) = %.3f units, K_ref(raw) = %.3f units; K_ref(y) per decimation ratio: %s"
          % (k["y"], k["raw"], ", ".join("%d: %.3f" % (r, v) for r, v in sorted(k["y_r"].items()))))
    assert 0.05 < k["y"] < 1e3 and 0.05 < k["raw"] < 1e3


@pytest.mark.parametrize("name", F.NAMES)
def test_restatement_against_the_rule(port, name):
    """lengths, band and slot counts are the rule's; at decimation 1 below 1 in magnitude y is the signal and one zero; the
    restatement's raw table is zero where the rule's is outside the near-threshold set; its errors in units are printed"""
    t, k = F.table(name), F.k_ref(port)
    worst_y = worst_raw = 0.0
    near = live = 0
    for u, (r, d) in enumerate(zip(F.rule(name), F.restatement(port, name))):
        assert len(d["y"]) == t.y_len(u) == len(r["y"]) and d["raw"].shape == (len(t.b), t.L1(u)) and d["cand"].shape[1] == 7 * t.S
        if t.r == 1 and r["acc"] == 0:
            assert np.array_equal(d["y"], np.append(t.xs[u], 0.0)) and np.array_equal(r["y"].astype(np.float64), d["y"])
        worst_y = max(worst_y, float(F.y_errors(r, d["y"]).max()))
        if t.stage == "raw":
            n, l = F.same_zero_pattern(t, u, r, d["raw"], k["raw"], False, wide=not t.stationary)
            near, live = near + n, live + l
            for j in t.bands:
                e = F.raw_errors(r["bands"][j], d["raw"][j], False)
                if not t.stationary:
                    e[F.near_threshold(r["bands"][j], k["raw"], False, t.floor, t.ceil, t.fs_d, True)] = 0.0
                worst_raw = max(worst_raw, float(e.max()))
    print("harvest front %s: restatement's worst error in units: y %.3f, raw %.3f; %d of %d live positions near a threshold%s"
          % (name, worst_y, worst_raw, near, live, "" if t.stationary else " under the utterance-wide unit"))
    assert worst_y <= k["y_r"][t.r] <= k["y"]
    if t.stationary:
        assert worst_raw <= k["raw"]


# The reference's own contour logic overruns its heap on many of these signals (a pure tone's candidates: mergeF0), after its
# front half has finished and been copied out.  So every utterance runs in a forked process of its own that writes y and raw into
# shared memory: what the front half produced is read whether or not the tail behind it survives.
_CHILD = """
import mmap, os, pickle, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import harvest_front as F
from oracle import ref
t = F.table(%r)
out = []
for u, x in enumerate(t.xs):
    yl, nb, L1 = t.y_len(u), len(t.b), t.L1(u)
    shared = np.frombuffer(mmap.mmap(-1, 8 * (yl + nb * L1)), dtype=np.float64)
    shared[:] = np.nan
    pid = os.fork()
    if pid == 0:
        ref.harvest_taps_into(x, t.fs, t.floor, t.ceil, y=shared[:yl], raw=shared[yl:])
        os._exit(0)
    status = os.waitpid(pid, 0)[1]
    out.append(dict(y=shared[:yl].copy(), raw=shared[yl:].copy().reshape(nb, L1), survived=status == 0))
sys.stdout.buffer.write(pickle.dumps(out))
"""


@pytest.mark.parametrize("name", [n for n in F.NAMES if F.table(n).with_ref])
def test_real_reference_beside_the_restatement(port, name):
    """the real reference's getWaveformAndSpectrum and getRawF0Candidates on the tables it survives (no DC offset, no 42-70 Hz
    voice, the stock target_fs and channels_in_octave), in a child process: its y is the restatement's bit for bit, its raw table
    has the rule's zero pattern outside the near-threshold set, and its own K is printed beside K_ref"""
    from oracle import ref
    if not ref.taps_available():
        pytest.skip("oracle/_ref/libworld_ref_taps.so not built (no reference sources here)")
    t, k = F.table(name), F.k_ref(port)
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), name)], stdout=subprocess.PIPE, check=True)
    taps = pickle.loads(out.stdout)
    ky = kr = apart = 0.0
    for u, (r, d, o) in enumerate(zip(F.rule(name), F.restatement(port, name), taps)):
        assert not np.isnan(o["y"]).any() and not np.isnan(o["raw"]).any(), (name, u, "the reference's front half did not finish")
        assert np.array_equal(o["y"], d["y"]), (name, u)
        ky = max(ky, float(F.y_errors(r, o["y"]).max()))
        if t.stage == "raw":
            assert o["raw"].shape == d["raw"].shape
            F.same_zero_pattern(t, u, r, o["raw"], k["raw"], False, wide=not t.stationary)
            for j in t.bands:
                br = r["bands"][j]
                e = F.raw_errors(br, o["raw"][j], False)
                both = (o["raw"][j] != 0) & (d["raw"][j] != 0) & (br["raw"] != 0)
                a = np.zeros(len(e))
                a[both] = np.abs(o["raw"][j] - d["raw"][j])[both] / br["unit_fir"][both]
                if not t.stationary:
                    wide = F.near_threshold(br, k["raw"], False, t.floor, t.ceil, t.fs_d, True)
                    e[wide], a[wide] = 0.0, 0.0
                kr, apart = max(kr, float(e.max())), max(apart, float(a.max()))
    print("harvest front %s: the real reference's own K: y %.3f, raw %.3f (K_ref %.3f, %.3f); restatement and reference %.3f units apart; "
          "the reference's tail survived %d of %d utterances" % (name, ky, kr, k["y"], k["raw"], apart, sum(o["survived"] for o in taps), len(taps)))
    assert ky <= k["y"]
    if t.stationary:
        assert apart <= kr + k["raw"]  # both within their own K of the rule


@pytest.mark.parametrize("name", F.RAW_TABLES)
def test_near_threshold_cap(port, name):
    """at most 1 % of a table's live positions lie in the near-threshold set, under the FIR form's bound and under the sliding
    forms': a condition the frequencies were chosen to meet, shown with the rule and K_ref alone"""
    t, k = F.table(name), F.k_ref(port)["raw"]
    for sliding in (False, True):
        near = live = 0
        for r in F.rule(name):
            for j in t.bands:
                br = r["bands"][j]
                if br["alive"]:
                    live += len(br["raw"])
                    near += int(F.near_threshold(br, k, sliding, t.floor, t.ceil, t.fs_d).sum())
        print("harvest front %s: %d of %d live positions near a threshold (%s bound)" % (name, near, live, "sliding" if sliding else "FIR"))
        assert live > 0 and 100 * near <= live


def band_of(t, f):
    return F.near_bands(t, [f], 0)[0]


def check_ratio(name):
    t = F.table(name)
    r = int(name.split("_")[1])
    assert t.r == r and len(t.xs[0]) % r != 0 and np.abs(t.xs[0]).max() < 1.0
    assert (t.fs == 48000 and t.target_fs != 8000.0) == (r in (5, 9))  # two of the untested ratios reached through target_fs
    rr = F.rule(name)[0]
    assert rr["acc"] == 0 and np.abs(rr["y"]).max() > 0.3 and (rr["u_y"] > 0).all()


def check_dec(name):
    t = F.table(name)
    if name == "dec_short":
        assert [len(x) for x in t.xs] == [8, 9, 10] and t.r == 2 and all(t.L1(u) == 3 for u in range(3))
        return
    lag = 140
    assert {lag - 1, lag, lag + 1, 32, 33} <= {len(x) for x in t.xs}
    assert {31, 32, 33, F.DS_SPAN - 1, F.DS_SPAN, F.DS_SPAN + 1} <= set(t.notes["y_lens"])
    assert all(r["acc"] == 0 for r in F.rule(name))


def check_dc(name):
    t = F.table(name)
    rs = F.rule(name)
    assert t.xs[0].max() == 1.0 and t.xs[1].max() == float(np.nextafter(1.0, 0.0)) and np.abs(t.xs[1]).max() < 1.0 <= np.abs(t.xs[0]).max()
    assert rs[0]["acc"] == rs[1]["acc"] == 0  # one sample of 1.0: acc becomes 1, the next negative sample takes it back below 1 -> 0
    assert rs[2]["acc"] == 2 * len(t.xs[2]) and rs[3]["acc"] == -2 * len(t.xs[3])  # 2.5 +- 0.4 truncates to 2 at every step
    for u in (4, 5):  # a sum that truncates differently from the mean of the doubles, far below 2^31
        assert abs(rs[u]["acc"]) < 1 << 20 and abs(rs[u]["acc"] - t.xs[u].sum()) > 100
        assert F.dc_rule(np.append(t.xs[u], 0.0), "dc_round")[1] != rs[u]["acc"]


def check_seam(name):
    t = F.table(name)
    rs = F.rule(name)
    adv = F.FIR_ADV if name.endswith("_fir") else F.SD_CH
    assert t.notes["adv"] == adv
    seen = set()
    for u, f, kind, border, off in t.notes["placed"]:
        e = rs[u]["bands"][band_of(t, f)]["zs"][kind]["e"]
        want = border + int(np.ceil(off))  # the edge index: the crossing lies between samples want - 1 and want
        assert want in e, (name, u, f, kind, border, off)
        seen.add((kind, border, want - border))
    assert seen == {(kind, b, o) for kind in range(4) for b in (adv, 2 * adv) for o in (-1, 0, 1)}
    assert {adv - 1, adv, adv + 1, 2 * adv - 1, 2 * adv, 2 * adv + 1} <= {t.y_len(u) for u in range(len(t.xs))}


def check_late(name):
    t = F.table(name)
    rs = F.rule(name)
    for u, f, pos in t.notes["placed"]:
        assert pos in rs[u]["bands"][band_of(t, f)]["zs"][0]["e"]
    assert {p % F.SD_CH for _, _, p in t.notes["placed"]} == set(range(2040, 2048)) | set(range(8))


def check_few(name):
    t = F.table(name)
    rs = F.rule(name)
    mins = {min(br["counts"]) for r in rs for br in r["bands"].values()}
    assert {0, 1, 2, 3, 4} <= mins  # no edge at all, one, two and three intervals -- dead -- beside three and four -- alive
    for r in rs:
        for br in r["bands"].values():
            assert br["alive"] == (min(br["counts"]) > 2) and (br["alive"] or not br["raw"].any())
    mixed = [br["counts"] for r in rs for br in r["bands"].values() if min(br["counts"]) == 2 and max(br["counts"]) >= 3]
    assert mixed  # a band that dies by one type alone
    assert any(br["alive"] and br["raw"].any() for r in rs for br in r["bands"].values())
    assert t.y_len(8) < 2 * F.half_len(t.fs_d, t.b[0]) + 1 and not any(br["alive"] for br in rs[8]["bands"].values())


def check_burst(name):
    t = F.table(name)
    for r in F.rule(name):
        exact = sum(int((br["f"][-200:] == 0).all() and (br["A"][-200:] == 0).all()) for br in r["bands"].values())
        assert exact == len(t.bands)  # behind the burst every band's sum is over zeros alone
        # an edge that exists by `<= 0` meeting an exact zero: some band's last falling edge lands on the first exact zero
    ends = 0
    for r in F.rule(name):
        for br in r["bands"].values():
            for kind, s in ((0, br["f"]), (1, -br["f"])):
                z = br["zs"][kind]
                if z is not None and s[z["e"][-1]] == 0:
                    ends += 1
    assert ends >= 20


def check_band_test(name):
    t = F.table(name)
    rs = F.rule(name)
    j, fr = t.notes["band"], F.BAND_TEST_FRAME
    b = t.b[j]
    lo1, hi1, lo9, hi9 = [rs[u]["bands"][j]["value"][fr] for u in range(4)]
    assert lo1 < b * 1.1 <= hi1 and lo9 < b * 0.9 <= hi9  # neighbouring doubles of tone frequency straddle each product
    assert float(np.nextafter(t.notes["close"][0], np.inf)) == t.notes["close"][1]
    u = t.notes["equal"]
    assert u is not None and rs[u]["bands"][j]["value"][fr] == b * 1.1 and rs[u]["bands"][j]["raw"][fr] == b * 1.1  # equality is kept
    n_close = len(t.notes["close"])
    # the firm tones, 1e-6 to either side of the tone on 1.1 b, of the tone on 0.9 b, of floor and of ceil: at that frame each is a
    # million times the allowed error from its threshold, and of each pair one is kept and one rejected
    k_big = 1e3  # (any K the restatement could have: firmness here does not hang on it)
    for i in range(0, 8, 2):
        kept = []
        for f in t.notes["firm"][i:i + 2]:
            br = rs[n_close + t.notes["firm"].index(f)]["bands"][j if i < 4 else band_of(t, f)]
            assert not F.near_threshold(br, k_big, True, t.floor, t.ceil, t.fs_d)[fr]
            kept.append(bool(br["raw"][fr] != 0))
        assert sorted(kept) == [False, True], (i, kept)


def check_runs(name):
    t = F.table(name)
    rs = F.rule(name)
    nb = len(t.b)
    want = {"runs_33": (9, 10), "runs_36": (10, 11)}[name]
    for u, n_lit in enumerate(want):
        cand, runs = F.detect_rule(F.rule_raw(t, rs[u]), t.S)
        mid = runs[80:120]
        assert all(len(r) == 1 and r[0][1] - r[0][0] == n_lit for r in mid), (name, u, mid[:3])
        assert (cand[80:120, 0] != 0).all() == (n_lit >= 10) and not cand[80:120, 1:].any()
    cand, runs = F.detect_rule(F.rule_raw(t, rs[2]), t.S)  # lights band 0: the forced zero there shortens the run to start at band 1
    raw = F.rule_raw(t, rs[2])
    assert (raw[0, 80:120] > 0).all() and all(r[0][0] == 1 for r in runs[80:120])
    if name == "runs_33":
        cand, runs = F.detect_rule(F.rule_raw(t, rs[3]), t.S)
        raw = F.rule_raw(t, rs[3])
        assert (raw[nb - 1, 80:120] > 0).all() and all(r[-1][1] == nb - 1 for r in runs[80:120])
    cand, runs = F.detect_rule(F.rule_raw(t, rs[4]), t.S)  # two runs in a frame: a second slot
    assert (cand[80:120, 0] != 0).all() and (cand[80:120, 1] != 0).all() and not cand[80:120, 2:].any()


def check_level(name):
    t = F.table(name)
    rs = F.rule(name)
    hl_max = F.half_len(t.fs_d, t.b[0])
    assert len(rs) == len(F.LEVELS) == 4 and sorted(F.LEVELS) == [1e-10, 0.5e-8, 2e-8, 1e-6]
    # the fall lies inside the first chunk, a window clear of either end of it; the zeros begin behind everything the first
    # chunk's sums ever read, and the second chunk reads them
    assert 2 * hl_max + 2 < F.LEVEL_FALL < F.SD_CH - 2 * hl_max and F.LEVEL_ZEROS >= (F.SD_CH + hl_max + 4) // 64 * 64 + 64
    for c, x, r in zip(F.LEVELS, t.xs, rs):
        assert np.abs(x[:F.LEVEL_FALL]).max() > 0.89 and 0.89 * c < np.abs(x[F.LEVEL_FALL:F.LEVEL_ZEROS]).max() <= 0.9 * c
        assert not x[F.LEVEL_ZEROS:].any() and x[F.LEVEL_FALL:F.LEVEL_ZEROS].all()
        assert r["quiet"] == [c < 1e-8, True], (c, r["quiet"])  # the threshold lies between 0.5e-8 and 2e-8
        for j in t.bands:
            br = r["bands"][j]
            firm = ~F.near_threshold(br, 1e3, False, t.floor, t.ceil, t.fs_d, wide=True)[F.LEVEL_FRAMES]  # (any K it could have)
            live = br["raw"][F.LEVEL_FRAMES] != 0
            assert br["alive"] and (firm & live).sum() >= 80, (c, j, int((firm & live).sum()))
            # those frames read the quiet stretch of the first chunk and nothing else: every edge of their interpolation lies
            # a window behind the fall and in front of the second chunk
            lo, hi = F.LEVEL_FRAMES.start * 8, (F.LEVEL_FRAMES.stop - 1) * 8
            assert lo - 2 * 8000.0 / t.b[j] > F.LEVEL_FALL + br["hl"] and hi + 2 * 8000.0 / t.b[j] < F.SD_CH


CHECKS = dict(level=check_level, ratio=check_ratio, dec=check_dec, dc=check_dc, seam=check_seam, late=check_late, few=check_few, burst=check_burst,
              band=check_band_test, runs=check_runs)


@pytest.mark.parametrize("name", F.NAMES)
def test_table_reaches_what_it_is_named_for(name):
    CHECKS[name.split("_")[0]](name)
    t = F.table(name)
    if t.stage == "raw" and name != "dc":
        assert all(np.abs(x).max() < 1.0 for x in t.xs)


def raw_mutant_ratio(name, mutant, k):
    """how far a mutant of the rule leaves the device's widest bound (the sliding forms'), as a multiple of it, over the positions
    the device test compares; a zero pattern that differs on a firm position counts as infinitely far"""
    t = F.table(name)
    worst = 0.0
    for r0, rm in zip(F.rule(name), F.rule(name, mutant)):
        for j in t.bands:
            b0, bm = r0["bands"][j], rm["bands"][j]
            firm = ~F.near_threshold(b0, k, True, t.floor, t.ceil, t.fs_d)
            if ((b0["raw"] != 0) != (bm["raw"] != 0))[firm].any():
                return np.inf
            both = firm & (b0["raw"] != 0)
            if both.any():
                worst = max(worst, float((np.abs(bm["raw"] - b0["raw"])[both] / F.allowed_hz(b0, k, True)[both]).max()))
    return worst


def test_ge_for_gt_in_the_band_test_is_out_of_a_devices_reach(port):
    """`>= 1.1 b` for `> 1.1 b` differs from the rule only where a candidate EQUALS the product: at the tone band_test placed
    there the rule keeps the candidate and the changed rule drops it.  That frame is by construction inside the near-threshold
    set, where a device is not held to the zero pattern (its value carries roundings): the rule has this tooth, no table can give
    it to a kernel, and it is not counted among the mutants that are caught.  The firm tones hold the comparison's direction."""
    t, k = F.table("band_test"), F.k_ref(port)
    u, j, fr = t.notes["equal"], t.notes["band"], F.BAND_TEST_FRAME
    a, b = F.rule("band_test")[u]["bands"][j], F.rule("band_test", "ge_upper")[u]["bands"][j]
    assert a["raw"][fr] != 0 and b["raw"][fr] == 0
    assert F.near_threshold(a, k["raw"], False, t.floor, t.ceil, t.fs_d)[fr]
    assert raw_mutant_ratio("band_test", "ge_upper", k["raw"]) < 1.0  # nothing a device is held to moves


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_mutant_of_the_rule_is_caught(port, mutant):
    name = F.MUTANT_TABLE[mutant]
    t, k = F.table(name), F.k_ref(port)
    if mutant in ("bias_hl", "fine_from_e", "lt0"):
        got = raw_mutant_ratio(name, mutant, k["raw"])
    elif mutant == "run9":
        got = 0.0
        for r in F.rule(name):
            raw = F.rule_raw(t, r)
            if not np.array_equal(F.detect_rule(raw, t.S)[0] != 0, F.detect_rule(raw, t.S, mutant)[0] != 0):
                got = np.inf
    else:  # coef12, dc_round: y against its bound
        got = 0.0
        for r0, rm in zip(F.rule(name), F.rule(name, mutant)):
            e = F.y_errors(r0, rm["y"].astype(np.float64))
            got = max(got, float(e.max()) / (2.0 * k["y_r"][t.r]))
    print("harvest front: mutant %s on %s leaves the bound %.3g x" % (mutant, name, got))
    assert got >= 100.0
