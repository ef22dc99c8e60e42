"""-m gpu: Harvest's refinement on the device -- hv_refine_group_kernel, hv_refine_packed_kernel and hv_refine_kernel, run alone on
candidate rows the test wrote (wc_harvest_debug_refine) -- against the CPU oracle's refinement on the same rows and samples
(wco_harvest_refine), position by position, and against the long double rule of tests/harvest_refine.py, whose tables these are
(tests/test_harvest_refine_rule.py proves what each one reaches and that the rule is sharp).

What is compared how:
 * the decimated signal the device refines is the one the oracle and the rule are given, bit for bit;
 * outside the near-threshold set (rule value within the bound of floor, ceiling or score 2.5) the device's rows are zero exactly
   where the oracle's and the rule's are, and nowhere else is there a value;
 * the refined F0 within 2 K_ref max(1, q / log2 N) units of the rule, 1 / score within as many units of u / f (units, K_ref, q:
   harvest_refine's docstring) -- nothing chosen in advance: K_ref is the oracle's own worst error in the same units;
 * default = slots = packed layout bit for bit on every table.

Measured on an MI355X: see DESIGN.md, "Harvest's refinement on written candidates".
"""
import numpy as np
import pytest

import harvest_refine as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


_handles, _device = {}, {}


def split(t, rows):
    at = np.concatenate([[0], np.cumsum([t.L1(u) for u in range(len(t.xs))])])
    return [rows[a:b] for a, b in zip(at[:-1], at[1:])]


def device(wca, name, mode=0):
    """the device's refinement of a table's rows in one call over its utterances: per utterance (cand1, score1); once per mode.
    mode: 0 the default dispatch, 1 the slot layout, 2 the packed layout"""
    t = R.table(name)
    if name not in _handles:
        h = wca.Harvest(t.fs, **t.options())
        h.compute_batch(t.xs)
        for u in range(len(t.xs)):
            assert np.array_equal(h.debug_fetch("y", u), t.y(u)), (name, u, "the device refines other samples than the oracle")
            assert len(h.debug_fetch("cand0", u)) == t.L1(u) * t.S, (name, u, "rows are not S wide")
        _handles[name] = h
    if (name, mode) not in _device:
        c1, s1 = _handles[name].debug_refine(t.rows(), by_slots=mode)
        _device[(name, mode)] = list(zip(split(t, c1), split(t, s1)))
    return _device[(name, mode)]


@pytest.mark.parametrize("name", R.NAMES)
def test_refinement_matches_the_oracle_and_the_rule(wca, port, name):
    t, k = R.table(name), R.k_ref(port)
    worst = dict(f=0.0, s=0.0, f_share=0.0, s_share=0.0, hz=0.0)
    for u, (r, (oc, os_, _), (dc, ds)) in enumerate(zip(R.rule(name), R.oracle(port, name), device(wca, name))):
        R.same_zero_pattern(t, r, dc, ds, k)
        firm = r["live"] & ~R.near_threshold(t, r, k)
        assert np.array_equal((dc != 0)[firm], (oc != 0)[firm]) and not (dc != 0)[~r["live"]].any(), (name, u)
        ef, es = R.errors(r, dc, ds)
        live = r["live"]
        bound = R.allowed(r, k)[live]
        assert (bound >= 2.0 * k).all()
        both = (dc != 0) & (oc != 0)
        worst["f"], worst["s"] = max(worst["f"], float(ef.max())), max(worst["s"], float(es.max()))
        worst["f_share"] = max(worst["f_share"], float((ef[live] / bound).max()))
        worst["s_share"] = max(worst["s_share"], float((es[live] / bound).max()))
        if both.any():
            worst["hz"] = max(worst["hz"], float(np.abs(dc - oc)[both].max()))
    print("harvest refinement %s: K_ref %.3f; device's worst error in units: F0 %.3f (%.3f of its bound), 1 / score %.3f (%.3f of its "
          "bound); max |device - oracle| %.3e Hz" % (name, k, worst["f"], worst["f_share"], worst["s"], worst["s_share"], worst["hz"]))
    assert worst["f"] > 0.0 and worst["s"] > 0.0, (name, "nothing was compared")
    assert worst["f_share"] <= 1.0, (name, "refined F0", worst)
    assert worst["s_share"] <= 1.0, (name, "1 / score", worst)


@pytest.mark.parametrize("name", R.NAMES)
def test_layouts_agree_bit_for_bit(wca, name):
    """frames in groups (or, for rows wider than 128 positions, the packed kernel), one wavefront per slot, one wavefront per frame:
    the same bits, at N = 4096, at both ends of an utterance, on full rows and over silence as well"""
    a = device(wca, name)
    for mode in (1, 2):
        for u, ((ac, as_), (bc, bs)) in enumerate(zip(a, device(wca, name, mode))):
            assert np.array_equal(ac, bc) and np.array_equal(as_, bs), (name, mode, u)
    assert any((c != 0).any() for c, _ in a)


def test_ragged_batch_equals_each_utterance_alone(wca):
    """a quiet short utterance between loud ones whose edge rows are full: a frame that read its neighbour's samples or candidate
    rows would differ from the same utterance alone in its call"""
    t = R.table("ragged")
    got = device(wca, "ragged")
    for u in range(len(t.xs)):
        h = wca.Harvest(t.fs, **t.options())
        h.compute_batch([t.xs[u]])
        c1, s1 = h.debug_refine(t.cand0[u])
        assert np.array_equal(c1, got[u][0]) and np.array_equal(s1, got[u][1]), u
    assert (got[1][0] != 0).any()
