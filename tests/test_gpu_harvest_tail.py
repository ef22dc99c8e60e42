"""-m gpu: Harvest's tail on the device -- hv_unreliable_kernel, the three hv_contour_kernel phases, hv_smooth_kernel and
hv_output_kernel, run alone on candidate rows the test wrote (wc_harvest_debug_tail) -- against the CPU oracle's tail on the same
rows (wco_harvest_tail).  The tables are those of tests/harvest_tail.py; tests/test_harvest_tail_rule.py proves what each one reaches.

What is compared how:
 * cand and score after the removal, f0_base and the contours after fixStep1..3 are selections among the values of the table
   (the divisions and ordered sums that decide are IEEE operations in the same order on both sides, the scores summed in mergeF0Sub
   are small integers): bit for bit;
 * fixStep4's t0 + coef * c and the smoothing filter may be contracted by one compiler and not by the other: f0_fixed, f0_1ms and
   the output within the project's 1e-6 Hz, their voiced / unvoiced pattern identical.
"""
import os

import numpy as np
import pytest

import harvest_tail as T

pytestmark = pytest.mark.gpu

F0_ABS = 1e-6
EXACT = ("cand", "score", "f0_base", "s1", "s2", "s3")
CLOSE = ("f0_fixed", "f0_1ms", "f0")
FETCH = dict(cand="cand", score="score", f0_base="base", s1="s1", s2="s2", s3="s3", f0_fixed="fixed", f0_1ms="f0_1ms")


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


def quiet(n, seed=0):
    """the call that sizes the batch: noise far below anything voiced"""
    return np.random.default_rng(1000 + seed).normal(0.0, 0.01, n)


def new_handle(wca, cio, fp=5.0, smooth_full=False):
    if smooth_full:
        os.environ["WC_HARVEST_SMOOTH"] = "full"
    try:
        return wca.Harvest(T.FS, frame_period=fp, channels_in_octave=cio)
    finally:
        if smooth_full:
            del os.environ["WC_HARVEST_SMOOTH"]


def run_tail(h, x_lengths, cand, score):
    """one call on quiet signals of the given lengths, then the tail on the rows: per utterance, everything the oracle returns"""
    h.compute_batch([quiet(n, k) for k, n in enumerate(x_lengths)])
    outs = h.debug_tail(cand, score)
    res = []
    for u, (tpos, f0) in enumerate(outs):
        r = dict(tpos=tpos, f0=f0)
        for key, name in FETCH.items():
            r[key] = h.debug_fetch(name, u)
        L = len(r["f0_base"])
        r["cand"], r["score"] = r["cand"].reshape(L, -1), r["score"].reshape(L, -1)
        res.append(r)
    return res


_device = {}


def device(wca, name, fp=5.0, smooth_full=False):
    """the device's result for a table alone in its call on a fresh handle, computed once"""
    key = (name, fp, smooth_full)
    if key not in _device:
        _device[key] = run_tail(new_handle(wca, T.TABLES[name][1], fp, smooth_full), *T.table(name))
    return _device[key]


def same_bits(a, b, where):
    for key in EXACT + CLOSE + ("tpos",):
        assert np.array_equal(a[key], b[key]), (where, key)


def check_against_oracle(dev, ref, where):
    worst = {}
    for key in EXACT:
        assert np.array_equal(dev[key], ref[key]), (where, key)
    assert np.array_equal(dev["tpos"], ref["tpos"]), where
    for key in CLOSE:
        assert np.array_equal(dev[key] == 0, ref[key] == 0), (where, key, "voiced/unvoiced pattern")
        worst[key] = float(np.abs(dev[key] - ref[key]).max())
    print("harvest tail %s: max |device - oracle| in Hz: " % (where,) + ", ".join("%s %.3e" % kv for kv in worst.items()))
    for key in CLOSE:
        assert worst[key] < F0_ABS, (where, key, worst[key])


@pytest.mark.parametrize("name", sorted(T.TABLES))
def test_tail_matches_the_oracle(wca, port, name):
    """every table, alone in its call: decisions bit for bit, values within 1e-6 Hz"""
    dev, ref = device(wca, name), T.reference(port, name)
    assert len(dev) == len(ref)
    for u, (d, r) in enumerate(zip(dev, ref)):
        check_against_oracle(d, r, (name, u))


@pytest.mark.parametrize("name", sorted(T.TABLES))
def test_smoothing_that_skips_is_bit_equal_on_the_tables(wca, name):
    """WC_HARVEST_SMOOTH=full walks every step of the filter; the default skips settled stretches.  The tables' constant sections
    settle exactly, again and again, and 70 sections take two rounds of lanes: same bits."""
    for u, (a, b) in enumerate(zip(device(wca, name), device(wca, name, smooth_full=True))):
        same_bits(a, b, (name, u))


@pytest.mark.parametrize("fp", [1.0, 2.5, 10.0])
def test_output_frame_periods(wca, port, fp):
    """hv_output_kernel at other frame periods than the default's 5 ms; 2.5 ms puts every other index on a rounding half"""
    dev, ref = device(wca, "step4_small", fp), T.reference(port, "step4_small", fp)
    check_against_oracle(dev[0], ref[0], ("step4_small", fp))
    assert len(dev[0]["f0"]) == len(ref[0]["f0"]) and (dev[0]["f0"] != 0).any()


def test_ragged_batch_of_tables(wca):
    """one call, four tables of different lengths -- 1200 frames with 148 sections, 37 frames, 500 frames, and the three frames of the
    shortest utterance Harvest takes: each result is that table's result alone in its call"""
    names = ("many_148", "short37", "three_sections", "tiny")
    tabs = [T.table(n) for n in names]
    got = run_tail(new_handle(wca, 40.0), *T.batch(*tabs))
    assert len(got) == len(names)
    for n, g in zip(names, got):
        same_bits(g, device(wca, n)[0], n)


def test_few_sections_after_many_on_one_handle(wca):
    """the section lists, channel windows and position bookkeeping of a call with 148 sections are still in the handle's scratch when a
    call with three sections at a smaller length follows: same bits as on a fresh handle"""
    h = new_handle(wca, 40.0)
    first = run_tail(h, *T.table("many_148"))
    same_bits(first[0], device(wca, "many_148")[0], "many_148")
    second = run_tail(h, *T.table("three_sections"))
    same_bits(second[0], device(wca, "three_sections")[0], "three_sections")
    assert int((second[0]["f0_1ms"] != 0).sum()) > 100
