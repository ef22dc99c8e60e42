"""CPU tests of the rule of voice morphing as tests/morph_rule.py restates it (the GPU tests hold the kernel to that restatement),
of the inputs the GPU tests share, and of the host helpers beside it, which stay as they are."""
import numpy as np
import pytest

import morph_rule as mr
import retime_rule as rr


def rows(n, bins=9, seed=1):
    """a voiced / unvoiced contour and two positive row matrices"""
    g = np.random.default_rng(seed)
    f0 = 100.0 + 50.0 * g.random(n)
    f0[g.random(n) < 0.3] = 0.0
    return f0, np.exp(g.normal(size=(n, bins))), g.random((n, bins))


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_weight_zero_is_retime_of_a_and_weight_one_retime_of_b():
    a, b = rows(40, seed=1), rows(31, seed=2)
    pa, pb = np.arange(0, 39, 0.6), np.linspace(30, -2, 65)
    m = len(pa)
    assert len(pb) == m
    for w, src, pos in ((0.0, a, pa), (1.0, b, pb)):
        got = mr.morph(a, b, pa, pb, np.full(m, w))
        for g, want in zip(got, rr.retime(*src, pos)):
            assert same(g, want)
    # the F0 weight alone decides the contour's source
    got = mr.morph(a, b, pa, pb, np.zeros(m), np.ones(m))
    assert same(got[0], rr.retime(*b, pb)[0]) and same(got[1], rr.retime(*a, pa)[1])


def test_swapping_the_sources_at_the_middle_weight():
    """(1 - w) and w are both 0.5: ap is the same sum with its terms swapped, bit for bit; sp goes through log and exp of the same
    two terms (1e-15: the sum commutes, so this is bit for bit in practice)"""
    a, b = rows(40, seed=3), rows(31, seed=4)
    pa, pb = np.arange(0, 39, 0.7), np.arange(0, 39, 0.7) * 0.5
    w = np.full(len(pa), 0.5)
    x, y = mr.morph(a, b, pa, pb, w), mr.morph(b, a, pb, pa, 1.0 - w)
    assert np.array_equal(x[2], y[2])
    assert np.abs(x[1] / y[1] - 1).max() <= 1e-15
    assert same(x[0], y[0])


def test_rows_are_two_products_one_sum_and_for_sp_one_exp():
    a, b = rows(10, seed=5), rows(10, seed=6)
    got = mr.morph(a, b, [3.0], [4.25], [0.3])
    apb = 0.75 * b[2][4] + 0.25 * b[2][5]
    spb = 0.75 * b[1][4] + 0.25 * b[1][5]
    assert np.array_equal(got[2][0], (1.0 - 0.3) * a[2][3] + 0.3 * apb)
    assert np.array_equal(got[1][0], np.exp((1.0 - 0.3) * np.log(a[1][3]) + 0.3 * np.log(spb)))
    # weights outside [0, 1] extrapolate
    out = mr.morph(a, b, [3.0], [4.0], [1.5])
    assert np.array_equal(out[2][0], (1.0 - 1.5) * a[2][3] + 1.5 * b[2][4])
    assert np.allclose(out[1][0], b[1][4] * np.sqrt(b[1][4] / a[1][3]), rtol=1e-13)


def test_voicing_follows_the_nearer_source():
    a, b = rows(6, seed=7), rows(6, seed=8)
    a[0][:], b[0][:] = 0.0, 0.0
    a[0][2], b[0][3] = 120.0, 240.0
    e = 2.0 ** -20
    wf = np.array([0.0, 0.5 - e, 0.5, 0.5 + e, 1.0, -0.5, 1.5])
    m = len(wf)
    f = lambda ia, ib: mr.morph(a, b, np.full(m, ia), np.full(m, ib), np.full(m, 0.5), wf)[0]
    both = f(2.0, 3.0)
    assert both[0] == 120.0 and both[4] == 240.0
    assert np.allclose(both[[1, 2, 3, 5, 6]], 120.0 * 2.0 ** wf[[1, 2, 3, 5, 6]], rtol=1e-14)  # a glide in log-F0, also beyond the ends
    assert list(f(2.0, 0.0)) == [120.0, 120.0, 0.0, 0.0, 0.0, 120.0, 0.0]  # only A voiced: fA while wf < 0.5
    assert list(f(0.0, 3.0)) == [0.0, 0.0, 0.0, 240.0, 240.0, 0.0, 240.0]  # only B voiced: fB while wf > 0.5
    assert list(f(0.0, 0.0)) == [0.0] * m
    # without an F0 weight the weight decides
    assert mr.morph(a, b, [2.0], [0.0], [0.25])[0][0] == 120.0 and mr.morph(a, b, [2.0], [0.0], [0.75])[0][0] == 0.0


def test_values_that_are_not_finite_spoil_their_own_frame_only():
    a, b = rows(20, seed=9), rows(25, seed=10)
    pa, pb = np.arange(0, 19, 0.5), np.arange(0, 19, 0.5) * 1.2
    m = len(pa)
    w, wf = mr.cycled_weights(m), mr.cycled_weights(m, 3)
    want = mr.morph(a, b, pa, pb, w, wf)
    assert all(np.isfinite(v).all() for v in want)
    bpa, bpb, bw, bwf = pa.copy(), pb.copy(), w.copy(), wf.copy()
    bpa[0], bpb[5], bw[17], bpa[m - 1], bw[20] = np.nan, np.inf, -np.inf, np.inf, np.nan
    bwf[9] = np.nan
    got = mr.morph(a, b, bpa, bpb, bw, bwf)
    bad = np.zeros(m, bool)
    bad[[0, 5, 17, m - 1, 20]] = True
    for q in range(3):
        assert np.isnan(got[q][bad]).all()
    assert np.isnan(got[0][9]) and np.isfinite(got[1][9]).all() and np.isfinite(got[2][9]).all()
    bad_f0 = bad.copy()
    bad_f0[9] = True
    assert np.array_equal(got[0][~bad_f0], want[0][~bad_f0])
    assert np.array_equal(got[1][~bad], want[1][~bad]) and np.array_equal(got[2][~bad], want[2][~bad])


def test_ratios_are_not_part_of_the_numpy_rule():
    a, b = rows(5), rows(5)
    with pytest.raises(NotImplementedError):
        mr.morph(a, b, [0.0], [0.0], [0.5], ratio_a=[1.1])


@pytest.mark.parametrize("with_f0_weight", [False, True])
def test_the_shared_batch(with_f0_weight):
    """the pairs, the weights and the maps of the GPU tests: about 400 output frames, every weight of the cycle in every voicing
    case that the rule tells apart, and the batch restatement is the pairs one by one"""
    fs, fft = 16000, 512
    d = mr.batch(fs, fft, 100, with_f0_weight)
    assert d["a_lengths"] == [61, 97, 74] and d["b_lengths"] == [97, 74, 61]
    m = sum(d["out_lengths"])
    assert 300 <= m <= 500 and all(len(d[k]) == m for k in ("pos_a", "pos_b", "weight"))
    assert np.array_equal(d["pos_a"][:d["out_lengths"][0]], d["pos_b"][:d["out_lengths"][0]])
    assert not np.array_equal(d["pos_a"][d["out_lengths"][0]:], d["pos_b"][d["out_lengths"][0]:])
    assert list(d["weight"][:8]) == mr.WEIGHTS
    if with_f0_weight:
        assert list(d["f0_weight"][:8]) == mr.WEIGHTS[3:] + mr.WEIGHTS[:3]
    fa = rr.retime_batch(d["a_lengths"], *d["a"], d["out_lengths"], d["pos_a"])[0]
    fb = rr.retime_batch(d["b_lengths"], *d["b"], d["out_lengths"], d["pos_b"])[0]
    wf = d["weight"] if d["f0_weight"] is None else d["f0_weight"]
    blend = (wf != 0) & (wf != 1)
    for below in (True, False):  # each case on either side of the middle weight
        side = blend & ((wf < 0.5) if below else (wf > 0.5))
        assert all(c > 0 for c in mr.voicing_cases(fa[side], fb[side])), (below, mr.voicing_cases(fa[side], fb[side]))
    got = mr.rule_of(d)
    assert all(np.isfinite(v).all() for v in got)
    o0, o1 = d["out_lengths"][0], d["out_lengths"][0] + d["out_lengths"][1]
    one = mr.morph(tuple(v[61:61 + 97] for v in d["a"]), tuple(v[97:97 + 74] for v in d["b"]), d["pos_a"][o0:o1], d["pos_b"][o0:o1],
                   d["weight"][o0:o1], None if d["f0_weight"] is None else d["f0_weight"][o0:o1])
    for q in range(3):
        assert np.array_equal(got[q][o0:o1], one[q])
    assert np.array_equal(mr.to_length(np.arange(5.0), 3), [0.0, 1.0, 2.0]) and np.array_equal(mr.to_length(np.arange(3.0), 5), [0.0, 1.0, 2.0, 2.0, 2.0])


def test_float64_rule_sits_near_its_long_double_evaluation():
    """the allowance of the GPU test (1e-12 relative) against what the rule's own log / exp arithmetic costs in float64: the blend
    of the shared batch evaluated in long double"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double on this platform: nothing to compare with")
    d = mr.batch(16000, 512, 100)
    sp = mr.rule_of(d)[1]
    spa = rr.retime_batch(d["a_lengths"], *d["a"], d["out_lengths"], d["pos_a"])[1].astype(np.longdouble)
    spb = rr.retime_batch(d["b_lengths"], *d["b"], d["out_lengths"], d["pos_b"])[1].astype(np.longdouble)
    w = d["weight"].astype(np.longdouble)[:, None]
    ref = np.exp((1 - w) * np.log(spa) + w * np.log(spb))
    err = float(np.abs(sp / ref - 1).max())
    print("numpy rule against long double: %.2e" % err)
    assert err < 1e-13


def test_time_map_and_its_siblings_stay():
    from world_class_amd import io
    assert np.array_equal(io.time_map(120, 0.5), rr.map_of("half_speed", 120))
    assert np.array_equal(io.time_map(5, [1.0, 2.0, 0.5]), [0.0, 1.0, 3.0])
    import inspect
    assert list(inspect.signature(io.time_map).parameters) == ["n_frames", "speed"]
    assert list(inspect.signature(io.retime_parameters).parameters) == ["f0", "sp", "ap", "position", "fs", "fft_size", "f0_scale", "spectral_ratio"]
