"""CPU tests of the rule of time-scale modification as tests/retime_rule.py restates it (the GPU tests hold the kernel to that
restatement bit for bit), and of the host helper io.time_map."""
import numpy as np
import pytest

import retime_rule as rr


def rows(n, bins=9, seed=1):
    """a voiced / unvoiced contour and two positive row matrices"""
    g = np.random.default_rng(seed)
    f0 = 100.0 + 50.0 * g.random(n)
    f0[g.random(n) < 0.3] = 0.0
    return f0, np.exp(g.normal(size=(n, bins))), g.random((n, bins))


def test_identity_map_returns_the_inputs_bit_for_bit():
    f0, sp, ap = rows(40)
    o = rr.retime(f0, sp, ap, np.arange(40.0))
    assert np.array_equal(o[0], f0) and np.array_equal(o[1], sp) and np.array_equal(o[2], ap)


def test_integer_positions_copy_rows_in_any_order():
    f0, sp, ap = rows(40)
    at = np.array([39, 0, 7, 7, 7, 12, 3, 38])
    o = rr.retime(f0, sp, ap, at.astype(np.float64))
    assert np.array_equal(o[0], f0[at]) and np.array_equal(o[1], sp[at]) and np.array_equal(o[2], ap[at])


def test_rows_are_two_products_and_one_sum():
    f0, sp, ap = rows(10)
    f0[:] = 120.0
    f0[3], f0[4] = 100.0, 200.0
    o = rr.retime(f0, sp, ap, [3.25])
    assert np.array_equal(o[1][0], 0.75 * sp[3] + 0.25 * sp[4]) and np.array_equal(o[2][0], 0.75 * ap[3] + 0.25 * ap[4])
    assert o[0][0] == 0.75 * 100.0 + 0.25 * 200.0


@pytest.mark.parametrize("voiced_first", [True, False])
def test_voicing_follows_the_nearer_neighbour(voiced_first):
    """between a voiced and an unvoiced frame: a == 0.5 is unvoiced; 2^-20 towards the voiced frame takes its F0 unchanged, 2^-20
    towards the unvoiced one gives 0"""
    f0, sp, ap = rows(6)
    f0[:] = 0.0
    f0[2 if voiced_first else 3] = 131.5
    e = 2.0 ** -20
    got = rr.retime(f0, sp, ap, [2.5, 2.5 - e, 2.5 + e, 2.0, 3.0])[0]
    if voiced_first:
        assert list(got) == [0.0, 131.5, 0.0, 131.5, 0.0]
    else:
        assert list(got) == [0.0, 0.0, 131.5, 0.0, 131.5]
    f0[:] = 0.0
    assert list(rr.retime(f0, sp, ap, [2.5, 2.25])[0]) == [0.0, 0.0]


def test_positions_beyond_the_ends_hold_the_end_frames():
    f0, sp, ap = rows(12)
    f0[0], f0[11] = 111.0, 222.0
    o = rr.retime(f0, sp, ap, [-3.0, -0.1, -1e300, 11.0, 11.5, 400.0, 1e300])
    assert list(o[0]) == [111.0] * 3 + [222.0] * 4
    assert all(np.array_equal(o[1][k], sp[0]) and np.array_equal(o[2][k], ap[0]) for k in range(3))
    assert all(np.array_equal(o[1][k], sp[11]) and np.array_equal(o[2][k], ap[11]) for k in range(3, 7))
    one = rr.retime(f0[:1], sp[:1], ap[:1], [0.0, 0.7, -2.0, 5.0])  # a single source frame is held everywhere
    assert list(one[0]) == [111.0] * 4 and all(np.array_equal(r, sp[0]) for r in one[1])


def test_positions_that_are_not_finite_spoil_their_own_frame_only():
    f0, sp, ap = rows(20)
    pos = np.arange(0, 19, 0.5)
    want = rr.retime(f0, sp, ap, pos)
    bad = pos.copy()
    at = [0, 5, 17, len(pos) - 1]
    bad[at] = [np.nan, np.inf, -np.inf, np.nan]
    got = rr.retime(f0, sp, ap, bad)
    keep = np.ones(len(pos), bool)
    keep[at] = False
    for w, g in zip(want, got):
        assert np.isnan(g[at]).all() and np.array_equal(g[keep], w[keep])
        assert np.isfinite(w).all()


def test_f0_scale_is_a_plain_product_per_output_frame():
    f0, sp, ap = rows(20)
    pos = np.arange(0, 19, 0.75)
    scale = 0.8 + np.arange(len(pos)) / 40.0
    scale[4] = np.nan
    plain = rr.retime(f0, sp, ap, pos)
    got = rr.retime(f0, sp, ap, pos, scale)
    assert np.array_equal(got[0], plain[0] * scale, equal_nan=True) and np.isnan(got[0][4])
    assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])


def test_the_batch_restatement_is_the_utterances_one_by_one():
    lengths, out_lengths = [7, 1, 12], [9, 0, 5]
    f0, sp, ap = rows(sum(lengths))
    pos = np.concatenate([np.linspace(0, 6, 9), np.linspace(11, 0, 5)])
    got = rr.retime_batch(lengths, f0, sp, ap, out_lengths, pos)
    a = rr.retime(f0[:7], sp[:7], ap[:7], pos[:9])
    b = rr.retime(f0[8:], sp[8:], ap[8:], pos[9:])
    for q in range(3):
        assert np.array_equal(got[q], np.concatenate([a[q], b[q]]))


@pytest.mark.parametrize("name", rr.MAPS)
def test_the_maps_of_the_gpu_tests(name):
    lengths = dict(zip(rr.MAPS, (120, 239, 80, 164, 144, 188, 142)))
    pos = rr.map_of(name, 120)
    assert len(pos) == lengths[name] and np.isfinite(pos).all()
    if name not in ("ramp", "hold_and_back"):  # (the ramp ends held at n - 1, the other holds and runs backwards)
        assert (np.diff(pos) > 0).all()
    if name not in ("overshoot", "hold_and_back"):
        assert pos.min() >= 0 and pos.max() <= 119
    else:
        assert pos.max() > 119
    assert len(rr.map_of(name, 61)) > 30


def test_time_map_for_a_scalar_speed():
    from world_class_amd import io
    for n, speed in ((120, 1.0), (120, 0.5), (120, 1.5), (120, 1.37), (2001, 0.73), (1, 2.0), (2, 3.0)):
        got = io.time_map(n, speed)
        assert got.dtype == np.float64 and np.array_equal(got, rr.time_map(n, speed))
        assert got[0] == 0 and got[-1] <= n - 1 < got[-1] + speed
    assert np.array_equal(io.time_map(120, 1.0), np.arange(120.0))
    assert np.array_equal(io.time_map(120, 0.5), rr.map_of("half_speed", 120))
    assert np.array_equal(io.time_map(120, 1.5), rr.map_of("speed_1.5", 120))
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            io.time_map(120, bad)


def test_time_map_for_a_speed_per_output_frame():
    from world_class_amd import io
    speed = 0.5 + np.arange(144) / 144
    got = io.time_map(120, speed)
    assert len(got) == 144 and got[0] == 0.0
    assert np.array_equal(got, rr.time_map(120, speed))
    assert np.array_equal(got[1:], np.cumsum(speed[:-1]))
    assert np.array_equal(io.time_map(5, [2.0]), [0.0])
    back = io.time_map(50, np.array([1.0, 1.0, -1.0, -1.0, 0.0, 0.25]))  # a map may hold or run backwards
    assert list(back) == [0.0, 1.0, 2.0, 1.0, 0.0, 0.0]
