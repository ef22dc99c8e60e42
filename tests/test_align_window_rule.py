"""CPU tests that pin the rule of the windowed alignment streams (tests/align_window_rule.py, the checker of
tests/test_gpu_align_window.py): with a window that holds the whole track it is the rule of the alignment streams
(tests/align_stream_rule.py) bit for bit at every hop; nothing depends on how the rows are cut into pushes; the window's start
never falls; under the monotone flag the position never falls, and nothing else changes where it did not fall anyway; and on a voice
that can be followed a narrow window gives the positions and costs of the whole track bit for bit."""
import numpy as np
import pytest

import align_stream_rule as asr
import align_window_rule as awr

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 40), (40, 7), (23, 31), (40, 40)]
HOPS = [1, 3, 64]
FOLLOW_WINDOWS = [(48, 16, 1), (48, 16, 8), (64, 16, 16), (32, 8, 8), (24, 8, 1)]
followable = awr.followable


def _same(got, want, what=None):
    assert got[0].tobytes() == want[0].tobytes(), (what, "position", got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (what, "cost", got[1], want[1])


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("n,m", SHAPES)
def test_a_window_over_the_whole_track_is_the_unwindowed_rule(n, m, open_begin, hop):
    rng = np.random.default_rng(1000 * n + m)
    a, b = rng.standard_normal((n, 6)), rng.standard_normal((m, 6))
    want = asr.follow(a, b, 1, 6, open_begin)
    for width in (m, m + 5):
        _same(awr.follow(a, b, 1, 6, open_begin, width, min(3, m - 1), hop), want, (width, hop))
    # integer-valued costs of 0 to 2: every comparison and the scan meet equal operands
    d = rng.integers(0, 3, (n, m)).astype(np.float64)
    f, g = asr.Follower(m=m, open_begin=open_begin), awr.WindowFollower(m=m, open_begin=open_begin, width=m, back=m - 1, hop=hop)
    _same(g.push_costs(d), f.push_costs(d), "ties")


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("open_begin", [False, True])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_rows_that_are_not_finite_under_a_window_over_the_whole_track(bad, open_begin, hop):
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((12, 4)), rng.standard_normal((9, 4))
    a[5] = bad
    got = awr.follow(a, b, 0, 4, open_begin, 9, 2, hop)
    _same(got, asr.follow(a, b, 0, 4, open_begin))
    assert np.isnan(got[0][5:]).all() and (got[1][6:] == np.inf).all()


@pytest.mark.parametrize("cuts", [[1] * 30, [30], [7, 0, 23], [29, 1], [1, 29], [10, 10, 10]])
def test_the_result_does_not_depend_on_the_pushes(cuts):
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((30, 5)), rng.standard_normal((17, 5))
    for open_begin in (False, True):
        for width, back, hop, mono in ((6, 2, 1, False), (6, 2, 4, True), (9, 0, 7, False), (17, 16, 64, True), (3, 1, 3, False)):
            want = awr.follow(a, b, 1, 5, open_begin, width, back, hop, mono)
            _same(awr.follow(a, b, 1, 5, open_begin, width, back, hop, mono, cuts), want, (width, back, hop, mono))


def test_the_windows_start_never_falls_and_follows_the_position():
    moved = 0
    for seed in range(6):
        rng = np.random.default_rng(40 + seed)
        a, b = rng.standard_normal((60, 4)), rng.standard_normal((50, 4))
        for open_begin in (False, True):
            for width, back, hop, mono in ((8, 3, 1, False), (8, 3, 5, False), (12, 0, 2, True), (5, 4, 1, True)):
                los = []
                pos, _ = awr.follow(a, b, 0, 4, open_begin, width, back, hop, mono, los=los)
                assert len(los) == 60 and los[0] == 0 and (np.diff(los) >= 0).all() and max(los) <= 50 - width
                for i in range(1, 60):
                    if i % hop:
                        assert los[i] == los[i - 1]
                    elif not np.isnan(pos[i - 1]):
                        assert los[i] == min(max(los[i - 1], int(pos[i - 1]) - back), 50 - width)
                moved += los[-1] > 0
    assert moved > 0


def test_the_monotone_position_never_falls():
    fell = 0
    for seed in range(8):
        rng = np.random.default_rng(60 + seed)
        a, b = rng.standard_normal((50, 4)), rng.standard_normal((40, 4))
        a[31 + seed] = np.nan if seed == 7 else a[31 + seed]
        for open_begin in (False, True):
            for width, back, hop in ((10, 4, 1), (10, 4, 6), (40, 39, 64), (16, 0, 3)):
                plain = awr.follow(a, b, 0, 4, open_begin, width, back, hop)
                mono = awr.follow(a, b, 0, 4, open_begin, width, back, hop, True)
                p = mono[0][~np.isnan(mono[0])]
                assert (np.diff(p) >= 0).all()
                q = plain[0][~np.isnan(plain[0])]
                if (np.diff(q) >= 0).all():
                    _same(mono, plain, (seed, width, back, hop))
                else:
                    fell += 1
                    assert mono[0].tobytes() != plain[0].tobytes()
    assert fell > 0


@pytest.mark.parametrize("s", range(20))
def test_where_the_position_is_monotone_anyway_the_flag_changes_nothing(s):
    voice, track, _ = followable(s)
    for width, back, hop in FOLLOW_WINDOWS:
        plain = awr.follow(voice, track, 0, 8, False, width, back, hop)
        assert (np.diff(plain[0]) >= 0).all()
        _same(awr.follow(voice, track, 0, 8, False, width, back, hop, True), plain, (width, back, hop))


@pytest.mark.parametrize("width,back,hop", FOLLOW_WINDOWS)
@pytest.mark.parametrize("s", range(20))
def test_a_followable_voice_gives_the_unwindowed_stream(s, width, back, hop):
    voice, track, want = followable(s)
    assert not np.isnan(want[0]).any() and (np.diff(want[0]) >= 0).all()
    _same(awr.follow(voice, track, 0, 8, False, width, back, hop), want)
