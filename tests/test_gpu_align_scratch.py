"""-m gpu: extended feature alignment where a leftover in the scratch could stand in for a cell a kernel failed to write.  d, D and
the choices live in the device's alignment scratch, which survives from call to call, so every comparison here runs behind a
call on the same lengths and settings with every feature NaN (tests/align_checks.py: poison_scratch).  Behind that poison: the
cost pass's tile planner at skewed shapes under a band (n of 1 to 3, n >> m, m >> n) under both step patterns, and 300 small pairs
in one batch (the bisection over the tile offsets, odd offsets everywhere).  Everything is held against the rule
(tests/align_ex_rule.py) bit for bit and against the device's own outputs (check_alignment_outputs)."""
import numpy as np
import pytest

import align_checks as ac
import align_ex_rule as ax
from test_gpu_align_ex import _random_batch, env  # noqa: F401 (env is the module's fixture)

pytestmark = pytest.mark.gpu
SKEWED = [(2, 300), (3, 500), (300, 2), (500, 3), (33, 1000), (1000, 33), (1, 700), (700, 1)]
MANY, MANY_SEED = 300, 20291
_made, _rules = {}, {}


def _many_shapes():
    rng = np.random.default_rng(MANY_SEED)
    return [(int(n), int(m)) for n, m in rng.integers(1, 13, (MANY, 2))]


def _batch(name):
    """a ragged batch of random rows at dims = 60, made once and left unchanged"""
    if name not in _made:
        shapes, seed = (SKEWED, 20290) if name == "skewed" else (_many_shapes(), MANY_SEED + 1)
        _made[name] = _random_batch(shapes, 60, seed)
    return _made[name]


def _rule(name, band, pattern, flags):
    key = (name, band, pattern, flags)
    if key not in _rules:
        a_lens, fa, b_lens, fb = _batch(name)
        _rules[key] = ax.align_batch(a_lens, fa, b_lens, fb, 1, 60, band, pattern, flags)
    return _rules[key]


@pytest.mark.parametrize("band", [1, 2, 40])
def test_skewed_shapes_under_a_band_pattern_0(env, band):
    want = _rule("skewed", band, 0, 0)
    ac.checked_align(env, _batch("skewed"), 60, (1, 60), band, 0, 0, want)
    assert all(np.isfinite(r["cost"]) for r in want)


@pytest.mark.parametrize("band", [1, 2, 40])
def test_skewed_shapes_under_a_band_pattern_1(env, band):
    """the slope limit makes these pairs infeasible (max - 1 > 2 * (min - 1) in all eight): the cost pass and the accumulation run as
    under pattern 0, and inf, K = 0, NaN maps and span (-1, -1) must come out for exactly the pairs the rule names"""
    want = _rule("skewed", band, 1, 0)
    got = ac.checked_align(env, _batch("skewed"), 60, (1, 60), band, 1, 0, want)
    for u, ((n, m), r) in enumerate(zip(SKEWED, want)):
        assert max(n, m) - 1 > 2 * (min(n, m) - 1) and r["cost"] == np.inf, (n, m)
        assert got[0][u] == np.inf and got[1][u] == 0 and got[5][2 * u:2 * u + 2].tolist() == [-1, -1]
        assert np.isnan(ac.split_outputs(got, *_batch("skewed")[0::2])[u]["b_on_a"]).all()


def test_skewed_shapes_behind_a_poison_call_of_a_larger_batch(env):
    """the poison call carries one more pair in front, so the scratch is larger than the checked call needs and every offset
    of the checked call's layout falls elsewhere in it"""
    import test_gpu_align_ex as tx
    a_lens, fa, b_lens, fb = _batch("skewed")
    big_a, big_b = [37] + a_lens, [53] + b_lens
    for pattern in (0, 1):
        ac.poison_scratch(env, big_a, big_b, 60, (1, 60), 2, pattern, 0)
        got = tx._align(env, a_lens, fa, b_lens, fb, 60, 1, 60, 2, pattern, 0)
        ac.check_batch(a_lens, fa, b_lens, fb, (1, 60), 2, pattern, 0, got)
        tx._assert_equals_rule(got, _rule("skewed", 2, pattern, 0), a_lens, b_lens)


@pytest.mark.parametrize("pattern,band,flags", [(0, 0, 0), (0, 2, 0), (1, 0, 0), (1, 2, 0), (1, 0, 3), (0, 0, 3)])
def test_many_small_pairs_in_one_batch(env, pattern, band, flags):
    want = _rule("many", band, pattern, flags)
    ac.checked_align(env, _batch("many"), 60, (1, 60), band, pattern, flags, want)
    finite = sum(bool(np.isfinite(r["cost"])) for r in want)
    if pattern == 1:  # feasible and infeasible pairs lie side by side
        assert finite >= MANY // 3 and MANY - finite >= MANY // 10, finite
    else:
        assert finite == MANY
