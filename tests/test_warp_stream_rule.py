"""CPU tests of the warp stream's rule (include/world_class_warp_stream.h): wc_warp_stream_committed is the predicate, counted by
brute force; an output below c(E) is the same on every map that shares its first E entries, through the library's own
wc_warp_map_positions; and the rule model (tests/warp_stream_rule.py) gives the whole map's positions for every cut into pushes, at
every delay, with and without the flush."""
import math

import numpy as np
import pytest

import warp_rule as W
import warp_stream_rule as S
from test_warp_rule import MAPS
from world_class_amd import WorldClassError, warp, warp_stream as ws

OPES = [240.0, 220.5, 110.25, 80.0, 7.1, 1.0, 1.0 / 3.0, 0.3, 1e-3]


@pytest.mark.parametrize("ope", OPES)
def test_committed_is_the_predicate_by_brute_force(ope):
    """c(E) for E in 0 .. 600: the first n that fails the predicate, every n tried (c does not fall as E grows, so the walk goes on
    where the last one stopped)"""
    assert ws.committed(0, ope) == S.committed(0, ope) == 0
    n = 0
    for entries in range(1, 601):
        while float(n) / ope <= float(entries - 1):
            n += 1
        assert ws.committed(entries, ope) == n == S.committed(entries, ope)
        if n != warp.map_out_length(entries, ope):
            print("c(%d) = %d at out_per_entry %r, wc_warp_map_out_length gives %d" % (entries, n, ope, warp.map_out_length(entries, ope)))
    for entries in (1, 2, 7, 600):
        assert S.committed_by_brute_force(entries, ope) == ws.committed(entries, ope)


def test_committed_refusals_and_large_counts():
    L = ws._L()
    for entries, ope in ((-1, 240.0), (5, 0.0), (5, -1.0), (5, math.nan), (5, math.inf), (2 ** 40, 2.0 ** 40)):
        assert L.wc_warp_stream_committed(entries, ope) < 0
        with pytest.raises(WorldClassError):
            ws.committed(entries, ope)
    assert ws.committed(2 ** 40 + 1, 240.0) == 2 ** 40 * 240 + 1   # (a stream's counters are 64-bit)
    assert ws.committed(2 ** 31 + 1, 0.5) == 2 ** 30 + 1


@pytest.mark.parametrize("name", ["long", "nan_entry", "falling", "range_ends"])
def test_an_output_below_the_committed_count_is_the_same_on_every_longer_map(name):
    m, ope, ipu = MAPS[name]
    whole = warp.map_positions(m, ope, ipu, ws.committed(len(m), ope))
    for entries in range(1, len(m) + 1):
        upto = ws.committed(entries, ope)
        assert upto <= len(whole)
        assert np.array_equal(warp.map_positions(m[:entries], ope, ipu, upto), whole[:upto])
    assert ws.committed(len(m), ope) == warp.map_out_length(len(m), ope)


def test_the_prefix_property_at_the_pairs_of_the_header():
    rng = np.random.default_rng(11)
    m = np.cumsum(rng.choice([0.0, 0.5, 1.0, 2.0], size=12)) + 3.0
    m[5] = math.nan
    m[8] = m[7] - 2.5   # a falling entry
    for ope, ipu in ((240.0, 220.5), (220.5, 240.0), (7.1, 3.3), (0.3, 5.0)):
        whole = W.map_positions(m, ope, ipu, S.committed(len(m), ope))
        for entries in range(1, len(m) + 1):
            upto = S.committed(entries, ope)
            assert W.map_positions(m[:entries], ope, ipu, upto) == whole[:upto]
            assert [int(p) for p in warp.map_positions(m[:entries], ope, ipu, upto)] == whole[:upto]


def cuts(n):
    """all at once; one row per push; pushes of 0, 1, 2, 3, ... rows"""
    growing, k = [], 0
    while sum(growing) < n:
        growing.append(min(k, n - sum(growing)))
        k += 1
    return {"at_once": [n], "one_each": [1] * n, "growing": growing}


def test_the_split_of_a_push():
    assert S.push_split(0, 5, 0) == (0, 5) and S.push_split(0, 2, 3) == (2, 0) and S.push_split(2, 4, 3) == (1, 3)
    assert S.push_split(3, 4, 3) == (0, 4) and S.push_split(7, 0, 3) == (0, 0) and S.push_split(1, 1, 3) == (1, 0)
    assert S.flush_split(2, 3) == (2, 2) and S.flush_split(3, 3) == (3, 3) and S.flush_split(9, 3) == (4, 3) and S.flush_split(9, 1) == (2, 1)
    for delay in (0, 1, 3):
        for rows in range(1, 9):
            for sizes in cuts(rows).values():   # however the rows are cut, all but the first `delay` become entries
                got, before = 0, 0
                for k in sizes:
                    unread, consumed = S.push_split(before, k, delay)
                    assert unread + consumed == k and unread == min(k, max(delay - before, 0))
                    got += consumed
                    before += k
                assert before == rows and got == max(rows - delay, 0)


@pytest.mark.parametrize("delay", [0, 1, 3])
@pytest.mark.parametrize("name", ["nan_entry", "b_on_a_220_5", "falling"])
def test_every_cut_gives_the_whole_maps_positions(name, delay):
    m, ope, ipu = MAPS[name]
    rows, tail = S.settled_rows(m, delay)
    assert len(rows) == len(m)
    for flush in (False, True):
        if flush and delay == 0:
            continue
        consumed = len(m) if flush else max(len(m) - delay, 0)
        want = W.map_positions(m[:consumed], ope, ipu, S.committed(consumed, ope)) if consumed else []
        for cut, sizes in cuts(len(rows)).items():
            s = S.Stream(delay, ope, ipu)
            got, at, per_push = [], 0, []
            for k in sizes:
                before = s.done
                got += s.push(rows[at:at + k])
                per_push.append(s.done - before)
                at += k
            assert at == len(rows) and len(s.entries) == max(len(m) - delay, 0)
            if flush:
                got += s.flush(tail)
            assert got == want, (cut, flush)
            assert s.done == len(want) == S.committed(consumed, ope)
            # a push that ends inside the first `delay` rows forms nothing
            seen = 0
            for k, n_out in zip(sizes, per_push):
                seen += k
                assert seen > delay or n_out == 0
    assert -777.0 not in [float(v) for v in m]
