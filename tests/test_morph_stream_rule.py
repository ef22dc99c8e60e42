"""CPU tests of the morph streams' rule (tests/morph_stream_rule.py, the restatement of include/world_class_stream.h): lockstep
streams at speed 1, and the counts, totals and backlogs of the four cases the GPU tests drive -- so that their max_backlog = 16 and
max_frames = 12 are known to be enough for the rule alone."""
import math

import pytest

import morph_stream_rule as ms


def test_lockstep_pushes_at_speed_one_sit_at_whole_positions():
    s = ms.Stream()
    want = 0
    for n in (1, 3, 2, 5, 1, 1, 4):
        assert s.count(n, n, 12) == n
        pos = s.push(n, n)
        assert pos == [(float(k), float(k)) for k in range(want, want + n)]
        want += n
        assert s.backlog(0) == 1 and s.backlog(1) == 1 and s.position(0) == want - 1.0
    assert s.frames == want == 17 and s.F == [17, 17]


def test_a_stream_without_frames_reports_nothing():
    s = ms.Stream()
    assert s.push(0, 0) == [] and s.push(3, 0) == [] and not s.formed
    assert math.isnan(s.position(0)) and math.isnan(s.position(1)) and (s.backlog(0), s.backlog(1)) == (3, 0) and s.frames == 0


# (case, pushes, formed frames, largest backlog, most frames per push)
TABLE = [("a", 33, 65, 3, 2), ("b", 38, 107, 6, 5), ("c", 22, 61, 7, 6), ("d", 4, 12, 12, 4)]


@pytest.mark.parametrize("case,pushes,formed,backlog,most", TABLE)
def test_counts_totals_and_backlogs_of_the_cases(case, pushes, formed, backlog, most):
    out = ms.run(case)
    assert len(out) == pushes
    assert sum(len(p["pos"]) for p in out) == formed == out[-1]["formed"]
    assert max(max(p["backlog"]) for p in out) == backlog <= 16
    assert max(len(p["pos"]) for p in out) == most <= 12
    assert out[-1]["received"] == ms.CASES[case]["frames"]
    flat = [q for p in out for q in p["pos"]]
    assert flat[0] == (0.0, 0.0)
    for x in (0, 1):  # positions only move forward, and never past the rows received
        assert all(b[x] > a[x] for a, b in zip(flat, flat[1:]))
    for p in out:
        assert all(q[0] <= p["received"][0] - 1 and q[1] <= p["received"][1] - 1 for q in p["pos"])


def test_case_a_runs_both_voices_to_their_last_rows():
    flat = [q for p in ms.run("a") for q in p["pos"]]
    assert flat == [(0.5 * k, 1.5 * k) for k in range(65)] and flat[-1] == (32.0, 96.0)


def test_case_b_changes_its_speeds_at_push_fifteen():
    out = ms.run("b")
    assert [p["speeds"] for p in out[:15]] == [(1.37, 1.0)] * 15 and all(p["speeds"] == (0.73, 0.55) for p in out[15:])
    flat = [q for p in out for q in p["pos"]]
    steps = {(round(b[0] - a[0], 9), round(b[1] - a[1], 9)) for a, b in zip(flat, flat[1:])}
    assert steps == {(1.37, 1.0), (0.73, 0.55)}


def test_case_d_forms_nothing_until_the_other_voice_arrives():
    out = ms.run("d")
    assert [len(p["pos"]) for p in out] == [0, 4, 4, 4] and out[0]["backlog"] == (12, 0)
    assert [p["backlog"] for p in out[1:]] == [(9, 1), (5, 1), (1, 1)]


def test_case_c_goes_over_a_backlog_of_six():
    """With max_backlog = 6 case c is over the bound at the first push that gives A rows while a kept row waits: its third push.
    (Its very first push leaves exactly six rows of A, which the rule's `backlog > max_backlog` admits, and the second forms frames
    0 .. 5 and leaves one row of each voice; the third adds A's next six behind the kept one: seven.)"""
    out = ms.run("c", max_backlog=6)
    assert [None if p is None else p["backlog"] for p in out] == [(6, 0), (1, 1), None]
    assert ms.run("c")[2]["backlog"] == (7, 1)
    assert ms.run("c", max_backlog=7)[-1] is not None and len(ms.run("c", max_backlog=7)) == 22


def test_the_count_stops_at_its_limit():
    s = ms.Stream()
    s.speed = [1e-300, 1e-300]
    assert s.count(2, 2, 12) == 13 and s.F == [0, 0]
    s.speed = [1.0, 1.0]
    assert s.count(12, 12, 12) == 12 and s.count(13, 13, 12) == 13
