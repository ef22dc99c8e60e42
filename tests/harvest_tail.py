"""Candidate tables for Harvest's tail (removal of unreliable candidates, contour fixing, smoothing, output), written by hand
so that every decision of that logic is met at its edge: exact ties, thresholds met exactly, more voiced sections than audio
has.  numpy only; every builder is deterministic and returns (x_lengths, cand, score): the sample counts of the utterances at
16 kHz and the refined candidate / score rows [1 ms frames of the batch, utterance after utterance][nc].

tests/test_harvest_tail_rule.py proves on the CPU, from the oracle's trace, that each table reaches the path it is named for;
tests/test_gpu_harvest_tail.py then compares the device with the oracle on the same tables.

Facts the tables rely on (reference src/harvest.cpp):
 * a candidate with score 0 never becomes f0_base (searchF0Base asks for score > 0) but is seen by the extension walks,
   so a "track" of score-0 candidates around a scored "run" is what extendF0 follows;
 * fixStep1 drops the first frame of every run of f0_base (its predecessors are 0), so a run on frames a .. b leaves the
   voiced section a+1 .. b, and the walk back from a+1 finds the run's own candidate on frame a again;
 * values are small integers (or one ulp beside them), so the relative errors 5/100, 18/100 and 1/125 round to the literals
   0.05, 0.18 and 0.008 on both sides.
"""
import numpy as np

FS = 16000
F0_FLOOR, F0_CEIL = 71.0, 800.0
NC = {40.0: 105, 80.0: 210}  # row width 7 S by channels_in_octave at the default floor and ceiling


def x_length(L1):
    """a sample count whose 1 ms frame count at 16 kHz is L1"""
    return (L1 - 1) * 16


def frames_1ms(n):
    return int(1000.0 * n / FS) + 1


class Rows:
    def __init__(self, L, nc):
        self.L, self.nc = L, nc
        self.cand = np.zeros((L, nc))
        self.score = np.zeros((L, nc))

    def put(self, frames, slot, f, score=0.0):
        frames = [frames] if np.isscalar(frames) else list(frames)
        f = np.broadcast_to(np.asarray(f, dtype=np.float64), (len(frames),))
        for i, v in zip(frames, f):
            assert 0 <= i < self.L and 0 <= slot < self.nc and self.cand[i, slot] == 0.0, (i, slot)
            assert F0_FLOOR <= v <= F0_CEIL
            self.cand[i, slot] = v
            self.score[i, slot] = score

    def run(self, first, last, slot, f, score=1.0):
        """scored candidates on frames first .. last: f0_base follows them; fixStep1 leaves the section first+1 .. last"""
        self.put(range(first, last + 1), slot, f, score)

    def table(self):
        return [x_length(self.L)], self.cand, self.score


def batch(*tables):
    return (sum((t[0] for t in tables), []), np.concatenate([t[1] for t in tables]), np.concatenate([t[2] for t in tables]))


def split(x_lengths, cand, score):
    """the utterances of a batch: [(x_length, cand, score)]"""
    out, at = [], 0
    for n in x_lengths:
        L = frames_1ms(n)
        out.append((n, cand[at:at + L], score[at:at + L]))
        at += L
    return out


def up(v):
    return float(np.nextafter(v, np.inf))


def down(v):
    return float(np.nextafter(v, -np.inf))


# ------------------------------------------------------------------------------------------------------------------------
# removal of unreliable candidates and f0_base
# ------------------------------------------------------------------------------------------------------------------------
REMOVAL_L = 85


def _removal(nc):
    r = Rows(REMOVAL_L, nc)
    L = r.L
    marks = {}  # kind -> [(frame, slot, kept)]
    base = {}   # frame -> f0_base expected there

    def mark(kind, frame, slot, kept):
        marks.setdefault(kind, []).append((frame, slot, kept))
    # support in frame 0 only / in frame L-1 only: the comparison copy never holds those rows
    r.put(0, 2, 100.0, 1.0); r.put(1, 2, 100.0, 1.0)
    mark("frame_0_only", 1, 2, False)
    r.put(L - 2, 2, 100.0, 1.0); r.put(L - 1, 2, 100.0, 1.0)
    mark("frame_last_only", L - 2, 2, False)
    # supporters across the edges of the kernel's 8-frame blocks: 7|8, 8|9
    r.put(7, 1, 200.0, 1.0); r.put(8, 6, 200.0, 1.0); r.put(8, 2, 300.0, 1.0); r.put(9, 7, 300.0, 1.0)
    for fr, sl in ((7, 1), (8, 6), (8, 2), (9, 7)):
        mark("block_edge", fr, sl, True)
    # exactly 5 %, from the next frame and from the previous one
    r.put(11, 3, 100.0, 1.0); r.put(12, 5, 105.0, 1.0)
    mark("at_5_percent_next_only", 11, 3, True)
    r.put(14, 0, 95.0, 1.0); r.put(15, 4, 100.0, 1.0)
    mark("at_5_percent_prev_only", 15, 4, True)
    mark("beyond_5_percent", 14, 0, False)  # 5 / 95
    # one ulp beyond
    r.put(18, 3, 100.0, 1.0); r.put(19, 5, up(105.0), 1.0)
    mark("one_ulp_beyond_next", 18, 3, False)
    r.put(21, 0, down(95.0), 1.0); r.put(22, 4, 100.0, 1.0)
    mark("one_ulp_beyond_prev", 22, 4, False)
    # live slots at 64 and above, at 128 and above
    r.put(26, 70, 250.0, 1.0); r.put(27, 100, 250.0, 1.0); r.put(26, 90, 600.0, 1.0)
    mark("slot_64_up", 26, 70, True); mark("slot_64_up", 27, 100, True); mark("slot_64_up", 26, 90, False)
    if nc > 128:
        r.put(26, 130, 350.0, 1.0); r.put(27, 205, 350.0, 1.0); r.put(27, 140, 700.0, 1.0)
        mark("slot_128_up", 26, 130, True); mark("slot_128_up", 27, 205, True); mark("slot_128_up", 27, 140, False)
    # a row with every slot live, supported only at its low end
    for k in range(nc):
        r.put(30, k, 72.0 + 3 * k, 1.0)
    for k in range(40):
        r.put(31, k, 72.0 + 3 * k, 1.0)
    # f0_base: equal top scores in two slots, the lower slot wins: j | j+32 and j | j+64 (one lane of the kernel), 5 | 9 (two lanes)
    for fr, (sa, fa), (sb, fb), sc in ((35, (2, 100.0), (34, 300.0), 5.0), (39, (3, 310.0), (67, 110.0), 7.0), (43, (5, 120.0), (9, 400.0), 3.0)):
        r.put(fr, sa, fa, sc); r.put(fr, sb, fb, sc)
        r.put(fr + 1, 0, fa, 1.0); r.put(fr + 1, 1, fb, 1.0)
        base[fr] = fa
        mark("base_tie", fr, sa, True); mark("base_tie", fr, sb, True)
    # ... and the top score belongs to a candidate that is removed
    r.put(47, 1, 500.0, 9.0); r.put(47, 8, 130.0, 2.0); r.put(48, 8, 130.0, 1.0)
    base[47] = 130.0
    mark("top_score_removed", 47, 1, False)
    # the last, partial block
    r.put(80, 4, 150.0, 1.0); r.put(81, 4, 150.0, 1.0)
    mark("partial_block", 80, 4, True); mark("partial_block", 81, 4, True)
    return r, marks, base


def removal(nc):
    return _removal(nc)[0].table()


def removal_marks(nc):
    """({kind: [(frame, slot, kept)]}, {frame: expected f0_base}); frame 30 is the row with every slot live"""
    return _removal(nc)[1:]


# ------------------------------------------------------------------------------------------------------------------------
# selectBestF0 in the extension walks: ties and the 0.18 threshold
# ------------------------------------------------------------------------------------------------------------------------
def _ties(nc):
    units = [(200.0, (5, 180.0), (9, 220.0), +1), (200.0, (5, 220.0), (9, 180.0), +1), (200.0, (9, 180.0), (5, 220.0), -1),
             (200.0, (7, 180.0), (71, 220.0), -1), (200.0, (7, 220.0), (71, 180.0), +1), (200.0, (40, 220.0), (104, 180.0), -1)]
    if nc > 128:
        units += [(200.0, (3, 180.0), (131, 220.0), +1), (200.0, (3, 220.0), (131, 180.0), -1), (200.0, (70, 180.0), (198, 220.0), -1),
                  (200.0, (140, 220.0), (150, 180.0), +1), (200.0, (209, 180.0), (130, 220.0), +1)]
    thresholds = [(118.0, +1, True), (up(118.0), +1, False), (82.0, -1, True), (down(82.0), -1, False)]
    P = 50
    r = Rows(P * (len(units) + len(thresholds)) + 20, nc)
    chosen, moves = [], []  # (frame, value the walk takes there); (section, direction, frames moved)
    for u, (ref, (sa, fa), (sb, fb), d) in enumerate(units):
        a = 10 + P * u
        r.run(a, a + 29, 0, ref)  # the section a+1 .. a+29; the walk back starts by taking frame a
        f1, f2 = (a + 30, a + 31) if d > 0 else (a - 1, a - 2)
        for fr in (f1, f2):  # (two frames: each candidate is kept by its twin next door)
            r.put(fr, sa, fa); r.put(fr, sb, fb)
        later = fa if sa > sb else fb
        chosen += [(f1, later), (f2, later)]
        moves.append((u, d, 2 if d > 0 else 3))
    for t, (f, d, ok) in enumerate(thresholds):
        u = len(units) + t
        a = 10 + P * u
        r.run(a, a + 29, 0, 100.0)
        f1, f2 = (a + 30, a + 31) if d > 0 else (a - 1, a - 2)
        r.put(f1, 4, f); r.put(f2, 4, f)
        if ok:
            chosen += [(f1, f), (f2, f)]
        moves.append((u, d, (2 if ok else 0) + (1 if d < 0 else 0)))
    return r, chosen, moves


def ties(nc):
    return _ties(nc)[0].table()


def ties_marks(nc):
    """([(frame, value chosen by the walk)], [(section, direction, frames its boundary moves)])"""
    return _ties(nc)[1:]


# ------------------------------------------------------------------------------------------------------------------------
# shapes of the walks
# ------------------------------------------------------------------------------------------------------------------------
WALKS_L = (700, 260)
# utterance 0, by section: (first, last) before and after the walks
WALKS_EXPECT_0 = [((2, 8), (0, 8)), ((251, 280), (150, 381)), ((451, 480), (450, 487)), ((521, 550), (520, 552)),
                  ((601, 630), (601, 630)), ((692, 698), (691, 699))]
WALKS_EXPECT_1 = [((41, 70), (0, 70)), ((191, 220), (190, 259))]


def walks(nc=105):
    L = WALKS_L[0]
    r = Rows(L, nc)
    r.put(0, 1, 300.0); r.run(1, 8, 1, 300.0)              # the first section fixStep1 can leave, 2 .. 8; back: clamped at 1 / 0
    r.put(range(100, 250), 2, 150.0); r.run(250, 280, 2, 150.0); r.put(range(281, 421), 2, 150.0)  # 101 frames each way
    r.run(450, 480, 3, 200.0); r.put((481, 482, 486, 487), 3, 200.0)   # three misses, then a hit: the walk goes on
    r.run(520, 550, 3, 200.0); r.put((551, 552, 557, 558), 3, 200.0)   # four misses: it stops
    # no move at all, either way: f0_base rises 100, 150, 200 on frames 599 .. 601, so fixStep1 keeps frame 601 by its linear
    # prediction and drops the two in front of it, and what lies in front of the section is more than 18 % away
    r.put(598, 4, 100.0); r.put(599, 4, 100.0, 1.0); r.put(599, 5, 150.0); r.put(600, 5, 150.0, 1.0)
    r.run(601, 630, 4, 200.0)
    r.run(L - 9, L - 2, 1, 300.0); r.put(L - 1, 1, 300.0)  # the last section, L-8 .. L-2; forward: clamped at L-2 / L-1
    t0 = r.table()
    L = WALKS_L[1]
    r = Rows(L, nc)
    r.put(range(0, 40), 6, 250.0); r.run(40, 70, 6, 250.0)              # 41 frames back to frame 0
    r.run(190, 220, 6, 250.0); r.put(range(221, L), 6, 250.0)          # 39 frames forward to frame L-1
    return batch(t0, r.table())


# ------------------------------------------------------------------------------------------------------------------------
# fixStep1, fixStep2 and the section lists
# ------------------------------------------------------------------------------------------------------------------------
STEPS_EDGE_FRAMES = (63, 64, 65, 255, 256, 257)
# five short utterances: sections (first, last) after fixStep1 that put every edge frame once first and once last
STEPS_EDGE_SECTIONS = [[(50, 63), (65, 80), (240, 255), (257, 270)], [(50, 64), (256, 270)], [(64, 80), (240, 256)],
                       [(50, 65), (255, 270)], [(63, 80), (240, 257)]]
STEPS_L = 340


def steps(nc=105):
    r = Rows(STEPS_L, nc)
    r.run(10, 19, 0, 125.0); r.run(20, 29, 0, 126.0)          # 1 / 125 = 0.008: kept, one section 11 .. 29
    r.run(40, 49, 0, 125.0); r.run(50, 59, 0, up(126.0))      # one ulp beyond: frame 50 dropped, sections 41 .. 49 and 51 .. 59
    r.run(70, 76, 0, 150.0)                                   # section 71 .. 76, ed - st = 5: cleared
    r.run(90, 97, 0, 150.0)                                   # section 91 .. 97, ed - st = 6: kept
    for k in range(70):                                       # 70 sections of two frames: more than one round of lanes to clear
        r.run(110 + 3 * k, 112 + 3 * k, 1, 300.0 if k % 2 == 0 else 400.0)
    tabs = [r.table()]
    for secs in STEPS_EDGE_SECTIONS:
        r = Rows(300, nc)
        for k, (st, ed) in enumerate(secs):
            r.run(st - 1, ed, 0, 200.0 if k % 2 == 0 else 300.0)
        tabs.append(r.table())
    return batch(*tabs)


# ------------------------------------------------------------------------------------------------------------------------
# many sections
# ------------------------------------------------------------------------------------------------------------------------
MANY_L = 1200
MANY_PERIOD = {49: 24, 97: 12, 148: 8}
MANY_LOW = (70, 80, 131, 141)  # sections (where there are that many) below 2200 / (ed - st) Hz


def many(n, nc=105):
    """n runs of eight frames, alternately 400 and 500 Hz: sections of seven frames.  Every section can be extended by the frame
    in front of it and by at least one frame behind it, so that every walk of the extension phase leaves a mark.  At n = 148 the
    runs touch: sections of seven frames, one frame between them -- as many as fit, the worst case of the channel storage.
    A few sections past the 64th (and past the 128th) are too low for their length, unlike the ones 64 places before them: extendSub
    must look at their own boundaries and values to drop them."""
    P = MANY_PERIOD[n]
    r = Rows(MANY_L, nc)
    for k in range(n):
        a = 4 + P * k
        f = 400.0 if k % 2 == 0 else 500.0
        if k in MANY_LOW:
            f = 120.0 + (k % 3) * 15
        r.run(a, a + 7, 10 + (k % 3) * 40, f)
        r.put(a + 8, 11 + (k % 3) * 40, f)
        if P > 8:
            r.put(a + 9, 11 + (k % 3) * 40, f)
    return r.table()


def channel_capacity(L1):
    """doubles of channel storage an utterance alone in its call has (wc_harvest.hip, hv_enqueue)"""
    return L1 + 209 * (L1 // 8 + 2) + 64


# ------------------------------------------------------------------------------------------------------------------------
# extendSub
# ------------------------------------------------------------------------------------------------------------------------
def _wobble(n):
    return 100.0 + (np.arange(n) * 37 % 11) / 70.0  # within fixStep1's 0.8 %; the sums of these are not exact


def extendsub(nc=105):
    # utterance 0: 100 Hz sections whose ed - st is on both sides of 2200 / mean; the mean is carried from section to section
    r = Rows(520, nc)
    a = 10
    for n in (23, 23, 24, 22, 16):  # ed - st = n - 1 once the walk back has taken the run's first frame
        r.run(a, a + n - 1, 0, 100.0)
        a += n + 20
    for n in (71, 141):             # sums over more than 64 and more than 128 frames
        r.run(a, a + n - 1, 0, _wobble(n))
        a += n + 20
    t0 = r.table()
    # utterance 1: no section is long enough (count == 0); the row at position 0 is still copied
    r = Rows(120, nc)
    r.run(10, 25, 0, 100.0); r.run(60, 75, 0, 100.0)
    t1 = r.table()
    # utterance 2: the first section that is kept does not start first: a later one extends back past it
    r = Rows(300, nc)
    r.run(50, 57, 0, 400.0)
    r.put(range(30, 140), 1, 100.0); r.run(140, 180, 1, 100.0)
    r.run(240, 270, 1, 100.0)
    return batch(t0, t1, r.table())


def py_walk(cand, row, origin, last_point, shift, allowed=0.18):
    """extendF0 (reference src/harvest.cpp:371-403) in plain Python, on the full-length row of one section"""
    tmp, shifted, miss = row[origin], origin, 0
    for i in range(abs(last_point - origin) + 1):
        idx = origin + shift * i + shift
        best, best_err = 0.0, allowed
        for c in cand[idx]:
            t = abs(tmp - c) / tmp
            if t > best_err:
                continue
            best, best_err = c, t
        row[idx] = best
        if best == 0.0:
            miss += 1
        else:
            tmp, miss, shifted = best, 0, idx
        if miss == 4:
            break
    return shifted


def py_extendsub(cand, s2, sections, reset):
    """extend and extendSub (reference :427-458) in plain Python: the sections' boundaries after the walks and which of them are kept;
    reset=True is the variant that starts every section's mean at zero"""
    L = len(s2)
    kept, bounds, mean = [], [], 0.0
    rows = []
    for st, ed in sections:
        row = np.zeros(L)
        row[st:ed + 1] = s2[st:ed + 1]
        ed2 = py_walk(cand, row, ed, min(L - 2, ed + 100), 1)
        st2 = py_walk(cand, row, st, max(1, st - 100), -1)
        rows.append(row)
        bounds.append((st2, ed2))
    for (st, ed), row in zip(bounds, rows):
        if reset:
            mean = 0.0
        for j in range(st, ed):
            mean += row[j]
        mean /= ed - st
        kept.append(2200.0 / mean < ed - st)
    return bounds, kept


# ------------------------------------------------------------------------------------------------------------------------
# mergeF0
# ------------------------------------------------------------------------------------------------------------------------
def merge(nc=105):
    """Two tracks, 100 Hz (slot 2) from frame 3 and 160 Hz (slot 7) from frame 5, that go on side by side; the scores decide which of
    them f0_base follows, in runs of eleven frames.  Every section extends along its own track, up to 101 frames each way, across the
    other track's sections: the sections of the first hundred frames all reach back to where their track begins."""
    L = 420
    r = Rows(L, nc)
    sa, sb = np.zeros(L), np.zeros(L)
    for k in range(24):  # 24 runs, alternately on the two tracks, a frame without scores between them
        a = 10 + 12 * k
        (sa if k % 2 == 0 else sb)[a:a + 11] = 2.0
        (sb if k % 2 == 0 else sa)[a:a + 11] = 1.0 if k % 4 < 2 else 0.0
    sa[300:] = 0.0; sb[300:] = 0.0
    for i in range(3, 311):
        r.put(i, 2, 100.0, sa[i])
    for i in range(5, 300):
        r.put(i, 7, 160.0, sb[i])
    r.run(305, 330, 9, 250.0, 3.0)  # begins where it is scored and outlasts the tracks: it scores higher where it meets them (s1 < s2)
    r.run(350, 380, 2, 100.0)       # far from the others: disjoint
    t0 = r.table()
    # both sums zero: a 100 Hz section whose walk ends on score-0 frames that a 160 Hz section's walk back reaches too
    r = Rows(200, nc)
    r.run(50, 90, 2, 100.0); r.put(range(91, 101), 2, 100.0)
    r.put(range(96, 106), 7, 160.0); r.run(106, 140, 7, 160.0)
    return batch(t0, r.table())


# ------------------------------------------------------------------------------------------------------------------------
# fixStep4 and the output
# ------------------------------------------------------------------------------------------------------------------------
def step4_small(nc=105):
    """gaps of 8 (filled) and 9 (left) between sections of different F0; the first section reaches frame 0 and the last one
    frame L-1 through their walks"""
    L = 400
    r = Rows(L, nc)
    r.put(range(0, 8), 0, 150.0); r.run(8, 40, 0, 150.0)
    r.run(49, 80, 1, 190.0)     # frames 41 .. 48 between: 8
    r.run(90, 120, 0, 150.0)    # 81 .. 89: 9
    r.run(129, 160, 1, 115.0)   # 121 .. 128: 8
    r.run(170, 200, 0, 150.0)   # 161 .. 169: 9
    r.run(340, 380, 1, 240.0); r.put(range(381, L), 1, 240.0)
    return r.table()


def step4_many(gap, nc=105):
    """70 sections of eight frames with `gap` frames between them: 69 gaps, all of them filled (8) or all left (9 -- and then the
    smoothing sees 70 sections, more than one round of lanes)"""
    r = Rows(MANY_L, nc)
    for k in range(70):
        a = 4 + (8 + gap) * k
        r.run(a, a + 7, 3, 400.0 + 8 * (k % 5))
    return r.table()


def tiny(nc=105):
    """the shortest utterance Harvest accepts: three frames"""
    r = Rows(3, nc)
    r.put(0, 0, 100.0, 1.0); r.put(1, 0, 100.0, 1.0); r.put(1, 1, 300.0, 2.0); r.put(2, 1, 300.0, 1.0)
    return r.table()


def short37(nc=105):
    r = Rows(37, nc)
    r.put(range(0, 5), 3, 200.0); r.run(5, 30, 3, 200.0); r.put(range(31, 37), 3, 200.0)
    return r.table()


def three_sections(nc=105):
    """three sections at a smaller L1 than the many-section tables (the stale-scratch test)"""
    r = Rows(500, nc)
    r.run(40, 90, 0, 120.0); r.put(range(91, 110), 0, 120.0)
    r.run(200, 260, 1, 180.0)
    r.put(range(380, 400), 2, 240.0); r.run(400, 450, 2, 240.0)
    return r.table()


# ------------------------------------------------------------------------------------------------------------------------
# the tables by name, with the channels_in_octave that gives their row width, and the oracle's result for them
# ------------------------------------------------------------------------------------------------------------------------
TABLES = {
    "removal_105": (lambda: removal(105), 40.0), "removal_210": (lambda: removal(210), 80.0),
    "ties_105": (lambda: ties(105), 40.0), "ties_210": (lambda: ties(210), 80.0),
    "walks": (walks, 40.0), "steps": (steps, 40.0),
    "many_49": (lambda: many(49), 40.0), "many_97": (lambda: many(97), 40.0), "many_148": (lambda: many(148), 40.0),
    "many_148_210": (lambda: many(148, 210), 80.0),
    "extendsub": (extendsub, 40.0), "merge": (merge, 40.0),
    "step4_small": (step4_small, 40.0), "step4_gap8": (lambda: step4_many(8), 40.0), "step4_gap9": (lambda: step4_many(9), 40.0),
    "tiny": (tiny, 40.0), "short37": (short37, 40.0), "three_sections": (three_sections, 40.0),
}
_built, _ref = {}, {}


def table(name):
    if name not in _built:
        _built[name] = TABLES[name][0]()
    return _built[name]


def reference(port, name, frame_period=5.0):
    """the oracle's tail on every utterance of the table, computed once per (table, frame period)"""
    key = (name, frame_period)
    if key not in _ref:
        _ref[key] = [port.harvest_tail(c, s, FS, n, frame_period) for n, c, s in split(*table(name))]
    return _ref[key]
