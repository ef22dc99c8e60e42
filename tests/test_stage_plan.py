"""The stage handles' host half (world_class_amd/csrc/wc_stage_plan.hpp: the batch layout, the draws of a stage per utterance, the
range of noise positions a call asks the draw table for) and the option readers (wc_options.hpp), compiled alone by the host
compiler -- once plain, once under the address and undefined-behaviour sanitizers -- and driven by tests/cpp/stage_plan_check.cpp.
Every line it prints is compared with the rule, restated below in Python's integers:

    layout   utterance u lies behind the utterances before it in each packed array a stage has; totals are sums; f_base is 0
    draws    CheapTrick (2 (N / 2) + 1 + N / 2 + 1) frames, D4C (2 int(3 fs / 40 / 2 + 1) + 1 + 3 (2 int(4 fs / 47 / 2 + 1) + 1)) frames,
             Synthesis one per output sample
    range    [min position, max position + draws) over the utterances that draw; one table while hi - lo <= 2^28
    options  is: equal to the word; off / on: first character '0' / '1'; int: atoll when set; set: present
"""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "world_class_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
RATES = (8000, 12000, 16000, 22050, 24000, 44100, 48000, 96000)
FFT_SIZES = (512, 1024, 2048, 4096)


@pytest.fixture(scope="module", params=sorted(BUILDS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_plan") / request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                   ["-o", exe, os.path.join(ROOT, "tests", "cpp", "stage_plan_check.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()

    return run


# ---- the layout ----
def layout_rule(mask, utts):
    """utts: (x_length, f0_length, out_length, position) per utterance; an array the mask leaves out counts as absent"""
    tot, out = [0, 0, 0], []
    for u in utts:
        lens = [u[k] if mask >> k & 1 else 0 for k in range(3)]
        offs = [tot[k] if mask >> k & 1 else 0 for k in range(3)]
        out.append(" | %d %d %d %d %d %d 0 %d" % (*offs, *lens, u[3] if mask & 8 else 0))
        tot = [t + n for t, n in zip(tot, lens)]
    return "%d %d %d" % tuple(tot) + "".join(out)


def layout_batches():
    rng = random.Random(5)
    batches = []
    for n in (1, 2, 7, 64):
        # CheapTrick / D4C: samples and frames, some utterances without frames; Synthesis: frames and output, some without output
        batches.append((1 | 2 | 8, [(rng.randrange(1, 500000), rng.choice([0, 0, rng.randrange(1, 3000)]), 0, rng.randrange(2 ** 40 + 1)) for _ in range(n)]))
        batches.append((2 | 4 | 8, [(0, rng.randrange(2, 3000), rng.choice([0, rng.randrange(1, 500000)]), rng.randrange(2 ** 40 + 1)) for _ in range(n)]))
        batches.append((1 | 2, [(rng.randrange(1, 500000), rng.randrange(0, 3000), 7, 11) for _ in range(n)]))  # no positions: all 0
        batches.append((1 | 2 | 4 | 8, [(rng.randrange(1, 500000), rng.randrange(2, 3000), rng.randrange(0, 500000), 2 ** 40) for _ in range(n)]))
    batches.append((1 | 2 | 8, [(1, 0, 0, 0)]))
    batches.append((2 | 4 | 8, [(0, 2, 0, 2 ** 40), (0, 2, 0, 0)]))
    batches.append((1 | 2 | 4 | 8, [(40000000, 8001, 40000000, 2 ** 40 - u) for u in range(64)]))  # the sample total passes 2^31
    return batches


def test_layout(program):
    batches = layout_batches()
    lines = ["layout %d %d " % (mask, len(utts)) + " ".join("%d %d %d %d" % u for u in utts) for mask, utts in batches]
    want = [layout_rule(mask, utts) for mask, utts in batches]
    assert want[-1].startswith("2560000000 512064 2560000000 | ") and " | 2520000000 504063 2520000000 40000000 8001 40000000 0 " in want[-1]
    got = program(lines)
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, (line[:200], g[:400], w[:400])


# ---- the draws of a stage per utterance ----
def ct_per_frame(fft_size):
    return 2 * (fft_size // 2) + 1 + fft_size // 2 + 1


def d4c_per_frame(fs):
    return 2 * int(3.0 * fs / 40.0 / 2.0 + 1.0) + 1 + 3 * (2 * int(4.0 * fs / 47.0 / 2.0 + 1.0) + 1)


def test_draw_counts(program):
    lengths = (-3, 0, 1, 2, 61, 2001, 2 ** 31 - 1)
    lines, want = [], []
    for n in FFT_SIZES:
        for k in lengths:
            lines.append("draws ct %d %d" % (n, k))
            want.append(str(ct_per_frame(n) * max(k, 0)))
    for fs in RATES:
        for k in lengths:
            lines.append("draws d4c %d %d" % (fs, k))
            want.append(str(d4c_per_frame(fs) * max(k, 0)))
    for k in lengths:
        lines.append("draws syn %d" % k)
        want.append(str(max(k, 0)))
    assert program(lines) == want


def test_d4c_bound_covers_what_a_frame_can_draw():
    """LoveTrain draws a window of 2 round(3 fs / max(f0, 40) / 2) + 1 samples, each of the three windows of the main pass one of
    2 round(4 fs / max(f0, 47) / 2) + 1 (matlab_round: to nearest, halves up)"""
    mround = lambda x: int(x + 0.5)
    for fs in RATES:
        bound = d4c_per_frame(fs)
        for f0 in range(1, 2001):
            draw = 2 * mround(3.0 * fs / max(f0, 40) / 2.0) + 1 + 3 * (2 * mround(4.0 * fs / max(f0, 47) / 2.0) + 1)
            assert draw <= bound, (fs, f0, draw, bound)


# ---- the draw range ----
def range_rule(pairs):
    live = [(p, n) for p, n in pairs if n > 0]
    if not live:
        return "empty 1"
    lo, hi = min(p for p, _ in live), max(p + n for p, n in live)
    return "%d %d %d" % (lo, hi, 1 if hi - lo <= 2 ** 28 else 0)


def test_draw_range(program):
    far = 2 ** 33 + 12345
    cases = [
        [],
        [(0, 0)], [(far, 0), (5, 0), (2 ** 63, 0)],                     # nothing draws: all-empty
        [(far, 0), (10, 5), (20, 7)], [(10, 5), (20, 7), (far, 0)],      # an utterance without draws first / last
        [(10, 5), (far, 0), (20, 7)], [(0, 0), (far, 100)], [(far, 100), (0, 0)],
        [(0, 2 ** 28)], [(0, 2 ** 28 + 1)], [(0, 2 ** 28 - 1)],          # the span rule on both sides of 2^28
        [(7, 1), (2 ** 28, 7)], [(7, 1), (2 ** 28 + 1, 7)], [(7, 1), (2 ** 28 - 1, 7)],
        [(2 ** 63 - 2, 100), (2 ** 63 + 2 ** 27, 5)], [(2 ** 63 - 2, 100), (2 ** 63 + 2 ** 29, 5)],  # near 2^63: no wrap
        [(2 ** 64 - 2 ** 20, 2 ** 19), (2 ** 63, 1)],
    ]
    rng = random.Random(9)
    for _ in range(40):
        base = rng.choice([0, 2 ** 28 - 500, 2 ** 40, 2 ** 63 - 1000])
        cases.append([(base + rng.randrange(2 ** rng.choice([4, 27, 29])), rng.choice([0, 0, 1, rng.randrange(1, 10 ** 6)])) for _ in range(rng.choice([1, 2, 7]))])
    lines = ["range " + " ".join("%d %d" % c for c in case) for case in cases]
    want = [range_rule(case) for case in cases]
    assert want[:3] == ["empty 1"] * 3 and want[8:11] == ["0 268435456 1", "0 268435457 0", "0 268435455 1"]
    assert want[14].endswith(" 1") and want[15].endswith(" 0")
    got = program(lines)
    assert got == want, [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]


def test_start_positions_alone(program):
    """the analysis streams apply the span rule to their streams' start positions: hi is the largest position itself"""
    cases = [[], [5], [5, 5], [0, 2 ** 28], [0, 2 ** 28 + 1], [2 ** 33 + 12345, 0], [2 ** 63, 2 ** 63 + 2 ** 28], [2 ** 64 - 1, 2 ** 64 - 1 - 2 ** 28 - 1]]
    lines = ["starts " + " ".join(map(str, c)) for c in cases]
    want = ["empty 1" if not c else "%d %d %d" % (min(c), max(c), 1 if max(c) - min(c) <= 2 ** 28 else 0) for c in cases]
    assert [w[-1] for w in want] == list("11110010")
    assert program(lines) == want


# ---- the options ----
# What every option of the four stage handles yielded before the readers existed, read off the creates: the variable, its reader
# (with the word), and the field values for the values worth trying.  `other` stands for unset, "", any other word and the word with
# a trailing character.
OPTIONS = {
    "wc_cheaptrick.hip": [
        ("WC_CT_IMPL", 'opt_is("WC_CT_IMPL", "block")', "block: wave = false; other: wave = true"),
        ("WC_CT_IMPL", 'opt_is("WC_CT_IMPL", "split")', "split: split = true (wave stays true); other: split = false"),
    ],
    "wc_d4c.hip": [
        ("WC_D4C_SPLIT", 'opt_off("WC_D4C_SPLIT")', "0, 00, 0x: split = false; unset, '', 1, words: split = true"),
        ("WC_D4C_SELECT", 'opt_is("WC_D4C_SELECT", "64")', "64: select64 = true; other (640, 6): false"),
        ("WC_D4C_BAND_WAVES", 'opt_is("WC_D4C_BAND_WAVES", "2")', "2: band_waves = 2; 3, unset, '', 20, 23, 4: band_waves = 3"),
        ("WC_D4C_LT_LIST", 'opt_off("WC_D4C_LT_LIST")', "0, 00: lt_listed = false; unset, '', 1: true"),
        ("WC_D4C_LONG", 'opt_is("WC_D4C_LONG", "halves")', "halves: long_halves = true; other: false"),
        ("WC_D4C_BAND_TAILS", 'opt_on("WC_D4C_BAND_TAILS")', "1, 10, 1x: count_tails = true; unset, '', 0, 01: false"),
        ("WC_D4C_IMPL", 'opt_is("WC_D4C_IMPL", "block")', "block: wave2 = false; other: true"),
    ],
    "wc_synthesis.hip": [
        ("WC_SYN_TIMEBASE", 'opt_is("WC_SYN_TIMEBASE", "serial")', "serial: serial_timebase = true; other: false"),
        ("WC_SYN_PHASE", 'opt_is("WC_SYN_PHASE", "single")', "single: phase_single = true; other: false"),
        ("WC_SYN_PULSES", 'opt_is("WC_SYN_PULSES", "utterance")', "utterance: pulses_by_utterance = true; other: false"),
        ("WC_SYN_IMPL", 'opt_is("WC_SYN_IMPL", "block")', "block: wave = false; other: true"),
        ("WC_SYN_OLA", 'opt_is("WC_SYN_OLA", "atomic")', "atomic: wave_atomic = true; other: false"),
        ("WC_SYN_SPLIT", 'opt_off("WC_SYN_SPLIT")', "0, 00: split = false; unset, '', 1: true"),
        ("WC_SYN_ROWS_BUDGET_MB", 'opt_int("WC_SYN_ROWS_BUDGET_MB", 0)', "set: rows_budget = atoll << 20 ('' and words: 0, 12abc: 12 MB); unset: an eighth of the memory"),
    ],
    "wc_harvest.hip": [
        ("WC_HARVEST_BANDPASS", 'opt_is("WC_HARVEST_BANDPASS", "fir")', "fir: use_fir = true; other: false"),
        ("WC_HARVEST_TIES", 'opt_is("WC_HARVEST_TIES", "ignore")', "ignore: ignore_ties = true; other: false"),
        ("WC_HARVEST_FORCE_TIE", 'opt_int("WC_HARVEST_FORCE_TIE", -1)', "set: force_tie = the number ('' and words: 0); unset: -1"),
        ("WC_HARVEST_QUIET", 'opt_is("WC_HARVEST_QUIET", "sliding")', "sliding: no_quiet = true; other: false"),
        ("WC_HARVEST_SDFT_LANES", 'opt_int("WC_HARVEST_SDFT_LANES", 0)', "set: sdft_lanes = the number; unset: 0"),
        ("WC_HARVEST_SDFT8_MAX", 'opt_int("WC_HARVEST_SDFT8_MAX", 3072)', "set: sdft8_max = the number; unset: 3072"),
        ("WC_DEBUG_SMALL_CAPS", 'opt_set("WC_DEBUG_SMALL_CAPS")', "set, to whatever ('' and 0 included): debug_small_caps = true; unset: false"),
        ("WC_HARVEST_DECIMATE", 'opt_is("WC_HARVEST_DECIMATE", "direct")', "direct: direct_decimation = chunked_decimation = true"),
        ("WC_HARVEST_DECIMATE", 'opt_is("WC_HARVEST_DECIMATE", "chunks")', "chunks: chunked_decimation = true, direct_decimation = false; other: both false"),
        ("WC_HARVEST_SMOOTH", 'opt_is("WC_HARVEST_SMOOTH", "full")', "full: smooth_full_walk = true; other: false"),
        ("WC_HARVEST_REFINE", 'opt_is(refine, "slots") ? 1 : opt_is(refine, "packed") ? 2 : opt_is(refine, "group2") ? 3 : opt_is(refine, "group8") ? 4 : 0',
         "slots, packed, group2, group8: refine_mode = 1, 2, 3, 4; other: 0"),
        ("WC_HARVEST_RAW", 'opt_is("WC_HARVEST_RAW", "lists")', "lists: raw_from_lists = true (raw_mode 0); other: false"),
        ("WC_HARVEST_RAW", 'opt_is("WC_HARVEST_RAW", "blocks") ? 1 : opt_is("WC_HARVEST_RAW", "four") ? 2 : 0', "blocks, four: raw_mode = 1, 2; other: 0"),
    ],
}
# (value, is("block"), off, on, int with default 7, set) -- "-": unset
READERS = [
    ("-", 0, 0, 0, 7, 0),
    ("=", 0, 0, 0, 0, 1),
    ("=block", 1, 0, 0, 0, 1),
    ("=blockx", 0, 0, 0, 0, 1),
    ("=bloc", 0, 0, 0, 0, 1),
    ("=0", 0, 1, 0, 0, 1),
    ("=00", 0, 1, 0, 0, 1),
    ("=01", 0, 1, 0, 1, 1),
    ("=1", 0, 0, 1, 1, 1),
    ("=10", 0, 0, 1, 10, 1),
    ("=12abc", 0, 0, 1, 12, 1),
    ("=-3", 0, 0, 0, -3, 1),
    ("=3072000000000", 0, 0, 0, 3072000000000, 1),
]


def test_option_readers(program):
    lines, want = [], []
    for value, is_, off, on, num, set_ in READERS:
        lines += ["opt is %s block" % value, "opt off %s" % value, "opt on %s" % value, "opt int %s 7" % value, "opt set %s" % value]
        want += [str(is_), str(off), str(on), str(num), str(set_)]
    # the one-character words of WC_D4C_BAND_WAVES and WC_D4C_SELECT: exact, not a prefix
    for value, word, is_ in (("=2", "2", 1), ("=20", "2", 0), ("=3", "2", 0), ("=", "2", 0), ("-", "2", 0), ("=64", "64", 1), ("=640", "64", 0), ("=6", "64", 0)):
        lines.append("opt is %s %s" % (value, word))
        want.append(str(is_))
    lines.append("opt int - -1")
    want.append("-1")
    got = program(lines)
    assert got == want, [(line, g, w) for line, g, w in zip(lines, got, want) if g != w]


def test_every_option_is_read_through_its_reader_at_the_top_of_create():
    # read elsewhere on purpose: a function-local static, a per-call switch of the tests and the benchmark, trace and debug builds
    elsewhere = {"WC_HARVEST_MID_LATE", "WC_SYN_HALVES", "WC_D4C_TRACE", "WC_SYN_TRACE_FILE", "WC_DEBUG_ONLY_PULSE"}
    for unit, table in OPTIONS.items():
        src = open(os.path.join(CSRC, unit)).read()
        assert '#include "wc_options.hpp"' in src
        reader = re.search(r"static void \w+_read_options\(\w+ \*\w+\) \{\n(.*?)\n\}\n", src, re.S).group(1)
        for name, call, _ in table:
            assert call in reader, (unit, name)
        assert set(re.findall(r'"(WC_[A-Z0-9_]+)"', reader)) == {name for name, _, _ in table}, unit
        assert set(re.findall(r'getenv\("(WC_[A-Z0-9_]+)"\)', src)) <= elsewhere, unit
        assert "strcmp" not in reader and "[0]" not in reader and "std::string" not in reader  # one spelling of "equals this word"


def test_the_host_half_is_stated_once():
    from world_class_amd import build
    for header in ("wc_stage_plan.hpp", "wc_options.hpp"):
        assert os.path.join(CSRC, header) in build.headers()
        assert "hip" not in open(os.path.join(CSRC, header)).read().split("#pragma once")[1].split("namespace wc")[0]  # no HIP include
    declared = [f for f in sorted(os.listdir(CSRC)) if re.search(r"^struct UttDesc\b", open(os.path.join(CSRC, f)).read(), re.M)]
    assert declared == ["wc_stage_plan.hpp"]
    assert '#include "wc_stage_plan.hpp"' in open(os.path.join(CSRC, "wc_internal.hpp")).read()
    plan = open(os.path.join(CSRC, "wc_stage_plan.hpp")).read()
    assert "static_assert(sizeof(UttDesc) == 48" in plan and "offsetof(UttDesc, rng_pos) == 40" in plan
    assert plan.count("1ull << 28") == 1
    for unit in ("wc_cheaptrick.hip", "wc_d4c.hip", "wc_synthesis.hip", "wc_pipeline.hip", "wc_stream.hip", "wc_synth_stream.hip"):
        src = open(os.path.join(CSRC, unit)).read()
        assert "DrawRange" in src and "1ull << 28" not in src and "f0_bound" not in src, unit
        assert "/ 47.0 / 2.0 + 1.0" not in src, unit  # D4C's bound per frame is d4c_draws'
