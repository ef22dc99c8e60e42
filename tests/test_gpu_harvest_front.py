"""-m gpu: Harvest's front half on the device -- the decimators (hv_decimate_scan_kernel by default, the chunked kernels behind
WC_HARVEST_DECIMATE), hv_dc_kernel, the sliding band-pass with its seam and quiet-chunk kernels, the FIR band-pass, the raw
candidate kernels and hv_detect_kernel -- read through Harvest.compute_batch and debug_fetch("y" | "raw" | "cand0") on the signals
of tests/harvest_front.py, against the long double rule there (tests/test_harvest_front_rule.py proves on the CPU what each table
reaches, measures K_ref and shows that the rule is sharp).

What is compared how:
 * y at decimation 1 is the signal and one zero, bit for bit; behind a decimator or a non-zero DC sum it lies within 2 K_ref(y)
   units u_y of the rule, K_ref(y) that of the table's own decimation ratio;
 * raw candidates: outside the near-threshold set zero exactly where the rule's are, band by band and frame by frame, and where
   the restatement's are; values within 2 K_ref(raw) units for the FIR form and 2 K_ref(raw) max(1, p / log2 N) for the sliding
   forms (units, p, N: harvest_front's docstring);
 * detection: the rule's detector run on the device's OWN raw table gives cand0 bit for bit (the kernel sums a run ascending,
   as the reference does, and divides once);
 * the forms the suite calls bit-identical are bit-identical on every band-pass table (1 and 8 lanes per band; the raw modes);
 * level_drop (falls to either side of the quiet-chunk threshold): the rule's zero pattern on the frames firm under the
   reference's utterance-wide unit, errors within twice the restatement's on the same frame plus the stationary bound, and the
   threshold's side bit for bit against WC_HARVEST_QUIET=sliding.
WC_HARVEST_TIES=ignore is set for every handle, so that each form answers for itself.

The rule of every table, the restatement on it and K_ref are computed once per session (harvest_front's caches): the first case
that asks for K_ref pays for all of them, about 15 s of CPU; every case after that takes a fraction of a second, one handle per
(table, form).

Measured on an MI355X: see DESIGN.md, "Harvest's front half on written signals".
"""
import os

import numpy as np
import pytest

import harvest_front as F

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},
    "lanes1": {"WC_HARVEST_SDFT_LANES": "1"},
    "lanes8": {"WC_HARVEST_SDFT_LANES": "8"},
    "fir": {"WC_HARVEST_BANDPASS": "fir"},
    "raw_lists": {"WC_HARVEST_RAW": "lists"},
    "raw_blocks": {"WC_HARVEST_RAW": "blocks"},
    "raw_four": {"WC_HARVEST_RAW": "four"},
    "direct": {"WC_HARVEST_DECIMATE": "direct"},
    "chunks": {"WC_HARVEST_DECIMATE": "chunks"},
    "quiet_sliding": {"WC_HARVEST_QUIET": "sliding"},
}
SWITCHES = sorted({k for env in FORMS.values() for k in env} | {"WC_HARVEST_TIES"})


@pytest.fixture(scope="module")
def wca():
    import world_class_amd as w
    w.lib()
    return w


def handle(wca, t, form):
    """a handle created under the form's development switches (they are read at creation)"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ["WC_HARVEST_TIES"] = "ignore"
    os.environ.update(FORMS[form])
    try:
        return wca.Harvest(t.fs, **t.options())
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


_device = {}


def fetch(h, t, u, n_utt_index):
    return dict(y=h.debug_fetch("y", n_utt_index), raw=h.debug_fetch("raw", n_utt_index).reshape(len(t.b), t.L1(u)),
                cand0=h.debug_fetch("cand0", n_utt_index).reshape(t.L1(u), t.S))


def device(wca, name, form="default"):
    """a table's utterances in one call under a form: per utterance dict(y, raw [bands][frames], cand0 [frames][S]); once"""
    if (name, form) not in _device:
        t = F.table(name)
        h = handle(wca, t, form)
        h.compute_batch(t.xs)
        _device[(name, form)] = [fetch(h, t, u, u) for u in range(len(t.xs))]
    return _device[(name, form)]


def check_y(name, form, got, k_all):
    """y against the rule, held to twice the restatement's error at the table's own decimation ratio (the recursion's error
    grows with the ratio: 1.1 units at r = 2, 70 to 80 at r = 12)"""
    t = F.table(name)
    k = k_all["y_r"].get(t.r, 0.0)
    worst = 0.0
    for u, (r, d) in enumerate(zip(F.rule(name), got)):
        assert len(d["y"]) == t.y_len(u), (name, form, u)
        if t.r == 1 and r["acc"] == 0:
            assert np.array_equal(d["y"], np.append(t.xs[u], 0.0)), (name, form, u, "y is not the signal and one zero")
        worst = max(worst, float(F.y_errors(r, d["y"]).max()))
    print("harvest front %s [%s]: K_ref(y) at r = %d %.3f (%.3f over all ratios); device's worst y error %.3f units (%.3f of its bound)"
          % (name, form, t.r, k, k_all["y"], worst, worst / (2.0 * k) if k else 0.0))
    assert worst <= 2.0 * k, (name, form, worst)
    return worst


@pytest.mark.parametrize("name", F.NAMES)
def test_decimated_signal_matches_the_rule(wca, port, name):
    check_y(name, "default", device(wca, name), F.k_ref(port))


@pytest.mark.parametrize("form", ["direct", "chunks"])
@pytest.mark.parametrize("name", ["dec_edges", "dec_short", "ratio_5", "ratio_11"])
def test_chunked_decimators_match_the_rule(wca, port, name, form):
    """the decimators of earlier rounds (chunks that warm up on 768 preceding samples, staged through LDS or read directly), each
    against the rule: at the scan kernel's block border, the 32-sample chunks, and inputs of 8, 9 and 10 samples, at and around the nine reflected ones"""
    check_y(name, form, device(wca, name, form), F.k_ref(port))


@pytest.mark.parametrize("form", ["default", "direct", "chunks"])
@pytest.mark.parametrize("name", ["dec_edges", "dec_short"])
def test_ragged_decimation_equals_each_utterance_alone(wca, name, form):
    """dec_edges is a ragged batch -- 17 to 15 617 decimated samples side by side, every utterance as loud as its neighbours --
    and dec_short one of 5 and 6: an utterance that read a neighbour's samples or chunk states would differ from the same
    utterance alone in its call.  Under each of the three decimators"""
    t = F.table(name)
    got = device(wca, name, form)
    h = handle(wca, t, form)
    for u in range(len(t.xs)):
        h.compute_batch([t.xs[u]])
        assert np.array_equal(h.debug_fetch("y", 0), got[u]["y"]), (name, form, u)


def check_raw(wca, port, name, form, sliding, held=True):
    t, k = F.table(name), F.k_ref(port)["raw"]
    got = device(wca, name, form)
    worst = share = worst_fir = 0.0
    near = live = compared = 0
    flips = 0
    for u, (r, o, d) in enumerate(zip(F.rule(name), F.restatement(port, name), got)):
        if held:
            n, l = F.same_zero_pattern(t, u, r, d["raw"], k, sliding)
            near, live = near + n, live + l
        for j in t.bands:
            br = r["bands"][j]
            firm = ~F.near_threshold(br, k, sliding, t.floor, t.ceil, t.fs_d)
            if t.stationary and held:  # ... and where the restatement's are
                assert np.array_equal((d["raw"][j] != 0)[firm], (o["raw"][j] != 0)[firm]), (name, form, u, j)
            flips += int(((d["raw"][j] != 0) != (br["raw"] != 0))[firm].sum())
            e = F.raw_errors(br, d["raw"][j], sliding)
            e[~firm] = 0.0
            compared += int((e > 0).sum())
            worst = max(worst, float(e.max()))
            if sliding:  # the same errors in the FIR form's units, which do not grow along the chunk
                e = F.raw_errors(br, d["raw"][j], False)
                e[~firm] = 0.0
                worst_fir = max(worst_fir, float(e.max()))
    share = worst / (2.0 * k)
    print("harvest front %s [%s]: K_ref(raw) %.3f; device's worst raw error %.3f units (%.3f of its %s bound) over %d values; "
          "%d of %d live positions near a threshold; %d firm positions with another zero pattern%s"
          % (name, form, k, worst, share, "sliding" if sliding else "FIR", compared, near, live, flips,
             "; in the FIR form's units, which do not grow, %.3f (%.3f of 2 K_ref)" % (worst_fir, worst_fir / (2.0 * k)) if sliding else ""))
    if held:
        assert compared > 0 or name == "few_edges", (name, form, "nothing was compared")
        assert share <= 1.0, (name, form, worst)
    return worst, flips


@pytest.mark.parametrize("name", F.PLAIN_RAW_TABLES)
def test_raw_candidates_of_the_sliding_form_match_the_rule(wca, port, name):
    """the default band-pass.  `burst` falls silent inside its only chunk, which the quiet test leaves to direct sums: it is held
    to the FIR form's bound"""
    check_raw(wca, port, name, "default", sliding=F.table(name).stationary)


@pytest.mark.parametrize("name", F.PLAIN_RAW_TABLES)
def test_raw_candidates_of_the_fir_form_match_the_rule(wca, port, name):
    check_raw(wca, port, name, "fir", sliding=False)


def level_errors(port, got, sliding):
    """level_drop, per fall: (frames compared, the device's worst error in Hz, the restatement's, the device's worst error as a
    multiple of its bound -- twice the restatement's error on the same frame plus the stationary bound --, firm positions whose
    zero pattern is not the rule's), over the frames that are firm under the reference's utterance-wide unit"""
    t, k = F.table("level_drop"), F.k_ref(port)["raw"]
    out = []
    for r, o, d in zip(F.rule("level_drop"), F.restatement(port, "level_drop"), got):
        n = flips = 0
        e_dev = e_ref = over = 0.0
        for j in t.bands:
            br = r["bands"][j]
            firm = ~F.near_threshold(br, k, False, t.floor, t.ceil, t.fs_d, wide=True)
            flips += int(((d["raw"][j] != 0) != (br["raw"] != 0))[firm].sum())
            both = firm & (d["raw"][j] != 0) & (br["raw"] != 0) & (o["raw"][j] != 0)
            dev, ref = np.abs(d["raw"][j] - br["raw"])[both], np.abs(o["raw"][j] - br["raw"])[both]
            bound = 2.0 * ref + F.allowed_hz(br, k, sliding)[both]
            n += int(both.sum())
            e_dev, e_ref, over = max(e_dev, float(dev.max())), max(e_ref, float(ref.max())), max(over, float((dev / bound).max()))
        out.append((n, e_dev, e_ref, over, flips))
    return out


@pytest.mark.parametrize("form", ["default", "fir"])
def test_level_falls_on_either_side_of_the_quiet_threshold(wca, port, form):
    """level_drop: 0.9, then 0.9 times 1e-6, 2e-8 (the chunk stays with the sliding sums), 0.5e-8 and 1e-10 (it is left to direct
    sums), then exact zeros.  On the frames firm under the reference's utterance-wide unit the zero pattern is the rule's and the
    error at most twice the restatement's on the same frame plus the stationary bound (harvest_front's docstring: the unit's A
    is the chunk's so far for sliding sums, the window's for direct ones; the FIR form is direct throughout)"""
    res = level_errors(port, device(wca, "level_drop", form), sliding=form == "default")
    for c, (n, e_dev, e_ref, over, flips) in zip(F.LEVELS, res):
        print("harvest front level_drop [%s] fall to %g: %d frames compared; device's worst error %.3g Hz, restatement's %.3g Hz; "
              "device at most %.3g of its bound; %d firm positions with another zero pattern" % (form, c, n, e_dev, e_ref, over, flips))
    for c, (n, e_dev, e_ref, over, flips) in zip(F.LEVELS, res):
        assert n >= 270 and flips == 0 and over <= 1.0, (form, c, n, flips, over)


def test_quiet_threshold_lies_between_the_levels(wca, port):
    """kQuietDrop on both sides, bit for bit.  WC_HARVEST_QUIET=sliding never falls back.  On the frames that read the quiet
    stretch of the first chunk alone, a fall to 1e-6 or 2e-8 -- above the threshold -- must give the bits of that form: the chunk
    was not left to direct sums.  A fall to 0.5e-8 or 1e-10 must not: it was.  What the fall-back buys is printed, not held"""
    t = F.table("level_drop")
    a, b = device(wca, "level_drop"), device(wca, "level_drop", "quiet_sliding")
    res = level_errors(port, b, sliding=False)
    for c, x, y, r, (n, e_dev, e_ref, over, flips) in zip(F.LEVELS, a, b, F.rule("level_drop"), res):
        print("harvest front level_drop [WC_HARVEST_QUIET=sliding] fall to %g: worst error %.3g Hz (restatement's %.3g Hz), %.3g of the "
              "bound of direct sums; %d firm positions with another zero pattern" % (c, e_dev, e_ref, over, flips))
        same = all(np.array_equal(x["raw"][j, F.LEVEL_FRAMES], y["raw"][j, F.LEVEL_FRAMES]) for j in t.bands)
        assert x["raw"][t.bands, F.LEVEL_FRAMES].any() and same == (not r["quiet"][0]) == (c > 1e-8), (c, same)


def test_what_the_quiet_fallback_buys(wca, port):
    """`burst` with WC_HARVEST_QUIET=sliding: the sliding sums carry the burst's roundings into the exact zeros behind it.  What
    the switch gives is recorded, not held; the default is held, and must be at least as close to the rule"""
    w0, f0 = check_raw(wca, port, "burst", "default", sliding=False)
    w1, f1 = check_raw(wca, port, "burst", "quiet_sliding", sliding=False, held=False)
    print("harvest front burst: WC_HARVEST_QUIET=sliding: worst error %.3g units (default %.3g), %d firm positions with another zero "
          "pattern (default %d)" % (w1, w0, f1, f0))
    assert f0 == 0 and f0 <= f1 and w0 <= w1


@pytest.mark.parametrize("name", F.RAW_TABLES)
def test_forms_called_bit_identical_are(wca, name):
    """one lane and eight lanes per (band, chunk) of the sliding band-pass, and the raw modes (edges from per-band lists, every
    block its own slice, four wavefronts per block): the same bits as the default, at the seams and on exact zeros too"""
    a = device(wca, name)
    for form in ("lanes1", "lanes8", "raw_lists", "raw_blocks", "raw_four"):
        for u, (x, y) in enumerate(zip(a, device(wca, name, form))):
            assert np.array_equal(x["raw"], y["raw"]) and np.array_equal(x["cand0"], y["cand0"]), (name, form, u)
    assert name == "few_edges" or any(x["raw"].any() for x in a)


@pytest.mark.parametrize("name", F.NAMES)
def test_detection_is_the_rule_on_the_devices_own_raw_table(wca, name):
    """vuv, the forced zeros at both end bands, runs of at least 10 bands, the ascending sum and the one division: cand0 bit for bit"""
    t = F.table(name)
    filled = 0
    for u, d in enumerate(device(wca, name)):
        want, _ = F.detect_rule(d["raw"], t.S)
        assert np.array_equal(want != 0, d["cand0"] != 0), (name, u, "zero pattern or slot order")
        assert np.array_equal(want, d["cand0"]), (name, u)
        filled = max(filled, int((want != 0).sum(1).max()))
    print("harvest front %s: detection bit for bit; at most %d slots filled in a frame" % (name, filled))
    if name.startswith("runs"):
        assert filled >= 2  # the two-tone utterance fills a second slot
