"""-m gpu: the enqueue-only calls queued deep on a caller's stream.  The headers promise, for the calls below, that a call "only
enqueues, on wc_set_stream's stream": no device-to-host copy, no synchronisation, the records going up through page-locked staging
that a later call reuses.  The modules' own tests bracket every call with synchronisations; here each family's sequence runs once
that way on the library's stream and then queued behind a long kernel on a torch stream (tests/enqueue_only.py), every input written
behind that kernel, with one synchronisation at the end, and must give the same bytes, guards, counts and getters.  One output per
family is held against the family's rule file here as well.

A. deep queue.  One staging per (device, stream) -- only the first call returns while the kernel in front runs: features.pack / mlpg
   / unpack and gv.stats / mlpg_gv / scale.  A record pair per handle -- the first two calls do: FilterStream.push / push_coded,
   MlpgStream and FeatureStream push / flush, Resampler.run_device, ResampleStream.push_device, VResampler.run_device,
   VResampleStream.push_device with set_step, warp.map_positions_device / warp_device / warp_along_map_device, WarpStream push /
   flush, AlignStream.set_track_device / push_settled_device / tail_device (plain, windowed, lagged).  Nothing to upload -- none may
   wait: codec.code_features_device / decode_features_device / decode_features_modified_device and io.pcm16_to_double_device /
   float_to_double_device / double_to_pcm16_device / modify_parameters_device.
B. hand-over between two streams: the scratch of the model features, and the filter stream handle.

The other entry points whose header says "only enqueues" or "Stream-ordered, enqueue-only" have a test on a caller's stream in their
own module and are not repeated here: the frame filter's run calls (test_gpu_filter.py), wc_gmm_convert_device (test_gpu_gmm.py),
the GMM trainer's posterior and accumulate (test_gpu_gmm_train.py), the retime, morph and per-frame modify calls of
world_class_io.h (test_gpu_retime.py, test_gpu_morph.py, test_gpu_modify_frames.py), both align calls (test_gpu_align.py,
test_gpu_align_ex.py), the morph and track-morph streams (test_gpu_morph_stream.py, test_gpu_track_morph*.py) and the coded pipeline
step (test_gpu_code_features.py, test_gpu_pipeline.py).  Calls that return positions or counts computed on the device (the stage
calls, the analysis stream) wait by contract and are not here."""
import numpy as np
import pytest

import enqueue_only as eo
import features_rule as fr
import filter_rule as flr
import filter_stream_rule as fsr
import gv_rule as gr
from test_gpu_features import LENGTHS as FT_LENGTHS, batch as ft_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import world_class_amd as w
    w.lib().wc_set_device(0)
    return w, torch


# ---- model features and global variance ---------------------------------------------------------------------------------------

FT_ND, FT_NAP = 25, 1
# two chains over rows of test_gpu_features.batch: 8 utterances of doubles at orders 3, then 5 of floats at orders 2
FT_CHAINS = [dict(tag="a", lengths=FT_LENGTHS, orders=3, fmt="f64", per_frame=False, max_iter=5),
             dict(tag="b", lengths=[5, 0, 130, 64, 300], orders=2, fmt="f32", per_frame=True, max_iter=1)]


def _ft_host():
    """the inputs of both chains: variant 1 of the batch (finite coded rows), a row of variances for chain a and one per frame for
    chain b, the global variance of tests/test_gpu_gv.py's model, a mask that leaves the voiced frames"""
    nd, n_ap = FT_ND, FT_NAP
    S = nd + 1 + n_ap
    scale = np.linspace(2.0, 0.2, S)
    host = {"gv_mean": 0.76 * scale * scale}
    host["gv_var"] = 0.1 * host["gv_mean"] ** 2
    for i, c in enumerate(FT_CHAINS):
        t = sum(c["lengths"])
        f0, sp, ap = ft_batch(nd, n_ap, 1)
        o = 100 * i   # (chain b reads other rows of the batch than chain a)
        rng = np.random.default_rng(40 + i)
        dt = np.float64 if c["fmt"] == "f64" else np.float32
        W = fr.width(nd, n_ap, c["orders"])
        host.update({"f0" + c["tag"]: f0[o:o + t], "sp" + c["tag"]: sp[o:o + t], "ap" + c["tag"]: ap[o:o + t],
                     "var" + c["tag"]: (10.0 ** rng.uniform(-2.0, 2.0, (t, W) if c["per_frame"] else W)).astype(dt),
                     "mask" + c["tag"]: np.where(fr.voiced(f0[o:o + t]), (1, 255)[i], 0).astype(np.uint8)})
    return host


def _ft_chain(torch, d, run, c, outs):
    """pack -> mlpg -> gv stats -> mlpg_gv -> scale -> unpack of one chain: six calls, every output in a buffer of its own (mlpg_gv and
    scale work in place: on a copy a torch kernel makes on the stream)"""
    from world_class_amd import features as ft, gv
    nd, n_ap, L, orders, fmt, tag = FT_ND, FT_NAP, c["lengths"], c["orders"], c["fmt"], c["tag"]
    t, S, W = sum(L), nd + 1 + n_ap, fr.width(nd, n_ap, orders)
    row_t = torch.float64 if fmt == "f64" else torch.float32
    rows = eo.guarded(torch, t * W, W, row_t)
    static = eo.guarded(torch, t * (S + 1), S + 1)
    g_mean, g_var = eo.guarded(torch, len(L) * S, S), eo.guarded(torch, len(L) * S, S)
    f0, csp, cap = eo.guarded(torch, t, 1), eo.guarded(torch, t * nd, nd), eo.guarded(torch, t * n_ap, n_ap)
    var, mask = d["var" + tag], d["mask" + tag]
    run(ft.pack, L, nd, n_ap, orders, d["f0" + tag], d["sp" + tag], d["ap" + tag], rows[0], -3.25, fmt)
    run(ft.mlpg, L, nd, n_ap, orders, rows[0], var, static[0], c["per_frame"], fmt)
    run(gv.stats, L, nd, n_ap, static[0], g_mean[0], g_var[0], mask)
    refined, scaled = (static[0].clone(), static[1]), (static[0].clone(), static[1])
    run(gv.mlpg_gv, L, nd, n_ap, orders, rows[0], var, d["gv_mean"], d["gv_var"], refined[0], mask, c["per_frame"], fmt, max_iter=c["max_iter"])
    run(gv.scale, L, nd, n_ap, d["gv_mean"], d["gv_var"], scaled[0], mask)
    run(ft.unpack, t, nd, n_ap, 1, refined[0], f0[0], csp[0], cap[0])
    outs += [rows, static, g_mean, g_var, refined, scaled, f0, csp, cap]


def test_model_features_and_global_variance_queued_deep(env):
    """the chain pack -> mlpg -> gv (stats, the refinement, the scaling) -> unpack queued twice, twelve calls: 8 utterances of doubles
    at orders 3, then 5 of floats at orders 2, so the one descriptor staging of the stream is rewritten by every call with another
    count.  Only the first call returns while the kernel in front runs: the second waits for the first one's copy out of the staging.
    Against the rule: chain a's mlpg and refinement on the device's own rows."""
    w, torch = env
    host = _ft_host()

    def calls(h, d, run):
        outs = []
        for c in FT_CHAINS:
            _ft_chain(torch, d, run, c, outs)
        return outs, None

    want, _, running = eo.deep_queue(w, torch, host, lambda: None, calls, pair=False, min_calls=12)
    c = FT_CHAINS[0]
    nd, n_ap, L, t = FT_ND, FT_NAP, c["lengths"], sum(c["lengths"])
    S, W = nd + 1 + n_ap, fr.width(nd, n_ap, 3)
    rows, static, refined = want[0].reshape(t, W), want[1].reshape(t, S + 1), want[4].reshape(t, S + 1)
    assert np.isfinite(static).all() and not eo.same_bytes(refined, static)
    assert eo.same_bytes(static, fr.mlpg(L, nd, n_ap, 3, rows, host["vara"], False))
    assert eo.same_bytes(refined, gr.mlpg_gv(L, nd, n_ap, 3, rows, host["vara"], False, host["gv_mean"], host["gv_var"], host["maska"], static, max_iter=5))
    assert want[9].dtype == np.float32 and np.isfinite(want[10]).all()   # chain b: rows of floats, finite statics


def test_model_features_scratch_is_handed_from_stream_to_stream(env):
    """pack, mlpg, the refinement and the stats share one scratch per device.  On stream A behind the long kernel: chain a's pack;
    on stream B: chain b's mlpg on rows of its own -- it parks its factors in the scratch that A's pack holds its contour in, so it
    may not start before that pack is through.  Then pack (A), mlpg (B), mlpg_gv (A), gv stats (B) with nothing in front."""
    w, torch = env
    from world_class_amd import features as ft, gv
    host = _ft_host()
    nd, n_ap = FT_ND, FT_NAP
    S = nd + 1 + n_ap
    ca, cb = FT_CHAINS
    ta, tb, Wa, Wb = sum(ca["lengths"]), sum(cb["lengths"]), fr.width(nd, n_ap, 3), fr.width(nd, n_ap, 2)
    rng = np.random.default_rng(8)
    host["meanb"] = rng.standard_normal((tb, Wb)).astype(np.float32)
    host["meana"] = rng.standard_normal((ta, Wa))
    host["stb"] = rng.standard_normal((tb, S + 1))

    def alloc(d):
        o = dict(rows_a=eo.guarded(torch, ta * Wa, Wa), static_b=eo.guarded(torch, tb * (S + 1), S + 1),
                 rows_b=eo.guarded(torch, tb * Wb, Wb, torch.float32), static_a=eo.guarded(torch, ta * (S + 1), S + 1),
                 mean_a=eo.guarded(torch, len(ca["lengths"]) * S, S), var_a=eo.guarded(torch, len(ca["lengths"]) * S, S),
                 refined_b=eo.guarded(torch, tb * (S + 1), S + 1))
        o["refined_b"][0][:tb * (S + 1)].copy_(d["stb"])   # (the refinement works in place)
        return o

    def first(h, d, o, run):
        run(ft.pack, ca["lengths"], nd, n_ap, 3, d["f0a"], d["spa"], d["apa"], o["rows_a"][0], -3.25, "f64")

    def second(h, d, o, run):
        run(ft.mlpg, cb["lengths"], nd, n_ap, 2, d["meanb"], d["varb"], o["static_b"][0], True, "f32")

    def rounds(h, d, o, run):
        run(ft.pack, cb["lengths"], nd, n_ap, 2, d["f0b"], d["spb"], d["apb"], o["rows_b"][0], 0.5, "f32")
        run(ft.mlpg, ca["lengths"], nd, n_ap, 3, d["meana"], d["vara"], o["static_a"][0], False, "f64")
        # (the stats read what the call two places back wrote on the same stream)
        run(gv.mlpg_gv, cb["lengths"], nd, n_ap, 2, d["meanb"], d["varb"], d["gv_mean"], d["gv_var"], o["refined_b"][0], d["maskb"], True, "f32", max_iter=2)
        run(gv.stats, ca["lengths"], nd, n_ap, o["static_a"][0], o["mean_a"][0], o["var_a"][0])

    want = eo.hand_over(w, torch, host, lambda: None, alloc, first, second, rounds)
    assert eo.same_bytes(want["static_a"].reshape(ta, S + 1), fr.mlpg(ca["lengths"], nd, n_ap, 3, host["meana"], host["vara"], False))


# ---- filter streams -----------------------------------------------------------------------------------------------------------

FLT_SETTINGS = {"hop1": (8000, 512, 0.125), "ties": (22050, 1024, 64.5 / 22.05)}   # of tests/test_gpu_filter_stream.py's SETTINGS
FLT_PUSHES, FLT_ND = 8, 24
# how far a stream's samples and rows have come behind each push, of the whole: some pushes bring a stream no samples, some no rows
FLT_CUM = ([0, .1, .1, .35, .5, .5, .8, 1., 1.], [0, 0, .3, .3, .6, .7, .7, 1., 1.])


def _flt_plan(name, kind):
    """Four streams over eight pushes.  Stream 0: exact rows; stream 1 never receives anything; stream 2: held rows, flushed at push
    3, reset in front of push 5 and then another signal; stream 3: surplus rows, the fractions swapped.  The last push flushes every
    stream.  A handle of kind POWER takes every odd push as a coded one (`to` and `from` rows of FLT_ND values).  -> the host arrays,
    the pushes [(ns, nr, flush, x_off, row_off, coded_off, coded, out)] with the counts tests/filter_stream_rule.py gives, the
    streams to reset in front of each push, the capacities, and stream 0's whole signal and rows"""
    fs, N, fp = FLT_SETTINGS[name]
    h, width = flr.hop(fp, fs), N // 2 + 1
    rng = np.random.default_rng(600 + N)
    # (stream, first push, last push: flushed there, samples, content, rows, which fractions lead)
    lives = [(0, 0, 7, int(12.3 * h) + 205, "noise", "exact", 0), (2, 0, 3, int(6 * h) + 102, "envelope", "held", 0),
             (2, 5, 7, int(4 * h) + 33, "noise", "exact", 1), (3, 0, 7, int(9.5 * h) + 60, "envelope", "surplus", 1)]
    U, P = 4, FLT_PUSHES
    table = [[(0, 0, 0)] * U for _ in range(P)]
    data = {}
    for i, (u, p0, p1, n, what, mode, lead) in enumerate(lives):
        x = rng.normal(size=n)
        rows = flr.mode_rows(what, mode, flr.segments(n, fp, fs), N, kind, seed=i)
        to, frm = 0.3 * rng.normal(size=(len(rows), FLT_ND)), 0.3 * rng.normal(size=(len(rows), FLT_ND))
        m = p1 - p0 + 1
        at = [int(round(j * 8.0 / m)) for j in range(m + 1)]
        cs = [int(round(FLT_CUM[lead][a] * n)) for a in at]
        cr = [int(round(FLT_CUM[1 - lead][a] * len(rows))) for a in at]
        for j in range(m):
            table[p0 + j][u] = (cs[j + 1] - cs[j], cr[j + 1] - cr[j], int(j == m - 1))
            data[p0 + j, u] = (x[cs[j]:cs[j + 1]], rows[cr[j]:cr[j + 1]], to[cr[j]:cr[j + 1]], frm[cr[j]:cr[j + 1]])
        if i == 0:
            whole = (x, rows)
    table[P - 1] = [(ns, nr, 1) for ns, nr, _ in table[P - 1]]
    cap_s = max(max(lv[3] for lv in lives), fsr.min_pending_samples(fp, fs)) + 1
    cap_r = flr.segments(max(lv[3] for lv in lives), fp, fs) + 3
    resets = {5: [2]}
    counts = [fsr.Counts(fs, fp, cap_s, cap_r) for _ in range(U)]
    parts = dict(x=[], rows=[], to=[], frm=[])
    pushes, xo, ro, co = [], 0, 0, 0
    for p in range(P):
        for u in resets.get(p, ()):
            counts[u] = fsr.Counts(fs, fp, cap_s, cap_r)
        coded = kind == flr.POWER and p % 2 == 1
        out = []
        for u in range(U):
            ns, nr, fl = table[p][u]
            _, _, c0, c1 = counts[u].step(ns, nr, fl)
            out.append(c1 - c0)
            if (p, u) in data:
                x, rows, to, frm = data[p, u]
                parts["x"].append(x)
                if coded:
                    parts["to"].append(to.ravel())
                    parts["frm"].append(frm.ravel())
                else:
                    parts["rows"].append(rows.ravel())
        ns, nr, fl = ([t[q] for t in table[p]] for q in range(3))
        pushes.append((ns, nr, fl, xo, ro, co, coded, out))
        xo, ro, co = xo + sum(ns), ro + (0 if coded else sum(nr)), co + (sum(nr) if coded else 0)
    host = {k: np.concatenate(v + [np.zeros(1)]) for k, v in parts.items()}
    assert sum(sum(q[7]) for q in pushes) == sum(lv[3] for lv in lives)   # a flush commits the rest: every sample comes out
    return host, pushes, resets, (cap_s, cap_r), whole


def _flt_getters(st, U=4):
    return [(st.samples_received(u), st.rows_received(u), st.segments_done(u), st.samples_committed(u), st.pending_samples(u), st.pending_rows(u))
            for u in range(U)]


def _flt_push(st, d, q, y, run, width):
    ns, nr, fl, xo, ro, co, coded, out = q
    if coded:
        return run(st.push_coded, ns, d["x"][xo:], nr, d["to"][co * FLT_ND:], d["frm"][co * FLT_ND:], FLT_ND, y, p_skip(q), fl)
    return run(st.push, ns, d["x"][xo:], nr, d["rows"][ro * width:], y, fl)


def p_skip(q):
    """skip_energy of a coded push: on where its first stream brings rows"""
    return q[1][0] > 0


def _flt_make(env, name, kind, plan, pushes_of=range(FLT_PUSHES)):
    """a handle that has made every push once, so that its scratch has its size, with every stream reset"""
    w, torch = env
    from world_class_amd.filter_stream import FilterStream
    fs, N, fp = FLT_SETTINGS[name]
    host, pushes, resets, caps, _ = plan

    def make():
        st = FilterStream(fs, N, fp, {flr.POWER: "power", flr.LOG: "log"}[kind], 4, *caps)
        d = {k: torch.from_numpy(a.copy()).cuda() for k, a in host.items()}
        y = torch.empty(4 * caps[0], dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for p in pushes_of:
            for u in resets.get(p, ()):
                st.reset(u)
            _flt_push(st, d, pushes[p], y, lambda fn, *a: fn(*a), N // 2 + 1)
        w.lib().wc_synchronize()
        for u in range(4):
            st.reset(u)
        return st
    return make


@pytest.mark.parametrize("kind", (flr.POWER, flr.LOG), ids=("power", "log"))
@pytest.mark.parametrize("name", list(FLT_SETTINGS))
def test_filter_stream_pushes_queued_deep(env, name, kind):
    """eight pushes on four streams (_flt_plan), the odd ones coded on a handle of kind POWER, a reset between two of them, every
    stream flushed by the last; the counts that come back and the getters after every push are the rule's and the synchronised
    run's.  The records go up through a pair: the first two pushes return while the kernel in front runs.  Against the rule
    (kind LOG, where every push brings rows): stream 0's outputs within filter_rule.K units of frame_filter on its whole signal."""
    w, torch = env
    fs, N, fp = FLT_SETTINGS[name]
    plan = _flt_plan(name, kind)
    host, pushes, resets, caps, (x0, rows0) = plan

    def calls(st, d, run):
        outs, meta = [], []
        for p, q in enumerate(pushes):
            for u in resets.get(p, ()):
                st.reset(u)
            y = eo.guarded(torch, sum(q[7]), 8)
            got = _flt_push(st, d, q, y[0], run, N // 2 + 1)
            assert got == q[7], (p, got, q[7])
            outs.append(y)
            meta.append((got, _flt_getters(st)))
        return outs, meta

    want, meta, running = eo.deep_queue(w, torch, host, _flt_make(env, name, kind, plan), calls, pair=True, min_calls=FLT_PUSHES)
    assert meta[-1][1][0][3] == len(x0) and meta[-1][1][1] == (0, 0, 0, 0, 0, 0)
    if kind == flr.LOG:
        y0 = np.concatenate([y[:q[7][0]] for y, q in zip(want, pushes)])
        ref, unit = flr.frame_filter(x0, rows0, kind, fs, N, fp), flr.unit(x0, rows0, kind, fs, N, fp)
        worst = float(np.abs(y0 - ref).max() / unit)
        print("filter stream %s, stream 0 against the rule: %.4f u (K = %s)" % (name, worst, flr.K))
        assert len(y0) == len(x0) and worst <= flr.K


@pytest.mark.parametrize("name", list(FLT_SETTINGS))
def test_filter_stream_handle_is_handed_from_stream_to_stream(env, name):
    """a handle of kind POWER: push 0 on stream A behind the long kernel, push 1 (coded) on stream B -- it reads the windows and the
    tails push 0 leaves, so it may not start before push 0 is through; pushes 2 to 7 then alternate A, B, A, B, A, B"""
    w, torch = env
    fs, N, fp = FLT_SETTINGS[name]
    plan = _flt_plan(name, flr.POWER)
    host, pushes, resets, caps, _ = plan

    def alloc(d):
        return {"y%d" % p: eo.guarded(torch, sum(q[7]), 8) for p, q in enumerate(pushes)}

    def some(ps):
        def go(st, d, o, run):
            meta = []
            for p in ps:
                for u in resets.get(p, ()):
                    st.reset(u)
                got = _flt_push(st, d, pushes[p], o["y%d" % p][0], run, N // 2 + 1)
                meta.append((got, _flt_getters(st)))
            return meta
        return go

    eo.hand_over(w, torch, host, _flt_make(env, name, flr.POWER, plan), alloc, some([0]), some([1]), some(range(2, FLT_PUSHES)))


# ---- the lagged streams: MLPG streams and feature streams -----------------------------------------------------------------------

LAG_ROWS = [0, 1, 2, 3, 7, 65, 200]      # the seven streams of tests/test_gpu_mlpg_stream.py and tests/test_gpu_feature_stream.py
LAG_LAGS = [5, 0, 1, 2, 5, 64, 5]        # lags 0, 1, 5 and 64 (and 2) in one push
LAG_AGAIN = (4, 1)                       # stream 4: ended by a flush behind push 1, reset to this lag in front of push 3


def _lag_steps(emitted):
    """Random cuts with pushes of no rows for the short streams, eights for the 200-row stream; stream 4 takes 5 rows, is flushed
    alone behind push 1, reset to another lag in front of push 3 and then takes all its 7 rows; a flush of all at the end.  -> the
    steps ("reset", u, lag), ("push", k, take, expect), ("flush", want, expect): take[u] the rows of stream u's data the push brings,
    expect the counts the rule gives"""
    from test_gpu_mlpg_stream import random_cuts
    rng = np.random.default_rng(11)
    n = len(LAG_ROWS)
    cuts = [random_cuts(r, rng) if r < 100 else [8] * (r // 8) + [0] for r in LAG_ROWS]
    cuts[4] = [5, 0, 0, 3, 0, 4]
    steps = [("reset", u, LAG_LAGS[u]) for u in range(n)]
    done, pos, lag = [0] * n, [0] * n, list(LAG_LAGS)
    for p in range(max(len(c) for c in cuts)):
        if p == 3:
            steps.append(("reset",) + LAG_AGAIN)
            done[4], pos[4], lag[4] = 0, 0, LAG_AGAIN[1]
        k = [c[p] if p < len(c) else 0 for c in cuts]
        steps.append(("push", k, [(pos[u], pos[u] + k[u]) for u in range(n)], [emitted(done[u] + k[u], lag[u]) - emitted(done[u], lag[u]) for u in range(n)]))
        done, pos = [a + b for a, b in zip(done, k)], [a + b for a, b in zip(pos, k)]
        if p == 1:
            steps.append(("flush", [int(u == 4) for u in range(n)], [min(lag[4], done[4]) if u == 4 else 0 for u in range(n)]))
    assert pos == LAG_ROWS and sum(1 for s in steps if s[0] != "reset") >= 20
    steps.append(("flush", [1] * n, [min(lag[u], done[u]) for u in range(n)]))
    return steps


def _lag_inputs(steps, per_stream):
    """per_stream: {name: the rows of every stream}; -> {name: the rows of every push packed in the order of the pushes}, and the
    offset (in rows) of every push"""
    parts, offs, o = {k: [] for k in per_stream}, [], 0
    for s in steps:
        if s[0] == "push":
            offs.append(o)
            for name, data in per_stream.items():
                parts[name] += [np.asarray(data[u])[a:b].reshape(b - a, int(np.prod(np.shape(data[u])[1:]))) for u, (a, b) in enumerate(s[2])]
            o += sum(s[1])
    return {k: np.concatenate(v + [np.zeros((1, v[0].shape[1]), dtype=v[0].dtype)]) for k, v in parts.items()}, offs


def _lag_calls(torch, steps, offs, width_out, out_dtype, push, flush, reset):
    """the sequence of a lagged stream handle: push(h, d, k, row_off, out) / flush(h, want, out) / reset(h, u, lag) make the calls"""
    def calls(h, d, run):
        outs, meta, i = [], [], 0
        for s in steps:
            if s[0] == "reset":
                reset(h, s[1], s[2])
                continue
            y = eo.guarded(torch, sum(s[-1]) * width_out, width_out, out_dtype)
            if s[0] == "push":
                got = run(push, h, d, s[1], offs[i], y[0])
                i += 1
            else:
                got = run(flush, h, s[1], y[0])
            assert got == s[-1], (s, got)
            outs.append(y)
            meta.append((got, [(h.rows_received(u), h.frames_emitted(u), h.get_lag(u)) for u in range(h.n_streams)]))
        return outs, meta
    return calls


def _lag_stream_rows(steps, want, u, width):
    """stream u's rows out of the outputs of the steps: (the pushes', the last flush's)"""
    outs = [s for s in steps if s[0] != "reset"]
    cut = lambda s, y: y.reshape(-1, width)[sum(s[-1][:u]):sum(s[-1][:u + 1])]
    return np.concatenate([cut(s, y) for s, y in zip(outs[:-1], want[:-1]) if s[0] == "push"]), cut(outs[-1], want[-1])


@pytest.mark.parametrize("orders,fmt,per_frame", [(3, "f64", True), (2, "f32", False)])
def test_mlpg_stream_pushes_queued_deep(env, orders, fmt, per_frame):
    """seven streams at lags 0, 1, 2, 5 and 64 in one handle, more than twenty pushes (some bring a stream no rows), a flush of one
    stream and its reset between pushes, a flush of all at the end.  The ledgers of a stream -- its state halves and its ring -- are
    on the device, advanced by the kernels of pushes that have not run yet when the next one is enqueued.  Against the rule: the
    200-row stream at lag 5 and the 65-row stream at lag 64, bit for bit."""
    w, torch = env
    import mlpg_stream_rule as ms
    import test_gpu_mlpg_stream as tm
    from world_class_amd.mlpg_stream import MlpgStream
    nd, n_ap = 25, 1
    W, S1 = fr.width(nd, n_ap, orders), nd + 2 + n_ap
    mean, var, var_row = tm.case(nd, n_ap, orders, fmt)
    steps = _lag_steps(ms.emitted)
    host, offs = _lag_inputs(steps, {"mean": tm.per_stream(mean), "var": tm.per_stream(var)})
    host["var_row"] = np.array(var_row)

    def push(h, d, k, off, y):
        return h.push_device(k, d["mean"][off * W:], d["var"][off * W:] if per_frame else d["var_row"], y, per_frame, fmt)

    calls = _lag_calls(torch, steps, offs, S1, torch.float64, push, lambda h, want, y: h.flush_device(want, y), lambda h, u, lag: h.reset(u, lag))
    make = lambda: MlpgStream(len(LAG_ROWS), nd, n_ap, orders, tm.MAX_ROWS, tm.MAX_LAG)
    want, meta, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=20)
    for u in (6, 5):
        pushed, tail = _lag_stream_rows(steps, want, u, S1)
        rule = tm.rule(nd, n_ap, orders, fmt, per_frame, u, LAG_LAGS[u])
        assert eo.same_bytes(pushed, rule[0]) and eo.same_bytes(tail, rule[1]) and np.isfinite(pushed).all(), u
    assert meta[-1][1][6] == (200, 200, 5) and meta[-1][1][4] == (7, 7, LAG_AGAIN[1])


@pytest.mark.parametrize("orders,fmt", [(3, "f64"), (2, "f32")])
def test_feature_stream_pushes_queued_deep(env, orders, fmt):
    """as the MLPG streams: seven streams of F0 and coded rows, the same pushes, flushes and resets; the rows come out packed with
    their deltas, a lag behind.  Against the rule on the device's own voiced logs: the 200-row and the 65-row stream, bit for bit."""
    w, torch = env
    import feature_stream_rule as fsr_
    import test_gpu_feature_stream as tf
    from world_class_amd import features as ft
    from world_class_amd.feature_stream import FeatureStream
    nd, n_ap = 25, 1
    W = fr.width(nd, n_ap, orders)
    f0, sp, ap = tf.case(nd, n_ap)
    steps = _lag_steps(fsr_.emitted)
    host, offs = _lag_inputs(steps, {"f0": tf.per_stream(f0), "sp": tf.per_stream(sp), "ap": tf.per_stream(ap)})
    out_t = torch.float64 if fmt == "f64" else torch.float32

    def push(h, d, k, off, y):
        return h.push_device(k, d["f0"][off:], d["sp"][off * nd:], d["ap"][off * n_ap:], y, fmt)

    calls = _lag_calls(torch, steps, offs, W, out_t, push, lambda h, want, y: h.flush_device(want, y, fmt), lambda h, u, lag: h.reset(u, lag, tf.FILL))
    make = lambda: FeatureStream(len(LAG_ROWS), nd, n_ap, orders, tf.MAX_ROWS, tf.MAX_LAG)
    want, meta, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=20)
    for u in (6, 5):
        pushed, tail = _lag_stream_rows(steps, want, u, W)
        rule = tf.rule((w, ft, torch), nd, n_ap, orders, u, LAG_LAGS[u])
        if fmt == "f32":
            with np.errstate(over="ignore"):
                rule = tuple(r.astype(np.float32) for r in rule)
        assert eo.same_bytes(pushed, rule[0]) and eo.same_bytes(tail, rule[1]), u
    assert meta[-1][1][6] == (200, 200, 5) and meta[-1][1][4] == (7, 7, LAG_AGAIN[1])


# ---- the two sample-rate converters: batches and streams ------------------------------------------------------------------------

SRC_T = {"f64": np.float64, "f32": np.float32, "i16": np.int16}


def _src_signals(seed, lengths):
    """signals of int16 values over 32768: exact in all three sample formats"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-32768, 32768, n).astype(np.float64) / 32768.0 for n in lengths]


def _src_as(x, fmt):
    return np.round(x * 32768.0).astype(np.int16) if fmt == "i16" else x.astype(SRC_T[fmt])


def _src_batch_calls(torch, batches, out_len):
    """batches: [(which handle, in_format, out_format, lengths, steps or None)], call i reading d["x<i>"]"""
    def calls(h, d, run):
        outs = []
        for i, (k, fi, fo, lengths, steps) in enumerate(batches):
            n_out = sum(out_len(k, n, s) for n, s in zip(lengths, steps or [None] * len(lengths)))
            y = eo.guarded(torch, n_out, 64, torch.float64 if fo == "f64" else torch.int16)
            run(h[k].run_device, d["x%d" % i], lengths, *(() if steps is None else (steps,)), y[0], fi, fo)
            outs.append(y)
        return outs, None
    return calls


def _grown(w, torch, host, new, calls, after=None):
    """make() for a handle whose records grow with a call: the handle makes the whole sequence once, synchronised"""
    def make():
        h = new()
        calls(h, {k: torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).cuda() for k, a in host.items()}, eo.Sync(w, torch))
        if after:
            after(h)
        return h
    return make


def test_resampler_batches_queued_deep(env):
    """six batches on two handles, 44.1 -> 48 kHz (6000 samples: the phase mapping, one tile) and 48 -> 24 kHz (6000 samples: the
    tiled mapping, more than one tile), with short utterances on the plain mapping beside them, 1 to 5 utterances per call, samples of
    int16, float and double in and double and int16 out.  Against the rule: the 48 -> 24 kHz batch of doubles, bit for bit."""
    w, torch = env
    import resample_rule as R
    from world_class_amd import resample as rs
    convs = [(44100, 48000), (48000, 24000)]
    assert rs.tiling(*convs[0])[1] <= rs.out_length(*convs[0], 6000) <= rs.tiling(*convs[0])[0] and rs.out_length(*convs[1], 6000) > rs.tiling(*convs[1])[0]
    batches = [(0, "i16", "f64", [5, 137, 6000], None), (1, "f64", "f64", [7, 63, 273, 6000], None), (0, "f32", "i16", [6000, 3], None),
               (1, "i16", "f64", [1, 4500], None), (0, "f64", "f64", [137, 5, 2 * 68 + 1, 6000, 20], None), (1, "f64", "i16", [6000], None)]
    xs = [_src_signals(70 + i, b[3]) for i, b in enumerate(batches)]
    host = {"x%d" % i: _src_as(np.concatenate(x), b[1]) for i, (x, b) in enumerate(zip(xs, batches))}
    calls = _src_batch_calls(torch, batches, lambda k, n, s: rs.out_length(*convs[k], n))
    make = _grown(w, torch, host, lambda: [rs.Resampler(*c) for c in convs], calls)
    want, _, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=6)
    up, down, half = rs.plan(*convs[1])
    G = rs.filter_taps(*convs[1])
    assert eo.same_bytes(want[1], np.concatenate([R.resample(x, up, down, G) for x in xs[1]]))


def test_vresampler_batches_queued_deep(env):
    """five batches on two handles, the default and the 256_segments plans of tests/test_gpu_vresample.py, a step per utterance, the
    lengths on both sides of segment_min and across a tile.  Against the rule: the first batch, bit for bit."""
    w, torch = env
    import test_gpu_vresample as tv
    import vresample_rule as R
    from world_class_amd import vresample as vr
    plans = [tv.plan_args("default"), tv.plan_args("256_segments")]
    ONE, UPR, (LO, HI) = tv.ONE, tv.UPR, tv.WIDE
    batches = [(0, "f64", "f64", [1, 200, 300, 3000, 273], [ONE, ONE + 1, ONE - 1, LO, HI]),
               (1, "f64", "f64", [8000, 7000, 5], [UPR, ONE, ONE + 1]), (0, "i16", "i16", [300, 5], [HI, LO]),
               (1, "f32", "f64", [9000, 100], [ONE + 1, UPR]), (0, "f64", "f64", [2100, 1, 137, 255, 257, 4000], [ONE, LO, UPR, ONE, ONE, HI])]
    seg = [vr.tiling(p["step_min"], p["step_max"], p["zeros"], 0.0, p["phase_bits"], p["degree"]) for p in plans]
    outs0 = [vr.out_length(s, n) for n, s in zip(*batches[0][3:])]
    assert min(outs0) < seg[0][1] <= max(outs0) and max(outs0) > seg[0][0] and vr.out_length(UPR, 8000) >= seg[1][1] > vr.out_length(ONE, 7000)
    xs = [_src_signals(80 + i, b[3]) for i, b in enumerate(batches)]
    host = {"x%d" % i: _src_as(np.concatenate(x), b[1]) for i, (x, b) in enumerate(zip(xs, batches))}
    calls = _src_batch_calls(torch, batches, lambda k, n, s: vr.out_length(s, n))
    make = _grown(w, torch, host, lambda: [vr.VResampler(**p) for p in plans], calls)
    want, _, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=5)
    C, bits = vr.filter_table(**plans[0]), vr.plan(**plans[0])[1].bit_length() - 1
    assert eo.same_bytes(want[0], np.concatenate([R.vresample(x, s, C, bits) for x, s in zip(xs[0], batches[0][4])]))


def _src_stream_calls(torch, pushes, n_streams, out_room):
    """pushes: [(in_format, out_format, n_new, flush, what comes first: [("step", u, step) | ("reset", u)])], push i reading d["x<i>"].
    An output has room for every stream's most; the counts that come back say how much of it is written"""
    def calls(h, d, run):
        outs, meta = [], []
        for i, (fi, fo, n_new, flush, first) in enumerate(pushes):
            for f in first:
                h.set_step(*f[1:]) if f[0] == "step" else h.reset(f[1])
            y = eo.guarded(torch, n_streams * out_room, 64, torch.float64 if fo == "f64" else torch.int16)
            got = run(h.push_device, n_new, d["x%d" % i] if sum(n_new) else None, flush, y[0], fi, fo)
            outs.append((y[0], sum(got)))
            meta.append((got, [(h.samples_received(u), h.samples_committed(u)) for u in range(n_streams)]))
        return outs, meta
    return calls


def _src_stream_host(pushes, signals):
    """signals[u]: the lives of stream u, a reset starting the next; -> the host arrays of the pushes"""
    life, at, host = [0] * len(signals), [0] * len(signals), {}
    for i, (fi, fo, n_new, flush, first) in enumerate(pushes):
        for f in first:
            if f[0] == "reset":
                assert at[f[1]] == len(signals[f[1]][life[f[1]]])
                life[f[1]], at[f[1]] = life[f[1]] + 1, 0
        parts = [signals[u][life[u]][at[u]:at[u] + n] for u, n in enumerate(n_new)]
        at = [a + n for a, n in zip(at, n_new)]
        host["x%d" % i] = _src_as(np.concatenate(parts + [np.zeros(1)]), fi)
    assert all(at[u] == len(signals[u][life[u]]) for u in range(len(signals)))
    return host


def test_resample_stream_pushes_queued_deep(env):
    """three streams at 48 -> 24 kHz (tiles of 2048 outputs), seven pushes: 5000 samples (2500 outputs: they straddle a tile), pushes
    that bring a stream nothing, int16 samples on one push and doubles on the next, a stream of fewer than K samples flushed early and
    reset, int16 out at the end, a flush of all.  The counts are wc_resample_committed's; against the rule: stream 0, bit for bit."""
    w, torch = env
    import resample_rule as R
    from world_class_amd import resample as rs
    conv, MAX = (48000, 24000), 5000
    up, down, half = rs.plan(*conv)
    pushes = [("f64", "f64", [5000, 0, 130], None, []), ("i16", "f64", [3000, 2100, 0], None, []), ("f64", "f64", [0, 5000, 3], [0, 0, 1], []),
              ("i16", "f64", [4100, 0, 0], None, []), ("f64", "f64", [64, 1, 500], None, [("reset", 2)]), ("f32", "i16", [5000, 4999, 0], None, []),
              ("f64", "f64", [0, 0, 0], [1, 1, 1], [])]
    sig = _src_signals(90, [17164, 12100, 133, 500])
    signals = [[sig[0]], [sig[1]], [sig[2], sig[3]]]
    assert len(sig[2]) < half and rs.out_length(*conv, 5000) > rs.tiling(*conv)[0]
    host = _src_stream_host(pushes, signals)
    new = lambda: rs.ResampleStream(*conv, 3, MAX)
    probe = new()
    room = probe.max_out_per_push
    probe.close()
    calls = _src_stream_calls(torch, pushes, 3, room)
    want, meta, running = eo.deep_queue(w, torch, host, new, calls, pair=True, min_calls=7)
    # the counts: the rule's, push by push
    seen, flushed = [0, 0, 0], [False] * 3
    for (fi, fo, n_new, flush, first), (got, getters) in zip(pushes, meta):
        for f in first:
            seen[f[1]], flushed[f[1]] = 0, False
        for u in range(3):
            now = flushed[u] or bool(flush and flush[u])
            assert got[u] == rs.committed(*conv, seen[u] + n_new[u], now) - rs.committed(*conv, seen[u], flushed[u])
            seen[u], flushed[u] = seen[u] + n_new[u], now
            assert getters[u] == (seen[u], rs.committed(*conv, seen[u], now))
    y0 = np.concatenate([y[:m[0][0]] for y, m in zip(want, meta)][:5] + [want[6][:meta[6][0][0]]])   # (push 5 came out as int16)
    ref = R.resample(sig[0], up, down, rs.filter_taps(*conv))
    n5 = meta[5][0][0]
    assert len(y0) + n5 == len(ref) and eo.same_bytes(y0, np.concatenate([ref[:len(y0) - meta[6][0][0]], ref[len(ref) - meta[6][0][0]:]]))
    assert np.array_equal(want[5][:n5], R.pcm16(ref[len(y0) - meta[6][0][0]:len(ref) - meta[6][0][0]]))


def test_vresample_stream_pushes_queued_deep(env):
    """three streams on the default plan (segment_min 256 outputs, tiles of 2048), seven pushes; set_step moves stream 0 in front of
    five of them and streams 1 and 2 once each: the step is a host setting and must bind to the push it precedes, with earlier
    pushes still in the queue.  The counts are the rule's at the positions that accumulate; against the rule: stream 0's outputs at
    those positions, bit for bit."""
    w, torch = env
    import test_gpu_vresample as tv
    import vresample_rule as R
    from world_class_amd import vresample as vr
    ONE, UPR, (LO, HI) = tv.ONE, tv.UPR, tv.WIDE
    MAX, half = 3000, vr.plan(LO, HI)[0]
    pushes = [("f64", "f64", [3000, 0, 100], None, [("step", 0, UPR), ("step", 2, ONE + 1)]), ("i16", "f64", [2000, 2500, 0], None, [("step", 0, ONE)]),
              ("f64", "f64", [0, 3000, 33], [0, 0, 1], []), ("f64", "f64", [150, 0, 0], None, [("step", 0, LO), ("step", 1, HI - 1)]),
              ("f32", "f64", [3000, 1, 500], None, [("reset", 2), ("step", 2, UPR)]), ("f64", "f64", [137, 3000, 0], None, [("step", 0, HI)]),
              ("f64", "f64", [0, 0, 0], [1, 1, 1], [("step", 0, ONE - 1)])]
    sig = _src_signals(91, [8287, 8501, 133, 500])
    signals = [[sig[0]], [sig[1]], [sig[2], sig[3]]]
    host = _src_stream_host(pushes, signals)
    new = lambda: vr.VResampleStream(LO, HI, 3, MAX)
    probe = new()
    room = probe.max_out_per_push
    probe.close()
    calls = _src_stream_calls(torch, pushes, 3, room)
    want, meta, running = eo.deep_queue(w, torch, host, new, calls, pair=True, min_calls=7)
    seen, flushed, pos, step, positions = [0, 0, 0], [False] * 3, [0, 0, 0], [HI] * 3, []
    mask = ONE - 1
    for (fi, fo, n_new, flush, first), (got, getters) in zip(pushes, meta):
        for f in first:
            if f[0] == "step":
                step[f[1]] = f[2]
            else:
                seen[f[1]], flushed[f[1]], pos[f[1]] = 0, False, 0
        for u in range(3):
            now = flushed[u] or bool(flush and flush[u])
            count = R.committed(pos[u] >> 32, pos[u] & mask, step[u], half, seen[u] + n_new[u], now) if not flushed[u] else 0
            assert got[u] == count, (u, got, count)
            if u == 0:
                positions += R.positions(step[0], count, pos[0])
            pos[u] += count * step[u]
            seen[u], flushed[u] = seen[u] + n_new[u], now
            assert getters[u][0] == seen[u]
    assert len(set(b - a for a, b in zip(positions[:-1], positions[1:]))) >= 5   # the spacing did move
    y0 = np.concatenate([y[:m[0][0]] for y, m in zip(want, meta)])
    assert eo.same_bytes(y0, R.vresample_at(sig[0], positions, vr.filter_table(LO, HI), R.DEFAULT[0]))


# ---- warping: the batch calls and the warp streams ------------------------------------------------------------------------------

def test_warp_calls_queued_deep(env):
    """map_positions_device -> warp_device on the positions it leaves on the device, warp_device on a near tile, a far tile and a
    short utterance of the plain group, warp_along_map_device on the maps of the first call, warp_device from int16 to int16: five
    calls on one handle (the plan "small" of tests/test_gpu_warp.py).  Against the rule: the near and the far tile, bit for bit;
    and the fourth call's outputs are the second's."""
    w, torch = env
    import test_gpu_warp as tw
    import warp_rule as W
    from world_class_amd import vresample as vr, warp, warp_stream as ws
    a = tw.plan_args("small")
    half, segs = vr.plan(**a)[:2]
    tile, span_max, segment_min, _ = warp.tiling(**a)
    near = span_max - (2 * half + 1)
    rng = np.random.default_rng(21)
    x = _src_signals(22, [9000, 3000])
    maps = [np.minimum(np.cumsum(rng.choice([0.0, 0.5, 1.0, 1.5, 2.0, 3.0], size=n)), 59.0) for n in (40, 25)]
    maps[1][7] = np.nan                                          # silence at the outputs that read it
    ope = ipu = 80.0
    outs1 = [warp.map_out_length(len(m), ope) for m in maps]
    pos3 = [tw.spread_tile(rng, tile, 200, near) + tw.spread_tile(rng, tile, 200, near + 1) + tw.R.positions(tw.ONE, 300, start=1000 * tw.ONE + 77),
            tw.spread_tile(rng, 100, -half, 2900)]
    pos5 = tw.R.positions(tw.UPR, 2000, start=-5 * tw.ONE)
    assert len(pos3[1]) < segment_min <= len(pos3[0]) and min(outs1) >= segment_min
    host = dict(x=np.concatenate(x), x16=_src_as(x[1], "i16"), maps=np.concatenate(maps), pos3=np.array(pos3[0] + pos3[1], dtype=np.int64),
                pos5=np.array(pos5, dtype=np.int64))
    lengths = [len(v) for v in x]

    def calls(r, d, run):
        pos1 = eo.guarded(torch, sum(outs1), 64, torch.int64)
        y2, y3, y4 = eo.guarded(torch, sum(outs1), 64), eo.guarded(torch, len(host["pos3"]), 64), eo.guarded(torch, sum(outs1), 64)
        y5 = eo.guarded(torch, len(pos5), 64, torch.int16)
        run(warp.map_positions_device, r, d["maps"], [40, 25], ope, ipu, outs1, pos1[0])
        run(warp.warp_device, r, d["x"], lengths, pos1[0], outs1, y2[0])
        run(warp.warp_device, r, d["x"], lengths, d["pos3"], [len(p) for p in pos3], y3[0])
        run(ws.warp_along_map_device, r, d["x"], lengths, d["maps"], [40, 25], ope, ipu, outs1, y4[0])
        run(warp.warp_device, r, d["x16"], lengths[1:], d["pos5"], [len(pos5)], y5[0], "i16", "i16")
        return [pos1, y2, y3, y4, y5], None

    make = _grown(w, torch, host, lambda: vr.VResampler(**a), calls)
    want, _, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=5)
    C, bits = vr.filter_table(**a), segs.bit_length() - 1
    assert eo.same_bytes(want[2], np.concatenate([W.warp_at(v, p, C, bits) for v, p in zip(x, pos3)]))
    assert eo.same_bytes(want[3], want[1]) and np.array_equal(want[0][:outs1[0]], W.map_positions(maps[0], ope, ipu, outs1[0]))


def test_warp_stream_pushes_queued_deep(env):
    """four streams on two resident tracks, delays 0, 1, 3 and 0, the maps of tests/test_gpu_warp_stream.py handed over as an
    alignment stream hands them over (every double written by a torch kernel on the stream), in pushes of 1, 3, 0, 2 and 5 rows
    that put the tiled and the plain group into one launch, stream 3 reset onto the other track between two pushes, and the flush
    of the two delayed streams.  The counts are the rule's; against the rule: stream 0's and stream 2's outputs (flush included)
    are warp_at at the map rule's positions, bit for bit."""
    w, torch = env
    import test_gpu_warp_stream as tws
    import warp_rule as W
    import warp_stream_rule as S
    from world_class_amd import vresample as vr, warp_stream as ws
    plan = dict(step_min=tws.R.ONE, step_max=1 << 33, zeros=4)
    n, E = 4, tws.ENTRIES
    delays, track_of = [0, 1, 3, 0], [0, 1, 0, 1]
    ope, ipu = list(tws.OPE[:n]), list(tws.IPU[:n])
    tracks = _src_signals(23, [tws.TRACK_LEN, tws.TRACK_LEN - 401])
    lives = [[tws.MAPS[0]], [tws.MAPS[1]], [tws.MAPS[2]], [tws.MAPS[3][:9], tws.MAPS[3]]]   # stream 3: nine rows, a reset, then all
    handed = [[S.settled_rows(m, delays[u]) for m in lives[u]] for u in range(n)]
    pattern = [1, 3, 0, 2, 5]
    steps, life, taken = [], [0] * n, [0] * n
    while any(taken[u] < len(handed[u][life[u]][0]) or life[u] + 1 < len(lives[u]) for u in range(n)):
        if life[3] == 0 and taken[3] == len(handed[3][0][0]):
            steps.append(("reset", 3, 0, 0, 220.5, 80.0))           # onto the other track, with other parameters
            life[3], taken[3] = 1, 0
        counts = [min(pattern[(len(steps) + u) % 5], len(handed[u][life[u]][0]) - taken[u]) for u in range(n)]
        steps.append(("push", counts, [handed[u][life[u]][0][taken[u]:taken[u] + c] for u, c in enumerate(counts)]))
        taken = [t + c for t, c in zip(taken, counts)]
    steps.append(("flush", [0, 1, 1, 0], [handed[u][0][1] if delays[u] else [] for u in range(n)]))
    doubles = [s[2] for s in steps if s[0] != "reset"]
    host = {"m%d" % i: np.array([v for part in p for v in part] + [0.0]) for i, p in enumerate(doubles)}
    host.update(t0=tracks[0], t1=tracks[1])

    def make():
        h = ws.WarpStream(plan["step_min"], plan["step_max"], n, 2, tws.TRACK_LEN, E, tws.MAX_DELAY, 240.0, zeros=4)
        for t, v in enumerate(tracks):
            h.set_track(t, v)
        for u in range(n):
            h.reset(u, track_of[u], delays[u], ope[u], ipu[u])
        return h

    def calls(h, d, run):
        outs, meta, i = [], [], 0
        for s in steps:
            if s[0] == "reset":
                h.reset(*s[1:])
                continue
            y = eo.guarded(torch, n * max(h.max_out_per_push, h.max_out_per_flush), 64)
            got = run(h.push_device if s[0] == "push" else h.flush_device, s[1], d["m%d" % i], y[0])
            i += 1
            outs.append((y[0], sum(got)))
            meta.append((got, [(h.rows_received(u), h.entries_consumed(u), h.samples_committed(u), h.get_delay(u)) for u in range(n)]))
        return outs, meta

    want, meta, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=10)
    # the counts: the rule's, from the counts alone
    rows, used, cur_ope = [0] * n, [0] * n, list(ope)
    kept = [s for s in steps]
    k = 0
    mine = {0: [], 2: []}
    for s in kept:
        if s[0] == "reset":
            rows[3], used[3], cur_ope[3] = 0, 0, s[4]
            continue
        got = meta[k][0]
        for u in range(n):
            if s[0] == "push":
                eat = S.push_split(rows[u], s[1][u], delays[u] if not (u == 3 and cur_ope[3] != ope[3]) else 0)[1]
                rows[u] += s[1][u]
            else:
                eat = S.flush_split(rows[u], delays[u])[1] if s[1][u] else 0
            assert got[u] == S.committed(used[u] + eat, cur_ope[u]) - S.committed(used[u], cur_ope[u]), (k, u)
            used[u] += eat
            if u in mine:
                mine[u].append(want[k][sum(got[:u]):sum(got[:u + 1])])
        k += 1
    C, bits = vr.filter_table(**plan), vr.plan(**plan)[1].bit_length() - 1
    for u in (0, 2):
        y = np.concatenate(mine[u])
        assert used[u] == E and len(y) == S.committed(E, ope[u])
        assert eo.same_bytes(y, W.warp_at(tracks[track_of[u]], W.map_positions(tws.MAPS[u], ope[u], ipu[u], len(y)), C, bits)), u


# ---- alignment streams: plain, windowed and lagged -----------------------------------------------------------------------------------

def test_align_stream_pushes_queued_deep(env):
    """three streams on two tracks: stream 0 plain, stream 1 with an open begin inside a moving window, stream 2 with a lag of 5
    (push_settled).  Both tracks are set on the stream; pushes of (3, 0, 64, 1, 0, 62) rows for stream 0 and other counts beside
    them; between two pushes stream 1 is taken off its track, the track is replaced by another (a queued copy into the slot earlier
    pushes read) and the stream starts over on it; the tail of the lagged stream at the end.  Against the rule: stream 0's positions
    and costs, bit for bit (tests/align_stream_rule.py)."""
    w, torch = env
    import align_stream_rule as asr
    import test_gpu_align_stream as ta
    from world_class_amd import stream
    D, n = ta.DIMS, 3
    voices = [ta.VOICE, ta.VOICE[::-1].copy(), ta.VOICE[5:]]
    own = (3, 0, 64, 1, 0, 62)
    others = [(7, 64, 0, 9, 30, 20), (64, 1, 2, 0, 33, 25)]
    win = (17, 5, 8, True)
    steps, taken = [("track", 0, "track0", 130), ("track", 1, "track1", 64), ("attach", 0), ("attach", 1), ("attach", 2)], [0] * n
    for r in range(len(own)):
        if r == 3:   # stream 1 leaves track 1, the track is replaced, the stream starts over on the new one
            steps += [("detach", 1), ("track", 1, "track1b", 24), ("attach", 1)]
            taken[1] = 0
        counts = [own[r], others[0][r], others[1][r]]
        steps.append(("push", counts, [(taken[u], taken[u] + c) for u, c in enumerate(counts)]))
        taken = [t + c for t, c in zip(taken, counts)]
    steps.append(("tail",))
    pushes = [s for s in steps if s[0] == "push"]
    host = {"rows%d" % i: np.concatenate([voices[u][a:b] for u, (a, b) in enumerate(s[2])] + [np.zeros((1, D))]) for i, s in enumerate(pushes)}
    host.update(track0=ta.TRACK, track1=ta.TRACK[60:124], track1b=ta.TRACK[40:64])

    def make():
        h = stream.AlignStream(D, n, 2, 130, 64)
        h.reserve_lag(8)
        return h

    def attach(h, u):
        h.reset(u, (0, 1, 0)[u], open_begin=u == 1)
        if u == 1:
            h.set_window(1, win[0], win[1], win[2], monotone=win[3])
        if u == 2:
            h.set_lag(2, 5)

    def calls(h, d, run):
        outs, meta, i = [], [], 0
        for s in steps:
            if s[0] == "track":
                run(h.set_track_device, s[1], s[3], d[s[2]])
            elif s[0] == "attach":
                attach(h, s[1])
            elif s[0] == "detach":
                h.reset(1, 0)
            elif s[0] == "push":
                tot = sum(s[1])
                o = [eo.guarded(torch, tot, 2) for _ in range(3)]
                run(h.push_settled_device, s[1], d["rows%d" % i], o[0][0], o[1][0], o[2][0])
                i += 1
                outs += o
            else:
                k = min(5 + 1, h.rows_received(2))
                o = eo.guarded(torch, k, 2)
                run(h.tail_device, [0, 0, 1], o[0])
                outs.append(o)
            meta.append([(h.rows_received(u), h.get_lag(u), h.get_window(u), h.track_length(u % 2)) for u in range(n)])
        return outs, meta

    want, meta, running = eo.deep_queue(w, torch, host, make, calls, pair=True, min_calls=9)
    pos = np.concatenate([want[3 * i][:s[1][0]] for i, s in enumerate(pushes)])
    cost = np.concatenate([want[3 * i + 1][:s[1][0]] for i, s in enumerate(pushes)])
    ta._same((pos, cost), asr.follow(ta.VOICE, ta.TRACK, 1, D, False), "stream 0")
    assert len(pos) == 130 and meta[-1][1][0] == taken[1] and meta[-1][2][:2] == (taken[2], 5) and len(want[-1]) == 6


# ---- the feature codec and the sample conversions -------------------------------------------------------------------------------

def test_codec_and_io_conversions_queued_as_a_chain(env):
    """pcm16 -> double -> pcm16 and float -> double; then, at (24 kHz, 1024) and at (48 kHz, 2048) -- the workgroup kernels and the
    one-wavefront kernels --: full rows -> code -> decode (the second size with a ratio per frame) -> modify -> code, every call
    reading what the call before it left on the device.  These calls keep their plan per (device, fs, fft_size) and upload nothing:
    none of them may wait.  Against the rule: the sample conversions exactly, the plain decode within the bounds of
    tests/test_gpu_codec.py of the reference codec's port."""
    w, torch = env
    import resample_rule as R
    from oracle import port_codec as pc
    from oracle.gen_golden import synth_params
    from world_class_amd import codec, io as wio
    n, nd = 37, 40
    sizes = [(24000, 1024), (48000, 2048)]
    rng = np.random.default_rng(33)
    pcm = rng.integers(-32768, 32768, 5001).astype(np.int16)
    pcm[:4] = [-32768, 32767, 0, -1]
    host = dict(pcm=pcm, flt=(3.0 * rng.uniform(-1, 1, 777)).astype(np.float32), ratio=np.where(np.arange(n) % 3, 1.0 + 0.01 * np.arange(n), 0.0))
    for i, (fs, fft) in enumerate(sizes):
        f0, sp, ap = synth_params(fs, fft, n, 77 + i)
        host.update({"f0%d" % i: f0, "sp%d" % i: sp, "ap%d" % i: ap})

    def calls(h, d, run):
        x, xf, p = eo.guarded(torch, len(pcm), 8), eo.guarded(torch, 777, 8), eo.guarded(torch, len(pcm), 8, torch.int16)
        run(wio.pcm16_to_double_device, d["pcm"], len(pcm), x[0])
        run(wio.float_to_double_device, d["flt"], 777, xf[0])
        run(wio.double_to_pcm16_device, x[0], len(pcm), p[0])
        outs = [x, xf, p]
        for i, (fs, fft) in enumerate(sizes):
            bins, n_ap = fft // 2 + 1, codec.number_of_aperiodicities(fs)
            csp, cap = eo.guarded(torch, n * nd, nd), eo.guarded(torch, n * n_ap, n_ap)
            sp, ap = eo.guarded(torch, n * bins, bins), eo.guarded(torch, n * bins, bins)
            csp2, cap2 = eo.guarded(torch, n * nd, nd), eo.guarded(torch, n * n_ap, n_ap)
            run(codec.code_features_device, fs, fft, n, nd, d["sp%d" % i], d["ap%d" % i], csp[0], cap[0])
            if i == 0:
                run(codec.decode_features_device, fs, fft, n, nd, csp[0], cap[0], sp[0], ap[0])
            else:
                run(codec.decode_features_modified_device, fs, fft, n, nd, csp[0], cap[0], d["ratio"], sp[0], ap[0])
            f0m, spm = (torch.cat([d["f0%d" % i], sp[0][:1] * float("nan")]), n), (sp[0].clone(), sp[1])   # (modify works in place)
            run(wio.modify_parameters_device, fs, fft, n, f0m[0], spm[0], 1.25, 0.9)
            run(codec.code_features_device, fs, fft, n, nd, spm[0], ap[0], csp2[0], cap2[0])
            outs += [csp, cap, sp, ap, f0m, spm, csp2, cap2]
        return outs, None

    want, _, running = eo.deep_queue(w, torch, host, lambda: None, calls, pair=True, min_calls=11)
    assert all(running[:3]), running
    assert eo.same_bytes(want[0], pcm.astype(np.float64) / 32768.0) and eo.same_bytes(want[1], host["flt"].astype(np.float64))
    assert np.array_equal(want[2], R.pcm16(want[0]))   # (wavwrite's quantisation: not the way back to pcm)
    fs, fft = sizes[0]
    csp, cap, sp, ap = want[3].reshape(n, nd), want[4].reshape(n, -1), want[5].reshape(n, -1), want[6].reshape(n, -1)
    e_sp, e_ap = np.abs(sp / pc.decode_spectral_envelope(csp, fs, fft) - 1).max(), np.abs(ap - pc.decode_aperiodicity(cap, fs, fft)).max()
    print("decode_features_device against the port of the reference codec: sp %.3e (relative), ap %.3e" % (e_sp, e_ap))
    assert e_sp < 1e-10 and e_ap < 1e-12
    assert eo.same_bytes(want[7], host["f00"] * 1.25) and not eo.same_bytes(want[8], want[5]) and np.isfinite(want[9]).all()
