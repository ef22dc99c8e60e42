"""The drive of tests/test_gpu_enqueue_only*.py: one sequence of enqueue-only calls, run synchronised on the library's stream and then
queued deep on a caller's stream behind a long kernel, compared byte for byte.

A test states its sequence once, as calls(h, d, run) -> (outs, meta):
  h     what make() returned (a handle, several, or None), made -- and grown to the sequence's largest call -- before anything is queued
  d     the test's host arrays on the device, by name, flat
  run   run(fn, *args) makes one library call; the sequence makes every call through it
  outs  a list of (tensor, n): a NaN-filled tensor of its own per output, n values of it written, the rest a guard
  meta  whatever the host learned: returned counts, getters
"""
import gc
import time

import numpy as np

LONG_N, LONG_PRODUCTS = 4096, 40   # the kernel in front, as tests/test_gpu_morph_stream.py queues it


class Sync:
    """every call between two synchronisations"""

    def __init__(self, w, torch):
        self.w, self.torch, self.running = w, torch, None

    def __call__(self, fn, *args, **kw):
        self.torch.cuda.synchronize()
        r = fn(*args, **kw)
        self.w.lib().wc_synchronize()
        self.torch.cuda.synchronize()
        return r


class Queued:
    """no synchronisation; notes after every call whether the kernel in front was still running"""

    def __init__(self, done):
        self.done, self.running, self.clock = done, [], []

    def __call__(self, fn, *args, **kw):
        t0 = time.perf_counter()
        r = fn(*args, **kw)
        t1 = time.perf_counter()
        self.running.append(not self.done.query())
        self.clock.append((t0, t1))
        return r


def long_kernel(torch, s):
    """LONG_PRODUCTS products of a LONG_N x LONG_N float matrix on the current stream s, and the event behind them"""
    junk = torch.randn(LONG_N, LONG_N, device="cuda")
    for _ in range(LONG_PRODUCTS):
        junk = junk @ junk * 1e-3
    done = torch.cuda.Event(enable_timing=True)
    done.record(s)
    return done, junk


def pinned(torch, host):
    return {k: torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).pin_memory() for k, a in host.items()}


def upload(torch, pins):
    """on the current stream: the copies out of page-locked memory, then a torch kernel that writes every input"""
    d = {}
    for k, p in pins.items():
        t = torch.zeros(len(p), dtype=p.dtype, device="cuda")
        t.copy_(p, non_blocking=True)
        d[k] = t.mul_(1)
    return d


def guarded(torch, n, guard, dtype=None):
    """n values and guard more behind them, all NaN (an integer type: its lowest value); -> (tensor, n)"""
    dtype = dtype or torch.float64
    fill = float("nan") if dtype.is_floating_point else torch.iinfo(dtype).min
    return torch.full((int(n) + int(guard),), fill, dtype=dtype, device="cuda"), int(n)


def fetch(outs):
    """the outputs on the host, every guard checked"""
    got = []
    for t, n in outs:
        a = t.cpu().numpy()
        assert len(a) > n, "an output without a guard"
        tail = a[n:]
        assert np.isnan(tail).all() if a.dtype.kind == "f" else (tail == np.iinfo(a.dtype).min).all(), "a guard was written"
        got.append(a[:n].copy())
    return got


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, x) in enumerate(zip(got, want)):
        assert same_bytes(g, x), "%s: output %d of %d differs from the synchronised run" % (what, i, len(got))


def synchronised(w, torch, host, make, calls):
    """the sequence on the library's stream, every call synchronised -> (outputs on the host, meta)"""
    torch.cuda.synchronize()
    d = {k: torch.from_numpy(np.ascontiguousarray(a).ravel().copy()).cuda() for k, a in host.items()}
    outs, meta = calls(make(), d, Sync(w, torch))
    torch.cuda.synchronize()
    return fetch(outs), meta


def deep_queue(w, torch, host, make, calls, pair, min_calls=4):
    """Runs the sequence synchronised on the library's stream (want), then on a torch stream s handed over by wc_set_stream: once
    synchronised on a handle of its own -- the kernels' code is loaded and whatever is kept per stream has its size -- and then
    queued: the long kernel, the event done, the inputs out of page-locked memory and written by a torch kernel, every call with no
    synchronisation, one s.synchronize() at the end.  The queued outputs and meta must equal want's; the first call (pair: the first
    two) must have returned while the long kernel ran.  -> (want, meta, running)"""
    want, want_meta = synchronised(w, torch, host, make, calls)
    pins = pinned(torch, host)
    h = make()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert w.lib().wc_set_stream(s.cuda_stream) == 0
    try:
        with torch.cuda.stream(s):
            warm_outs, warm_meta = calls(make(), upload(torch, pins), Sync(w, torch))
            torch.cuda.synchronize()
            front = torch.cuda.Event(enable_timing=True)
            front.record(s)
            gc.collect()
            gc.disable()   # (a collection of the host's between two calls would look like a call that waited)
            t_front = time.perf_counter()
            done, junk = long_kernel(torch, s)
            q = Queued(done)
            t_done = time.perf_counter()
            d = upload(torch, pins)
            t_up = time.perf_counter()
            outs, meta = calls(h, d, q)
        s.synchronize()  # once
    finally:
        gc.enable()
        assert w.lib().wc_set_stream(None) == 0
    running = q.running
    print("the kernel in front ran %.1f ms; on the host, from its enqueue: done recorded at %.2f ms, inputs queued at %.2f ms, calls returned at %s ms"
          % (front.elapsed_time(done), 1e3 * (t_done - t_front), 1e3 * (t_up - t_front), " ".join("%.2f" % (1e3 * (b - t_front)) for a, b in q.clock[:6])))
    print("queued %d calls; the kernel in front still ran behind call: %s" % (len(running), "".join("1" if r else "0" for r in running)))
    assert len(running) >= min_calls
    assert running[0], "the precondition: the first call returned after the kernel in front had finished"
    assert_same(fetch(warm_outs), want, "synchronised on the caller's stream")
    assert warm_meta == want_meta
    assert_same(fetch(outs), want, "queued")
    assert meta == want_meta, (meta, want_meta)
    if pair:
        assert running[1], "the second call waited for the kernel in front: %s" % running
    return want, want_meta, running


def hand_over(w, torch, host, make, alloc, first, second, rounds):
    """Part B.  alloc(d) -> the outputs by name, {name: (tensor, n)}, each NaN-guarded (or a guarded copy of an input where a call works in place);
    first(h, d, o, run) and second(h, d, o, run) are one call each on independent inputs, rounds(h, d, o, run) four more; each gives
    its meta.  Synchronised on the library's stream for want; then on two torch streams: on A the long kernel, done, first; on B
    second and an event e2 behind it.  done must not have happened when second returns; when e2 has, done must have: the second
    call waited on the device for what the first one shares with it.  rounds then alternates A, B, A, B (its run switches the stream
    before every call) with nothing in front and no synchronisation between the calls."""
    lib = w.lib()

    names = []

    def all_three(h, d, run):
        o = alloc(d)
        names[:] = list(o)
        return list(o.values()), (first(h, d, o, run), second(h, d, o, run), rounds(h, d, o, run))

    want, want_meta = synchronised(w, torch, host, make, all_three)
    pins = pinned(torch, host)
    h = make()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        for s in (a, b):   # whatever is kept per stream has its size, the code is loaded
            assert lib.wc_set_stream(s.cuda_stream) == 0
            with torch.cuda.stream(s):
                all_three(make(), upload(torch, pins), Sync(w, torch))
        torch.cuda.synchronize()
        d = upload(torch, pins)
        o = alloc(d)
        torch.cuda.synchronize()
        plain = lambda fn, *args, **kw: fn(*args, **kw)
        gc.collect()
        gc.disable()   # (as in deep_queue: the precondition below is a matter of milliseconds)
        assert lib.wc_set_stream(a.cuda_stream) == 0
        with torch.cuda.stream(a):
            done, junk = long_kernel(torch, a)
            m1 = first(h, d, o, plain)
        assert lib.wc_set_stream(b.cuda_stream) == 0
        with torch.cuda.stream(b):
            m2 = second(h, d, o, plain)
            e2 = torch.cuda.Event()
            e2.record(b)
        early = done.query()
        gc.enable()
        assert not early, "the precondition: the kernel in front had finished before the second call was enqueued"
        e2.synchronize()
        assert done.query(), "the call on the second stream finished before the work it had to wait for"
        torch.cuda.synchronize()
        turn = [0]

        def alternating(fn, *args, **kw):
            s = (a, b)[turn[0] % 2]
            turn[0] += 1
            assert lib.wc_set_stream(s.cuda_stream) == 0
            return fn(*args, **kw)

        m3 = rounds(h, d, o, alternating)
        assert turn[0] >= 4
        torch.cuda.synchronize()
    finally:
        gc.enable()
        assert lib.wc_set_stream(None) == 0
    assert list(o) == names
    assert_same(fetch(list(o.values())), want, "handed from stream to stream")
    assert (m1, m2, m3) == want_meta
    return dict(zip(names, want))
