"""close() of every handle class of the mirror on the device: the smallest handle its create accepts, one call, close twice and del
-- the handle is gone, the library has recorded no error -- and then the same handle created and used again, which a double destroy
or a staging array freed under a live reference would break."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, FFT, BINS, ND = 16000, 1024, 513, 4


def _signal():
    return 0.3 * np.sin(2 * np.pi * 150.0 * np.arange(3200) / FS)


def _frames(w):
    n = w.get_samples(FS, 3200, 5.0)
    return np.arange(n) * 0.005, np.full(n, 150.0)


def _full_row():
    return np.array([150.0]), np.full((1, BINS), 1e-3), np.full((1, BINS), 0.5)


def _cheaptrick(w):
    h = w.CheapTrick(FS)
    return h, lambda: h.compute(_signal(), *_frames(w)).shape == (len(_frames(w)[0]), h.bins)


def _d4c(w):
    h = w.D4C(FS)
    return h, lambda: h.compute(_signal(), *_frames(w), FFT).shape == (len(_frames(w)[0]), BINS)


def _synthesis(w):
    h = w.Synthesis(FS, FFT, 5.0)
    n = len(_frames(w)[0])
    return h, lambda: len(h.compute(np.full(n, 150.0), np.full((n, BINS), 1e-3), np.full((n, BINS), 0.5))) == h.out_length(n)


def _harvest(w):
    h = w.Harvest(FS)
    return h, lambda: len(h.compute(_signal())[1]) == h.get_samples(3200)


def _pipeline(w):
    h = w.Pipeline(FS)
    return h, lambda: h.run_batch([_signal()])[0]["sp"].shape[1] == h.bins


def _gmm(w):
    from world_class_amd import gmm
    h = gmm.Gmm([1.0], [[0.0, 0.0]], np.eye(2)[None], 1)
    return h, lambda: h.convert_host(np.zeros((1, 1)))[0].shape == (1, 1)


def _gmm_trainer(w):
    from world_class_amd import gmm_train
    h = gmm_train.GmmTrainer(1, 1, 1)

    def use():
        h.set_model([1.0], [[0.0, 0.0]], np.eye(2)[None])
        return len(h.fit_host(np.array([[0.0, 0.1], [1.0, 0.9], [-1.0, -1.1]]), 1)) == 1
    return h, use


def _analyzer(w):
    from world_class_amd import stream
    h = stream.StreamAnalyzer(FS, 1, frame_period=5.0, chunk_ms=40, lookback_ms=40, lookahead_ms=40)
    return h, lambda: set(h.push([_signal()[:h.chunk_samples]])[0]) == {"tpos", "f0", "sp"}


def _synthesizer(w):
    from world_class_amd import stream
    h = stream.StreamSynthesizer(FS, FFT, 5.0, n_streams=1, max_frames=1)
    f0, sp, ap = _full_row()

    def use():  # (a stream needs two frames before its flush: two pushes of max_frames each)
        got = h.push([f0], [sp], [ap]) + h.push([f0], [sp], [ap], [1])
        return h.frames_received(0) == 2 and sum(len(y) for y in got) == h.samples_committed(0) > 0
    return h, use


def _morph(w):
    from world_class_amd import stream
    h = stream.MorphStream(FS, FFT, n_streams=1, max_frames=1)
    return h, lambda: len(h.push([_full_row()], [_full_row()])[0]) == 3


def _align(w):
    from world_class_amd import stream
    h = stream.AlignStream(dims=2, n_streams=1, n_tracks=1, max_track_frames=1, max_rows_per_push=1)

    def use():
        h.set_track(0, [[0.0, 1.0]])
        h.reset(0, 0)
        return [len(v) for v in h.push([[[0.0, 1.0]]])[0]] == [1, 1]
    return h, use


def _track_morph(w):
    from world_class_amd import stream
    h = stream.TrackMorph(FS, FFT, n_streams=1, n_tracks=1, max_track_frames=1, max_frames=1)

    def use():
        h.set_track(0, *_full_row())
        h.reset(0, 0)
        return len(h.push([_full_row()], [[0.0]])[0]) == 3
    return h, use


def _coded_track_morph(w):
    from world_class_amd import codec, stream
    h = stream.CodedTrackMorph(FS, FFT, ND, n_streams=1, n_tracks=1, max_track_frames=1, max_frames=1)
    row = np.array([150.0]), np.zeros((1, ND)), np.full((1, codec.number_of_aperiodicities(FS)), -1.0)

    def use():
        h.set_track(0, *row)
        h.reset(0, 0)
        return len(h.push([row], [[0.0]])[0]) == 3
    return h, use


MAKERS = [_cheaptrick, _d4c, _synthesis, _harvest, _pipeline, _gmm, _gmm_trainer, _analyzer, _synthesizer, _morph, _align, _track_morph,
          _coded_track_morph]


@pytest.mark.parametrize("make", MAKERS, ids=[m.__name__.strip("_") for m in MAKERS])
def test_close_twice_and_del_then_the_same_handle_again(make):
    import world_class_amd as w
    from world_class_amd._binding import _Handle
    w.lib().wc_set_device(0)
    h, use = make(w)
    assert isinstance(h, _Handle) and h._h
    assert use()
    staged = [d for d in (h._staging() if hasattr(h, "_staging") else ()) if d is not None]
    before = w.last_error()
    h.close()
    assert h._h is None and all(d.ptr is None for d in staged)
    h.close()
    assert h._h is None
    del h, use
    assert w.last_error() == before
    h, use = make(w)
    assert h._h and use()
    h.close()
    assert w.last_error() == before
