"""The spectrum steps of a stream bank without a GPU: the surface, the frame arithmetic, the argument checks (all before
any device work), the float64 model of the step-wise contract (tests/stream_spectrum_model.py) against the offline oracle
and the streaming audio models, and the per-frame metric of tests/test_gpu_stream_spectrum.py against planted defects."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_model as M
from tests import stream_ns_model as MN
from tests import stream_spectrum_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CELLS = [c for c in PB.TILE_CELLS if c["path"].startswith("stream")]


def test_surface():
    from noisereduce_amd import stream
    B, G = stream.StreamBank, stream.StreamGate
    assert list(inspect.signature(stream.frames_applied).parameters) == ["n", "W", "H", "lag"]
    assert list(inspect.signature(B.frames).parameters) == ["self", "slot"]
    sig = inspect.signature(B.push_spectrum)
    assert list(sig.parameters) == ["self", "blocks", "return_mask"] and sig.parameters["return_mask"].default is False
    sig = inspect.signature(B.flush_spectrum)
    assert list(sig.parameters) == ["self", "slots", "blocks", "return_mask"]
    assert sig.parameters["blocks"].default is None and sig.parameters["return_mask"].default is False
    assert list(inspect.signature(G.push_spectrum).parameters) == ["self", "block", "return_mask"]
    assert list(inspect.signature(G.flush_spectrum).parameters)[0] == "self"
    assert "return_mask" in inspect.signature(G.flush_spectrum).parameters
    # what was there stays as it was
    assert list(inspect.signature(B.push).parameters) == ["self", "blocks"]
    assert list(inspect.signature(B.flush).parameters) == ["self", "slots", "blocks"]
    assert list(inspect.signature(G.push).parameters) == ["self", "block"]


def test_header_prototypes_and_exports_agree_on_the_new_entry_points():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    lib = _ffi.load_library()
    for name, nargs in (("sg_stream_push_spectrum", 12), ("sg_stream_bank_frames", 3)):
        m = re.search(r"SG_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_ffi._PROTOTYPES[name][1]), name
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    body = header[header.index("typedef struct sg_stream_spec_rec {"):header.index("} sg_stream_spec_rec;")]
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert fields == [f[0] for f in _ffi.SgStreamSpecRec._fields_] == ["spec_offset", "mask_offset", "stride"]
    assert ctypes.sizeof(_ffi.SgStreamSpecRec) == 24
    # nothing that was there moved
    assert ctypes.sizeof(_ffi.SgStreamRec) == 48 and lib.sg_version() == 100
    assert _ffi.SG_STREAM_HEAD_VERSION == 1 and "#define SG_STREAM_HEAD_VERSION 1" in header
    assert hasattr(_ffi.Gate, "stream_push_spectrum") and hasattr(_ffi.Gate, "stream_bank_frames")


@pytest.mark.parametrize("W,H", [(400, 160), (1024, 256), (1500, 333)])
def test_frames_applied_is_the_brute_force_count(W, H):
    from noisereduce_amd import stream
    h = W // 2
    for lag in (0, 2, 7):
        prev = 0
        for n in range(0, W + 40 * H + 1):
            # frames t whose mask is final: t + lag is a frame that lies inside the first n samples
            brute = sum(1 for t in range(0, 45) if t + lag <= M.t_dec(n, W, H))
            a = stream.frames_applied(n, W, H, lag)
            assert a == brute == SM.frames_applied(n, W, H, lag), (n, lag)
            assert a >= prev
            prev = a
            assert stream.emitted(n, W, H, lag) == M.emitted(n, W, H, lag) == max(0, a * H - h), (n, lag)
    bank = stream.StreamBank(48000, 2, thresholds_db=np.zeros(513), n_fft=1024)
    assert bank.frames(0) == 0 and bank.frames(1) == 0


def test_arguments_are_checked_before_any_device_work():
    import torch
    from noisereduce_amd import stream
    thr = np.zeros(513)
    bank = stream.StreamBank(48000, 2, thresholds_db=thr, max_block=4800)
    z = np.zeros(10, np.float32)
    bad = [lambda: bank.push_spectrum([(0, z), (0, z)]),                               # a slot listed twice
           lambda: bank.push_spectrum([(1, z), (np.int64(1), z)], return_mask=True),
           lambda: bank.flush_spectrum([0, 0]),
           lambda: bank.push_spectrum({0: np.zeros(4801, np.float32)}),                # over max_block
           lambda: bank.push_spectrum({0: torch.zeros(4801)}),
           lambda: bank.push_spectrum({0: z, 1: torch.zeros(10)}),                     # numpy and tensor blocks mixed
           lambda: bank.push_spectrum({0: torch.zeros(10)}),                           # a tensor that is not on the GPU
           lambda: bank.push_spectrum({0: np.zeros(10, np.int16)}),
           lambda: bank.push_spectrum({2: z}),
           lambda: bank.flush_spectrum([0]),                                           # shorter than win_length
           lambda: bank.flush_spectrum([0], {0: np.zeros(1023, np.float32)}, return_mask=True),
           lambda: bank.flush_spectrum([5])]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert bank._bank is None, i
    g = stream.StreamGate(48000, thresholds_db=thr, max_block=4800)
    for f in (lambda: g.push_spectrum(np.zeros(4801, np.float32), return_mask=True), lambda: g.flush_spectrum(),
              lambda: g.flush_spectrum(np.zeros(100, np.float32), return_mask=True)):
        with pytest.raises(ValueError):
            f()
    assert g.bank._bank is None
    nobody = stream.StreamBank(48000, 1)
    with pytest.raises(ValueError):
        nobody.push_spectrum({0: z}, return_mask=True)                                 # no noise profile yet


def _cell_gate(cell, case, u):
    cfg = u["cfg"]
    smooth = cfg["filt"] is not None
    ntl = cfg["nt"] if smooth else 0
    if cell["stationary"]:
        return SM.stationary_gate(u["thresh"], cfg["n_fft"], cfg["W"], cfg["H"], cfg["prop"], cfg["nf"], cfg["nt"], smooth), ntl
    L = int(case["lookahead_ms"] / ((cfg["H"] / PB.SR) * 1000))
    return SM.nonstationary_gate(cfg["n_fft"], cfg["W"], cfg["H"], cfg["prop"], cfg["nf"], cfg["nt"], smooth, cfg["iir_b"], L,
                                 cfg["thresh_n_mult"], cfg["slope"]), ntl + L


@pytest.mark.parametrize("cell", STREAM_CELLS, ids=[PB.tile_cell_id(c) for c in STREAM_CELLS])
def test_model_is_the_offline_gated_spectrogram_and_inverts_to_the_streamed_audio(cell):
    """Step by step, from scratch: the concatenated frames are the oracle's Z * mask of the whole signal, the frame counts
    are A(n1) - A(n0), and O.istft_scipy of them is the audio of the streaming models."""
    case, units = PB.tile_case(cell), PB.tile_oracle(cell)[0]
    u = units[0]
    cfg = u["cfg"]
    W, H = cfg["W"], cfg["H"]
    y = np.atleast_2d(case["y"]).astype(np.float64)[0]
    N = len(y)
    gate, lag = _cell_gate(cell, case, u)
    cuts = case["plans"]["random"]
    blocks = np.split(y, cuts)
    steps = SM.spectrum_model(blocks, gate, W, H, lag)
    assert len(steps) == len(blocks) + 1
    n = a = 0
    for blk, (Yp, mp, Zp) in zip(blocks, steps):
        n += len(blk)
        assert Yp.shape[1] == mp.shape[1] == SM.frames_applied(n, W, H, lag) - a
        a += Yp.shape[1]
    Y = np.concatenate([s[0] for s in steps], axis=1)
    mk = np.concatenate([s[1] for s in steps], axis=1)
    T = SM.frames_total(N, W, H)
    assert Y.shape == u["Z"].shape == (cfg["n_fft"] // 2 + 1, T) and T == case["frames"]
    want = u["Z"] * u["mask"]
    peak = np.max(np.abs(want))
    assert np.max(np.abs(mk - u["mask"])) <= 1e-12
    assert np.max(np.abs(Y - want)) <= PB.F64_REL * peak
    assert not np.any(Y.imag[[0, -1]])
    # ... and the same frames invert to the streamed audio, block plan by block plan
    smooth = cfg["filt"] is not None
    if cell["stationary"]:
        outs, live = M.stream_model(blocks, u["thresh"], cfg["n_fft"], W, H, cfg["prop"], cfg["nf"], cfg["nt"], smooth)
        assert live is False
    else:
        L = lag - (cfg["nt"] if smooth else 0)
        outs = MN.stream_ns_model(blocks, cfg["n_fft"], W, H, cfg["prop"], cfg["nf"], cfg["nt"], smooth, cfg["iir_b"], L,
                                  cfg["thresh_n_mult"], cfg["slope"])
    audio = np.concatenate(outs)
    back = O.istft_scipy(Y, cfg["n_fft"], W, H)
    full = np.zeros(N)
    full[:min(N, len(back))] = back[:N]
    assert np.max(np.abs(full - audio)) <= PB.F64_REL * max(1.0, np.max(np.abs(audio)))


def test_model_reports_frames_under_a_bounded_lookahead_step_by_step():
    """A non-stationary gate with a SHORT lookahead: the frames a step reports never change afterwards, whatever comes
    next -- the model of a stream cut in blocks equals the model of the stream pushed whole."""
    rng = np.random.default_rng(5)
    n_fft, W, H, L = 256, 256, 64, 3
    y = O.synth_signal(W + 30 * H + 7, sr=8000, seed=3).astype(np.float64)
    gate = SM.nonstationary_gate(n_fft, W, H, 0.8, 2, 2, True, 0.3, L)
    lag = 2 + L
    whole = SM.spectrum_model([y], gate, W, H, lag)
    cut = SM.spectrum_model(np.split(y, sorted(rng.integers(0, len(y), 9))), gate, W, H, lag)
    for i in (0, 1):
        a = np.concatenate([s[i] for s in whole], axis=1)
        b = np.concatenate([s[i] for s in cut], axis=1)
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(a))


def test_metric_flags_a_planted_defect_in_exactly_the_frames_it_touches():
    cell = next(c for c in STREAM_CELLS if c["path"] == "stream-S" and c["n_fft"] == 512 and c["col"] == 0)
    u = PB.tile_oracle(cell)[0][0]
    want = u["Z"] * u["mask"]
    T = want.shape[1]
    kw = dict(f64_rel=PB.F64_REL, eps32=PB.EPS32, pool=PB.POOL)
    for narrow, ct in ((False, np.complex128), (True, np.complex64)):
        good = want.astype(ct)
        assert len(SM.bad_frames(good, want, u["Z"], narrow, **kw)) == 0
        loud = int(np.argmax(np.abs(want).max(axis=0)))
        # a wrong scale on one frame (a float32 window sum in place of the float64 one is 1e-7; here 1e-5)
        Y = good.copy()
        Y[:, loud] *= ct(1.0 + 1e-5)
        assert SM.bad_frames(Y, want, u["Z"], narrow, **kw).tolist() == [loud]
        # a Nyquist bin with an imaginary part, however small -- and a negative zero
        for v in (1e-30, -0.0):
            Y = good.copy()
            Y.imag[-1, 7] = v
            assert SM.bad_frames(Y, want, u["Z"], narrow, **kw).tolist() == [7]
        # frame A(n) duplicated at a step seam: every frame from the seam on is its neighbour
        seam = T // 2
        Y = np.concatenate([good[:, :seam + 1], good[:, seam:-1]], axis=1)
        bad = SM.bad_frames(Y, want, u["Z"], narrow, **kw)
        moved = np.flatnonzero(np.abs(want[:, 1:] - want[:, :-1]).max(axis=0) > 0) + 1
        assert len(bad) and bad.min() == seam + 1 and set(bad.tolist()) <= set(moved[moved > seam].tolist())
        assert len(bad) >= 0.9 * np.sum(moved > seam)
