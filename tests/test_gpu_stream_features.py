"""The feature steps of a stream bank on the GPU (StreamBank.set_filterbank / push_features / flush_features,
sg_stream_set_filterbank / sg_stream_push_features): every feature of every reported frame against
the float64 model of tests/stream_features_model.py -- the oracle's Z times the mask the step returned, then the formula --
within the derived bound E of that module, against the engine's own complex128 spectrum within the summation terms alone,
and the invariances of the contract bit for bit.  The stream cases and block plans are tests/test_gpu_stream_spectrum.py's
(tests/parity_budget.py's stream cells), run here as float64 blocks so that the mask comes back unrounded; a float32
twin of every stream must be that result rounded once."""
import numpy as np
import pytest
import torch

from noisereduce_amd import _ffi, stream
from noisereduce_amd.torchgate import mel_filterbank
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_features_model as FM
from tests import stream_spectrum_model as SM

pytestmark = pytest.mark.gpu

_STAGES = {"k_rg_decide", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola"}


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else v


def _run(bank, plans, mode="features", fkw=None, as_tensor=False):
    """plans: {slot: (signal (N,) or (C, N), cuts)}.  Step i pushes every stream's i-th block; then all are flushed.
    mode: "features" / "spectrum" / "push" (every step of that kind) or "alt" (push, push_spectrum, push_features in turn,
    the flush included).  Returns {slot: dict(y, feat, mask, Y, smask, fspans, sspans, steps)}: the concatenated samples;
    the features and masks of the feature steps with the frame ranges they reported; the same of the spectrum steps."""
    fkw = dict(fkw or {})
    blocks = {s: np.split(np.asarray(y), c, axis=-1) for s, (y, c) in plans.items()}
    res = {s: dict(y=[], feat=[], mask=[], Y=[], smask=[], fspans=[], sspans=[]) for s in plans}
    steps = max(len(b) for b in blocks.values())
    W, H = bank.win_length, bank.hop_length

    def kind(i):
        return mode if mode != "alt" else ("push", "spectrum", "features")[i % 3]

    def take(out, before, k, total=None):
        for s, o in out.items():
            r = res[s]
            if k == "push":
                r["y"].append(_np(o))
                continue
            a1 = bank.frames(s) if total is None else total[s]
            assert o[1].shape[-1] == o[2].shape[-1] == a1 - before[s], (s, k, o[1].shape, before[s], a1)
            r["y"].append(_np(o[0]))
            a, b, c = ("feat", "mask", "fspans") if k == "features" else ("Y", "smask", "sspans")
            r[a].append(_np(o[1]))
            r[b].append(_np(o[2]))
            r[c].append((before[s], a1))

    for i in range(steps):
        step = {s: b[i] for s, b in blocks.items() if i < len(b)}
        if as_tensor:
            step = {s: torch.from_numpy(np.ascontiguousarray(v)).cuda() for s, v in step.items()}
        before = {s: bank.frames(s) for s in step}
        k = kind(i)
        out = (bank.push(step) if k == "push" else bank.push_spectrum(step, return_mask=True) if k == "spectrum" else
               bank.push_features(step, return_mask=True, **fkw))
        take(out, before, k)
    before = {s: bank.frames(s) for s in plans}
    total = {s: SM.frames_total(bank.received(s), W, H) for s in plans}
    k = kind(steps)
    out = (bank.flush(list(plans)) if k == "push" else bank.flush_spectrum(list(plans), return_mask=True) if k == "spectrum"
           else bank.flush_features(list(plans), return_mask=True, **fkw))
    take(out, before, k, total)
    fin = {}
    for s, r in res.items():
        cat = lambda v: np.concatenate(v, axis=-1) if v else None      # noqa: E731
        fin[s] = dict(y=cat(r["y"]), feat=cat(r["feat"]), mask=cat(r["mask"]), Y=cat(r["Y"]), smask=cat(r["smask"]),
                      fspans=r["fspans"], sspans=r["sspans"], steps=steps + 1)
    return fin


def _frames_of(spans):
    return np.concatenate([np.arange(a0, a1) for a0, a1 in spans]) if spans else np.zeros(0, int)


def _bank_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("stationary", "chunk_size", "padding")}


def _cell_bank(cell, case, n_slots):
    N, C = case["y"].shape[-1], case["C"]
    if cell["stationary"]:
        return stream.StreamBank(PB.SR, n_slots, channels=C, y_noise=case["y_noise"], max_block=N, **_bank_kw(case["kw"]))
    return stream.StreamBank(PB.SR, n_slots, channels=C, stationary=False, lookahead_ms=case["lookahead_ms"], max_block=N,
                             **_bank_kw(case["kw"]))


def _fkw(c):
    return dict(power=c["power"], log=c["log"], eps=c["eps"], scale=c["scale"])


# ---- 1. the oracle, frame by frame, filter by filter -----------------------------------------------------------------------
@pytest.mark.parametrize("fc", FM.CASES, ids=[FM.case_id(c) for c in FM.CASES])
def test_features_are_the_formula_on_the_oracles_gated_spectrogram(fc):
    cell = fc["cell"]
    case, units = PB.tile_case(cell), PB.tile_oracle(cell)[0]
    tag = FM.case_id(fc)
    y64 = case["y"].astype(np.float64)
    N, C = y64.shape[-1], case["C"]
    F, T = units[0]["Z"].shape
    W = units[0]["cfg"]["W"]
    fb = FM.bank(fc["bank"], cell["n_fft"])
    M = fb.shape[1]
    bank = _cell_bank(cell, case, 5)
    bank.set_filterbank(fb)
    if cell["stationary"]:
        assert np.max(np.abs(bank.thresholds() - units[0]["thresh"])) <= 1e-9
    g = bank.gate
    g.profile_enable(True)
    try:
        g.profile_read(reset=True)
        plans = {s: (y64, case["plans"][k]) for s, k in enumerate(PB.STREAM_PLANS)}
        plans[4] = (y64.astype(np.float32), case["plans"]["prime"])      # (the signals are float32-valued: the same stream)
        got = _run(bank, plans, fkw=_fkw(fc))
        launched = {k.split(" ")[0]: v[1] for k, v in g.profile_read(reset=True).items() if v[1] > 0}
    finally:
        g.profile_enable(False)
    steps = got[0]["steps"]
    assert launched == {k: steps for k in _STAGES}, (tag, steps, launched)      # the same four stages, once each per step
    fshape, mshape = ((M, T), (F, T)) if C == 1 else ((C, M, T), (C, F, T))
    for s in range(4):
        r = got[s]
        assert r["feat"].shape == fshape and r["feat"].dtype == np.float64, (tag, s, r["feat"].shape, r["feat"].dtype)
        assert r["mask"].shape == mshape and r["mask"].dtype == np.float64
        assert r["y"].shape == y64.shape and r["y"].dtype == np.float64
        assert r["fspans"][0][0] == 0 and r["fspans"][-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(r["fspans"], r["fspans"][1:]))
        if s:
            for key in ("y", "feat", "mask"):
                assert np.array_equal(r[key], got[0][key], equal_nan=True), "%s: %s of block plan %r differs from the " \
                    "whole stream's" % (tag, key, PB.STREAM_PLANS[s])
    r32 = got[4]
    assert r32["feat"].dtype == np.float32 and r32["mask"].dtype == np.float32 and r32["y"].dtype == np.float32
    assert np.array_equal(r32["feat"], got[0]["feat"].astype(np.float32), equal_nan=True)
    assert np.array_equal(r32["mask"], got[0]["mask"].astype(np.float32), equal_nan=True)
    F3, M3, F32 = got[0]["feat"].reshape(C, M, T), got[0]["mask"].reshape(C, F, T), r32["feat"].reshape(C, M, T)
    for ch, u in enumerate(units):
        for feat, what in ((F3[ch], "float64"), (F32[ch], "float32")):
            bad = FM.check("%s channel %d %s" % (tag, ch, what), feat, u["Z"], M3[ch], fb, fc["power"], fc["scale"],
                           fc["log"], fc["eps"], W)
            assert len(bad) == 0, "%s channel %d %s: %d cells over their bound, first (m, t) %s" % (
                tag, ch, what, len(bad), bad[:6].tolist())
    bank.close()


# ---- 2. the engine's own spectrum: the summation terms alone ---------------------------------------------------------------
@pytest.mark.parametrize("fc", FM.CASES, ids=[FM.case_id(c) for c in FM.CASES])
def test_features_are_the_formula_on_the_engines_own_spectrum(fc):
    cell = fc["cell"]
    case = PB.tile_case(cell)
    tag = FM.case_id(fc)
    y64 = case["y"].astype(np.float64)
    C = case["C"]
    fb = FM.bank(fc["bank"], cell["n_fft"])
    cuts = case["plans"]["random"]
    a, b = _cell_bank(cell, case, 1), _cell_bank(cell, case, 1)
    a.set_filterbank(fb)
    fa = _run(a, {0: (y64, cuts)}, fkw=_fkw(fc))[0]
    sb = _run(b, {0: (y64, cuts)}, mode="spectrum")[0]
    assert sb["Y"].dtype == np.complex128 and fa["feat"].dtype == np.float64
    assert np.array_equal(fa["mask"], sb["smask"], equal_nan=True) and np.array_equal(fa["y"], sb["y"], equal_nan=True)
    assert fa["fspans"] == sb["sspans"]
    F, T = sb["Y"].shape[-2:]
    M = fb.shape[1]
    Y3, F3 = sb["Y"].reshape(C, F, T), fa["feat"].reshape(C, M, T)
    for ch in range(C):
        bad = FM.check("%s channel %d, own Y" % (tag, ch), F3[ch], None, None, fb, fc["power"], fc["scale"], fc["log"],
                       fc["eps"], a.win_length, engine_Y=Y3[ch])
        assert len(bad) == 0, "%s channel %d: %d cells beyond the summation terms, first (m, t) %s" % (
            tag, ch, len(bad), bad[:6].tolist())
    a.close()
    b.close()


# ---- 1b. the other bank kinds: bounded lookahead, adaptive, precision="float64" with int16 blocks --------------------------
@pytest.mark.parametrize("kind", ["nonstationary-short", "adaptive", "exact-int16"])
def test_features_of_the_other_bank_kinds_against_the_oracles_transform(kind):
    sr, n_fft, W, H = 16000, 512, 400, 160
    N = W + 37 * H + 11
    rng = np.random.default_rng(19)
    y = O.synth_signal(N, sr=sr, seed=21, dtype=np.float32)
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H, max_block=N)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, 6))
    if kind == "nonstationary-short":
        bank = stream.StreamBank(sr, 2, stationary=False, lookahead_ms=3.5 * H / sr * 1000, time_constant_s=0.1, **kw)
        assert bank.lookahead_frames == 3
        plans, fc = {0: (y, cuts), 1: (y.astype(np.float64), cuts)}, dict(bank="mel40", power=2, scale="scipy", log=True, eps=1e-10)
    elif kind == "adaptive":
        bank = stream.StreamBank(sr, 2, noise_from_stream=True, noise_memory_s=0.5, **kw)
        plans, fc = {0: (y, cuts), 1: (y.astype(np.float64), cuts)}, dict(bank="wide300", power=1, scale="torch", log=False, eps=1e-6)
    else:
        bank = stream.StreamBank(sr, 2, y_noise=0.1 * rng.standard_normal(sr // 2), precision="float64", **kw)
        yi = np.round(y * 20000.0).astype(np.int16)
        plans, fc = {0: (yi, cuts), 1: (yi.astype(np.float64), cuts)}, dict(bank="zero_nyq", power=2, scale="scipy", log=True, eps=1e-10)
    fb = FM.bank(fc["bank"], n_fft, sr)
    bank.set_filterbank(fb)
    lag = bank.nt + bank.lookahead_frames
    got = _run(bank, plans, fkw=_fkw(fc))
    r = got[1]
    n = a = 0
    for blk, (a0, a1) in zip(np.split(plans[1][0], cuts), r["fspans"]):      # the frame counts of every step
        n += len(blk)
        assert (a0, a1) == (a, SM.frames_applied(n, W, H, lag)), (kind, n, a0, a1)
        a = a1
    T = SM.frames_total(N, W, H)
    assert r["fspans"][-1] == (a, T) and r["feat"].shape == (fb.shape[1], T) and r["feat"].dtype == np.float64
    if kind == "exact-int16":      # float64 for an int16 block too, and bit for bit the float64 twin's
        assert got[0]["feat"].dtype == np.float64 and got[0]["y"].dtype == np.int16
        assert np.array_equal(got[0]["feat"], r["feat"]) and np.array_equal(got[0]["mask"], r["mask"])
    else:
        assert got[0]["feat"].dtype == np.float32
        assert np.array_equal(got[0]["feat"], r["feat"].astype(np.float32), equal_nan=True)
    Z = SM.transform(np.asarray(plans[1][0], dtype=np.float64), T, n_fft, W, H)
    for feat in (r["feat"], got[0]["feat"]):
        bad = FM.check("%s %s" % (kind, feat.dtype), feat, Z, r["mask"], fb, fc["power"], fc["scale"], fc["log"], fc["eps"], W)
        assert len(bad) == 0, (kind, len(bad), bad[:6].tolist())
    bank.close()


# ---- 1c. the order of the sum -----------------------------------------------------------------------------------------------
def test_filters_sum_in_ascending_k():
    """Partial sums that overflow in ascending order and not in descending (tests/stream_features_model.py's order case)."""
    oc = FM.order_case()
    y, n_fft, W, H = oc["y"], oc["n_fft"], oc["W"], oc["H"]
    bank = stream.StreamBank(PB.SR, 1, thresholds_db=np.zeros(n_fft // 2 + 1), n_fft=n_fft, freq_mask_smooth_hz=None,
                             time_mask_smooth_ms=None, max_block=len(y), precision="float64")
    bank.set_filterbank(oc["fb"])
    r = _run(bank, {0: (y, [777, 3000])}, fkw=dict(power=2, scale="torch"))[0]
    T = SM.frames_total(len(y), W, H)
    Z = SM.transform(y, T, n_fft, W, H)
    bad, want, inside = FM.order_bad(r["feat"], Z, r["mask"], oc)
    assert len(bad) == 0, (bad[:6].tolist(), r["feat"][:, inside][:, :4], want[:, inside][:, :4])
    assert np.all(np.isinf(r["feat"][0, inside])) and np.all(np.isfinite(r["feat"][1, inside]))
    bank.close()


# ---- 3. bitwise invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stationary", [True, False], ids=["S", "NS"])
def test_features_do_not_depend_on_split_slot_company_or_kind_of_step(stationary):
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(41)
    N = W + 29 * H + 3
    y = O.synth_signal(N, sr=sr, seed=5, dtype=np.float32)
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H, max_block=2 * N)
    if stationary:
        kw["y_noise"] = 0.1 * rng.standard_normal(sr // 2)
    else:
        kw.update(stationary=False, lookahead_ms=2.5 * H / sr * 1000, time_constant_s=0.1)
    fb = mel_filterbank(sr, n_fft, 40)
    fkw = dict(power=2, log=True)
    splits = [[], sorted(int(c) for c in rng.integers(0, N + 1, 8)), [H - 1, H - 1, H, W + 1, W + 2, 3 * W + 7],
              list(range(333, N, 333))]      # whole; random; 0, 1, H - 1 samples and more than win_length; odd

    def bank_of(n):
        b = stream.StreamBank(sr, n, **kw)
        b.set_filterbank(fb)
        return b

    alone_bank = bank_of(1)
    alone = _run(alone_bank, {0: (y, splits[1])}, fkw=fkw)[0]
    alone_bank.close()
    T = SM.frames_total(N, W, H)
    assert alone["feat"].shape == (40, T) and alone["feat"].dtype == np.float32
    # three more block splits, in slots 0 .. 2 of one bank
    b3 = bank_of(3)
    got = _run(b3, {0: (y, splits[0]), 1: (y, splits[2]), 2: (y, splits[3])}, fkw=fkw)
    b3.close()
    for s in range(3):
        for key in ("y", "feat", "mask"):
            assert np.array_equal(got[s][key], alone[key], equal_nan=True), (s, key)
    # slot 5 among seven busy streams of other lengths, types and splits (one carries a NaN)
    b7 = bank_of(7)
    plans = {5: (y, splits[1])}
    for s in (0, 1, 2, 3, 4, 6):
        n = int(rng.integers(W, 2 * N))
        v = O.synth_signal(n, sr=sr, seed=100 + s, dtype=(np.float32, np.float64)[s % 2])
        if s == 3:
            v[n // 3] = np.nan
        plans[s] = (v, PB.stream_cuts(PB.STREAM_PLANS[s % 4], n, W, H, rng))
    got = _run(b7, plans, fkw=fkw)
    b7.close()
    for key in ("y", "feat", "mask"):
        assert got[5][key].dtype == np.float32 and np.array_equal(got[5][key], alone[key], equal_nan=True), key
    assert got[1]["feat"].dtype == np.float64 and got[2]["feat"].dtype == np.float32      # each slot its own type
    assert np.isnan(got[3]["feat"]).any() and not np.isnan(got[5]["feat"]).any()
    # push / push_spectrum / push_features in turn: the shared frames, the samples of push, the mask of push_spectrum
    runs = {}
    for mode in ("push", "spectrum", "alt"):
        b = bank_of(1)
        runs[mode] = _run(b, {0: (y, splits[3])}, mode=mode, fkw=fkw)[0]
        b.close()
    alt = runs["alt"]
    for mode in ("push", "spectrum", "alt"):
        assert np.array_equal(runs[mode]["y"], alone["y"], equal_nan=True), mode
    fi, si = _frames_of(alt["fspans"]), _frames_of(alt["sspans"])
    assert 0 < len(fi) < T and 0 < len(si) < T and not set(fi) & set(si)
    assert np.array_equal(alt["feat"], alone["feat"][:, fi], equal_nan=True)
    assert np.array_equal(alt["mask"], runs["spectrum"]["smask"][:, fi], equal_nan=True)
    assert np.array_equal(alone["mask"], runs["spectrum"]["smask"], equal_nan=True)
    assert np.array_equal(alt["Y"], runs["spectrum"]["Y"][:, si], equal_nan=True)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
def test_edges():
    sr, n_fft = 48000, 1024
    W, H, F = 1024, 256, 513
    rng = np.random.default_rng(43)
    noise = 0.1 * rng.standard_normal(sr // 2)
    N = W + 20 * H + 9
    y = O.synth_signal(N, sr=sr, seed=9, dtype=np.float32)
    fb = FM.bank("zero_nyq", n_fft)
    M = fb.shape[1]
    bank = stream.StreamBank(sr, 3, n_fft=n_fft, y_noise=noise, max_block=N)
    # no filterbank yet: the Python layer raises, and so does the C entry point itself (SG_E_INVALID -> ValueError)
    with pytest.raises(ValueError, match="no filterbank set"):
        bank.push_features({0: y[:100]})
    g = bank.gate
    x = torch.zeros(100, device="cuda")
    rec = [_ffi.SgStreamRec(slot=0, flush=0, n_samples=100, in_offset=0, in_stride=100, out_offset=0, out_stride=0)]
    frec = [_ffi.SgStreamFeatRec(feat_offset=0, feat_stride=0, mask_offset=0, mask_stride=0)]
    with pytest.raises(ValueError, match="no filterbank set"):
        g.stream_push_features(bank._bank, x, torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), None, rec, frec,
                               2, 0, 1e-10, 0.0)
    arr, farr = (_ffi.SgStreamRec * 1)(*rec), (_ffi.SgStreamFeatRec * 1)(*frec)
    rc = g.lib.sg_stream_push_features(bank._bank, x.data_ptr(), _ffi.SG_F32, x.data_ptr(), _ffi.SG_F32, x.data_ptr(),
                                       _ffi.SG_F32, None, 2, 0, 1e-10, 0.0, arr, farr, 1, g._stream())
    assert rc == _ffi.SG_E_INVALID and bank.received(0) == 0
    bank.set_filterbank(fb)
    nt = bank.nt
    assert nt > 0
    whole = _run(bank, {0: (y, [])}, fkw=dict(log=True))[0]
    T = SM.frames_total(N, W, H)
    assert whole["feat"].shape == (M, T) and whole["feat"].dtype == np.float32
    # the all-zero filter: ln(eps) rounded to the type, or exactly 0
    assert np.all(whole["feat"][1] == np.float32(np.log(1e-10)))
    lin = _run(bank, {0: (y, [])}, fkw=dict(log=False))[0]
    assert np.all(lin["feat"][1] == 0) and not np.any(np.signbit(lin["feat"][1]))
    wide = _run(bank, {0: (y.astype(np.float64), [])}, fkw=dict(log=True, eps=1e-3))[0]
    assert wide["feat"].dtype == np.float64 and np.all(wide["feat"][1] == wide["feat"][1, 0])
    assert abs(wide["feat"][1, 0] - np.log(1e-3)) <= 4 * 2.0 ** -52 * abs(np.log(1e-3))      # (the log's four ulp)
    # steps of 0 and 1 samples around the sample that completes the first applied frame: (M, 0) where no frame is applied
    e = nt * H - W // 2 + W
    cuts = [e - 2, e - 1, e - 1, e, e, e + 1, N // 2, N // 2]
    n = a = 0
    parts = []
    for blk in np.split(y, cuts):
        n += len(blk)
        s, f, m = bank.push_features({1: blk}, log=True, return_mask=True)[1]
        a1 = SM.frames_applied(n, W, H, nt)
        assert f.shape == (M, a1 - a) and m.shape == (F, a1 - a) and f.dtype == m.dtype == np.float32, (n, f.shape)
        assert len(s) == stream.emitted(n, W, H, nt) - stream.emitted(n - len(blk), W, H, nt)
        assert bank.frames(1) == a1
        a = a1
        parts.append(f)
    assert [v.shape[1] for v in parts[:5]] == [0, 0, 0, 1, 0]
    s, f = bank.flush_features([1], log=True)[1]      # a flush with no last block reports up to frames_total
    parts.append(f)
    assert np.array_equal(np.concatenate(parts, axis=1), whole["feat"]) and bank.frames(1) == 0
    # a refused filterbank leaves the earlier one answering, bit for bit; a replaced one answers as itself
    broken = fb.copy()
    broken[7, 0] = np.inf
    with pytest.raises(ValueError):
        bank.set_filterbank(broken)
    with pytest.raises(ValueError, match="non-finite"):
        g.stream_set_filterbank(bank._bank, broken)      # the C entry point itself
    again = _run(bank, {2: (y, [N // 3])}, fkw=dict(log=True))[2]
    assert np.array_equal(again["feat"], whole["feat"])
    mel = mel_filterbank(sr, n_fft, 40)
    bank.set_filterbank(mel)
    other = stream.StreamBank(sr, 1, n_fft=n_fft, y_noise=noise, max_block=N)
    other.set_filterbank(mel)      # (pending until its first step)
    r0, r1 = _run(bank, {0: (y, [N // 2])}, fkw=dict(log=True))[0], _run(other, {0: (y, [])}, fkw=dict(log=True))[0]
    assert r0["feat"].shape == (40, T) and np.array_equal(r0["feat"], r1["feat"])
    other.close()
    # device tensors in, device tensors out: feat is the transposed view of (k, M) storage, filters contiguous
    yt = torch.from_numpy(np.stack([y, y[::-1].copy()])).cuda()
    two = stream.StreamBank(sr, 1, channels=2, n_fft=n_fft, y_noise=noise, max_block=N)
    two.set_filterbank(mel)
    s, f, m = two.push_features({0: yt[:, :N // 2]}, log=True, return_mask=True)[0]
    k = SM.frames_applied(N // 2, W, H, nt)
    for v, R in ((f, 40), (m, F)):
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (2, R, k)
        assert v.stride(-2) == 1 and v.stride(-1) == R and v.transpose(-1, -2).is_contiguous()
    s2, f2 = two.flush_features([0], {0: yt[:, N // 2:]}, log=True)[0]
    assert isinstance(f2, torch.Tensor) and f2.is_cuda and tuple(f2.shape) == (2, 40, T - k)
    assert np.array_equal(torch.cat([f, f2], dim=-1)[0].cpu().numpy(), r0["feat"])
    two.close()
    # a mixed float32 / float64 step gives each slot its own type
    mixed = bank.push_features({0: y[:4 * W], 1: y[:4 * W].astype(np.float64)}, log=True)
    assert mixed[0][1].dtype == np.float32 and mixed[1][1].dtype == np.float64 and mixed[0][0].dtype == np.float32
    assert np.array_equal(mixed[0][1], mixed[1][1].astype(np.float32))
    bank.reset([0, 1])
    # a StreamGate: the same frames
    sg = stream.StreamGate(sr, y_noise=noise, n_fft=n_fft, max_block=N)
    sg.set_filterbank(mel)
    a = sg.push_features(y[:N // 3], log=True)
    b = sg.flush_features(y[N // 3:], log=True, return_mask=True)
    assert len(a) == 2 and len(b) == 3
    assert np.array_equal(np.concatenate([a[1], b[1]], axis=1), r0["feat"])
    assert np.array_equal(np.concatenate([a[0], b[0]]), r0["y"])
    sg.close()
    bank.close()


# ---- 5. a moved stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stationary", [True, False], ids=["S", "NS"])
def test_a_moved_stream_continues_its_features_bit_for_bit(stationary):
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(47)
    N = W + 31 * H + 7
    y = O.synth_signal(N, sr=sr, seed=13, dtype=np.float32)
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H)
    if stationary:
        kw["y_noise"] = 0.1 * rng.standard_normal(sr // 2)
    else:
        kw.update(stationary=False, lookahead_ms=2.5 * H / sr * 1000, time_constant_s=0.1)
    fb = mel_filterbank(sr, n_fft, 23)
    fkw = dict(power=1, log=True, scale="torch", eps=1e-6)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, 7))
    blocks = np.split(y, cuts)
    home = stream.StreamBank(sr, 2, max_block=N, **kw)
    home.set_filterbank(fb)
    stay = _run(home, {1: (y, cuts)}, fkw=fkw)[1]
    parts = dict(y=[], feat=[], mask=[])

    def take(o):
        for key, v in zip(("y", "feat", "mask"), o):
            parts[key].append(v)

    for blk in blocks[:4]:
        take(home.push_features({0: blk}, return_mask=True, **fkw)[0])
    state = home.snapshot([0])[0]
    away = stream.StreamBank(sr, 3, max_block=N // 2 + 100, **kw)
    away.set_filterbank(fb)      # the filterbank is the bank's, not the stream's: the destination holds the same one
    away.restore({2: state})
    assert away.frames(2) == home.frames(0) and away.received(2) == home.received(0)
    for blk in blocks[4:]:
        for piece in np.array_split(blk, 3):      # (the other bank's max_block is smaller)
            take(away.push_features({2: piece}, return_mask=True, **fkw)[2])
    take(away.flush_features([2], return_mask=True, **fkw)[2])
    for key in ("y", "feat", "mask"):
        assert np.array_equal(np.concatenate(parts[key], axis=-1), stay[key], equal_nan=True), key
    home.close()
    away.close()
