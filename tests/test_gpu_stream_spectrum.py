"""The spectrum steps of a stream bank on the GPU (StreamBank.push_spectrum / flush_spectrum, sg_stream_push_spectrum):
every reported frame against the float64 oracle's Z * mask, the causal floor against the streaming model, the frames
against the audio of the same run on every bank kind, and the invariances of the contract bit for bit.

Per frame t, with want = Z * (the mask the step returned) in float64:
  complex128:  max_k |Y - want| <= F64_REL * max(frame peak of |Z|, 1e-3 * global peak)
  complex64:   that plus 4 * EPS32 * max_k |want|, pooled over t - POOL .. t + POOL
(tests/stream_spectrum_model.py's frame_bound; the constants are tests/parity_budget.py's).  The transforms and the mask are
float64 on the device, so only the output's own rounding is allowed."""
import numpy as np
import pytest
import torch

from noisereduce_amd import stream
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_spectrum_model as SM

pytestmark = pytest.mark.gpu

DEVICE_TOL = 2e-6      # of peak: tests/test_gpu_stream.py's bound for float32 audio
_STAGES = {"k_rg_decide", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola"}
_KW = dict(f64_rel=PB.F64_REL, eps32=PB.EPS32, pool=PB.POOL)
_CELLS = [c for c in PB.TILE_CELLS if c["path"].startswith("stream")]


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else v


def _run(bank, plans, mode="spectrum", return_mask=True, as_tensor=False):
    """plans: {slot: (signal (N,) or (C, N), cuts)}.  Step i pushes every stream's i-th block; then all are flushed.
    mode: "spectrum" (every step a spectrum step), "push" (none), "alt" (every other one, the flush included or not by
    parity).  Returns {slot: dict(y, Y, mask, spans)}: the concatenated samples, frames and masks, and ``spans`` = the frame
    range (a0, a1) every spectrum step reported, in order."""
    blocks = {s: np.split(np.asarray(y), c, axis=-1) for s, (y, c) in plans.items()}
    res = {s: dict(y=[], Y=[], mask=[], spans=[], counts=[]) for s in plans}
    steps = max(len(b) for b in blocks.values())

    def take(out, before, spec, total=None):
        for s, o in out.items():
            r = res[s]
            if not spec:
                r["y"].append(_np(o))
                continue
            r["y"].append(_np(o[0]))
            r["Y"].append(_np(o[1]))
            if return_mask:
                r["mask"].append(_np(o[2]))
            a1 = bank.frames(s) if total is None else total[s]
            r["spans"].append((before[s], a1))
            assert o[1].shape[-1] == a1 - before[s], (s, o[1].shape, before[s], a1)

    for i in range(steps):
        step = {s: b[i] for s, b in blocks.items() if i < len(b)}
        if as_tensor:
            step = {s: torch.from_numpy(np.ascontiguousarray(v)).cuda() for s, v in step.items()}
        before = {s: bank.frames(s) for s in step}
        spec = mode == "spectrum" or (mode == "alt" and i % 2 == 0)
        take(bank.push_spectrum(step, return_mask=return_mask) if spec else bank.push(step), before, spec)
    before = {s: bank.frames(s) for s in plans}
    W, H = bank.win_length, bank.hop_length
    total = {s: SM.frames_total(bank.received(s), W, H) for s in plans}
    spec = mode == "spectrum" or (mode == "alt" and steps % 2 == 0)
    take(bank.flush_spectrum(list(plans), return_mask=return_mask) if spec else bank.flush(list(plans)), before, spec, total)
    out = {}
    for s, r in res.items():
        out[s] = dict(y=np.concatenate(r["y"], axis=-1), spans=r["spans"], steps=steps + 1,
                      Y=np.concatenate(r["Y"], axis=-1) if r["Y"] else None,
                      mask=np.concatenate(r["mask"], axis=-1) if r["mask"] else None)
    return out


def _bank_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("stationary", "chunk_size", "padding")}


def _check_frames(tag, Y, Mret, u):
    """One channel's frames against Z * (returned mask), per frame."""
    narrow = Y.dtype == np.complex64
    assert Y.shape == u["Z"].shape and Mret.shape == u["Z"].shape, (tag, Y.shape, Mret.shape, u["Z"].shape)
    want = u["Z"] * Mret.astype(np.float64)
    err, ok = SM.frame_error(Y, want), SM.frame_bound(want, u["Z"], narrow, **_KW)
    print("%s: largest frame error / bound %.3g" % (tag, float(np.max(err / ok))))
    bad = SM.bad_frames(Y, want, u["Z"], narrow, **_KW)
    assert len(bad) == 0, "%s: frames %s of %d over their bound: error %s, bound %s" % (
        tag, bad[:10].tolist(), Y.shape[1], err[bad[:10]], ok[bad[:10]])


# ---- 1. the oracle, per frame ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", _CELLS, ids=[PB.tile_cell_id(c) for c in _CELLS])
def test_frames_are_the_oracles_gated_spectrogram(cell):
    case, units = PB.tile_case(cell), PB.tile_oracle(cell)[0]
    tag = PB.tile_cell_id(cell)
    dt = np.dtype(case["dtype"])
    ct, rt = (np.complex64, np.float32) if dt == np.float32 else (np.complex128, np.float64)
    y = case["y"].astype(dt)
    N, C = y.shape[-1], case["C"]
    F, T = units[0]["Z"].shape
    if cell["stationary"]:
        bank = stream.StreamBank(PB.SR, 4, channels=C, y_noise=case["y_noise"], max_block=N, **_bank_kw(case["kw"]))
        assert np.max(np.abs(bank.thresholds() - units[0]["thresh"])) <= 1e-9
    else:
        bank = stream.StreamBank(PB.SR, 4, channels=C, stationary=False, lookahead_ms=case["lookahead_ms"], max_block=N,
                                 **_bank_kw(case["kw"]))
        assert bank.lookahead_frames >= case["frames"] - 1
    g = bank.gate
    g.profile_enable(True)
    try:
        g.profile_read(reset=True)
        got = _run(bank, {s: (y, case["plans"][k]) for s, k in enumerate(PB.STREAM_PLANS)})
        launched = {k.split(" ")[0]: v[1] for k, v in g.profile_read(reset=True).items() if v[1] > 0}
    finally:
        g.profile_enable(False)
    steps = got[0]["steps"]
    assert launched == {k: steps for k in _STAGES}, (tag, steps, launched)
    shape = (F, T) if C == 1 else (C, F, T)
    for s, k in enumerate(PB.STREAM_PLANS):
        r = got[s]
        assert r["y"].shape == y.shape and r["y"].dtype == dt, (tag, k)
        assert r["Y"].shape == shape and r["Y"].dtype == ct, (tag, k, r["Y"].shape, r["Y"].dtype)
        assert r["mask"].shape == shape and r["mask"].dtype == rt, (tag, k, r["mask"].shape, r["mask"].dtype)
        assert r["spans"][0][0] == 0 and r["spans"][-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(r["spans"], r["spans"][1:]))
        if s:
            for key in ("y", "Y", "mask"):
                assert np.array_equal(r[key], got[0][key], equal_nan=True), "%s: %s of block plan %r differs from the " \
                    "whole stream's" % (tag, key, k)
    Y3, M3 = got[0]["Y"].reshape(C, F, T), got[0]["mask"].reshape(C, F, T)
    assert not np.any(Y3.imag[:, [0, -1], :]) and not np.any(np.signbit(Y3.imag[:, [0, -1], :]))
    for ch, u in enumerate(units):
        _check_frames("%s channel %d" % (tag, ch), Y3[ch], M3[ch], u)
        if cell["stationary"]:
            cells, w = PB.mask_diff(M3[ch], u, bound=PB.mask_bound(u["cfg"]))
            assert len(cells) == 0, "%s channel %d: final mask off by up to %.3g (bound %.3g) at %d cells, first %s" % (
                tag, ch, w, PB.mask_bound(u["cfg"]), len(cells), cells[:6].tolist())
        else:
            emu = PB.emulate_stages_f32(u)
            PB._field_rule(M3[ch], u["mask"], emu[2], "%s channel %d final mask" % (tag, ch))
    bank.close()


# ---- 2. the causal floor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [256, 4096])
def test_frames_under_the_causal_floor_are_the_streaming_models(n_fft):
    cf = PB.causal_floor_case(n_fft)
    u, y = cf["unit"], cf["y"]
    N = len(y)
    bank = stream.StreamBank(PB.SR, 1, y_noise=cf["noise"], max_block=N, **_bank_kw(cf["kw"]))
    assert np.max(np.abs(bank.thresholds() - u["thresh"])) <= 1e-9
    rng = np.random.default_rng(n_fft)
    r = _run(bank, {0: (y, PB.stream_cuts("random", N, u["cfg"]["W"], u["cfg"]["H"], rng))})[0]
    assert r["Y"].dtype == np.complex64
    _check_frames("causal-%d" % n_fft, r["Y"], r["mask"], u)
    cells, w = PB.mask_diff(r["mask"], u, bound=PB.mask_bound(u["cfg"]))
    assert len(cells) == 0, (w, cells[:6].tolist())
    # ... and not the offline oracle's: the floor is live in this input
    assert len(PB.mask_diff(r["mask"], cf["offline"], bound=PB.mask_bound(u["cfg"]))[0]) > 0
    bank.close()


# ---- 3. the frames invert to the audio of the same run, on every bank kind ---------------------------------------------
def _istft(Y, N, n_fft, W, H):
    with np.errstate(invalid="ignore"):
        back = O.istft_scipy(Y.astype(np.complex128), n_fft, W, H)
    full = np.zeros(N)
    full[:min(N, len(back))] = back[:N]
    return full


@pytest.mark.parametrize("kind", ["fixed", "nonstationary", "adaptive", "exact"])
def test_frames_invert_to_the_audio_of_the_same_run(kind):
    sr, n_fft, W, H = 16000, 512, 400, 160
    N = W + 37 * H + 11
    rng = np.random.default_rng(17)
    y = O.synth_signal(N, sr=sr, seed=21, dtype=np.float32)
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H, max_block=N)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, 6))
    if kind == "fixed":
        bank = stream.StreamBank(sr, 2, y_noise=0.1 * rng.standard_normal(sr // 2), **kw)
        plans = {1: (y, cuts)}
    elif kind == "nonstationary":
        bank = stream.StreamBank(sr, 2, stationary=False, lookahead_ms=3.5 * H / sr * 1000, time_constant_s=0.1, **kw)
        assert bank.lookahead_frames == 3
        plans = {1: (y, cuts)}
    elif kind == "adaptive":
        bank = stream.StreamBank(sr, 2, noise_from_stream=True, noise_memory_s=0.5, **kw)
        plans = {1: (y, cuts)}
    else:
        bank = stream.StreamBank(sr, 2, y_noise=0.1 * rng.standard_normal(sr // 2), precision="float64", **kw)
        yi = np.round(y * 20000.0).astype(np.int16)
        plans = {0: (yi, cuts), 1: (yi.astype(np.float64), cuts)}
    lag = bank.nt + bank.lookahead_frames
    got = _run(bank, plans)
    r = got[1]
    # the frame counts of every step
    n = a = 0
    for blk, (a0, a1) in zip(np.split(plans[1][0], cuts), r["spans"]):
        n += len(blk)
        assert (a0, a1) == (a, SM.frames_applied(n, W, H, lag)), (kind, n, a0, a1)
        a = a1
    assert r["spans"][-1] == (a, SM.frames_total(N, W, H))
    im = r["Y"].imag[[0, -1], :]
    assert not np.any(im) and not np.any(np.signbit(im))
    back = _istft(r["Y"], N, n_fft, W, H)
    peak = float(np.max(np.abs(r["y"])))
    if kind == "exact":
        assert r["Y"].dtype == np.complex128 and r["y"].dtype == np.float64
        tol = PB.F64_REL
        # the int16 slot: the same frames, bit for bit, and its samples are the float64 ones truncated
        assert got[0]["Y"].dtype == np.complex128 and got[0]["y"].dtype == np.int16
        assert np.array_equal(got[0]["Y"], r["Y"]) and np.array_equal(got[0]["mask"], r["mask"])
        assert np.array_equal(got[0]["y"], np.trunc(r["y"]).astype(np.int16))
    else:
        assert r["Y"].dtype == np.complex64 and r["y"].dtype == np.float32
        tol = DEVICE_TOL
    err = float(np.max(np.abs(back - r["y"].astype(np.float64)))) / peak
    print("[spectrum] %s: istft(Y) against the samples of the run: %.3g of peak (bound %.3g)" % (kind, err, tol))
    assert err <= tol, (kind, err)
    bank.close()


# ---- 4. no behaviour change, free mixing -------------------------------------------------------------------------------
@pytest.mark.parametrize("stationary", [True, False], ids=["S", "NS"])
def test_push_and_push_spectrum_mix_freely(stationary):
    sr, n_fft, W, H = 48000, 1024, 1024, 256
    N = W + 33 * H + 5
    rng = np.random.default_rng(23)
    y = np.stack([O.synth_signal(N, sr=sr, seed=31 + c, dtype=np.float32) for c in range(2)])
    cuts = list(range(300, N, 301))
    kw = dict(n_fft=n_fft, channels=2, max_block=N)
    if stationary:
        kw["y_noise"] = 0.1 * rng.standard_normal(sr // 2)
    else:
        kw.update(stationary=False, lookahead_ms=4.2 * H / sr * 1000, time_constant_s=0.05)
    runs = {}
    for mode in ("push", "spectrum", "alt"):
        bank = stream.StreamBank(sr, 1, **kw)
        runs[mode] = _run(bank, {0: (y, cuts)}, mode=mode)[0]
        bank.close()
    assert np.array_equal(runs["push"]["y"], runs["spectrum"]["y"], equal_nan=True)
    assert np.array_equal(runs["push"]["y"], runs["alt"]["y"], equal_nan=True)
    full, alt = runs["spectrum"], runs["alt"]
    assert full["Y"].shape[-1] == SM.frames_total(N, W, H) and 0 < alt["Y"].shape[-1] < full["Y"].shape[-1]
    idx = np.concatenate([np.arange(a0, a1) for a0, a1 in alt["spans"]])
    assert len(idx) == alt["Y"].shape[-1]
    assert np.array_equal(alt["Y"], full["Y"][..., idx], equal_nan=True)
    assert np.array_equal(alt["mask"], full["mask"][..., idx], equal_nan=True)


# ---- 5. independence ---------------------------------------------------------------------------------------------------
def test_frames_do_not_depend_on_the_slot_or_on_the_other_streams():
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(41)
    noise = 0.1 * rng.standard_normal(sr // 2)
    N = W + 29 * H + 3
    y = O.synth_signal(N, sr=sr, seed=5, dtype=np.float32)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, 8))
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H, y_noise=noise, max_block=2 * N)
    alone_bank = stream.StreamBank(sr, 1, **kw)
    alone = _run(alone_bank, {0: (y, cuts)})[0]
    alone_bank.close()
    assert alone["Y"].dtype == np.complex64
    for companions in (np.float32, np.float64, None):      # all float32, all float64, alternating -- one carries a NaN
        bank = stream.StreamBank(sr, 40, **kw)
        plans = {37: (y, cuts)}
        for s in range(40):
            if s == 37:
                continue
            n = int(rng.integers(W, 2 * N))
            dt = companions or (np.float32, np.float64)[s % 2]
            v = O.synth_signal(n, sr=sr, seed=100 + s, dtype=dt)
            if s == 5:
                v[n // 3] = np.nan
            plans[s] = (v, PB.stream_cuts(PB.STREAM_PLANS[s % 4], n, W, H, rng))
        got = _run(bank, plans)
        bank.close()
        r = got[37]
        assert r["Y"].dtype == np.complex64 and r["mask"].dtype == np.float32 and r["y"].dtype == np.float32
        for key in ("y", "Y", "mask"):
            assert np.array_equal(r[key], alone[key], equal_nan=True), (companions, key)
        assert np.isnan(got[5]["Y"]).any() and not np.isnan(r["Y"]).any()
        assert got[4]["Y"].dtype == (np.complex64 if (companions or np.float32) == np.float32 else np.complex128)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------
def test_edges():
    sr, n_fft = 48000, 1024
    W, H, F = 1024, 256, 513
    rng = np.random.default_rng(43)
    noise = 0.1 * rng.standard_normal(sr // 2)
    N = W + 20 * H + 9
    y = O.synth_signal(N, sr=sr, seed=9, dtype=np.float32)
    bank = stream.StreamBank(sr, 3, n_fft=n_fft, y_noise=noise, max_block=N)
    nt = bank.nt
    assert nt > 0
    whole = _run(bank, {0: (y, [])})[0]
    assert whole["Y"].shape == (F, SM.frames_total(N, W, H))
    # steps of 0 and 1 samples around the sample that completes the first applied frame
    e = nt * H - W // 2 + W
    cuts = [e - 2, e - 1, e - 1, e, e, e + 1, N // 2, N // 2]
    n, a = 0, 0
    Ys = []
    for blk in np.split(y, cuts):
        n += len(blk)
        s, Y, m = bank.push_spectrum({1: blk}, return_mask=True)[1]
        a1 = SM.frames_applied(n, W, H, nt)
        assert Y.shape == m.shape == (F, a1 - a) and Y.dtype == np.complex64 and m.dtype == np.float32, (n, Y.shape)
        assert len(s) == stream.emitted(n, W, H, nt) - stream.emitted(n - len(blk), W, H, nt)
        assert bank.frames(1) == a1
        a = a1
        Ys.append(Y)
    assert [v.shape[1] for v in Ys[:5]] == [0, 0, 0, 1, 0]
    # a flush with no last block
    s, Y = bank.flush_spectrum([1])[1]
    Ys.append(Y)
    assert np.array_equal(np.concatenate(Ys, axis=1), whole["Y"]) and bank.frames(1) == 0
    # a stream of exactly win_length samples, as one max_block block of another bank
    small = stream.StreamBank(sr, 1, n_fft=n_fft, y_noise=noise, max_block=W)
    s, Y, m = small.push_spectrum({0: y[:W]}, return_mask=True)[0]
    assert Y.shape == (F, SM.frames_applied(W, W, H, nt)) == (F, 0) and len(s) == 0
    s, Y, m = small.flush_spectrum([0], return_mask=True)[0]
    T = SM.frames_total(W, W, H)
    assert Y.shape == m.shape == (F, T) and len(s) == W and T == 5
    gate = SM.stationary_gate(small.thresholds(), n_fft, W, H, 1.0, small._gate_kw["n_grad_freq"], nt, True)
    Z, mm = gate(y[:W].astype(np.float64), T)
    assert len(SM.bad_frames(Y, Z * m.astype(np.float64), Z, True, **_KW)) == 0
    assert np.max(np.abs(m - mm)) <= PB.mask_bound(dict(prop=1.0))
    small.close()
    # device tensors in, device tensors out: Y is the transposed view of (k, F) storage, bins contiguous
    yt = torch.from_numpy(np.stack([y, y[::-1].copy()])).cuda()
    two = stream.StreamBank(sr, 1, channels=2, n_fft=n_fft, y_noise=noise, max_block=N)
    s, Y, m = two.push_spectrum({0: yt[:, :N // 2]}, return_mask=True)[0]
    k = SM.frames_applied(N // 2, W, H, nt)
    for v, dt in ((Y, torch.complex64), (m, torch.float32)):
        assert isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == dt and tuple(v.shape) == (2, F, k)
        assert v.stride(-2) == 1 and v.stride(-1) == F and v.transpose(-1, -2).is_contiguous()
    s2, Y2, m2 = two.flush_spectrum([0], {0: yt[:, N // 2:]}, return_mask=True)[0]
    assert isinstance(Y2, torch.Tensor) and Y2.is_cuda and tuple(Y2.shape) == (2, F, whole["Y"].shape[1] - k)
    assert np.array_equal(torch.cat([Y, Y2], dim=-1)[0].cpu().numpy(), whole["Y"])
    two.close()
    # a StreamGate: the same frames
    g = stream.StreamGate(sr, y_noise=noise, n_fft=n_fft, max_block=N)
    a = g.push_spectrum(y[:N // 3])
    b = g.flush_spectrum(y[N // 3:], return_mask=True)
    assert len(a) == 2 and len(b) == 3
    assert np.array_equal(np.concatenate([a[1], b[1]], axis=1), whole["Y"])
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole["y"])
    g.close()
    bank.close()


# ---- 7. moving a stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stationary", [True, False], ids=["S", "NS"])
def test_a_moved_stream_continues_its_frames_bit_for_bit(stationary):
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(47)
    N = W + 31 * H + 7
    y = O.synth_signal(N, sr=sr, seed=13, dtype=np.float32)
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H)
    if stationary:
        kw["y_noise"] = 0.1 * rng.standard_normal(sr // 2)
    else:
        kw.update(stationary=False, lookahead_ms=2.5 * H / sr * 1000, time_constant_s=0.1)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, 7))
    blocks = np.split(y, cuts)
    home = stream.StreamBank(sr, 2, max_block=N, **kw)
    stay = _run(home, {1: (y, cuts)})[1]
    parts = dict(y=[], Y=[], mask=[])

    def take(o):
        for key, v in zip(("y", "Y", "mask"), o):
            parts[key].append(v)

    for blk in blocks[:4]:
        take(home.push_spectrum({0: blk}, return_mask=True)[0])
    state = home.snapshot([0])[0]
    away = stream.StreamBank(sr, 3, max_block=N // 2 + 100, **kw)
    away.restore({2: state})
    assert away.frames(2) == home.frames(0) and away.received(2) == home.received(0)
    for blk in blocks[4:]:
        for piece in np.array_split(blk, 3):      # (the other bank's max_block is smaller)
            take(away.push_spectrum({2: piece}, return_mask=True)[2])
    take(away.flush_spectrum([2], return_mask=True)[2])
    for key in ("y", "Y", "mask"):
        assert np.array_equal(np.concatenate(parts[key], axis=-1), stay[key], equal_nan=True), key
    home.close()
    away.close()
