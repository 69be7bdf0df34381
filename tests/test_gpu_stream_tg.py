"""StreamBank(algorithm="torchgate") on the GPU: the stream of TorchGate's non-stationary gate against the float64 oracle
(O.torchgate_T), against TorchGate itself on the same device and against the float64 model of tests/stream_tg_model.py --
audio, mask and filterbank features; bitwise independence of the block split, the slot, the other streams and the kind of
the steps; the exact bank; digital silence; launches per step, reset, a second bank on one handle; what is refused.

All at sr 16000 on rows of white noise, a tone and a ten times louder burst (tests/gated_stft_cases.make_x's row).  Every
tolerance is one the suite already holds the same quantity to: ORACLE_TOL (tests/test_gpu_stream_ns.py) for audio, 1e-4 for a
non-stationary mask and for features (tests/test_gpu_gated_stft.py, tests/test_gpu_gated_filterbank.py), 1e-12 for the exact
bank's float64 mask rows (noisereduce_amd/stream.py)."""
import functools

import numpy as np
import pytest
import torch

from noisereduce_amd import _ffi, stream
from noisereduce_amd.torchgate import TorchGate, mel_filterbank
from oracle import spectralgate_oracle as O
from tests import stream_tg_model as M

pytestmark = pytest.mark.gpu

SR = 16000
ORACLE_TOL = 1e-4      # of peak: the project's bar
MASK_TOL = 1e-4
EXACT_MASK_TOL = 1e-12
FEAT_TOL = 1e-4        # of the stream's largest feature
SMOOTH = {"on": (500, 50), "off": (None, None)}
# (n_fft, win_length, hop_length), K, prop_decrease, smoothing
CASES = [((256, 256, 64), 20, 1.0, "on"), ((256, 256, 64), 7, 1.0, "on"), ((256, 256, 64), 1, 1.0, "on"),
         ((256, 256, 64), 20, 1.0, "off"), ((512, 400, 160), 20, 1.0, "on"), ((512, 400, 160), 20, 0.6, "on"),
         ((1024, 1024, 256), 20, 1.0, "on")]
IDS = ["%d-%d-%d-K%d-p%g-%s" % (g + (K, p, s)) for g, K, p, s in CASES]
FEATS = [(2, False), (1, False), (2, True), (1, True)]
EPS = 1e-6


def make_x(N, seed):
    rng = np.random.default_rng(seed)
    s = np.arange(N)
    env = 1.0 + 9.0 * ((s >= int(0.40 * N)) & (s < int(0.52 * N)))
    return 0.1 * env * rng.standard_normal(N) + 0.5 * np.sin(2 * np.pi * 440.0 * s / SR)


def _nt(case):
    (n_fft, W, H), K, p, smooth = case
    return O.mask_smoothing_widths(SR, n_fft, H, *SMOOTH[smooth])[1] if smooth == "on" else 0


def lengths(case):
    """T < K with every box cut on both sides; and edge frames next to interior ones."""
    (n_fft, W, H), K, p, smooth = case
    return 2 * W + 13, max(2 * W + 13, (K + 2 * _nt(case) + 12) * H + 13)


def gate_kw(case):
    (n_fft, W, H), K, p, smooth = case
    fhz, tms = SMOOTH[smooth]
    return dict(n_fft=n_fft, win_length=W, hop_length=H, n_movemean_nonstationary=K, prop_decrease=p,
                freq_mask_smooth_hz=fhz, time_mask_smooth_ms=tms)


@functools.lru_cache(maxsize=None)
def reference(ci, N, dtype_name="float32"):
    """(x at the run's type, oracle audio, oracle X, oracle mask, model audio, model mask): computed once, never modified."""
    case = CASES[ci]
    x = make_x(N, seed=1000 * ci + N % 997).astype(dtype_name)
    W = case[0][1]
    y, st = O.torchgate_T(x[None].astype(np.float64), SR, nonstationary=True, window=M.hann_float32(W), return_stages=True,
                          **gate_kw(case))
    ym, sm = M.stream_tg_model(x.astype(np.float64), SR, **gate_kw(case))
    out = (x, y[0], st["X"][0], st["mask"][0], ym, sm["mask"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def filterbank(n_fft):
    return mel_filterbank(SR, n_fft, 80)


def torch_gate(case):
    return TorchGate(sr=SR, nonstationary=True, **gate_kw(case)).to("cuda")


def make_bank(case, n_streams, max_block, precision=None, fb=True):
    bank = stream.StreamBank(SR, n_streams, max_block=max_block, precision=precision, algorithm="torchgate", stationary=False,
                             **gate_kw(case))
    if fb:
        bank.set_filterbank(filterbank(case[0][0]))
    return bank


def cuts_of(kind, N, H, seed=0):
    if kind == "whole":
        return []
    if kind == "hop":
        return list(range(H, N, H))
    if kind == "b37":
        return list(range(37, N, 37))
    if kind == "random":      # block lengths in [0, max_block = N], every third one empty
        rng = np.random.default_rng(seed)
        c, at, i = [], 0, 0
        while at < N:
            at += 0 if i % 3 == 1 else int(rng.integers(0, N + 1))
            c.append(min(at, N))
            i += 1
        return c
    if kind == "single":      # single samples over the first 600
        return list(range(1, 601))
    raise KeyError(kind)


SPLITS = ("hop", "b37", "random", "single")


def run(bank, y, cuts, slot=0, power=2, log=False, others=None, mix=False):
    """The stream y in `slot`, cut at `cuts`, through push_features steps (mix: every other step a plain push) and one
    flush_features; `others`: {slot: (signal, cuts)} pushed alongside.  Returns (audio (N,), mask (F, frames), feat (M, frames),
    [(first, last + 1) frame of every reporting step])."""
    kw = dict(power=power, log=log, eps=EPS, scale="torch", return_mask=True)
    blocks = np.split(y, cuts)
    oth = {s: np.split(v, c) for s, (v, c) in (others or {}).items()}
    outs, fe, mk, cols = [], [], [], []
    for i, blk in enumerate(blocks):
        step = {slot: blk}
        step.update({s: b[i] for s, b in oth.items() if i < len(b)})
        f0 = bank.frames(slot)
        if mix and i % 2:
            outs.append(bank.push(step)[slot])
            continue
        o, f, m = bank.push_features(step, **kw)[slot]
        outs.append(o), fe.append(f), mk.append(m), cols.append((f0, f0 + f.shape[-1]))
    f0 = bank.frames(slot)
    o, f, m = bank.flush_features([slot] + list(oth), **kw)[slot]
    outs.append(o), fe.append(f), mk.append(m), cols.append((f0, f0 + f.shape[-1]))
    return np.concatenate(outs), np.concatenate(mk, axis=-1), np.concatenate(fe, axis=-1), cols


# ---- 1-3: audio, mask, features -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_stream_is_torchgate_of_the_whole_signal(ci, which):
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    N = lengths(case)[which == "long"]
    x, want, X, mask, model, _ = reference(ci, N)
    T, n = N // H + 1, H * (N // H)
    assert want.shape == (n,) and mask.shape == (n_fft // 2 + 1, T) and (which == "long" or K < 20 or T < K)
    tg = torch_gate(case)
    bank = stream.StreamBank.from_torchgate(tg, 2, max_block=N)
    assert bank.lookahead_frames == K - 1 - (K - 1) // 2 and bank.latency_samples == W + (_nt(case) + bank.lookahead_frames + 1) * H
    fb = filterbank(n_fft)
    bank.set_filterbank(fb)
    xd = torch.from_numpy(x.copy()).cuda()
    dev = tg(xd[None])[0].cpu().numpy()
    peak = np.max(np.abs(want))
    fb64 = fb.numpy().astype(np.float64)
    for power, log in FEATS:
        got, gmask, gfeat, cols = run(bank, x, cuts_of("b37", N, H) if (power, log) == (1, True) else [], slot=1, power=power, log=log)
        assert got.shape == (N,) and got.dtype == np.float32 and gmask.shape == mask.shape and gfeat.shape == (80, T)
        assert cols[-1][1] == T
        if (power, log) == FEATS[0]:
            e_or, e_dev = np.max(np.abs(got[:n] - want)) / peak, np.max(np.abs(got[:n] - dev)) / peak
            e_mod = np.max(np.abs(got - model)) / np.max(np.abs(model))
            e_mask = np.max(np.abs(gmask - mask))
            print(f"[stream-tg] {IDS[ci]} N={N}: oracle {e_or:.2e}  TorchGate on the device {e_dev:.2e}  model (all N) {e_mod:.2e}  "
                  f"mask {e_mask:.2e}")
            assert e_or <= ORACLE_TOL and e_dev <= ORACLE_TOL and e_mod <= ORACLE_TOL, (e_or, e_dev, e_mod)
            assert e_mask <= MASK_TOL, e_mask
        lin = np.einsum("km,kt->mt", fb64, np.abs(X * mask) ** power)
        want_f = np.log(lin + EPS) if log else lin
        dev_f = tg.gated_filterbank(xd[None], fb, power=power, log=log, eps=EPS)[0].cpu().numpy()
        big = np.max(np.abs(want_f))
        e_f, e_fd = np.max(np.abs(gfeat - want_f)) / big, np.max(np.abs(gfeat - dev_f)) / big
        print(f"[stream-tg] {IDS[ci]} N={N} power={power} log={log}: features oracle {e_f:.2e}  gated_filterbank {e_fd:.2e}")
        assert e_f <= FEAT_TOL and e_fd <= FEAT_TOL, (power, log, e_f, e_fd)
    bank.close()


# ---- 4: bitwise independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_bitwise_independence_of_split_slot_neighbours_and_step_kind(ci):
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    for N in lengths(case) if ci in (0, 4) else lengths(case)[1:]:
        x = reference(ci, N)[0]
        bank = make_bank(case, 8, N)
        ref = run(bank, x, [])
        for kind in SPLITS:
            got = run(bank, x, cuts_of(kind, N, H, seed=ci))
            for a, b, what in zip(got[:3], ref[:3], ("audio", "mask", "features")):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (kind, N, what)
        # another slot, next to 7 other streams of other lengths and splits
        others = {}
        for s in (0, 1, 2, 3, 4, 6, 7):
            n_s = W + 29 * s + (N * (s + 1)) // 9
            others[s] = (make_x(n_s, seed=50 + s).astype(np.float32), cuts_of(("hop", "b37", "random")[s % 3], n_s, H, seed=s)[:N // 37])
        got = run(bank, x, cuts_of("b37", N, H), slot=5, others=others)
        for a, b, what in zip(got[:3], ref[:3], ("audio", "mask", "features")):
            assert a.tobytes() == b.tobytes(), ("slot 5 of 8", N, what)
        # push and push_features steps interleaved: the audio is the same, the reported frames are the same frames
        audio, gmask, gfeat, cols = run(bank, x, cuts_of("hop", N, H), slot=3, mix=True)
        assert audio.tobytes() == ref[0].tobytes()
        sel = np.concatenate([np.arange(a, b) for a, b in cols])
        assert len(sel) > 0 and (len(sel) < ref[1].shape[-1] or N == lengths(case)[0])      # (a short stream reports at its flush)
        assert gmask.tobytes() == np.ascontiguousarray(ref[1][:, sel]).tobytes()
        assert gfeat.tobytes() == np.ascontiguousarray(ref[2][:, sel]).tobytes()
        bank.close()


# ---- 5: the exact bank ---------------------------------------------------------------------------------------------------
def test_exact_bank_float64_float32_and_int16_blocks_in_one_step():
    ci = 5      # (512, 400, 160), K = 20, prop_decrease 0.6
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    N = lengths(case)[1]
    x64, want, X, mask, model, mmask = reference(ci, N, "float64")
    x32 = make_x(N, seed=7).astype(np.float32)
    x16 = np.round(make_x(N, seed=8) * 4000.0).astype(np.int16)
    bank = make_bank(case, 4, N, precision="float64")
    def pushed_alone(v, slot):
        outs = [bank.push({slot: b})[slot] for b in np.split(v, cuts_of("b37", N, H))]
        return np.concatenate(outs + [bank.flush([slot])[slot]])

    alone = {s: pushed_alone(v, s) for s, v in ((0, x64), (1, x32), (2, x16), (3, x16.astype(np.float64)))}
    # float64 blocks: float64-accurate audio and mask rows
    got, gmask = run(bank, x64, cuts_of("hop", N, H), slot=0)[:2]
    assert got.tobytes() == alone[0].tobytes()      # push_features steps, another split: the audio of push, bit for bit
    mixed = run(bank, x64, cuts_of("b37", N, H), slot=0, mix=True)[0]
    assert mixed.tobytes() == alone[0].tobytes()    # ... and push and push_features steps interleaved
    assert got.dtype == np.float64 and gmask.dtype == np.float64
    n = H * (N // H)
    e_or, e_mod, e_mask = np.max(np.abs(got[:n] - want)) / np.max(np.abs(want)), np.max(np.abs(got - model)) / np.max(np.abs(model)), \
        np.max(np.abs(gmask - mask))
    print(f"[stream-tg] exact bank {IDS[ci]} N={N}: oracle {e_or:.2e}  model {e_mod:.2e}  mask {e_mask:.2e} (oracle) "
          f"{np.max(np.abs(gmask - mmask)):.2e} (model)")
    assert e_or <= 1e-12 and e_mod <= 1e-12, (e_or, e_mod)
    assert e_mask <= EXACT_MASK_TOL, e_mask
    # the three types in one step, each cut its own way: bitwise the stream pushed alone
    cuts = {0: cuts_of("hop", N, H), 1: cuts_of("random", N, H, seed=1), 2: cuts_of("b37", N, H)}
    blocks = {s: np.split(v, cuts[s]) for s, v in ((0, x64), (1, x32), (2, x16))}
    outs = {s: [] for s in blocks}
    for i in range(max(len(b) for b in blocks.values())):
        for s, o in bank.push({s: b[i] for s, b in blocks.items() if i < len(b)}).items():
            outs[s].append(o)
    for s, o in bank.flush([0, 1, 2]).items():
        outs[s].append(o)
    for s, v in ((0, x64), (1, x32), (2, x16)):
        o = np.concatenate(outs[s])
        assert o.dtype == v.dtype and o.tobytes() == alone[s].tobytes(), s
    # int16 is trunc of the float64 result of the same samples (NaN -> 0: there is none here)
    f = alone[3]
    assert np.all(np.isfinite(f)) and np.array_equal(alone[2], np.trunc(f).astype(np.int16))
    bank.close()


# ---- 6: digital silence ----------------------------------------------------------------------------------------------------
def test_digital_silence_is_nan_where_offline_is_nan_and_ends():
    ci = 4
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    nt = _nt(case)
    quiet = W + (K + 5 - 1) * H             # K + 5 frames of zeros: six frames whose whole box is silent, S = 0 / 0
    N = 2 * ((K + 2 * nt + 12) * H) + quiet
    x = make_x(N, seed=61).astype(np.float32)
    a = (N - quiet) // 2 + 7
    x[a:a + quiet] = 0.0
    model, st = M.stream_tg_model(x.astype(np.float64), SR, direct=True, **gate_kw(case))
    assert np.isnan(st["raw"]).any() and not np.isnan(st["raw"]).all(axis=0)[:5].any()
    bank = make_bank(case, 2, N)
    ref = run(bank, x, [])
    assert np.array_equal(np.isnan(ref[0]), np.isnan(model))
    bad = np.isnan(model)
    assert bad.sum() >= 6 * H and np.isnan(ref[1]).any()
    assert np.array_equal(np.isnan(ref[1]), np.isnan(st["mask"]))
    last = np.flatnonzero(bad)[-1]
    assert last < N - 8 * H and np.all(np.isfinite(ref[0][last + 1:]))      # finite again after it
    ok = ~bad
    e = np.max(np.abs(ref[0][ok] - model[ok])) / np.max(np.abs(model[ok]))
    print(f"[stream-tg] digital silence: {bad.sum()} NaN samples, the others {e:.2e} of peak from the model")
    assert e <= ORACLE_TOL
    got = run(bank, x, cuts_of("b37", N, H), slot=1)
    for u, v in zip(got[:3], ref[:3]):
        assert u.tobytes() == v.tobytes()
    bank.close()


# ---- 7: the shape of a step ----------------------------------------------------------------------------------------------
def test_launches_per_step_do_not_depend_on_the_step():
    case = CASES[4]
    counts = []
    for S, n, feats in ((3, 1, False), (64, 1, True), (3, 4000, True), (64, 4000, False)):
        bank = make_bank(case, S, 4000)
        x = {s: torch.from_numpy(make_x(n, seed=s).astype(np.float32)).cuda() for s in range(S)}
        step = (lambda: bank.push_features(x, scale="torch")) if feats else (lambda: bank.push(x))
        step()
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        step()
        counts.append({k: v[1] for k, v in g.profile_read(reset=True).items()})
        g.profile_enable(False)
        bank.close()
    assert all(c == counts[0] for c in counts), counts
    assert sum(counts[0].values()) == 4
    # ... the count of the existing non-stationary bank
    ns = stream.StreamBank(SR, 3, stationary=False, n_fft=512, win_length=400, hop_length=160, max_block=4000, lookahead_ms=50.0)
    x = {s: torch.from_numpy(make_x(4000, seed=s).astype(np.float32)).cuda() for s in range(3)}
    ns.push(x)
    ns.gate.profile_enable(True)
    ns.gate.profile_read(reset=True)
    ns.push(x)
    assert {k: v[1] for k, v in ns.gate.profile_read(reset=True).items()} == counts[0]
    ns.close()


def test_reset_reuses_a_slot_and_a_second_bank_on_the_handle_is_independent():
    ci = 4
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    N = lengths(case)[1]
    x = reference(ci, N)[0]
    bank = make_bank(case, 2, N)
    ref = run(bank, x, [])
    other = make_x(N, seed=77).astype(np.float32)
    bank.push({0: other[:N // 2]})
    bank.reset([0])
    assert bank.received(0) == 0 and bank.frames(0) == 0
    got = run(bank, x, cuts_of("hop", N, H))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], ref[:3]))
    # a second bank created on the same handle, fed between the first one's steps
    g = bank.gate
    raw = g.stream_create_ex(_ffi.Gate.stream_desc(1, 1, N, _ffi.SG_STREAM_NONSTATIONARY, 0))
    assert g.stream_state_bytes_ex(_ffi.Gate.stream_desc(2, 1, N, _ffi.SG_STREAM_NONSTATIONARY, 0)) == bank.state_bytes
    lag = bank.nt + bank.lookahead_frames
    assert g.stream_bank_emitted(raw, N // 2) == stream.emitted(N // 2, W, H, lag) == g.stream_bank_emitted(bank._bank, N // 2)
    assert g.stream_bank_frames(raw, N // 2) == stream.frames_applied(N // 2, W, H, lag)
    first = bank.push({1: x[:N // 2]})[1]
    xd, od = torch.from_numpy(other).cuda(), torch.empty(N, device="cuda")
    g.stream_push(raw, xd, od, [_ffi.SgStreamRec(slot=0, flush=1, n_samples=N, in_offset=0, in_stride=N, out_offset=0, out_stride=N)])
    rest = bank.flush([1], {1: x[N // 2:]})[1]
    assert np.concatenate([first, rest]).tobytes() == ref[0].tobytes()
    assert od.cpu().numpy().tobytes() == run(bank, other, [])[0].tobytes()
    g.stream_destroy(raw)
    bank.close()


# ---- 8: what is refused --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bank_untouched():
    ci = 4
    case = CASES[ci]
    (n_fft, W, H), K, p, smooth = case
    N = lengths(case)[1]
    x = reference(ci, N)[0]
    bank = make_bank(case, 2, N)
    ref = run(bank, x, [])[0]
    first = bank.push({0: x[:N // 2]})[0]
    g, b = bank.gate, bank._bank
    for f in (lambda: bank.snapshot([0]), lambda: bank.restore({0: None}), lambda: bank.push_spectrum({0: x[:10]}),
              lambda: bank.flush_spectrum([0]), lambda: bank.push_features({0: x[:10]}, scale="scipy")):
        with pytest.raises(ValueError):
            f()
    # the C ABI says the same, with a message
    blob = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="sg_stream_export"):
        g.stream_export(b, [0], blob, [0])
    with pytest.raises(ValueError, match="sg_stream_export_bytes"):
        g.stream_export_bytes(b, 0)
    with pytest.raises(ValueError, match="sg_stream_import"):
        g.stream_import(b, [0], blob, [0], [_ffi.SgStreamHead()])
    xd, od = torch.from_numpy(x[:64].copy()).cuda(), torch.empty(64, device="cuda")
    spec = torch.empty(64 * (n_fft // 2 + 1), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError, match="sg_stream_push_spectrum"):
        g.stream_push_spectrum(b, xd, od, spec, None, [_ffi.SgStreamRec(slot=0, flush=0, n_samples=64, in_offset=0, in_stride=64,
                                                                       out_offset=0, out_stride=64)],
                               [_ffi.SgStreamSpecRec(spec_offset=0, mask_offset=0, stride=0)])
    with pytest.raises(ValueError, match="lookahead_frames must be 0"):
        g.stream_create_ex(_ffi.Gate.stream_desc(1, 1, 1000, _ffi.SG_STREAM_NONSTATIONARY, 3))
    for kind in (_ffi.SG_STREAM_FIXED, _ffi.SG_STREAM_ADAPTIVE):
        with pytest.raises(ValueError, match="SG_STREAM_NONSTATIONARY only"):
            g.stream_create_ex(_ffi.Gate.stream_desc(1, 1, 1000, kind, 0))
    with pytest.raises(ValueError):
        g.stream_state_bytes_ex(_ffi.Gate.stream_desc(1, 1, 1000, _ffi.SG_STREAM_NONSTATIONARY, 3))
    assert g.stream_counters(b, 0) == (N // 2, len(first))
    rest = bank.flush([0], {0: x[N // 2:]})[0]
    assert np.concatenate([first, rest]).tobytes() == ref.tobytes()
    bank.close()
    # a stationary variant-T handle, and one with an odd win_length
    kw = dict(variant=_ffi.SG_VARIANT_T, n_fft=512, hop_length=100, top_db=40.0, ddof=1, nonstat_thresh=1.3, nonstat_slope=10.0)
    desc = _ffi.Gate.stream_desc(1, 1, 1000, _ffi.SG_STREAM_NONSTATIONARY, 0)
    st = _ffi.Gate("cuda", stationary=True, win_length=400, window=torch.hann_window(400).double().numpy(), **kw)
    with pytest.raises(ValueError, match="stationary"):
        st.stream_create_ex(desc)
    st.close()
    odd = _ffi.Gate("cuda", stationary=False, win_length=401, window=torch.hann_window(401).double().numpy(), **kw)
    with pytest.raises(ValueError, match="even win_length"):
        odd.stream_create_ex(desc)
    odd.close()
    with pytest.raises(ValueError):
        stream.StreamBank(SR, 1, n_fft=512, win_length=401, algorithm="torchgate", stationary=False)
