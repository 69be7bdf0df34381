"""``TorchGate.gated_filterbank(x, fb, lengths=...)`` on the GPU (sg_gate_features_rows / sg_gate_features_rows_backward,
csrc/rows_feat.hip: k_rw_feat, k_rw_feat_bwd): every row of a padded batch against the float64 statement on the row alone
-- the features frame by frame, the gradient hop block by hop block (tests/gated_filterbank_rows_cases.py: rows of 9, 9,
16, 17, 18 and 25 frames around the tiles of 8 and 16 frames) -- and the contract's invariants: the route, the mask of
gated_stft(lengths=) bit for bit, float32 = float64 rounded once, padding never read, rows independent, sub-batches,
all-full routing, the backward, the launch count, the refusals.

tests/test_gated_filterbank_rows_host.py holds that the checks flag planted defects.  No tolerance is defined here:
K.feature_check and K.log_allowed are tests/gated_filterbank_cases.py's, FACTOR and F64_REL tests/parity_budget.py's, TOL
tests/test_gpu_rows.py's (1e-4: DESIGN section 14a's bar for the end-to-end gradient).  The figures per cell go to the file
named by GATED_FILTERBANK_ROWS_PARITY_OUT, if set (profiles/parity_budget_gated_filterbank_rows.json is that file from an
MI355X run of this module alone)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import gated_filterbank_cases as K
from tests import gated_filterbank_rows_cases as FR
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB
from tests.test_gpu_rows import TOL, edge_lengths, make_rows

pytestmark = pytest.mark.gpu
SR = R.SR
EPS = FR.EPS

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_record():
    yield
    path = os.environ.get("GATED_FILTERBANK_ROWS_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "f64_rel_allowed": PB.F64_REL, "cells": dict(sorted(_RECORD.items()))},
                      f, indent=1)


def _note(name, **kw):
    rec = _RECORD.setdefault(name, {})
    for k, v in kw.items():
        rec[k] = max(rec.get(k, 0.0), float(v))


def _tdt(name):
    return torch.float32 if name == "float32" else torch.float64


def _tg(**kw):
    from noisereduce_amd.torchgate import TorchGate
    return TorchGate(sr=SR, **kw).cuda()


def _fbt(fb):
    return torch.from_numpy(np.array(fb))


def _feat(tg, x, fbt, lens, xn=None, xn_lens=None, **kw):
    out, M = tg.gated_filterbank(x.cuda(), fbt, None if xn is None else xn.cuda(), return_mask=True, lengths=lens,
                                 xn_lengths=xn_lens, **kw)
    return out.detach().cpu(), M.cpu()


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 1. the route ------------------------------------------------------------------------------------------------------
def test_ragged_lengths_take_the_native_route(monkeypatch):
    from noisereduce_amd.torchgate import TorchGate
    c = R.cell("E-1024-1024-256")
    tg = _tg(**R.gate_kwargs(c))
    x, fbt = R.rows(c).cuda(), _fbt(FR.bank("mel40", 1024))
    want = tg.gated_stft(x, lengths=c["lens"], return_mask=True)[1]

    def boom(*a, **k):
        raise AssertionError("gated_filterbank(lengths=) went through gated_stft")
    monkeypatch.setattr(TorchGate, "gated_stft", boom)
    out, M = tg.gated_filterbank(x, fbt, return_mask=True, lengths=c["lens"], log=True)
    assert tuple(out.shape) == (6, 40, 25) and out.transpose(1, 2).is_contiguous() and torch.equal(M, want)
    assert tg._gate_for(x.device).rows_batches() == 1


def test_other_n_fft_still_takes_the_composed_route(monkeypatch):
    from noisereduce_amd.torchgate import TorchGate
    tg = _tg(n_fft=400)
    lens = [8000, 4000, 2001]
    x = make_rows(lens, 8000, 0).cuda()
    fbt = _fbt(FR.bank("mel40", 400))
    calls = []
    real = TorchGate.gated_stft

    def spy(self, *a, **k):
        calls.append(k.get("lengths"))
        return real(self, *a, **k)
    monkeypatch.setattr(TorchGate, "gated_stft", spy)
    out = tg.gated_filterbank(x, fbt, lengths=lens, log=True)
    assert calls and calls[0] is not None and tuple(out.shape) == (3, 40, 81)
    dead = torch.log(torch.zeros((), device="cuda") + 1e-6)       # the composed formula on a zero spectrum, in torch's float32
    for i, n in enumerate(lens):
        assert bool((out[i, :, 1 + n // 100:] == dead).all())


# ---- 2. forward: every cell ------------------------------------------------------------------------------------------------
def _check_forward(c, gate, dtype, bname, tag):
    """Both powers (one for a bank with negative entries), log off and on, of one cell under one bank.  Returns the largest
    err / budget (float32) or err / bound (float64) and the largest log err / allowed."""
    us = R.units(c, gate, dtype)
    tg = _tg(**R.gate_kwargs(c, gate))
    x = R.rows(c, dtype, pad=float("nan"))
    fb = FR.bank(bname, c["n_fft"])
    fbt = _fbt(fb)
    B, F, T, M = len(c["lens"]), c["n_fft"] // 2 + 1, 1 + c["L"] // c["H"], fb.shape[1]
    frames = R.frames_of(c)
    _, mask_spec = tg.gated_stft(x.cuda(), return_mask=True, lengths=c["lens"])
    worst = worst_log = 0.0
    for power in FR.bank_powers(bname):
        lin, Mk = _feat(tg, x, fbt, c["lens"], power=float(power))
        assert tuple(lin.shape) == (B, M, T) and lin.dtype == _tdt(dtype) and lin.stride() == (T * M, 1, M)
        assert tuple(Mk.shape) == (B, F, T) and Mk.dtype == torch.float32
        assert torch.equal(Mk, mask_spec.cpu()), "%s: the mask is not gated_stft(lengths=)'s" % tag
        if dtype == "float32":
            lin64, Mk64 = _feat(tg, x.double(), fbt, c["lens"], power=float(power))
            assert lin64.dtype == torch.float64 and torch.equal(Mk64, Mk)
            assert torch.equal(lin64.float(), lin), "%s power %d: float32 is not float64 rounded once" % (tag, power)
        got, Mn = lin.numpy(), Mk.numpy()
        assert np.isfinite(got).all(), tag
        for i, u in enumerate(us):
            Ti = frames[i]
            assert np.all(got[i][:, Ti:] == 0) and not np.signbit(got[i][:, Ti:]).any() and not Mn[i][:, Ti:].any(), (tag, i)
            if dtype == "float32":
                bad, ratio = K.feature_check(got[i][:, :Ti], u["Z"], Mn[i][:, :Ti], fb, power, u["emu_spec"])
                assert bad.size == 0, "%s power %d row %d: frames %s of %d over their bound (largest error / budget %.2f)" % (
                    tag, power, i, bad[:12].tolist(), Ti, ratio)
            else:
                want = K.features64(u["Z"], Mn[i][:, :Ti], fb, power)
                err = np.max(np.abs(got[i][:, :Ti] - want), axis=0)
                peak = np.max(np.abs(want), axis=0)
                bound = PB.F64_REL * np.maximum(peak, 1e-3 * peak.max())
                ratio = float(np.max(err / bound))
                assert ratio <= 1.0, "%s power %d row %d: float64 features off by %.3g of the bound" % (tag, power, i, ratio)
            worst = max(worst, ratio)
        if bname == "zero_last":
            assert not got[:, -1, :].any()
        if bname == "neg":
            assert (got < 0).any()
            continue
        lg, Ml = _feat(tg, x, fbt, c["lens"], power=float(power), log=True, eps=EPS)
        assert tuple(lg.shape) == (B, M, T) and lg.dtype == _tdt(dtype) and torch.equal(Ml, Mk)
        if dtype == "float32":
            lg64, _ = _feat(tg, x.double(), fbt, c["lens"], power=float(power), log=True, eps=EPS)
            assert torch.equal(lg64.float(), lg), "%s power %d log: float32 is not float64 rounded once" % (tag, power)
        lgn = lg.numpy()
        for i in range(B):
            Ti = frames[i]
            assert np.all(lgn[i][:, Ti:] == FR.dead_value(True, dtype)), (tag, i)
            want_log = np.log(got[i][:, :Ti].astype(np.float64) + EPS)
            lerr = float(np.max(np.abs(lgn[i][:, :Ti].astype(np.float64) - want_log) / K.log_allowed(want_log)))
            worst_log = max(worst_log, lerr)
            assert lerr <= 1.0, (tag, power, i, lerr)
        if bname == "zero_last":
            assert np.all(lgn[:, -1, :] == FR.dead_value(True, dtype))
    print("[gated_filterbank rows] %s: largest err / %s %.3g, log err / allowed %.3g" % (
        tag, "budget" if dtype == "float32" else "float64 bound", worst, worst_log))
    return worst, worst_log


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", FR.CELLS, ids=R.cell_id)
def test_every_row_matches_the_statement_on_the_row_alone(c, gate, dtype):
    worst, worst_log = _check_forward(c, gate, dtype, "mel40", "%s %s %s mel40" % (c["name"], gate, dtype))
    _note("%s-%s" % (c["name"], gate), **{"features_" + dtype: worst, "log_" + dtype: worst_log})


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("name,bname", FR.VARIATION, ids=["%s-%s" % v for v in FR.VARIATION])
def test_banks(name, bname, dtype):
    worst, worst_log = _check_forward(R.cell(name), "stat", dtype, bname, "%s stat %s %s" % (name, dtype, bname))
    _note("%s-stat-%s" % (name, bname), **{"features_" + dtype: worst, "log_" + dtype: worst_log})


# ---- 3. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gate", [("E-1024-1024-256", "stat"), ("E-1024-1024-256", "nonstat"), ("E-2048-2048-512", "stat")])
def test_padding_is_never_read_and_rows_are_independent(name, gate):
    c = R.cell(name)
    tg = _tg(**R.gate_kwargs(c, gate))
    fbt = _fbt(FR.bank("mel40", c["n_fft"]))
    lens, L, W, H = c["lens"], c["L"], c["W"], c["H"]
    T = 1 + L // H
    kw = dict(log=True, eps=EPS)
    x = R.rows(c)
    base = _feat(tg, x, fbt, lens, **kw)
    assert bool(torch.isfinite(base[0]).all())
    for pad in (float("nan"), float("inf")):
        assert _same(_feat(tg, R.rows(c, pad=pad), fbt, lens, **kw), base)
    other = x.clone()
    for i, n in enumerate(lens):
        other[i, n:] = make_rows([L], L, 50 + i)[0, n:]
    assert _same(_feat(tg, other, fbt, lens, **kw), base)
    wide = torch.full((len(lens), L + 1000), float("nan"))
    wide[:, :L] = R.rows(c, pad=float("nan"))
    fw, mw = _feat(tg, wide, fbt, lens, **kw)
    assert _same((fw[:, :, :T], mw[:, :, :T]), base)
    assert bool((fw[:, :, T:] == float(FR.dead_value(True, "float32"))).all()) and bool((mw[:, :, T:] == 0).all())
    xnan = R.rows(c, pad=float("nan"))
    rev = _feat(tg, xnan.flip(0), fbt, lens[::-1], **kw)
    assert _same((rev[0].flip(0), rev[1].flip(0)), base)
    for i in (0, 3):
        one = torch.cat([xnan[i:i + 1], torch.full((1, 7), float("nan"))], 1)
        f1, m1 = _feat(tg, one, fbt, lens[i:i + 1], **kw)
        assert _same((f1[:, :, :T], m1[:, :, :T]), (base[0][i:i + 1], base[1][i:i + 1]))
    if gate == "stat":
        Ln = max(2 * W, 9000)
        nlens = edge_lengths(W, H, Ln, len(lens), 4)
        a = _feat(tg, x, fbt, lens, make_rows(nlens, Ln, 9), nlens, **kw)
        b = _feat(tg, x, fbt, lens, make_rows(nlens, Ln, 9, pad=float("nan")), nlens, **kw)
        assert _same(a, b) and not torch.equal(a[1], base[1])


@pytest.mark.parametrize("gate", R.GATES)
def test_sub_batches_give_the_same_bits(gate):
    """The 4096 cell: its frequency-smoothed field (forward) and its frame segments (backward) exceed a 1 MiB budget."""
    from noisereduce_amd import _ffi
    c = R.cell("E-4096-4096-1024")
    tg = _tg(**R.gate_kwargs(c, gate))
    fb = FR.bank("mel40", c["n_fft"])
    lens, L = c["lens"], c["L"]
    x = R.rows(c, pad=float("nan")).cuda()
    whole = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg))
    small = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg, max_workspace_bytes=1 << 20))
    try:
        whole.set_filterbank(fb)
        small.set_filterbank(fb)
        for kw in (dict(power=2, log=True), dict(power=1, log=False)):
            f0, m0 = whole.gate_features_rows(x, lens, save_mask=True, **kw)
            assert whole.rows_batches() == 1
            f1, m1 = small.gate_features_rows(x, lens, save_mask=True, **kw)
            assert small.rows_batches() > 1
            assert torch.equal(f0, f1) and torch.equal(m0, m1)
            want = tg.gated_filterbank(x, _fbt(fb), lengths=lens, power=float(kw["power"]), log=kw["log"])
            assert torch.equal(f0.transpose(1, 2), want)
            g = torch.randn(f0.shape, generator=torch.Generator().manual_seed(3)).cuda()
            gx0 = whole.gate_features_rows_backward(x, g, m0, lens, **kw)
            assert whole.rows_batches() == 1
            gx1 = small.gate_features_rows_backward(x, g, m0, lens, **kw)
            assert small.rows_batches() > 1
            assert torch.equal(gx0, gx1) and bool(torch.isfinite(gx0).all()) and bool(gx0.any())
    finally:
        whole.close()
        small.close()


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True), dict(n_fft=2048)])
def test_all_full_lengths_are_the_full_length_call(kw):
    B, L = 5, 9000
    x = make_rows([L] * B, L, 8).cuda()
    xn = make_rows([6000], 6000, 9).cuda()
    tg = _tg(**kw)
    fbt = _fbt(FR.bank("mel40", kw.get("n_fft", 1024)))
    for fk in (dict(), dict(log=True, power=1.0)):
        want = tg.gated_filterbank(x, fbt, return_mask=True, **fk)
        assert _same(tg.gated_filterbank(x, fbt, return_mask=True, lengths=[L] * B, **fk), want)
        assert _same(tg.gated_filterbank(x, fbt, return_mask=True, lengths=torch.full((B,), L, device="cuda"), **fk), want)
        assert _same(tg.gated_filterbank(x, fbt, xn, return_mask=True, lengths=[L] * B, xn_lengths=[6000], **fk),
                     tg.gated_filterbank(x, fbt, xn, return_mask=True, **fk))


# ---- 4. backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("c", FR.BWD_CELLS, ids=R.cell_id)
def test_backward_is_the_adjoint_of_each_row_alone(c, dtype):
    """Per hop block on [0, len_i), with the mask the forward returned; both powers, log off and on.  The upstream
    gradient holds NaN in the frames the backward must not read."""
    us = R.units(c, "stat", dtype)
    tg = _tg(**R.gate_kwargs(c, "stat"))
    fb = FR.bank("mel40", c["n_fft"])
    lens, L, F = c["lens"], c["L"], c["n_fft"] // 2 + 1
    x = R.rows(c, dtype, pad=float("nan")).cuda()
    g = tg._gate_for(x.device)
    tag = "%s %s" % (c["name"], dtype)
    gn = FR.upstream(c, fb.shape[1], dtype)                                 # (B, M, T), what the kernel is given
    gt = torch.from_numpy(np.ascontiguousarray(gn.transpose(0, 2, 1))).cuda()    # (B, T, M)
    assert gt.dtype == _tdt(dtype) and bool(torch.isnan(gt).any())
    worst = {}
    with g.lock:
        g.set_filterbank(fb)
        for power in FR.POWERS:
            for log in (False, True):
                kw = dict(power=power, log=log, eps=EPS)
                _, mask = g.gate_features_rows(x, lens, save_mask=True, **kw)
                gx = g.gate_features_rows_backward(x, gt, mask, lens, **kw)
                assert gx.shape == (len(lens), L) and gx.dtype == _tdt(dtype)
                assert torch.equal(g.gate_features_rows_backward(x, gt, mask, lens, **kw), gx), "%s: two runs differ" % tag
                assert torch.equal(g.gate_features_rows_backward(x, torch.nan_to_num(gt, nan=0.0), mask, lens, **kw), gx), \
                    "%s: grad beyond a row's own frames was read" % tag
                gx = gx.cpu().numpy()
                assert np.isfinite(gx).all(), "%s: the NaN beyond a row's own frames reached the gradient" % tag
                Mn = mask[:, :, :F].transpose(1, 2).cpu().numpy()
                for i, n in enumerate(lens):
                    Ti = R.frames_of(c)[i]
                    assert not gx[i, n:].any() and gx[i, :n].any(), (tag, power, log, i)
                    unit = FR.grad_unit(us[i], Mn[i][:, :Ti], fb, gn[i][:, :Ti].astype(np.float64), power, log, n)
                    bad, ratio = FR.grad_check(gx[i, :n], unit)
                    key = "adjoint_p%d_%s_%s" % (power, "log" if log else "lin", dtype)
                    worst[key] = max(worst.get(key, 0.0), ratio)
                    assert len(bad) == 0, "%s power %d log %s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                        tag, power, log, i, bad[:10].tolist(), ratio)
    print("[gated_filterbank rows] %s: largest adjoint err / bud %s" % (tag, {k: round(v, 3) for k, v in worst.items()}))
    _note("%s-stat" % c["name"], **worst)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("power", FR.POWERS)
def test_zero_filter_contributes_no_gradient(power, log):
    c = R.cell("E-512-512-128")
    tg = _tg(**R.gate_kwargs(c))
    xg = R.rows(c, pad=float("nan")).cuda().requires_grad_()
    out = tg.gated_filterbank(xg, _fbt(FR.bank("zero_last", 512)), power=float(power), log=log, lengths=c["lens"])
    g = torch.zeros_like(out)
    g[:, -1, :] = 1.0
    out.backward(g)
    assert not xg.grad.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_power_one_on_a_silent_row(dtype):
    c = R.cell("E-1024-1024-256")
    tg = _tg(**R.gate_kwargs(c))
    x = R.rows(c).to(dtype)
    x[1] = 0.0
    fbt = _fbt(FR.bank("mel40", 1024))
    for log in (False, True):
        xg = x.clone().cuda().requires_grad_()
        out = tg.gated_filterbank(xg, fbt, power=1.0, log=log, lengths=c["lens"])
        assert bool(torch.isfinite(out).all())
        out.backward(torch.ones_like(out))
        assert bool(torch.isfinite(xg.grad).all())
        assert not xg.grad[1].any() and xg.grad[0].any() and xg.grad[2].any()
        if not log:
            assert not out[1].any()


@pytest.mark.parametrize("kw,dtype,fk", [(dict(), torch.float32, dict(log=True)),
                                         (dict(nonstationary=True, prop_decrease=0.7), torch.float64, dict(power=1.0)),
                                         (dict(n_fft=512, win_length=400, hop_length=90), torch.float32, dict())])
def test_loss_backward_matches_autograd_on_each_row_alone(kw, dtype, fk):
    n_fft = kw.get("n_fft", 1024)
    W = kw.get("win_length") or n_fft
    H = kw.get("hop_length") or W // 4
    L = 7000
    lens = edge_lengths(W, H, L, 6, 12)
    x = make_rows(lens, L, 12, dtype, pad=float("nan")).cuda().requires_grad_()
    tg = _tg(**kw)
    fb = FR.bank("mel40", n_fft)
    power, log = int(fk.get("power", 2)), bool(fk.get("log", False))
    out, M = tg.gated_filterbank(x, _fbt(fb), return_mask=True, lengths=lens, eps=EPS, **fk)
    assert out.requires_grad and not M.requires_grad
    Wt = torch.randn(out.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(out.dtype).cuda()
    for i, n in enumerate(lens):
        Wt[i, :, 1 + n // H:] = float("nan")             # ... whose gradient there is NaN and never read
    torch.where(torch.isnan(Wt), torch.zeros_like(out), out * Wt).sum().backward()
    gx = x.grad.detach().cpu()
    assert gx.dtype == dtype and gx.shape == x.shape and bool(torch.isfinite(gx).all())
    w = torch.hann_window(W).double()
    Wc, Mc, fb64 = Wt.cpu().double(), M.detach().cpu().double(), torch.from_numpy(np.array(fb)).double()
    for i, n in enumerate(lens):
        Ti = 1 + n // H
        x2 = x.detach().cpu()[i:i + 1, :n].double().clone().requires_grad_()
        X = torch.stft(x2, n_fft, H, W, window=w, center=True, pad_mode="constant", return_complex=True)
        Y2 = X * Mc[i:i + 1, :, :Ti]
        p = Y2.real ** 2 + Y2.imag ** 2 if power == 2 else Y2.abs()
        f2 = torch.matmul(p.transpose(1, 2), fb64).transpose(1, 2)
        if log:
            f2 = torch.log(f2 + EPS)
        ref_out = f2.detach()[0]
        assert float((ref_out - out.detach().cpu()[i, :, :Ti].double()).abs().max() / ref_out.abs().max()) < TOL
        (f2 * Wc[i:i + 1, :, :Ti]).sum().backward()
        ref = x2.grad[0]
        assert float((gx[i, :n].double() - ref).abs().max() / ref.abs().max()) < TOL, (i, n)
        assert bool((gx[i, n:] == 0).all()), (i, n)


# ---- 5. launch count ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonstationary", [False, True])
def test_launch_count_does_not_depend_on_the_batch(nonstationary):
    rng = np.random.default_rng(2)
    tg = _tg(n_fft=256, nonstationary=nonstationary)
    fbt = _fbt(FR.bank("mel40", 256))
    counts = []
    for B, L in ((3, 2000), (300, 3000)):
        lens = [int(n) for n in rng.integers(512, L + 1, B)]
        lens[0] = L - 1
        x = make_rows(lens, L, 1).cuda().requires_grad_()
        g = tg._gate_for(x.device)
        tg.gated_filterbank(x.detach(), fbt, lengths=lens)        # (binds the bank: its upload is not a launch of the call)
        g.profile_enable(True)
        g.profile_read(reset=True)
        out = tg.gated_filterbank(x, fbt, lengths=lens, log=True)
        fwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        assert g.rows_batches() == 1
        out.sum().backward()
        bwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        g.profile_enable(False)
        counts.append((fwd, bwd))
    assert counts[0] == counts[1]
    assert sum(counts[0][0].values()) == (4 if nonstationary else 5) and sum(counts[0][1].values()) == 2, counts[0]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_engine_refuses():
    from noisereduce_amd import _ffi
    c = R.cell("E-1024-1024-256")
    tg = _tg(**R.gate_kwargs(c))
    x = R.rows(c).cuda()
    B, L = x.shape
    gate = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg))
    gate400 = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(_tg(n_fft=400)))
    try:
        with pytest.raises(Exception, match="no filterbank set"):
            gate.gate_features_rows(x, c["lens"])
        lens = (ctypes.c_int64 * B)(*c["lens"])
        out = torch.empty((B, gate.n_frames(L), 40), device="cuda")

        def call(h, power):
            return h.lib.sg_gate_features_rows(h._h, x.data_ptr(), _ffi.SG_F32, B, L, x.stride(0), lens, None, 0, 0, 0, None,
                                               power, 0, 1e-6, out.data_ptr(), None, h._stream())
        assert call(gate, 2) == _ffi.SG_E_INVALID and b"no filterbank set" in gate.lib.sg_last_error(gate._h)
        gate.set_filterbank(FR.bank("mel40", 1024))
        assert call(gate, 3) == _ffi.SG_E_INVALID and b"power must be 1 or 2" in gate.lib.sg_last_error(gate._h)
        assert call(gate, 2) == 0
        with pytest.raises(ValueError, match=r"sg_gate_features_rows: lengths\[1\] = 100"):
            gate.gate_features_rows(x, [L, 100, L, L, L, L])
        assert call(gate400, 2) == _ffi.SG_E_UNSUPPORTED
        gx = torch.empty((B, L), device="cuda")
        rc = gate400.lib.sg_gate_features_rows_backward(gate400._h, x.data_ptr(), _ffi.SG_F32, B, L, x.stride(0), lens,
                                                        out.data_ptr(), out.data_ptr(), 2, 0, 1e-6, gx.data_ptr(), L,
                                                        gate400._stream())
        assert rc == _ffi.SG_E_UNSUPPORTED
        torch.cuda.synchronize()
    finally:
        gate.close()
        gate400.close()
    assert _ffi.load_library().sg_version() == 100
