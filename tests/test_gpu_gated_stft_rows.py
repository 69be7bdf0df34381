"""``TorchGate.gated_stft(x, lengths=...)`` on the GPU (sg_gate_spectrum_rows / sg_gate_spectrum_rows_backward,
csrc/rows.hip: k_rw_spec, k_rw_spec_bwd): every row of a padded batch against the float64 oracle on the row alone, frame
by frame and hop block by hop block (tests/gated_stft_rows_cases.py: rows of 9, 9, 16, 17, 18 and 25 frames around the
tiles of 8 and 16 frames), against today's kernels on the row alone, and the contract's invariants -- padding never read,
rows independent, sub-batches, all-full routing, the backward, the launch count, the per-row route of other n_fft.

tests/test_gated_stft_rows_host.py holds the inputs' conditions and that the metrics flag planted defects.  No tolerance is
defined here: FACTOR, F64_REL, DELTA_DB and mask_bound are tests/parity_budget.py's, TOL / TOL_PATHS are
tests/test_gpu_rows.py's (1e-4: DESIGN section 14's bar for the non-stationary mask and the end-to-end gradient).  The
figures per cell go to the file named by GATED_STFT_ROWS_PARITY_OUT, if set (profiles/parity_budget_gated_stft_rows.json
is that file from an MI355X run of this module alone)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import gated_stft_cases as C
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB
from tests.test_gpu_rows import TOL, TOL_PATHS, edge_lengths, make_rows, noise_of

pytestmark = pytest.mark.gpu
SR = R.SR

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_record():
    yield
    path = os.environ.get("GATED_STFT_ROWS_PARITY_OUT")
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


def _gated(tg, x, lens, xn=None, xn_lens=None):
    Y, M = tg.gated_stft(x.cuda(), None if xn is None else xn.cuda(), return_mask=True, lengths=lens, xn_lengths=xn_lens)
    return Y.cpu(), M.cpu()


# ---- 1. per-row parity on every cell -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", R.CELLS, ids=R.cell_id)
def test_every_row_matches_the_oracle_on_the_row_alone(c, gate, dtype):
    us = R.units(c, gate, dtype)
    tg = _tg(**R.gate_kwargs(c, gate))
    x = R.rows(c, dtype)
    F, T = c["n_fft"] // 2 + 1, 1 + c["L"] // c["H"]
    Y, M = _gated(tg, x, c["lens"])
    assert tuple(Y.shape) == tuple(M.shape) == (len(c["lens"]), F, T) and M.dtype == torch.float32
    assert Y.dtype == (torch.complex64 if dtype == "float32" else torch.complex128)
    assert Y.transpose(1, 2).is_contiguous()
    assert tg.stft_lengths(torch.tensor(c["lens"], device="cuda")).tolist() == R.frames_of(c)
    Y, M = Y.numpy(), M.numpy()
    tag = "%s %s %s" % (c["name"], gate, dtype)
    worst = worst64 = mask_err = 0.0
    for i, u in enumerate(us):
        Ti = R.frames_of(c)[i]
        assert not Y[i, :, Ti:].real.any() and not Y[i, :, Ti:].imag.any() and not M[i, :, Ti:].any(), (tag, i)
        assert not np.signbit(Y[i, :, Ti:].real).any() and not np.signbit(Y[i, :, Ti:].imag).any(), (tag, i)
        y, m = Y[i, :, :Ti], M[i, :, :Ti]
        assert np.isfinite(m).all() and np.isfinite(y.real).all() and np.isfinite(y.imag).all(), (tag, i)
        bad, ratio = C.spectrum_check(y, u["Z"], m, u["cfg"], emu=u["emu_spec"])
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: frames %s of %d over their bound (largest error / budget %.2f)" % (
            tag, i, bad[:12].tolist(), Ti, ratio)
        if dtype == "float64":
            rel = float(np.abs(y - u["Z"] * m.astype(np.float64)).max() / np.abs(u["Z"]).max())
            worst64 = max(worst64, rel)
            assert rel <= PB.F64_REL, (tag, i, rel)
        if gate == "stat":
            cells, w = PB.mask_diff(m, u, bound=PB.mask_bound(u["cfg"], integer_taps=False))
            assert len(cells) == 0, "%s row %d: mask off by up to %.3g at %d cells, first %s" % (tag, i, w, len(cells), cells[:6].tolist())
        else:
            w = float(np.abs(m.astype(np.float64) - u["mask"]).max())
            assert w <= TOL, (tag, i, w)
        mask_err = max(mask_err, w)
    print("[gated_stft rows] %s: spectrum err / bud %.3f, complex128 rel %.3g, mask err %.3g" % (tag, worst, worst64, mask_err))
    _note("%s-%s" % (c["name"], gate), **{"spectrum_" + dtype: worst, "mask_err_" + dtype: mask_err})
    if dtype == "float64":
        _note("%s-%s" % (c["name"], gate), complex128_rel=worst64)


# ---- 2. the mask is sg_process_rows' ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", R.CELLS, ids=R.cell_id)
def test_mask_is_bitwise_the_mask_of_process_rows(c, gate):
    tg = _tg(**R.gate_kwargs(c, gate))
    x = R.rows(c, "float32", pad=float("nan")).cuda()
    g = tg._gate_for(x.device)
    _, m_spec = g.gate_spectrum_rows(x, c["lens"], save_mask=True)
    _, m_rows = g.process_rows(x, c["lens"], save_mask=True)
    assert torch.equal(m_spec, m_rows)
    if gate == "stat":
        Ln = max(2 * c["W"], 3000)
        nlens = edge_lengths(c["W"], c["H"], Ln, len(c["lens"]), 4)
        xn = make_rows(nlens, Ln, 9, pad=float("nan")).cuda()
        _, m_spec = g.gate_spectrum_rows(x, c["lens"], xn, nlens, save_mask=True)
        _, m_rows2 = g.process_rows(x, c["lens"], xn, nlens, save_mask=True)
        assert torch.equal(m_spec, m_rows2) and not torch.equal(m_spec, m_rows)
        _, m_spec = g.gate_spectrum_rows(x, c["lens"], xn[:1], nlens[:1], save_mask=True)
        _, m_rows3 = g.process_rows(x, c["lens"], xn[:1], nlens[:1], save_mask=True)
        assert torch.equal(m_spec, m_rows3) and not torch.equal(m_spec, m_rows2)


# ---- 3. against today's kernels on the row alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("gate,xn_mode", [("stat", None), ("stat", "shared"), ("stat", "rows_len"), ("nonstat", None)])
@pytest.mark.parametrize("name", ["E-256-256-64", "E-1024-1024-256", "G-2048-1500-333", "E-4096-4096-1024"])
def test_every_row_matches_todays_paths_on_the_row_alone(name, gate, xn_mode):
    c = R.cell(name)
    kw = R.gate_kwargs(c, gate)
    tg = _tg(**kw)
    x, lens, W, H = R.rows(c, "float32", pad=float("nan")), c["lens"], c["W"], c["H"]
    xn = xn_lens = None
    if xn_mode == "shared":
        xn = make_rows([max(2 * W, 5000)], max(2 * W, 5000), 100 + c["seed"])
    elif xn_mode == "rows_len":
        Ln = max(2 * W, 7000)
        xn_lens = edge_lengths(W, H, Ln, len(lens), 200 + c["seed"])
        xn = make_rows(xn_lens, Ln, 100 + c["seed"], pad=float("nan"))
    Y, _ = _gated(tg, x, lens, xn, xn_lens)
    y = tg(x.cuda(), None if xn is None else xn.cuda(), lengths=lens, xn_lengths=xn_lens).cpu()
    win = torch.hann_window(W)
    worst = worst_i = 0.0
    for i, n in enumerate(lens):
        Ti = 1 + n // H
        ni = noise_of(xn, xn_lens, i)
        alone = tg.gated_stft(x[i:i + 1, :n].cuda(), None if ni is None else ni.cuda()).cpu()[0]
        assert alone.shape == (c["n_fft"] // 2 + 1, Ti)
        worst = max(worst, float((Y[i, :, :Ti] - alone).abs().max() / alone.abs().max()))
        inv = torch.istft(Y[i:i + 1, :, :Ti], c["n_fft"], H, W, window=win, center=True)[0]
        lo = H * (n // H)
        assert inv.shape[0] == lo
        worst_i = max(worst_i, float((inv - y[i, :lo]).abs().max() / y[i, :lo].abs().max()))
    print("[gated_stft rows] %s %s xn=%s: vs gated_stft alone %.3e, istft vs forward(lengths=) %.3e" % (name, gate, xn_mode, worst, worst_i))
    assert worst <= TOL_PATHS, (name, gate, worst)
    assert worst_i <= TOL_PATHS, (name, gate, worst_i)


def test_stationary_decision_bits_equal_todays_path():
    """Smoothing off, prop_decrease = 1: the returned mask IS the decision bits, and both paths decide in float64."""
    kw = dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
    W, H, L = 1024, 256, 9000
    lens = edge_lengths(W, H, L, 8, 5)
    x = make_rows(lens, L, 5)
    tg = _tg(**kw)
    _, M = _gated(tg, x, lens)
    for i, n in enumerate(lens):
        Ti = 1 + n // H
        _, m1 = tg.gated_stft(x[i:i + 1, :n].cuda(), return_mask=True)
        assert torch.equal(M[i, :, :Ti], m1[0].cpu()), (i, n)
        assert bool((M[i, :, Ti:] == 0).all())
        assert set(np.unique(M[i, :, :Ti].numpy()).tolist()) <= {0.0, 1.0}
        assert 0.01 <= float(M[i, :, :Ti].mean()) <= 0.99


def test_nonstationary_ignores_xn():
    c = R.cell("E-1024-1024-256")
    tg = _tg(**R.gate_kwargs(c, "nonstat"))
    x = R.rows(c, "float32")
    Y0, M0 = _gated(tg, x, c["lens"])
    Y1, M1 = _gated(tg, x, c["lens"], torch.full((1, 5000), float("nan")), [3000])
    assert torch.equal(Y0, Y1) and torch.equal(M0, M1)


# ---- 4. invariants -------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(torch.view_as_real(a[0].contiguous()), torch.view_as_real(b[0].contiguous())) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True, prop_decrease=0.7), dict(n_fft=2048)])
def test_padding_is_never_read(kw):
    n_fft = kw.get("n_fft", 1024)
    W, H, L = n_fft, n_fft // 4, 14000
    lens = edge_lengths(W, H, L, 7, 3)
    tg = _tg(**kw)
    base = _gated(tg, make_rows(lens, L, 3), lens)
    T = 1 + L // H
    for pad in (float("nan"), float("inf")):
        assert _same(_gated(tg, make_rows(lens, L, 3, pad=pad), lens), base)
    other = make_rows(lens, L, 3)
    for i, n in enumerate(lens):
        other[i, n:] = make_rows([L], L, 50 + i)[0, n:]
    assert _same(_gated(tg, other, lens), base)
    wide = torch.full((len(lens), L + 1000), float("nan"))
    wide[:, :L] = make_rows(lens, L, 3, pad=float("nan"))
    Yw, Mw = _gated(tg, wide, lens)
    assert _same((Yw[:, :, :T], Mw[:, :, :T]), base)
    assert bool((torch.view_as_real(Yw[:, :, T:].contiguous()) == 0).all()) and bool((Mw[:, :, T:] == 0).all())
    for i, n in enumerate(lens):
        assert bool((torch.view_as_real(base[0][i, :, 1 + n // H:].contiguous()) == 0).all())
        assert bool(torch.isfinite(torch.view_as_real(base[0][i].contiguous())).all())
    if not kw.get("nonstationary"):
        Ln = 9000
        nlens = edge_lengths(W, H, Ln, 7, 4)
        a = _gated(tg, make_rows(lens, L, 3), lens, make_rows(nlens, Ln, 9), nlens)
        b = _gated(tg, make_rows(lens, L, 3), lens, make_rows(nlens, Ln, 9, pad=float("nan")), nlens)
        wide_n = torch.full((7, Ln + 1000), float("inf"))
        wide_n[:, :Ln] = make_rows(nlens, Ln, 9)
        cc = _gated(tg, make_rows(lens, L, 3), lens, wide_n, nlens)
        assert _same(a, b) and _same(a, cc)
        assert not torch.equal(a[1], base[1])


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True), dict(n_fft=2048)])
def test_rows_are_independent(kw):
    from noisereduce_amd import _ffi
    n_fft = kw.get("n_fft", 1024)
    W, H, L = n_fft, n_fft // 4, 20000       # (the frame segments of the backward alone exceed the 1 MiB budget below)
    lens = edge_lengths(W, H, L, 9, 6)
    x = make_rows(lens, L, 6, pad=float("nan"))
    tg = _tg(**kw)
    T = 1 + L // H
    base = _gated(tg, x, lens)
    rev = _gated(tg, x.flip(0), lens[::-1])
    assert _same((rev[0].flip(0), rev[1].flip(0)), base)
    for i in (0, 1, 4, 8):
        # (widened by a few unread samples: a lone row that fills its tensor is an all-full call -- today's path)
        one = torch.cat([x[i:i + 1], torch.full((1, 7), float("nan"))], 1)
        Y1, M1 = _gated(tg, one, lens[i:i + 1])
        assert _same((Y1[:, :, :T], M1[:, :, :T]), (base[0][i:i + 1], base[1][i:i + 1]))
    bad = x.clone()
    bad[2, 1000] = float("nan")
    Yb, Mb = _gated(tg, bad, lens)
    keep = [i for i in range(len(lens)) if i != 2]
    assert _same((Yb[keep], Mb[keep]), (base[0][keep], base[1][keep]))
    assert bool(torch.isnan(torch.view_as_real(Yb[2].contiguous())).any())
    # sub-batches of any size give the same rows, forward and backward
    whole = tg._gate_for(torch.device("cuda", torch.cuda.current_device()))
    small = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg, max_workspace_bytes=1 << 20))
    try:
        xc = x.cuda()
        p0, m0 = whole.gate_spectrum_rows(xc, lens, save_mask=True)
        assert whole.rows_batches() == 1
        p1, m1 = small.gate_spectrum_rows(xc, lens, save_mask=True)
        assert small.rows_batches() > 1
        assert torch.equal(p0, p1) and torch.equal(m0, m1)
        assert torch.equal(torch.view_as_complex(p0).transpose(1, 2).cpu(), base[0])
        g = torch.randn(p0.shape, generator=torch.Generator().manual_seed(3)).cuda()
        gx0 = whole.gate_spectrum_rows_backward(g, m0, L, lens)
        assert whole.rows_batches() == 1
        gx1 = small.gate_spectrum_rows_backward(g, m0, L, lens)
        assert small.rows_batches() > 1
        assert torch.equal(gx0, gx1) and bool(torch.isfinite(gx0).all())
    finally:
        small.close()


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True), dict(n_fft=2048)])
def test_all_full_lengths_take_todays_path_bitwise(kw):
    B, L = 5, 9000
    x = make_rows([L] * B, L, 8).cuda()
    xn = make_rows([6000], 6000, 9).cuda()
    tg = _tg(**kw)

    def same(a, b):
        return torch.equal(torch.view_as_real(a[0].contiguous()), torch.view_as_real(b[0].contiguous())) and torch.equal(a[1], b[1])
    want = tg.gated_stft(x, return_mask=True)
    assert same(tg.gated_stft(x, return_mask=True, lengths=[L] * B), want)
    assert same(tg.gated_stft(x, return_mask=True, lengths=torch.full((B,), L, device="cuda")), want)
    assert same(tg.gated_stft(x, xn, True, [L] * B, [6000]), tg.gated_stft(x, xn, True))
    assert torch.equal(torch.view_as_real(tg.gated_stft(x, lengths=[L] * B).contiguous()), torch.view_as_real(want[0].contiguous()))


# ---- 5. backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", R.E_CELLS, ids=R.cell_id)
def test_backward_is_the_adjoint_of_each_row_alone(c, gate, dtype):
    """The rows of 9 and 17 frames (and the four others of the cell), per hop block on [0, len_i), with the mask the
    forward returned.  The gradient fields hold NaN in the frames the backward must not read."""
    tg = _tg(**R.gate_kwargs(c, gate))
    x = R.rows(c, dtype, pad=float("nan")).cuda()
    g = tg._gate_for(x.device)
    _, mask = g.gate_spectrum_rows(x, c["lens"], save_mask=True)
    F, L = c["n_fft"] // 2 + 1, c["L"]
    M = mask[:, :, :F].transpose(1, 2).cpu().numpy()               # (B, F, T)
    cfg = R.units(c, gate, dtype)[0]["cfg"]
    assert {9, 17} <= set(R.frames_of(c))
    tag = "%s %s %s" % (c["name"], gate, dtype)
    worst = {}
    for name, G in R.grad_fields(c, dtype).items():
        pairs = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(G.transpose(0, 2, 1)))).cuda()    # (B, T, F, 2)
        assert pairs.dtype == _tdt(dtype)
        gx = g.gate_spectrum_rows_backward(pairs, mask, L, c["lens"])
        assert gx.shape == (len(c["lens"]), L) and gx.dtype == _tdt(dtype)
        again = g.gate_spectrum_rows_backward(pairs, mask, L, c["lens"])
        assert torch.equal(gx, again), "%s %s: two runs differ" % (tag, name)
        zeroed = torch.nan_to_num(pairs, nan=0.0)
        assert torch.equal(g.gate_spectrum_rows_backward(zeroed, mask, L, c["lens"]), gx), \
            "%s %s: grad_Y beyond a row's own frames was read" % (tag, name)
        gx = gx.cpu().numpy()
        assert np.isfinite(gx).all(), "%s %s: the NaN beyond a row's own frames reached the gradient" % (tag, name)
        for i, n in enumerate(c["lens"]):
            Ti = R.frames_of(c)[i]
            assert not gx[i, n:].any(), (tag, name, i)
            bad, ratio = C.spec_adjoint_check(gx[i, :n], G[i, :, :Ti], M[i, :, :Ti], cfg, n)
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert len(bad) == 0, "%s %s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                tag, name, i, bad[:10].tolist(), ratio)
            if name != "dense":
                assert gx[i, :n].any(), (tag, name, i)
    # (a single cell is one rounding of the same float32 segment in the kernel and in the emulation: its ratio is 1)
    print("[gated_stft rows] %s: largest adjoint err / bud %s" % (tag, {k: round(v, 3) for k, v in worst.items()}))
    _note("%s-%s" % (c["name"], gate), **{"adjoint_%s_%s" % (k, dtype): v for k, v in worst.items()})


@pytest.mark.parametrize("kw,dtype", [(dict(), torch.float32), (dict(nonstationary=True, prop_decrease=0.7), torch.float64),
                                      (dict(n_fft=512, win_length=400, hop_length=90), torch.float32)])
def test_loss_backward_matches_autograd_on_each_row_alone(kw, dtype):
    n_fft = kw.get("n_fft", 1024)
    W = kw.get("win_length") or n_fft
    H = kw.get("hop_length") or W // 4
    L = 7000
    lens = edge_lengths(W, H, L, 6, 12)
    x = make_rows(lens, L, 12, dtype, pad=float("nan")).cuda().requires_grad_()
    tg = _tg(**kw)
    Y, M = tg.gated_stft(x, return_mask=True, lengths=lens)
    assert Y.requires_grad and not M.requires_grad
    gen = torch.Generator().manual_seed(4)
    Wt = torch.randn(Y.shape, generator=gen, dtype=torch.float64) + 1j * torch.randn(Y.shape, generator=gen, dtype=torch.float64)
    Wt = Wt.to(Y.dtype).cuda()
    for i, n in enumerate(lens):
        Wt[i, :, 1 + n // H:] = float("nan")             # ... whose gradient there is NaN and never read
    Yz = torch.where(torch.isnan(Wt.real), torch.zeros_like(Y), Y * Wt.conj())
    loss = Yz.real.sum() + (Y.abs() ** 2)[..., :9].sum()
    loss.backward()
    gx = x.grad.detach().cpu()
    assert gx.dtype == dtype and gx.shape == x.shape and bool(torch.isfinite(gx).all())
    w = torch.hann_window(W).double()
    Wc, Mc = Wt.cpu().to(torch.complex128), M.detach().cpu().double()
    for i, n in enumerate(lens):
        Ti = 1 + n // H
        x2 = x.detach().cpu()[i:i + 1, :n].double().clone().requires_grad_()
        X = torch.stft(x2, n_fft, H, W, window=w, center=True, pad_mode="constant", return_complex=True)
        Y2 = X * Mc[i:i + 1, :, :Ti]
        assert float((Y2.detach()[0] - Y.detach().cpu()[i, :, :Ti]).abs().max() / Y2.detach().abs().max()) < TOL
        l2 = (Y2 * Wc[i:i + 1, :, :Ti].conj()).real.sum() + (Y2.abs() ** 2)[..., :9].sum()
        l2.backward()
        ref = x2.grad[0]
        assert float((gx[i, :n].double() - ref).abs().max() / ref.abs().max()) < TOL, (i, n)
        assert bool((gx[i, n:] == 0).all()), (i, n)


# ---- 6. launch count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonstationary", [False, True])
def test_launch_count_does_not_depend_on_the_batch(nonstationary):
    rng = np.random.default_rng(2)
    tg = _tg(n_fft=256, nonstationary=nonstationary)
    counts = []
    for B, L in ((3, 2000), (300, 3000)):
        lens = [int(n) for n in rng.integers(512, L + 1, B)]
        lens[0] = L - 1
        x = make_rows(lens, L, 1).cuda().requires_grad_()
        g = tg._gate_for(x.device)
        g.profile_enable(True)
        g.profile_read(reset=True)
        Y = tg.gated_stft(x, lengths=lens)
        fwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        assert g.rows_batches() == 1
        torch.view_as_real(Y).sum().backward()
        bwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        g.profile_enable(False)
        counts.append((fwd, bwd))
    assert counts[0] == counts[1]
    assert sum(counts[0][0].values()) == (4 if nonstationary else 5) and sum(counts[0][1].values()) == 2, counts[0]


# ---- 7. an n_fft the table-driven kernels are not built for ---------------------------------------------------------------------------
def test_other_n_fft_gates_row_by_row_and_the_engine_refuses_them():
    tg = _tg(n_fft=400)
    lens = [8000, 4000, 2001]
    x = make_rows(lens, 8000, 0).cuda().requires_grad_()
    xn = make_rows([3000], 3000, 1).cuda()
    Y, M = tg.gated_stft(x, xn, return_mask=True, lengths=lens, xn_lengths=[2500])
    T = 1 + 8000 // 100
    assert tuple(Y.shape) == tuple(M.shape) == (3, 201, T) and Y.dtype == torch.complex64 and Y.transpose(1, 2).is_contiguous()
    for i, n in enumerate(lens):
        Ya, Ma = tg.gated_stft(x[i:i + 1, :n], xn[:, :2500], return_mask=True)
        Ti = 1 + n // 100
        assert torch.equal(torch.view_as_real(Y[i, :, :Ti].detach().contiguous()), torch.view_as_real(Ya[0].detach().contiguous()))
        assert torch.equal(M[i, :, :Ti], Ma[0])
        assert bool((torch.view_as_real(Y[i, :, Ti:].detach().contiguous()) == 0).all()) and bool((M[i, :, Ti:] == 0).all())
    (Y.abs() ** 2).sum().backward()
    gx = x.grad
    assert bool(torch.isfinite(gx).all()) and bool((gx[1, 4000:] == 0).all()) and bool((gx[2, 2001:] == 0).all())
    assert bool(gx[1, :4000].any())
    g = tg._gate_for(x.device)
    with pytest.raises(NotImplementedError, match="sg_gate_spectrum_rows: n_fft must be a power of two"):
        g.gate_spectrum_rows(x.detach(), lens)
    # and refuses bad lengths by itself
    tg2 = _tg()
    g2 = tg2._gate_for(x.device)
    with pytest.raises(ValueError, match=r"sg_gate_spectrum_rows: lengths\[1\] = 100"):
        g2.gate_spectrum_rows(x.detach(), [8000, 100, 4000])
    with pytest.raises(ValueError, match=r"sg_gate_spectrum_rows_backward: lengths\[2\] = 9000"):
        g2.gate_spectrum_rows_backward(torch.zeros((3, 32, 513, 2), device="cuda"), torch.zeros((3, 32, 528), device="cuda"),
                                       8000, [8000, 4000, 9000])
