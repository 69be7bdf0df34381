"""TorchGate.gated_stft on the GPU (sg_gate_spectrum / sg_gate_spectrum_backward, csrc/spec.hip; the composed route for an
n_fft the kernels are not built for) against the float64 oracle stages, torch autograd in float64 and the numpy adjoint of
tests/gated_stft_cases.py.  The inputs and their conditions: tests/gated_stft_cases.py, tests/test_gated_stft_host.py."""
import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import gated_stft_cases as C

pytestmark = pytest.mark.gpu

TOL = 1e-4            # the project's parity bar (tests/test_gpu_parity.py)
MASK_TOL = 2.4e-7     # two float32 ulps at 1.0 (measured: <= 1.6e-7 through the float smoothing kernels)
DTYPES = [torch.float32, torch.float64]


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _setup(case, variant, dtype):
    from noisereduce_amd.torchgate import TorchGate
    x = torch.from_numpy(C.make_x(case, _np_dtype(dtype))).cuda()
    xn = C.make_xn(case, C.VARIANTS[variant][1], _np_dtype(dtype))
    xn = None if xn is None else torch.from_numpy(xn).cuda()
    tg = TorchGate(sr=C.CASES[case]["sr"], **C.gate_kwargs(case, variant)).cuda()
    return tg, x, xn


def _pairs(z):
    z = np.asarray(z)
    return np.stack([z.real, z.imag])


def _istft(tg, Y):
    w = torch.hann_window(tg.win_length, device=Y.device).to(Y.real.dtype)
    return torch.istft(Y, tg.n_fft, tg.hop_length, tg.win_length, window=w, center=True)


def _gate_like(tg, **extra):
    """A handle of its own with the parameters TorchGate._gate_for passes (plus e.g. max_workspace_bytes)."""
    from noisereduce_amd import _ffi
    nf, nt = tg._n_grad
    return _ffi.Gate("cuda", variant=_ffi.SG_VARIANT_T, stationary=not tg.nonstationary, n_fft=tg.n_fft,
                     win_length=tg.win_length, hop_length=tg.hop_length, n_grad_freq=nf, n_grad_time=nt,
                     smooth_mask=tg.smoothing_filter is not None, prop_decrease=tg.prop_decrease,
                     n_std_thresh=tg.n_std_thresh_stationary, top_db=40.0, ddof=1, n_movemean=tg.n_movemean_nonstationary,
                     nonstat_thresh=tg.n_thresh_nonstationary, nonstat_slope=1.0 / tg.temp_coeff_nonstationary,
                     window=torch.hann_window(tg.win_length).double().numpy(), **extra)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case,variant", C.RUNS, ids=C.RUN_IDS)
def test_spectrum_mask_forward_and_layout(case, variant, dtype):
    """Assertions 1 - 4: the spectrum and the mask against the oracle stages, torch.istft(Y) against forward, the layout."""
    from noisereduce_amd import _ffi
    tg, x, xn = _setup(case, variant, dtype)
    _, st = C.oracle(case, variant, np.dtype(_np_dtype(dtype)).name)
    want = st["X"] * st["mask"]
    B, F, T = want.shape
    Y, mask = tg.gated_stft(x, xn, return_mask=True)
    # 4. layout: torch.stft's own
    assert tuple(Y.shape) == (B, F, T) and Y.stride() == (T * F, 1, F)
    assert Y.dtype == (torch.complex64 if dtype == torch.float32 else torch.complex128)
    assert tuple(mask.shape) == (B, F, T) and mask.dtype == torch.float32 and not mask.requires_grad
    assert mask.stride()[1] == 1 and mask.stride()[2] == (F + 15) // 16 * 16      # a view of the padded buffer, no copy
    assert torch.equal(Y.contiguous() * 1, Y * 1) and torch.equal(Y.contiguous().abs(), Y.abs())
    only = tg.gated_stft(x, xn)
    assert torch.equal(torch.view_as_real(only), torch.view_as_real(Y))
    # 1. spectrum
    got = Y.cpu().numpy()
    err = O.rel_err(_pairs(got), _pairs(want))
    row_err = max(np.abs(got[b] - want[b]).max() / np.abs(want[b]).max() for b in range(B))
    # 2. mask
    m = mask.cpu().numpy()
    mask_err = float(np.abs(m - st["mask"]).max())
    print(f"[gated_stft] {case}-{variant} {dtype}: spectrum rel err {err:.3e}, worst row {row_err:.3e}, mask err {mask_err:.3e}")
    assert err < TOL and row_err < TOL, (err, row_err)
    gate = tg._gate_for(x.device)
    if variant == "nonstat":
        assert mask_err < 1e-4, mask_err
    else:
        assert mask_err <= MASK_TOL, mask_err
        with gate.with_options([(_ffi.SG_OPT_FORCE_NOFAST, 1)]):
            _, m2 = gate.process_batch(x, xn, save_mask=True)
        assert torch.equal(m2[:, :, :F], mask.transpose(1, 2)), \
            "max diff %.3e" % float((m2[:, :, :F] - mask.transpose(1, 2)).abs().max())
    # 3. consistency with forward
    y = tg(x, xn)
    back = _istft(tg, Y)
    assert back.shape == y.shape
    ferr = O.rel_err(back.cpu().numpy(), y.cpu().numpy())
    print(f"[gated_stft] {case}-{variant} {dtype}: istft(Y) vs forward {ferr:.3e}")
    assert ferr < TOL, ferr


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case,variant", C.BACKWARD_RUNS, ids=C.BACKWARD_IDS)
def test_backward(case, variant, dtype):
    """Assertion 5: x.grad against torch autograd in float64 through torch.stft(x64) * M and against the numpy adjoint;
    the loss through torch.istft(Y) against forward's backward; nothing flows to xn."""
    tg, x, xn = _setup(case, variant, dtype)
    n, W, H = tg.n_fft, tg.win_length, tg.hop_length
    L = x.shape[1]
    x.requires_grad_()
    if xn is not None:
        xn.requires_grad_()
    Y, mask = tg.gated_stft(x, xn, return_mask=True)
    assert Y.requires_grad and not mask.requires_grad
    gen = torch.Generator().manual_seed(11)
    G = torch.complex(torch.randn(Y.shape, generator=gen, dtype=torch.float64),
                      torch.randn(Y.shape, generator=gen, dtype=torch.float64)).cuda()
    loss = (torch.view_as_real(Y) * torch.view_as_real(G.to(Y.dtype))).sum()
    loss.backward()
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    assert xn is None or xn.grad is None
    gx = x.grad.detach().double().cpu().numpy()
    Gq = G.to(Y.dtype).to(torch.complex128)   # the gradient the kernel saw
    # reference 1: torch autograd in float64 with the same mask
    w = torch.hann_window(W).double().cuda()
    x64 = x.detach().double().clone().requires_grad_()
    X = torch.stft(x64, n, H, W, window=w, center=True, pad_mode="constant", return_complex=True)
    (torch.view_as_real(X * mask.double()) * torch.view_as_real(Gq)).sum().backward()
    ref1 = x64.grad.cpu().numpy()
    # reference 2: the numpy adjoint
    ref2 = C.adjoint_np(Gq.cpu().numpy(), mask.cpu().numpy(), n, W, H, L, C.window64(case))
    e1 = np.abs(gx - ref1).max() / np.abs(ref1).max()
    e2 = np.abs(gx - ref2).max() / np.abs(ref2).max()
    print(f"[gated_stft] {case}-{variant} {dtype}: backward vs autograd {e1:.3e}, vs numpy adjoint {e2:.3e}")
    assert e1 < TOL and e2 < TOL, (e1, e2)
    # the triangle: a loss through torch.istft(Y) is forward's backward
    x.grad = None
    y1 = _istft(tg, tg.gated_stft(x, xn))
    gy = torch.randn(y1.shape, generator=gen, dtype=torch.float64).to(y1.dtype).cuda()
    y1.backward(gy)
    g1 = x.grad.detach().double().clone()
    x.grad = None
    tg(x, xn).backward(gy)
    g2 = x.grad.detach().double()
    e3 = float((g1 - g2).abs().max() / g2.abs().max())
    print(f"[gated_stft] {case}-{variant} {dtype}: istft(Y) backward vs forward's {e3:.3e}")
    assert e3 < TOL, e3


@pytest.mark.parametrize("case,variant", [("a", "plain"), ("c", "plain"), ("a", "nonstat")], ids=["a", "c", "a-nonstat"])
def test_rows_are_independent_and_runs_repeat(case, variant):
    """Assertion 6."""
    tg, x, _ = _setup(case, variant, torch.float32)
    x.requires_grad_()
    Y, mask = tg.gated_stft(x, return_mask=True)
    R, M = torch.view_as_real(Y).detach(), mask.clone()
    i = 1
    alone, m_alone = tg.gated_stft(x[i:i + 1].detach(), return_mask=True)
    assert torch.equal(torch.view_as_real(alone)[0], R[i]) and torch.equal(m_alone[0], M[i])
    other = x.detach().clone()
    other[0] = other[0].flip(0) * 1.7
    other[2] = torch.randn_like(other[2])
    assert torch.equal(torch.view_as_real(tg.gated_stft(other))[i], R[i])
    poisoned = x.detach().clone()
    poisoned[0] = float("nan")
    Yp, mp = tg.gated_stft(poisoned, return_mask=True)
    assert torch.equal(torch.view_as_real(Yp)[1:], R[1:]) and torch.equal(mp[1:], M[1:])
    # two consecutive calls: identical bits, forward and backward
    G = torch.randn_like(R)
    (torch.view_as_real(Y) * G).sum().backward()
    g1 = x.grad.clone()
    x.grad = None
    Y2 = tg.gated_stft(x)
    assert torch.equal(torch.view_as_real(Y2), R)
    (torch.view_as_real(Y2) * G).sum().backward()
    assert torch.equal(x.grad, g1)


@pytest.mark.parametrize("case,variant,budget", [("a", "plain", 1 << 10), ("a", "xnB", 1 << 10), ("b", "plain", 1 << 10),
                                                 ("b", "nonstat", 1 << 10), ("g", "plain", 8 << 20)],
                         ids=["a", "a-xnB", "b", "b-nonstat", "g"])
def test_workspace_budget_split_is_invisible(case, variant, budget):
    """A budget that splits the batch into at least two sub-batches gives bitwise the unsplit spectrum, mask and gradient."""
    tg, x, xn = _setup(case, variant, torch.float32)
    if tg.nonstationary:
        xn = None
    big, small = _gate_like(tg), _gate_like(tg, max_workspace_bytes=budget)
    try:
        Y0, m0 = big.gate_spectrum(x, xn, save_mask=True)
        Y1, m1 = small.gate_spectrum(x, xn, save_mask=True)
        F = tg.n_fft // 2 + 1
        assert torch.equal(Y0, Y1) and torch.equal(m0[:, :, :F], m1[:, :, :F])
        Yt, mt = tg.gated_stft(x, xn, return_mask=True)
        assert torch.equal(torch.view_as_real(Yt), Y0.permute(0, 2, 1, 3)) and torch.equal(mt, m0[:, :, :F].transpose(1, 2))
        G = torch.randn_like(Y0)
        g0 = big.gate_spectrum_backward(G, m0, x.shape[1])
        g1 = small.gate_spectrum_backward(G, m0, x.shape[1])
        assert torch.equal(g0, g1)
    finally:
        big.close()
        small.close()


@pytest.mark.parametrize("case", ["a", "b", "e"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_guard_bands(case, dtype):
    """Assertion 7: nothing outside spec, mask and grad_x is written; x with a row stride and NaN between the rows."""
    tg, x, _ = _setup(case, "plain", dtype)
    gate = tg._gate_for(x.device)
    B, L = x.shape
    F, T = tg.n_fft // 2 + 1, 1 + L // tg.hop_length
    FS = (F + 15) // 16 * 16
    Y0, m0 = gate.gate_spectrum(x, save_mask=True)
    PAD, S = 64, 1234.5
    big = torch.full((B * T * F * 2 + 2 * PAD,), S, dtype=dtype, device="cuda")
    bigm = torch.full((B * T * FS + 2 * PAD,), S, dtype=torch.float32, device="cuda")
    wide = torch.full((B, L + 37), float("nan"), dtype=dtype, device="cuda")
    wide[:, :L] = x
    xv = wide[:, :L]
    assert xv.stride(0) == L + 37
    Y1, m1 = gate.gate_spectrum(xv, out=big[PAD:-PAD].view(B, T, F, 2), mask_out=bigm[PAD:-PAD].view(B, T, FS))
    assert torch.equal(Y1, Y0) and torch.equal(m1[:, :, :F], m0[:, :, :F])
    for t in (big, bigm):
        assert bool((t[:PAD] == S).all()) and bool((t[-PAD:] == S).all())
    G = torch.randn_like(Y0)
    g0 = gate.gate_spectrum_backward(G, m0, L)
    bigg = torch.full((B, L + 40), S, dtype=dtype, device="cuda")
    g1 = gate.gate_spectrum_backward(G, m0, L, out=bigg[:, 20:20 + L])
    assert torch.equal(g1, g0)
    assert bool((bigg[:, :20] == S).all()) and bool((bigg[:, 20 + L:] == S).all())


def test_c_level_errors_leave_the_handle_usable():
    """Assertion 8."""
    from noisereduce_amd import _ffi
    tg, x, _ = _setup("a", "plain", torch.float32)
    gate = tg._gate_for(x.device)
    B, L = x.shape
    good, gmask = gate.gate_spectrum(x, save_mask=True)

    def still_fine():
        again, m = gate.gate_spectrum(x, save_mask=True)
        assert torch.equal(again, good)
        assert torch.equal(gate.gate_spectrum_backward(good, m, L), gate.gate_spectrum_backward(good, gmask, L))

    with pytest.raises(ValueError, match="x must be bigger than 2048"):
        gate.gate_spectrum(x[:, :2047].contiguous())
    still_fine()
    with pytest.raises(ValueError, match="xn rows"):
        gate.gate_spectrum(x, x[:2, :2100].contiguous())
    still_fine()
    with pytest.raises(ValueError, match="x must be bigger than 2048"):
        gate.gate_spectrum_backward(good[:, :4].contiguous(), gmask, 1024)
    still_fine()
    # null pointers, straight through the C ABI
    st = gate._stream()
    with torch.cuda.device(gate.device):
        rc = gate.lib.sg_gate_spectrum(gate._h, None, _ffi.SG_F32, B, L, L, None, 0, 0, 0, good.data_ptr(), None, st)
        assert rc == _ffi.SG_E_INVALID and gate.lib.sg_last_error(gate._h)
        rc = gate.lib.sg_gate_spectrum(gate._h, x.data_ptr(), _ffi.SG_F32, B, L, L, None, 0, 0, 0, None, None, st)
        assert rc == _ffi.SG_E_INVALID and gate.lib.sg_last_error(gate._h)
        rc = gate.lib.sg_gate_spectrum_backward(gate._h, good.data_ptr(), _ffi.SG_F32, B, L, None, x.data_ptr(), L, st)
        assert rc == _ffi.SG_E_INVALID and gate.lib.sg_last_error(gate._h)
        rc = gate.lib.sg_gate_spectrum(gate._h, x.data_ptr(), _ffi.SG_I16, B, L, L, None, 0, 0, 0, good.data_ptr(), None, st)
        assert rc == _ffi.SG_E_INVALID
    still_fine()
    kw = dict(stationary=True, n_fft=1024, win_length=1024, hop_length=256)
    s_gate = _ffi.Gate("cuda", variant=_ffi.SG_VARIANT_S, **kw)
    try:
        with pytest.raises(ValueError, match="variant-T"):
            s_gate.gate_spectrum(x)
        with pytest.raises(ValueError, match="variant-T"):
            s_gate.gate_spectrum_backward(good, gmask, L)
    finally:
        s_gate.close()
    odd = _ffi.Gate("cuda", variant=_ffi.SG_VARIANT_T, stationary=True, n_fft=400, win_length=400, hop_length=100)
    try:
        with pytest.raises(NotImplementedError, match="n_fft=400"):
            odd.gate_spectrum(x)
        y = odd.process_batch(x)                       # the handle still gates
        assert bool(torch.isfinite(y).all())
    finally:
        odd.close()
    still_fine()
