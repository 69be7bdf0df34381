"""TorchGate.gated_filterbank on the GPU (sg_gate_features / sg_gate_features_backward, csrc/feat.hip; the composed route for
an n_fft the kernels are not built for and for ragged lengths) held to the float64 statement of
tests/gated_filterbank_cases.py: the features frame by frame, the gradient per hop block.  The rule and what it catches:
tests/test_gated_filterbank_host.py."""
import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import gated_filterbank_cases as K
from tests import gated_stft_cases as C
from tests import parity_budget as PB

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
DTYPE_IDS = ["f32", "f64"]


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _setup(case, variant, dtype):
    from noisereduce_amd.torchgate import TorchGate
    x = torch.from_numpy(C.make_x(case, _np_dtype(dtype))).cuda()
    xn = C.make_xn(case, C.VARIANTS[variant][1], _np_dtype(dtype))
    xn = None if xn is None else torch.from_numpy(xn).cuda()
    tg = TorchGate(sr=C.CASES[case]["sr"], **C.gate_kwargs(case, variant)).cuda()
    return tg, x, xn


def _fb(bname, case):
    return torch.from_numpy(K.bank(bname, case).copy())


def _ln_eps(dtype):
    """ln(eps) rounded to the output type."""
    return np.array(np.log(np.float64(K.EPS))).astype(_np_dtype(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cell", K.FWD_CELLS, ids=K.FWD_IDS)
def test_forward_mask_log_and_layout(cell, dtype):
    """Both powers, log off and on: the linear features per frame against the float64 composition with the kernel's own
    mask; the mask bitwise gated_stft's; ln(lin + eps) against the float32 rounding of that expression; the layout."""
    case, variant, bname = cell
    tg, x, xn = _setup(case, variant, dtype)
    ref = K.reference(case, variant, np.dtype(_np_dtype(dtype)).name)
    fb = K.bank(bname, case)
    fbt = _fb(bname, case)
    B, F, T = ref["X"].shape
    M = fb.shape[1]
    _, mask_spec = tg.gated_stft(x, xn, return_mask=True)
    for power in K.cell_powers(bname):
        lin, mask = tg.gated_filterbank(x, fbt, xn, power=float(power), return_mask=True)
        assert tuple(lin.shape) == (B, M, T) and lin.dtype == dtype and lin.stride() == (T * M, 1, M)
        assert tuple(mask.shape) == (B, F, T) and mask.dtype == torch.float32 and not mask.requires_grad
        assert torch.equal(mask, mask_spec)
        assert torch.equal(tg.gated_filterbank(x, fbt, xn, power=float(power)), lin)
        got, Mk = lin.cpu().numpy(), mask.cpu().numpy()
        assert np.isfinite(got).all()
        worst = 0.0
        for b in range(B):
            bad, ratio = K.feature_check(got[b], ref["X"][b], Mk[b], fb, power, ref["emu"][b])
            worst = max(worst, ratio)
            assert bad.size == 0, (power, b, bad, ratio)
        if bname == "zero_last":
            assert not got[:, -1, :].any()
        if bname == "neg":
            assert (got < 0).any()          # nothing clamps a negative sum
            continue
        lg = tg.gated_filterbank(x, fbt, xn, power=float(power), log=True, eps=K.EPS)
        assert tuple(lg.shape) == (B, M, T) and lg.dtype == dtype and lg.stride() == (T * M, 1, M)
        lg = lg.cpu().numpy().astype(np.float64)
        want_log = np.log(got.astype(np.float64) + K.EPS)
        lerr = np.abs(lg - want_log) / K.log_allowed(want_log)
        print(f"[gated_filterbank] {case}-{variant}-{bname} {dtype} power {power}: worst err / budget {worst:.3f}, "
              f"log err / allowed {lerr.max():.3f}")
        assert lerr.max() <= 1.0, (power, float(lerr.max()))
        if bname == "zero_last":
            assert np.all(lg[:, -1, :] == _ln_eps(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cell", K.BWD_CELLS, ids=K.BWD_IDS)
def test_backward(cell, dtype):
    """grad_x against C.adjoint_np of the float64 G per hop block (mask: the kernel's; upstream gradient: seeded normal),
    both powers, log off and on."""
    case, variant, bname = cell
    tg, x, xn = _setup(case, variant, dtype)
    ref = K.reference(case, variant, np.dtype(_np_dtype(dtype)).name)
    fb = K.bank(bname, case)
    fbt = _fb(bname, case)
    c = C.CASES[case]
    g = K.upstream(case, bname)
    gt = torch.from_numpy(g).to(dtype).cuda()
    g = gt.cpu().numpy().astype(np.float64)           # what the kernel was given
    for power in K.POWERS:
        for log in (False, True):
            xg = x.clone().requires_grad_(True)
            out, mask = tg.gated_filterbank(xg, fbt, xn, power=float(power), log=log, eps=K.EPS, return_mask=True)
            out.backward(gt)
            gx, Mk = xg.grad.cpu().numpy(), mask.cpu().numpy()
            assert gx.shape == (c["B"], c["L"]) and xg.grad.dtype == dtype and np.isfinite(gx).all()
            worst = 0.0
            for b in range(c["B"]):
                G64 = K.spectrum_grad(ref["X"][b], Mk[b], fb, g[b], power, log)
                G32 = K.spectrum_grad32(ref["emu"][b], Mk[b], fb, g[b], power, log)
                bad, ratio = K.grad_check(gx[b], G64, G32, case, c["L"])
                worst = max(worst, ratio)
                assert bad.size == 0, (power, log, b, bad, ratio)
            print(f"[gated_filterbank] backward {case}-{bname} {dtype} power {power} log {log}: worst err / budget {worst:.3f}")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("power", K.POWERS)
def test_zero_filter_contributes_no_gradient(power, log):
    tg, x, _ = _setup("a", "plain", torch.float32)
    fbt = _fb("zero_last", "a")
    xg = x.clone().requires_grad_(True)
    out = tg.gated_filterbank(xg, fbt, power=float(power), log=log)
    g = torch.zeros_like(out)
    g[:, -1, :] = 1.0
    out.backward(g)
    assert not xg.grad.any()


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_power_one_on_digital_silence(dtype):
    """|X| = 0 everywhere in a row: finite features, and the derivative of |X| at 0 taken as 0 -- a zero gradient, no NaN."""
    tg, x, _ = _setup("a", "plain", dtype)
    x = x.clone()
    x[1] = 0.0
    fbt = _fb("mel80", "a")
    for log in (False, True):
        xg = x.clone().requires_grad_(True)
        out = tg.gated_filterbank(xg, fbt, power=1.0, log=log)
        assert torch.isfinite(out).all()
        out.backward(torch.ones_like(out))
        assert torch.isfinite(xg.grad).all()
        assert not xg.grad[1].any() and xg.grad[0].any() and xg.grad[2].any()
        if not log:
            assert not out[1].any()


def test_two_runs_give_the_same_bits():
    tg, x, _ = _setup("f", "plain", torch.float32)
    fbt = _fb("mel80", "f")
    g = torch.from_numpy(K.upstream("f", "mel80")).float().cuda()
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        out = tg.gated_filterbank(xg, fbt, log=True)
        out.backward(g)
        runs.append((out.detach().clone(), xg.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("case", ["a", "h"])
def test_all_full_lengths_are_the_full_length_call(case):
    tg, x, _ = _setup(case, "plain", torch.float32)
    fbt = _fb("mel40", case)
    B, L = x.shape
    for kw in (dict(), dict(log=True, power=1.0)):
        want, wm = tg.gated_filterbank(x, fbt, return_mask=True, **kw)
        got, gm = tg.gated_filterbank(x, fbt, return_mask=True, lengths=[L] * B, **kw)
        assert torch.equal(got, want) and torch.equal(gm, wm)
        assert torch.equal(tg.gated_filterbank(x, fbt, lengths=torch.full((B,), L), **kw), want)


@pytest.mark.parametrize("power", K.POWERS)
def test_ragged_lengths(power):
    """lengths= (the composed route): every row within the forward budget of the float64 composition on the row alone,
    as the call on the row alone is; the tail frames hold 0 / ln(eps); no gradient beyond lengths[i]."""
    case = "a"
    tg, x, _ = _setup(case, "plain", torch.float32)
    fb = K.bank("mel80", case)
    fbt = _fb("mel80", case)
    n_fft, W, H = C.geometry(case)
    cfg = K.cfg_of(case)
    lens = [2300, 2111, 2048]
    xg = x.clone().requires_grad_(True)
    lin, mask = tg.gated_filterbank(xg, fbt, power=float(power), return_mask=True, lengths=lens)
    lg = tg.gated_filterbank(x, fbt, power=float(power), log=True, lengths=lens)
    lin.sum().backward()
    T = lin.shape[-1]
    Tn = tg.stft_lengths(lens)
    got, Mk, lgn, gx = lin.detach().cpu().numpy(), mask.cpu().numpy(), lg.cpu().numpy(), xg.grad.cpu().numpy()
    assert T == 1 + x.shape[1] // H
    for i, n in enumerate(lens):
        Ti = int(Tn[i])
        assert Ti == 1 + n // H
        row = x[i, :n].cpu().numpy().astype(np.float64)
        X64 = O.stft_torch(row[None], n_fft, W, H, cfg["window"])[0]
        emu = PB.spectrum_f32(dict(x=row, cfg=cfg))
        bad, ratio = K.feature_check(got[i][:, :Ti], X64, Mk[i][:, :Ti], fb, power, emu)
        assert bad.size == 0, (i, bad, ratio)
        alone, am = tg.gated_filterbank(x[i:i + 1, :n], fbt, power=float(power), return_mask=True)
        bad, ratio = K.feature_check(alone[0].cpu().numpy(), X64, am[0].cpu().numpy(), fb, power, emu)
        assert bad.size == 0, (i, bad, ratio)
        assert not got[i][:, Ti:].any() and not Mk[i][:, Ti:].any()
        assert np.all(lgn[i][:, Ti:] == _ln_eps(torch.float32))
        assert not gx[i, n:].any() and gx[i, :n].any()


def test_the_bank_cache_sees_a_new_bank_and_an_edit_in_place():
    tg, x, _ = _setup("c", "plain", torch.float32)
    fb1 = _fb("mel40", "c")
    a = tg.gated_filterbank(x, fb1)
    fb2 = fb1 * 2.0                                   # another object, other values
    b = tg.gated_filterbank(x, fb2)
    assert torch.equal(b, tg.gated_filterbank(x, fb2)) and not torch.equal(a, b)
    assert torch.allclose(b, 2.0 * a, rtol=1e-6, atol=0.0)
    assert torch.equal(tg.gated_filterbank(x, fb1), a)
    v = fb1._version
    fb1[:, 0] = 0.0                                   # an edit in place: same address, _version bumped
    assert fb1._version > v
    c = tg.gated_filterbank(x, fb1)
    assert not c[:, 0, :].any() and torch.equal(c[:, 1:, :], a[:, 1:, :])
    # a device bank and a numpy bank are taken too
    assert torch.equal(tg.gated_filterbank(x, fb2.cuda()), b)
    assert torch.equal(tg.gated_filterbank(x, fb2.numpy()), b)
    # a second module with the same parameters shares the handle: each call still sees its own bank
    from noisereduce_amd.torchgate import TorchGate
    tg2 = TorchGate(sr=C.CASES["c"]["sr"], **C.gate_kwargs("c", "plain")).cuda()
    assert torch.equal(tg2.gated_filterbank(x, fb2), b) and torch.equal(tg.gated_filterbank(x, fb1), c)


def test_entry_points_refuse_as_sg_gate_spectrum_does():
    from noisereduce_amd import _ffi
    from tests.test_gpu_gated_stft import _gate_like
    tg, x, _ = _setup("c", "plain", torch.float32)
    gate = _gate_like(tg)
    with pytest.raises(Exception, match="no filterbank set"):
        gate.gate_features(x)
    # the C entry point says so itself (a caller of the C ABI has no wrapper in front of it)
    out = torch.empty((x.shape[0], gate.n_frames(x.shape[1]), 40), device="cuda")
    rc = gate.lib.sg_gate_features(gate._h, x.data_ptr(), _ffi.SG_F32, x.shape[0], x.shape[1], x.stride(0), None, 0, 0, 0, 2, 0,
                                   1e-6, out.data_ptr(), None, gate._stream())
    assert rc == _ffi.SG_E_INVALID and b"no filterbank set" in gate.lib.sg_last_error(gate._h)
    gate.set_filterbank(K.bank("mel40", "c"))
    first = gate.gate_features(x)
    with pytest.raises(Exception, match="power must be 1 or 2"):
        gate.gate_features(x, power=3)
    bad = K.bank("mel40", "c").copy()
    bad[5, 5] = np.inf
    with pytest.raises(Exception, match="non-finite"):
        gate.set_filterbank(bad)
    assert torch.equal(gate.gate_features(x), first)               # a refused bank leaves the earlier one in place
    tg_h, xh, _ = _setup("h", "plain", torch.float32)
    gate_h = _gate_like(tg_h)
    with pytest.raises(Exception, match="powers of two from 256 to 4096"):
        gate_h.set_filterbank(K.bank("mel40", "h"))
    assert _ffi.load_library().sg_version() == 100
