"""TorchGate.forward(x, lengths=...) on the GPU: every row of a padded batch against the reference's algorithm on the
row alone (torch port and numpy oracle), against today's full-length kernels on the row alone, and the contract's
invariants (padding never read, rows independent, all-full routing, backward, launch count, errors)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import spectralgate_oracle as O  # noqa: E402
from oracle.torchgate_torch_port import torchgate_cpu  # noqa: E402
from tests.parity_budget import torchgate_gate_kwargs as _gate_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu
SR = 16000
TOL = 1e-4        # parity bar against the oracles (tests/test_gpu_parity.py)
TOL_PATHS = 2e-6  # cross-path bound (tests/test_gpu_batch_fuzz.py, tests/test_gpu_rowgate.py)


def make_rows(lens, L, seed, dtype=torch.float32, pad=0.0):
    """0.1 * noise + 0.5 * a 440 Hz tone gated on and off, row i valid on [0, lens[i]) and `pad` after it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((len(lens), L), pad, dtype=torch.float64)
    for i, n in enumerate(lens):
        t = torch.arange(n, dtype=torch.float64) / SR
        period = 0.5 if n >= 8000 else n / SR / 2.5
        x[i, :n] = 0.1 * torch.randn(n, generator=g, dtype=torch.float64) + \
            0.5 * torch.sin(2 * math.pi * 440 * t) * ((t % period) < period / 2)
    return x.to(dtype)


def edge_lengths(W, H, L, count, seed):
    """Lengths from [2 W, L]: both ends, multiples of H and their neighbours, then uniform draws."""
    rng = np.random.default_rng(seed)
    k = (2 * W + H - 1) // H + 1
    fixed = [2 * W, L, k * H, k * H - 1 if k * H - 1 >= 2 * W else 2 * W, k * H + 1, 2 * W + 1, H * (L // H), H * (L // H) - 1]
    fixed = [min(max(n, 2 * W), L) for n in fixed]
    out = fixed[:count] + [int(n) for n in rng.integers(2 * W, L + 1, max(0, count - len(fixed)))]
    return out


# name -> (TorchGate kwargs, L, B, xn mode, dtype); xn mode: None / "shared" / "rows" / "rows_len" (padded noise rows)
CASES = {
    "default_f32": (dict(), 16000, 8, None, torch.float32),
    "default_f64_prop07": (dict(prop_decrease=0.7), 12000, 6, None, torch.float64),
    "default_shared_xn": (dict(), 9000, 5, "shared", torch.float32),
    "default_rows_xn": (dict(prop_decrease=0.7), 9000, 5, "rows", torch.float32),
    "default_rows_xn_len": (dict(), 9000, 6, "rows_len", torch.float64),
    "nonstat_f32": (dict(nonstationary=True), 16000, 8, None, torch.float32),
    "nonstat_f64_prop07": (dict(nonstationary=True, prop_decrease=0.7), 12000, 6, None, torch.float64),
    "n256_many": (dict(n_fft=256), 2000, 300, None, torch.float32),
    "n256_nonstat_win200_hop37": (dict(n_fft=256, win_length=200, hop_length=37, nonstationary=True), 3000, 9, None, torch.float32),
    "n512_win400_hop90_nosmooth": (dict(n_fft=512, win_length=400, hop_length=90, freq_mask_smooth_hz=None,
                                        time_mask_smooth_ms=None), 5000, 9, None, torch.float32),
    "n1024_hop200_freq_off": (dict(hop_length=200, freq_mask_smooth_hz=None, prop_decrease=0.7), 9000, 8, "shared", torch.float32),
    "n2048_time_off": (dict(n_fft=2048, time_mask_smooth_ms=None), 16000, 8, None, torch.float32),
    "n2048_nonstat_nosmooth": (dict(n_fft=2048, win_length=1500, hop_length=300, nonstationary=True,
                                    freq_mask_smooth_hz=None, time_mask_smooth_ms=None), 12000, 6, None, torch.float64),
    "n4096": (dict(n_fft=4096, time_mask_smooth_ms=200), 30000, 6, None, torch.float32),
    "n4096_nonstat_win3000_hop700": (dict(n_fft=4096, win_length=3000, hop_length=700, nonstationary=True, prop_decrease=0.7),
                                     24000, 5, None, torch.float32),
}


def build_case(name):
    kw, L, B, xn_mode, dtype = CASES[name]
    n_fft = kw.get("n_fft", 1024)
    W = kw.get("win_length") or n_fft
    H = kw.get("hop_length") or W // 4
    seed = sorted(CASES).index(name)
    lens = edge_lengths(W, H, L, B, seed)
    x = make_rows(lens, L, seed, dtype)
    xn, xn_lens = None, None
    if xn_mode == "shared":
        xn = make_rows([max(2 * W, 5000)], max(2 * W, 5000), 100 + seed, dtype)
    elif xn_mode == "rows":
        xn = make_rows([max(2 * W, 6000)] * B, max(2 * W, 6000), 100 + seed, dtype)
    elif xn_mode == "rows_len":
        Ln = max(2 * W, 7000)
        xn_lens = edge_lengths(W, H, Ln, B, 200 + seed)
        xn = make_rows(xn_lens, Ln, 100 + seed, dtype, pad=float("nan"))
    return kw, W, H, lens, x, xn, xn_lens


def noise_of(xn, xn_lens, i):
    if xn is None:
        return None
    r = xn[i if xn.shape[0] > 1 else 0]
    if xn_lens is not None:
        r = r[:xn_lens[i if len(xn_lens) > 1 else 0]]
    return r[None]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def gate_rows(tg, x, lens, xn=None, xn_lens=None):
    return tg(x.cuda(), None if xn is None else xn.cuda(), lengths=lens, xn_lengths=xn_lens).cpu()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_row_matches_the_oracles_on_the_row_alone(name):
    from noisereduce_amd.torchgate import TorchGate
    kw, W, H, lens, x, xn, xn_lens = build_case(name)
    tg = TorchGate(sr=SR, **kw).cuda()
    y = gate_rows(tg, x, lens, xn, xn_lens)
    assert y.shape == (len(lens), H * (x.shape[1] // H)) and y.dtype == x.dtype
    win = torch.hann_window(W).double().numpy()
    worst_port = worst_np = 0.0
    for i, n in enumerate(lens):
        xi, ni = x[i:i + 1, :n], noise_of(xn, xn_lens, i)
        want, st = O.torchgate_T(xi.double().numpy(), SR, xn=None if ni is None else ni.double().numpy(), window=win,
                                 return_stages=True, **kw)
        frac = float(np.mean(st["raw"] > 0.5))
        assert 0.01 <= frac <= 0.99, (name, i, n, frac)   # an all-pass or all-block mask would hide an error
        lo = H * (n // H)
        assert want.shape[-1] == lo
        port = torchgate_cpu(xi, SR, xn=ni, **kw)
        e_np, e_port = rel(y[i, :lo], want[0]), rel(y[i, :lo], port[0])
        worst_np, worst_port = max(worst_np, e_np), max(worst_port, e_port)
        assert bool((y[i, lo:] == 0).all()), (name, i)
    print(f"[rows] {name}: worst vs numpy oracle {worst_np:.3e}, vs torch port {worst_port:.3e}")
    assert worst_np <= TOL, (name, worst_np)
    assert worst_port <= TOL, (name, worst_port)


@pytest.mark.parametrize("name", ["default_f32", "default_f64_prop07", "default_rows_xn_len", "nonstat_f32",
                                  "n256_nonstat_win200_hop37", "n512_win400_hop90_nosmooth", "n1024_hop200_freq_off",
                                  "n2048_time_off", "n4096"])
def test_every_row_matches_todays_path_on_the_row_alone(name):
    from noisereduce_amd.torchgate import TorchGate
    kw, W, H, lens, x, xn, xn_lens = build_case(name)
    tg = TorchGate(sr=SR, **kw).cuda()
    y = gate_rows(tg, x, lens, xn, xn_lens)
    worst = 0.0
    for i, n in enumerate(lens[:40]):
        ni = noise_of(xn, xn_lens, i)
        alone = tg(x[i:i + 1, :n].cuda(), None if ni is None else ni.cuda()).cpu()
        worst = max(worst, rel(y[i, :alone.shape[1]], alone[0]))
    print(f"[rows] {name}: worst vs today's path {worst:.3e}")
    assert worst <= TOL_PATHS, (name, worst)


def test_stationary_decision_bits_equal_todays_path():
    """Smoothing off, prop_decrease = 1: the saved mask IS the decision bits, and both paths decide in float64."""
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    kw = dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
    W, H, L = 1024, 256, 9000
    lens = edge_lengths(W, H, L, 8, 5)
    x = make_rows(lens, L, 5).cuda()
    tg = TorchGate(sr=SR, **kw).cuda()
    gate = tg._gate_for(x.device)
    _, mask = gate.process_rows(x, lens, save_mask=True)
    F = 513
    for i, n in enumerate(lens):
        try:  # natural bin order
            gate.set_option(_ffi.SG_OPT_FORCE_NOFAST, 1)
            _, m1 = gate.process_batch(x[i:i + 1, :n].contiguous(), None, save_mask=True)
        finally:
            gate.set_option(_ffi.SG_OPT_FORCE_NOFAST, 0)
        T = 1 + n // H
        assert m1.shape[1] == T
        assert torch.equal(mask[i, :T, :F], m1[0, :, :F]), (i, n)
        assert bool((mask[i, T:] == 0).all())
        assert set(np.unique(mask[i, :T, :F].cpu().numpy()).tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True, prop_decrease=0.7), dict(n_fft=2048)])
def test_padding_is_never_read(kw):
    from noisereduce_amd.torchgate import TorchGate
    n_fft = kw.get("n_fft", 1024)
    W, H, L = n_fft, n_fft // 4, 14000
    lens = edge_lengths(W, H, L, 7, 3)
    tg = TorchGate(sr=SR, **kw).cuda()
    base = gate_rows(tg, make_rows(lens, L, 3), lens)
    for pad in (float("nan"), float("inf")):
        assert torch.equal(gate_rows(tg, make_rows(lens, L, 3, pad=pad), lens), base)
    other = make_rows(lens, L, 3)
    for i, n in enumerate(lens):
        other[i, n:] = make_rows([L], L, 50 + i)[0, n:]
    assert torch.equal(gate_rows(tg, other, lens), base)
    wide = torch.full((len(lens), L + 1000), float("nan"))
    wide[:, :L] = make_rows(lens, L, 3, pad=float("nan"))
    yw = gate_rows(tg, wide, lens)
    assert torch.equal(yw[:, :base.shape[1]], base) and bool((yw[:, base.shape[1]:] == 0).all())
    for i, n in enumerate(lens):
        assert bool((base[i, H * (n // H):] == 0).all())
    if not kw.get("nonstationary"):
        Ln = 9000
        nlens = edge_lengths(W, H, Ln, 7, 4)
        a = gate_rows(tg, make_rows(lens, L, 3), lens, make_rows(nlens, Ln, 9), nlens)
        b = gate_rows(tg, make_rows(lens, L, 3), lens, make_rows(nlens, Ln, 9, pad=float("nan")), nlens)
        wide_n = torch.full((7, Ln + 1000), float("inf"))
        wide_n[:, :Ln] = make_rows(nlens, Ln, 9)
        c = gate_rows(tg, make_rows(lens, L, 3), lens, wide_n, nlens)
        assert torch.equal(a, b) and torch.equal(a, c)
        assert not torch.equal(a, base)


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True)])
def test_rows_are_independent(kw):
    from noisereduce_amd.torchgate import TorchGate
    W, H, L = 1024, 256, 12000
    lens = edge_lengths(W, H, L, 9, 6)
    x = make_rows(lens, L, 6, pad=float("nan"))
    tg = TorchGate(sr=SR, **kw).cuda()
    y = gate_rows(tg, x, lens)
    rev = gate_rows(tg, x.flip(0), lens[::-1]).flip(0)
    assert torch.equal(rev, y)
    for i in (0, 1, 4, 8):
        # (widened by a few unread samples: a lone row that fills its tensor is an all-full call -- today's path)
        one = torch.cat([x[i:i + 1], torch.full((1, 7), float("nan"))], 1)
        assert torch.equal(gate_rows(tg, one, lens[i:i + 1])[0, :y.shape[1]], y[i])
    # sub-batches of any size give the same rows
    from noisereduce_amd import _ffi
    small = _ffi.Gate("cuda", **_gate_kwargs(tg, max_workspace_bytes=1 << 20))
    ys = small.process_rows(x.cuda(), lens).cpu()
    assert small.rows_batches() > 1
    assert torch.equal(ys, y)
    small.close()
    bad = x.clone()
    bad[2, 1000] = float("nan")
    yb = gate_rows(tg, bad, lens)
    keep = [i for i in range(len(lens)) if i != 2]
    assert torch.equal(yb[keep], y[keep])
    assert bool(torch.isnan(yb[2]).any())


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True), dict(n_fft=512)])
def test_all_full_lengths_take_todays_path_bitwise(kw):
    from noisereduce_amd.torchgate import TorchGate
    B, L = 5, 9000
    x = make_rows([L] * B, L, 8).cuda()
    xn = make_rows([6000], 6000, 9).cuda()
    tg = TorchGate(sr=SR, **kw).cuda()
    assert torch.equal(tg(x, lengths=[L] * B), tg(x))
    assert torch.equal(tg(x, lengths=torch.full((B,), L, device="cuda")), tg(x))
    assert torch.equal(tg(x, xn, lengths=[L] * B, xn_lengths=[6000]), tg(x, xn))


@pytest.mark.parametrize("kw,dtype", [(dict(), torch.float32), (dict(), torch.float64),
                                      (dict(nonstationary=True, prop_decrease=0.7), torch.float32),
                                      (dict(n_fft=512, win_length=400, hop_length=90), torch.float64)])
def test_backward_matches_autograd_on_each_row_alone(kw, dtype):
    """The construction of test_torchgate_backward_matches_autograd (tests/test_gpu_parity.py), row by row."""
    from noisereduce_amd.torchgate import TorchGate
    n_fft = kw.get("n_fft", 1024)
    W = kw.get("win_length") or n_fft
    H = kw.get("hop_length") or W // 4
    L = 7000
    lens = edge_lengths(W, H, L, 6, 12)
    x = make_rows(lens, L, 12, dtype, pad=float("nan")).cuda().requires_grad_()
    tg = TorchGate(sr=SR, **kw).cuda()
    y = tg(x, lengths=lens)
    assert y.requires_grad
    torch.manual_seed(4)
    gy = torch.randn_like(y)
    y.backward(gy)
    gx = x.grad.detach().clone()
    assert gx.dtype == dtype and gx.shape == x.shape
    gate = tg._gate_for(x.device)
    _, mask = gate.process_rows(x.detach(), lens, save_mask=True)
    w = torch.hann_window(W).double().cuda()
    for i, n in enumerate(lens):
        T, lo = 1 + n // H, H * (n // H)
        M = mask[i, :T, :n_fft // 2 + 1].t().double()[None]
        x2 = x.detach()[i:i + 1, :n].double().clone().requires_grad_()
        X = torch.stft(x2, n_fft, H, W, window=w, center=True, pad_mode="constant", return_complex=True)
        y2 = torch.istft(X * M, n_fft, H, W, window=w, center=True)
        assert y2.shape[1] == lo
        assert float((y2.detach()[0] - y.detach()[i, :lo].double()).abs().max() / y2.detach().abs().max()) < TOL
        y2.backward(gy[i:i + 1, :lo].double())
        ref = x2.grad[0]
        assert float((gx[i, :n].double() - ref).abs().max() / ref.abs().max()) < TOL, (i, n)
        assert bool((gx[i, n:] == 0).all()), (i, n)
    # grad_out beyond a row's own output is ignored
    gy2 = gy.clone()
    for i, n in enumerate(lens):
        gy2[i, H * (n // H):] = float("nan")
    x.grad = None
    tg(x, lengths=lens).backward(gy2)
    assert torch.equal(x.grad, gx)


@pytest.mark.parametrize("nonstationary", [False, True])
def test_launch_count_does_not_depend_on_the_batch(nonstationary):
    from noisereduce_amd.torchgate import TorchGate
    rng = np.random.default_rng(2)
    tg = TorchGate(sr=SR, nonstationary=nonstationary).cuda()
    counts = []
    for B, L in ((3, 9000), (300, 16000)):
        lens = [int(n) for n in rng.integers(2048, L + 1, B)]
        lens[0] = L - 1
        x = make_rows(lens, L, 1).cuda().requires_grad_()
        g = tg._gate_for(x.device)
        g.profile_enable(True)
        g.profile_read(reset=True)
        y = tg(x, lengths=lens)
        fwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        assert g.rows_batches() == 1
        y.backward(torch.ones_like(y))
        bwd = {k: v[1] for k, v in g.profile_read(reset=True).items()}
        g.profile_enable(False)
        counts.append((fwd, bwd))
    assert counts[0] == counts[1]
    assert sum(counts[0][0].values()) == (5 if nonstationary else 6) and sum(counts[0][1].values()) == 2


def test_errors():
    from noisereduce_amd.torchgate import TorchGate
    tg = TorchGate(sr=SR).cuda()
    x = make_rows([8000] * 3, 8000, 0).cuda()
    with pytest.raises(ValueError, match=r"lengths\[1\] = 2047"):
        tg(x, lengths=[8000, 2047, 4000])
    with pytest.raises(ValueError, match=r"lengths\[2\] = 8001"):
        tg(x, lengths=[8000, 4000, 8001])
    with pytest.raises(ValueError, match="must hold 3 integers"):
        tg(x, lengths=[8000, 4000])
    with pytest.raises(ValueError, match=r"xn_lengths\[0\] = 100"):
        tg(x, x[:1], lengths=[8000, 4000, 4000], xn_lengths=[100])
    with pytest.raises(RuntimeError, match="GPU only"):
        tg(x.cpu(), lengths=[8000, 4000, 4000])
    # the C ABI refuses the same lengths by itself
    g = tg._gate_for(x.device)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 100"):
        g.process_rows(x, [8000, 100, 4000])
    # an n_fft the table-driven kernels are not built for loops over the rows through the full-length path
    tg2 = TorchGate(sr=SR, n_fft=1000).cuda()
    lens = [8000, 4000, 2001]
    y = tg2(x, lengths=lens)
    for i, n in enumerate(lens):
        alone = tg2(x[i:i + 1, :n])
        assert torch.equal(y[i, :alone.shape[1]], alone[0]) and bool((y[i, alone.shape[1]:] == 0).all())
