"""TorchGate.gated_filterbank without a GPU: the C ABI's three entry points, mel_filterbank against its formulas, the
support tables csrc/feat_tables.hpp builds, the budget rule of tests/gated_filterbank_cases.py on the oracle alone (every
cell of tests/test_gpu_gated_filterbank.py has room, planted defects do not), the numpy statement of the backward against
finite differences, and the validation errors that come before any device work."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from noisereduce_amd import _ffi
from noisereduce_amd.torchgate import TorchGate, mel_filterbank
from noisereduce_amd.torchgate import filterbank as FBK
from oracle import spectralgate_oracle as O
from tests import gated_filterbank_cases as K
from tests import gated_stft_cases as C
from tests import parity_budget as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noisereduce_amd", "csrc")
NEW = ("sg_set_filterbank", "sg_gate_features", "sg_gate_features_backward")


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    for name in NEW:
        assert re.search(r"SG_API int %s\(sg_handle\* h," % name, header), name
        assert name in _ffi.exported_symbols()
    lib = _ffi.load_library()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r" T %s$" % name, out, re.M), name


def test_feat_hip_restates_the_team_shapes_of_spec_hip():
    """k_feat_* cover the frames k_spec_* cover (SPEC_Q): the three definitions are the same text in both files."""
    spec = open(os.path.join(CSRC, "spec.hip")).read()
    feat = open(os.path.join(CSRC, "feat.hip")).read()
    for line in ("constexpr int spec_nt() { return N >= 2048 ? 256 : (N <= 128 ? 16 : (N == 256 ? 32 : 64)); }",
                 "constexpr int spec_teams() { return N >= 2048 ? 1 : (spec_nt<N>() < 64 ? 256 / spec_nt<N>() : "
                 "(N * sizeof(cx<float>) > 16384 ? 2 : 4)); }",
                 "constexpr int SPEC_FPW = 4;"):
        assert line in spec and line in feat, line
    assert C.spec_q_from_source() == C.SPEC_Q


# ---- mel_filterbank ------------------------------------------------------------------------------------------------
def _edges(sr, n_mels, f_min, f_max, scale):
    if scale == "htk":
        to_mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)                    # noqa: E731
        to_hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)                   # noqa: E731
    else:
        step = np.log(6.4) / 27.0
        to_mel = lambda f: 15.0 + np.log(f / 1000.0) / step if f >= 1000.0 else 3.0 * f / 200.0    # noqa: E731
        to_hz = lambda m: np.where(m >= 15.0, 1000.0 * np.exp(step * (m - 15.0)), 200.0 * m / 3.0)  # noqa: E731
    return to_hz(np.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2))


@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", [(16000, 1024, 80, 0.0, None), (48000, 4096, 128, 0.0, None),
                                                        (16000, 256, 40, 0.0, None), (22050, 512, 24, 50.0, 8000.0)])
def test_mel_filterbank_closed_form(sr, n_fft, n_mels, f_min, f_max, scale, norm):
    fb = mel_filterbank(sr, n_fft, n_mels, f_min=f_min, f_max=f_max, scale=scale, norm=norm)
    F = n_fft // 2 + 1
    assert isinstance(fb, torch.Tensor) and fb.dtype == torch.float32 and fb.shape == (F, n_mels)
    assert fb.device.type == "cpu"
    fb = fb.numpy().astype(np.float64)
    e = _edges(sr, n_mels, f_min, sr / 2.0 if f_max is None else f_max, scale)
    assert np.all(np.diff(e) > 0) and abs(e[0] - f_min) < 1e-9 * sr
    f = np.arange(F) * sr / n_fft
    for m in range(n_mels):
        lo, c, hi = e[m], e[m + 1], e[m + 2]
        tri = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
        if norm == "slaney":
            tri = tri * 2.0 / (hi - lo)
        assert np.max(np.abs(fb[:, m] - tri)) <= 2.0 ** -23 * max(1.0, tri.max()), m
    assert np.all(fb >= 0)
    # a bin is covered by at most two filters, and they are neighbours
    nz = fb > 0
    assert nz.sum(axis=1).max() <= 2
    for k in np.flatnonzero(nz.sum(axis=1) == 2):
        ms = np.flatnonzero(nz[k])
        assert ms[1] == ms[0] + 1


@pytest.mark.parametrize("scale", ["htk", "slaney"])
def test_mel_filterbank_peaks_and_areas(scale):
    """The triangles as functions of frequency: 1 at the centre frequency without norm (evaluated where a bin sits on the
    centre: a bank whose edges are bin frequencies), area 1 in Hz with norm="slaney"."""
    sr, n_fft, n_mels = 16000, 1024, 20
    e = _edges(sr, n_mels, 0.0, sr / 2.0, scale)
    # peaks: the formula at f = centre is min((c - lo) / (c - lo), (hi - c) / (hi - c)) = 1; on the bins it is below 1 by the
    # distance to the nearest bin only
    fb = mel_filterbank(sr, n_fft, n_mels, scale=scale).numpy().astype(np.float64)
    df = sr / n_fft
    for m in range(n_mels):
        lo, c, hi = e[m], e[m + 1], e[m + 2]
        assert fb[:, m].max() <= 1.0 + 2.0 ** -23
        assert fb[:, m].max() >= 1.0 - 0.5 * df / min(c - lo, hi - c) - 1e-6
    # a fine grid (n_fft = 2^17: 0.12 Hz) integrates a normalised triangle to 1
    fine = mel_filterbank(sr, 1 << 17, n_mels, scale=scale, norm="slaney").numpy().astype(np.float64)
    area = fine.sum(axis=0) * sr / (1 << 17)
    assert np.max(np.abs(area - 1.0)) < 1e-3, area


def test_mel_filterbank_refuses():
    for kw in (dict(scale="bark"), dict(norm="l2"), dict(f_min=9000.0), dict(f_min=-1.0)):
        with pytest.raises(ValueError):
            mel_filterbank(16000, 1024, 40, **kw)
    with pytest.raises(ValueError):
        mel_filterbank(16000, 1024, 0)


# ---- support tables --------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include <vector>
#include "feat_tables.hpp"
int main(int argc, char** argv) {
  int F = 0, M = 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(&F, 4, 1, f) != 1 || fread(&M, 4, 1, f) != 1) return 2;
  std::vector<float> fb((size_t)F * M), fbT((size_t)F * M);
  if (fread(fb.data(), 4, fb.size(), f) != fb.size()) return 2;
  fclose(f);
  std::vector<int32_t> kh(2 * M), mh(2 * F);
  const bool ok = sg::feat_tables(fb.data(), F, M, fbT.data(), kh.data(), mh.data());
  FILE* o = fopen(argv[2], "wb");
  int32_t okw = ok;
  fwrite(&okw, 4, 1, o);
  fwrite(fbT.data(), 4, fbT.size(), o);
  fwrite(kh.data(), 4, kh.size(), o);
  fwrite(mh.data(), 4, mh.size(), o);
  fclose(o);
  return 0;
}
"""


@pytest.fixture(scope="module")
def tables_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("feat_tables")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    return exe


def _c_tables(exe, fb, tmp_path):
    F, M = fb.shape
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([F, M], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(fb, dtype=np.float32).tobytes())
    subprocess.run([str(exe), str(inp), str(out)], check=True, timeout=60)
    raw = np.fromfile(out, dtype=np.int32)
    ok = bool(raw[0])
    fbT = raw[1:1 + F * M].view(np.float32).reshape(M, F)
    kh = raw[1 + F * M:1 + F * M + 2 * M].reshape(M, 2)
    mh = raw[1 + F * M + 2 * M:].reshape(F, 2)
    return ok, fbT, kh, mh


@pytest.mark.parametrize("name", ["mel80", "dense24", "zero_last", "neg", "one"])
def test_support_tables(name, tables_exe, tmp_path):
    fb = K.bank(name, "a")
    F, M = fb.shape
    ok, fbT, kh, mh = _c_tables(tables_exe, fb, tmp_path)
    assert ok and np.array_equal(fbT, fb.T)
    nz = fb != 0
    # the hulls hold every non-zero, and are tight
    for m in range(M):
        ks = np.flatnonzero(nz[:, m])
        assert (kh[m].tolist() == [ks[0], ks[-1] + 1]) if ks.size else (kh[m].tolist() == [0, 0]), m
    for k in range(F):
        ms = np.flatnonzero(nz[k])
        assert (mh[k].tolist() == [ms[0], ms[-1] + 1]) if ms.size else (mh[k].tolist() == [0, 0]), k
    # the transposed hulls agree with the forward ones: (k, m) inside one exactly where a non-zero could sit for the other
    in_k = (np.arange(F)[:, None] >= kh[None, :, 0]) & (np.arange(F)[:, None] < kh[None, :, 1])
    in_m = (np.arange(M)[None, :] >= mh[:, None, 0]) & (np.arange(M)[None, :] < mh[:, None, 1])
    assert not np.any(nz & ~in_k) and not np.any(nz & ~in_m)
    assert np.array_equal(in_k.any(axis=0), in_m.any(axis=0)) and np.array_equal(in_k.any(axis=1), in_m.any(axis=1))
    # the numpy restatement the GPU tests lean on is the same tables
    kh2, mh2 = FBK.support_tables(fb)
    assert np.array_equal(kh, kh2) and np.array_equal(mh, mh2)
    if name == "dense24":
        assert np.all(kh == [0, F]) and np.all(mh == [0, M])
    if name == "zero_last":
        assert kh[-1].tolist() == [0, 0] and mh[:, 1].max() == M - 1
    if name == "mel80":
        assert nz.sum() <= 2 * F


def test_support_tables_refuse_a_non_finite_entry(tables_exe, tmp_path):
    fb = K.bank("mel40", "c").copy()
    fb[17, 3] = np.inf
    assert not _c_tables(tables_exe, fb, tmp_path)[0]
    fb[17, 3] = np.nan
    assert not _c_tables(tables_exe, fb, tmp_path)[0]


# ---- the budget rule on the oracle alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", K.FWD_CELLS, ids=K.FWD_IDS)
def test_every_frame_has_a_budget_and_a_float32_evaluation_fits(cell):
    case, variant, bname = cell
    ref = K.reference(case, variant, "float32")
    fb = K.bank(bname, case)
    rows = range(C.CASES[case]["B"]) if case != "g" else (0, 80, 160)
    for power in K.cell_powers(bname):
        for b in rows:
            M32 = ref["mask"][b].astype(np.float32)
            want, bud, allowed = K.feature_budget(ref["X"][b], M32, fb, power, ref["emu"][b])
            assert want.shape == (fb.shape[1], ref["X"].shape[-1])
            # a frame without a budget is one whose neighbourhood (t - POOL .. t + POOL) the gate closed completely (the
            # unsmoothed mask does that to a quiet tail): want is 0 there and the rule then asks for exactly 0
            open_ = PB._pool(M32.max(axis=0)) > 0
            assert np.all(bud[open_] > 0), (power, b, np.flatnonzero(open_ & (bud <= 0)))
            assert not np.any(want[:, ~open_]) and (variant == "nosmooth" or np.all(open_))
            # the order a lane sums in, in float32, sits well inside the allowance
            seq = K.features32_seq(ref["emu"][b], M32, fb, power)
            err = np.max(np.abs(seq.astype(np.float64) - want), axis=0)
            assert np.all(err <= 0.5 * allowed), (power, b, float(np.max(err / allowed)))


def _drop(fb, which):
    """The bank with, per filter, its last bin (``k_hi - 1``) or, per bin, its last filter (``m_hi - 1``) set to 0."""
    kh, mh = FBK.support_tables(fb)
    out = fb.copy()
    if which == "bin":
        for m in range(fb.shape[1]):
            if kh[m, 1] > kh[m, 0]:
                out[kh[m, 1] - 1, m] = 0.0
    else:
        for k in range(fb.shape[0]):
            if mh[k, 1] > mh[k, 0]:
                out[k, mh[k, 1] - 1] = 0.0
    return out


@pytest.mark.parametrize("power", K.POWERS)
@pytest.mark.parametrize("cell", [("a", "plain", "mel80"), ("c", "plain", "mel40"), ("e", "plain", "mel128"),
                                  ("a", "nonstat", "mel80"), ("g", "plain", "dense24")], ids=lambda c: "%s-%s-%s" % c)
def test_planted_defects_are_caught(cell, power):
    case, variant, bname = cell
    ref = K.reference(case, variant, "float32")
    fb = K.bank(bname, case)
    b = 0
    X, emu = ref["X"][b], ref["emu"][b]
    M32 = ref["mask"][b].astype(np.float32)
    assert M32.max() > 0
    T = X.shape[-1]

    def bad(got):
        return K.feature_check(got, X, M32, fb, power, emu)[0]

    assert bad(K.features64(X, M32, fb, power)).size == 0
    assert bad(K.features64(X, M32, _drop(fb, "filter"), power)).size > 0.5 * T, "filter m_hi - 1 dropped"
    # (the last bin of every filter of a dense bank is the Nyquist bin, which carries little of these signals: some frames)
    assert bad(K.features64(X, M32, _drop(fb, "bin"), power)).size > (0 if bname == "dense24" else 0.5 * T), "bin k_hi - 1 dropped"
    assert bad(K.features64(X, M32, fb, 3 - power)).size > 0.5 * T, "power swapped"
    if fb[-1].any():
        # the Nyquist bin carries little of a low-passed signal: caught in the frames where its share is above the allowance
        want, _, allowed = K.feature_budget(X, M32, fb, power, emu)
        share = np.max(np.abs(want - K.features64(X, M32, fb, power, nyquist=False)), axis=0)
        assert np.array_equal(bad(K.features64(X, M32, fb, power, nyquist=False)), np.flatnonzero(share > allowed))
    if power == 2 and np.any((M32 > 0) & (M32 < 1)):
        assert bad(K.features64(X, M32, fb, 2, mask_once=True)).size > 0, "mask applied once"


def test_the_nyquist_bin_is_held_where_a_filter_weighs_it():
    """A bank whose single filter is the Nyquist bin alone: leaving that bin out is caught in every frame with signal."""
    case = "a"
    ref = K.reference(case, "plain", "float32")
    F = ref["X"].shape[1]
    fb = np.zeros((F, 1), dtype=np.float32)
    fb[-1, 0] = 1.0
    M32 = np.ones(ref["X"][0].shape, dtype=np.float32)
    for power in K.POWERS:
        got = K.features64(ref["X"][0], M32, fb, power, nyquist=False)
        bad, _ = K.feature_check(got, ref["X"][0], M32, fb, power, ref["emu"][0])
        assert bad.size == ref["X"].shape[-1]


# ---- the numpy statement of the backward ---------------------------------------------------------------------------
LD = np.longdouble


def _stft_ld(x, n_fft, W, H, win):
    """O.stft_torch of one row in extended precision (x87 long double: 64-bit mantissa), the transform as a matrix
    product: (F, T).  The finite differences below divide a difference of forward values by a step of 1e-6; in float64
    the rounding of those values alone is 1e-8 of the quotient."""
    L = x.shape[0]
    wf = O._centered_window(n_fft, W, win).astype(LD)
    p = n_fft // 2
    ext = np.concatenate([np.zeros(p, dtype=LD), x.astype(LD), np.zeros(p, dtype=LD)])
    T = 1 + L // H
    frames = ext[np.arange(n_fft)[None, :] + H * np.arange(T)[:, None]] * wf[None, :]
    pi = 4 * np.arctan(LD(1))
    jk = (np.arange(n_fft)[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft
    ang = (-2 * pi / n_fft) * jk.astype(LD)
    return (frames @ (np.cos(ang) + 1j * np.sin(ang))).T


def _stencil(f, x, v, h):
    """Fourth-order central difference of t -> f(x + t v) at 0."""
    return (8 * (f(x + h * v) - f(x - h * v)) - (f(x + 2 * h * v) - f(x - 2 * h * v))) / (12 * h)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("power", K.POWERS)
@pytest.mark.parametrize("case,bname", [("a", "mel80"), ("c", "mel40"), ("b", "dense24")])
def test_backward_statement_is_the_adjoint_of_the_jacobian(case, bname, power, log):
    """<J v, g> == <v, J^T g> to 1e-9: J v from finite differences of the forward with the mask cells fixed, J^T g =
    adjoint_np of G = gp * d|Y|^p / dY (float64)."""
    assert np.finfo(LD).eps < 1e-18, "needs an extended-precision long double"
    c = C.CASES[case]
    n_fft, W, H = C.geometry(case)
    win = C.window64(case)
    L = c["L"]
    rng = np.random.default_rng(77)
    x = C.make_x(case)[0]
    fb = K.bank(bname, case)
    F, T = n_fft // 2 + 1, 1 + L // H
    M32 = rng.uniform(0.25, 1.0, size=(F, T)).astype(np.float32)
    fbl, Ml = fb.astype(LD), M32.astype(LD)

    def fwd(xx):
        lin = fbl.T @ (np.abs(_stft_ld(xx, n_fft, W, H, win)) * Ml) ** power
        return np.log(lin + LD(K.EPS)) if log else lin

    X0 = O.stft_torch(x[None], n_fft, W, H, win)[0]
    assert np.max(np.abs(_stft_ld(x, n_fft, W, H, win).astype(np.complex128) - X0)) < 1e-11 * np.abs(X0).max()
    assert np.abs(X0).min() > 0                                  # no zero bin (power = 1 is smooth here)
    g = rng.standard_normal((fb.shape[1], T))
    v = rng.standard_normal(L)
    # two steps move the smallest |X| by a hundredth of itself: the stencil's h^4 term is (1e-2)^4 / 30 of that one bin's
    # share and far less for the others, and the rounding of the forward values (1e-19 of 1e4) over h is 1e-9 of nothing
    V = O.stft_torch(v[None], n_fft, W, H, win)[0]
    h = LD(5e-3 * np.abs(X0).min() / np.abs(V).max())
    lhs = float(np.sum(_stencil(fwd, x.astype(LD), v.astype(LD), h) * g.astype(LD)))
    G = K.spectrum_grad(X0, M32, fb, g, power, log)
    rhs = float(np.dot(v, K.grad_x64(G, case, L)))
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs)), (lhs, rhs, float(h))


def test_float32_statement_of_G_follows_the_float64_one():
    ref = K.reference("a", "plain", "float32")
    fb = K.bank("mel80", "a")
    g = K.upstream("a", "mel80")[0]
    M32 = ref["mask"][0].astype(np.float32)
    for power in K.POWERS:
        for log in (False, True):
            G64 = K.spectrum_grad(ref["X"][0], M32, fb, g, power, log)
            G32 = K.spectrum_grad32(ref["emu"][0], M32, fb, g, power, log)
            assert G32.dtype == np.complex64
            assert np.max(np.abs(G32 - G64)) <= 1e-3 * np.max(np.abs(G64))


# ---- validation, before any device work ----------------------------------------------------------------------------
def test_validation_errors_come_before_device_work():
    tg = TorchGate(sr=16000)                      # never moved to a GPU: a call that got past validation raises RuntimeError
    x = torch.zeros(2, 4096)
    F = 513
    good = mel_filterbank(16000, 1024, 80)
    with pytest.raises(RuntimeError):
        tg.gated_filterbank(x, good)
    for bad in (torch.zeros(512, 80), torch.zeros(F), torch.zeros(F, 0), torch.zeros(F, 1025), torch.zeros(2, F, 8),
                np.zeros((F + 1, 40), dtype=np.float32), torch.zeros(F, 4, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            tg.gated_filterbank(x, bad)
    for v in (float("nan"), float("inf"), -float("inf")):
        fb = good.clone()
        fb[100, 7] = v
        with pytest.raises(ValueError):
            tg.gated_filterbank(x, fb)
    with pytest.raises(ValueError):
        tg.gated_filterbank(x, good.clone().requires_grad_(True))
    for power in (0.5, 3, 0, "2", True):
        with pytest.raises(ValueError):
            tg.gated_filterbank(x, good, power=power)
    with pytest.raises(ValueError):
        tg.gated_filterbank(x, good, eps=float("nan"))
    # a numpy bank and an integer power pass validation too
    with pytest.raises(RuntimeError):
        tg.gated_filterbank(x, good.numpy(), power=1)
    with pytest.raises(RuntimeError):
        tg.gated_filterbank(x, torch.zeros(F, 1024), power=2)
