"""Every device-tensor entry point of ``_ffi.Gate`` on unaligned, strided, repeated and overlapping views of a poisoned
buffer (tests/view_cases.py), against the same call on ``V.aligned_clone(view)`` on the same handle.  tests/test_views_host.py
holds the layouts themselves, ``_ffi._rows`` and ``_ffi._dense`` on CPU tensors.

Per call (``_on_views``): the layout sits at the residues it is there for (``V.assert_claims`` on the device); every returned
tensor -- samples, saved mask (its F written columns), gradient, spectrum, features -- equals the aligned call's byte for byte;
no sample is non-finite where the aligned call's is finite (a NaN poison sample that leaked in); the caller's allocation is
byte for byte what it was; ``gate.check_errors()`` is clean.  ``off<k>`` / ``pitch1`` (and ``oddL`` where the case's rows are
odd already) keep the case's samples, so the view call is ALSO held to the cell's cached float64 oracle by the checker of the
entry point's own GPU test (named at each test): view and clone cannot both be wrong in the same way.  The largest
local_error / budget of those checks goes to the file named by VIEWS_PARITY_OUT, if set (profiles/views.json is that file from
an MI355X run); the bound is ``PB.FACTOR`` as everywhere, nothing here defines a tolerance.

What was read before the first run (csrc/, every place that picks a vector or a per-sample side by an address):

* ``geom.hpp`` ``view_sample`` / ``frame_ptr_f32``: a sample is loaded only for ``0 <= s < Lp`` and ``lo <= g < hi``; the
  whole-frame pointer only when ``[g, g + len)`` lies inside ``[lo, hi)``.  Every per-sample side below goes through one of
  them (or through the explicit ``p0 / p1 / g_lo / g_hi`` tests of an epilogue), so it stays inside ``[view.lo, view.hi)`` of
  its row -- with ``process_chunks``' halos ``lo = -halo_left``, ``hi = N + halo_right`` from the SHIFTED pointer.
* ``fastpath.hpp`` ``blk_vec`` (k_apply_fast, k_decide_fast, k_mag_fast), ``vec16``, ``fast256 / fast512 / fast2048 / fast64``
  and ``onepass_tile.hpp`` ``tile_src``: the span's first address ``sp`` is formed from x, row * stride, chunk * cs - pad and
  the tile's offset, and ``(uintptr_t)sp & 15`` (``& 7`` for the 8-byte int16 loads) is part of the flag; the span is a
  multiple of 16 bytes, so every 16-byte load of ``stage_span_vec`` is aligned when its first one is.  Both sides store the
  same floats to the same LDS slots: no arithmetic differs.  The non-LEAN frame gather of k_apply_fast tests ``& 7`` of the
  lane's own float2 address and needs ``inside``; else the rolled ``view_sample`` gather.
* ``rowgate.hpp`` ``span_vec`` / ``rowbwd.hpp`` ``vec``: the ROW's base ``x + row * stride`` is tested, per row (one workgroup
  per row); indices are multiples of 4 (padL = 512) clamped into ``[0, (Lp & ~3) - 4]``, the ragged end is patched sample by
  sample inside ``[0, Lp)``.
* every ``dst & 15`` (``& 7``: int16) epilogue (fastpath.hpp, rowgate.hpp, rowbwd.hpp, apply64.hpp, onepass_tile.hpp): the
  lane's own destination is tested after the whole hop was shown to lie inside ``[p0, p1) x [g_lo, g_hi)``; the other side
  stores sample by sample under the same four tests.  Same values either way.
* ``onepass_plan.hpp`` ``inv``: requires ``src & 15 == 0``, ``dst & 15 == 0`` AND ``stride & 3``, ``cs & 3``, ``ostride & 3``,
  ``g_step & 3 == 0``.  An odd pitch (``pitch1``, ``oddL``) fails ``stride & 3`` and leaves NO unit interior, so the flag is
  never applied to a row whose residue differs from row 0's; ``off<k>`` fails ``src & 15``.  Those launches take the kernel's
  field-by-field ``tile_src`` / ``tile_fast``, which test the address of the tile at hand.
* ``fused.hpp`` ``k_unit_absmax``: ``a_lo`` is derived from the address of ``src + s_lo``; head ``[s_lo, min(a_lo, s_hi))``
  and tail ``[a_lo + 4 n4, s_hi)`` (8 n8: int16) are scalar, the middle aligned; all inside ``[s_lo, s_hi)``.
* ``spec.hip`` / ``feat.hip`` / ``kernels.hpp`` frame loads are scalar (``fp[2 j]``, ``fp[2 j + 1]``) whatever the address.

No defect showed in reading.  No route's unaligned side reorders floating-point operations -- the sides differ in how samples
reach LDS or memory, never in a sum -- so every route is held to equal bits; none is held to the oracle INSTEAD.

Output side: ``gate_spectrum(out=, mask_out=)``, ``gate_spectrum_backward(out=)`` and ``process_chunks(out=)`` write into
``off<k>`` / ``pitch1`` (a contiguous ``out``: a flat offset) inside poison; the tensor equals the aligned call's and every
element of the allocation outside it still holds poison.  Fresh outputs: TorchGate's ``Lout = H (T - 1)`` is a multiple of 256
wherever H = 256, so a fresh (B, Lout) output has aligned rows there by construction; ``n512-win`` / ``lds-512-w400-h101``
(H = 101, odd Lout) and the gradients ``(B, L)`` of the odd-L cells put rows 1, 2, 3 of a fresh output off a 16-byte
boundary.

Left out: ``StreamBank`` and ``reduce_noise_batch`` pack what they are given into fresh flat buffers with per-item offsets of
their own; tests/test_gpu_batch_fuzz.py and the prime-cut plans of the stream tests hold those.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import gated_filterbank_cases as K
from tests import gated_filterbank_rows_cases as FR
from tests import gated_stft_cases as C
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB
from tests import stagewise_checks as SC
from tests import view_cases as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
_RATIOS = {}


def _note(entry, ratio):
    _RATIOS[entry] = max(_RATIOS.get(entry, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("VIEWS_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _tdt(name):
    return V._TORCH[name] if isinstance(name, str) else name


def _names(dtype, copies=V.COPY_LAYOUTS):
    return ["off%d" % k for k in V.offsets(dtype)] + ["pitch1", "oddL"] + list(copies)


def _lay(name, a):
    """Layout ``name`` of the samples ``a`` on the device, at the residues it claims."""
    a = _np(a)
    if name.startswith("flat_off"):
        lay = V.make_flat(a, int(name[8:]), DEV)
    else:
        lay = V.make(name, V.odd_rows(a) if name == "oddL" else a, DEV)
    V.assert_claims(lay)
    return lay


def _flat_nd(t, k):
    """A contiguous tensor of any rank, k elements off a 16-byte boundary inside poison: (layout, view of t's shape)."""
    t = _np(t)
    lay = V.make_flat(np.ascontiguousarray(t).reshape(-1), k, DEV)
    V.assert_claims(lay)
    return lay, lay.view.view(tuple(t.shape))


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _real(t):
    t = t.contiguous()
    return torch.view_as_real(t) if t.is_complex() else t


def _same(tag, got, want):
    """Every tensor of ``got`` byte for byte that of ``want``; first, nothing non-finite where ``want`` is finite."""
    got, want = _tuple(got), _tuple(want)
    assert len(got) == len(want), tag
    for i, (a, b) in enumerate(zip(got, want)):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, (tag, i, a.shape, b.shape, a.dtype, b.dtype)
        a, b = _real(a), _real(b)
        if a.dtype.is_floating_point:
            leaked = torch.isfinite(b) & ~torch.isfinite(a)
            assert not bool(leaked.any()), "%s, output %d: %d values are not finite where the aligned call's are, first at %s: " \
                "poison leaked in" % (tag, i, int(leaked.sum()), leaked.nonzero()[0].tolist())
        ne = (V.raw_bytes(a) != V.raw_bytes(b)).view(-1, a.element_size()).any(dim=1)
        assert not bool(ne.any()), "%s, output %d: %d of %d values differ from the aligned call's, first at flat index %d " \
            "(%r against %r)" % (tag, i, int(ne.sum()), ne.numel(), int(ne.nonzero()[0]),
                                 a.reshape(-1)[int(ne.nonzero()[0])].item(), b.reshape(-1)[int(ne.nonzero()[0])].item())


def _on_views(tag, gate, lays, call, aligned=None):
    """``call(*views)`` against ``call(*aligned clones)`` (``aligned``: the aligned inputs where they are not the clones) with
    the assertions every entry point shares.  Returns what the view call returned."""
    before = [V.raw_bytes(l.store).clone() for l in lays]
    clones = [V.aligned_clone(l.view) for l in lays] if aligned is None else list(aligned)
    for c in clones:
        assert c.is_contiguous() and c.data_ptr() % 16 == 0, tag
    got = call(*[l.view for l in lays])
    want = call(*clones)
    gate.check_errors()
    for l, b in zip(lays, before):
        assert torch.equal(V.raw_bytes(l.store), b), "%s: the call changed the caller's allocation (%s)" % (tag, l.name)
    _same(tag, got, want)
    return got


def _poison_out(shape, dtype, name):
    """An output tensor of ``shape`` laid out by ``name`` (off<k> / pitch1 for 2-D, flat_off<k> for a contiguous tensor of
    any rank) inside a poisoned allocation, itself holding poison: (store, view)."""
    dt = _tdt(dtype)
    n = int(np.prod(shape))
    if name.startswith("flat_off"):
        k = int(name[8:])
        store = V.poison(V.MARGIN + n + V.SLACK, dt).to(DEV)
        view = store[V.MARGIN + k:V.MARGIN + k + n].view(tuple(shape))
        want = (k * store.element_size()) % 16
    else:
        B, L = shape
        P = V._up8(L) + (1 if name == "pitch1" else V.SLACK)
        k = 0 if name == "pitch1" else int(name[3:])
        store = V.poison(V.MARGIN + B * P + V.MARGIN, dt).to(DEV)
        view = store[V.MARGIN:V.MARGIN + B * P].view(B, P)[:, k:k + L]
        want = (k * store.element_size()) % 16
        if B > 1:
            assert (view.data_ptr() + view.stride(0) * view.element_size()) % 16 == ((k + (name == "pitch1")) * view.element_size()) % 16
    assert store.data_ptr() % 16 == 0 and view.data_ptr() % 16 == want, (name, view.data_ptr() % 16, want)
    return store, view


def _outside_is_poison(tag, store, view):
    touched = torch.zeros(store.numel(), dtype=torch.bool)
    touched.as_strided(tuple(view.shape), view.stride(), view.storage_offset()).fill_(True)
    rest = V.is_poison(store.cpu())[~touched]
    assert rest.numel() >= 2 * V.MARGIN and bool(rest.all()), "%s: %d elements of the allocation outside the output tensor " \
        "were written" % (tag, int((~rest).sum()))


def _torchgate_handle(kw, sr):
    from noisereduce_amd.torchgate import TorchGate
    tg = TorchGate(sr=sr, **kw).cuda()
    return tg, tg._gate_for(torch.device("cuda", torch.cuda.current_device()))


# ---- process_batch (TorchGate.forward's full-length routes) -----------------------------------------------------------------
# t128 row_decide, t129 t2, rg-64 k_row_gate (span_vec), b16-nofast k_apply_istft + k_ola, n512 / n2048 register apply, n400
# mixed radix, n512-win H = 101 (odd Lout), f64 the float64 loads, ns-box non-stationary, xnB-15 / xn1-long noise rows
PB_CELLS = ["t128", "t129", "rg-64", "b16-nofast", "n512", "n2048", "n400", "n512-win", "f64", "ns-box", "xnB-15", "xn1-long"]
PB_ORACLE = {"t128": ("off1", "pitch1"), "f64": ("off1",), "xnB-15": ("off1",)}


@pytest.mark.parametrize("name", PB_CELLS)
def test_process_batch(name):
    """Oracle: ``_check_rows`` of tests/test_gpu_torchgate_routes.py (PB.local_check per hop block, mask_bound / _field_rule)."""
    from tests import test_gpu_torchgate_routes as TR
    cell = PB.r_cell(name)
    case = PB.r_case(cell)
    x = case["x"].astype(case["dtype"])
    xn = None if case["xn"] is None else case["xn"].astype(case["dtype"])
    F = cell["n_fft"] // 2 + 1
    names = _names(case["dtype"]) if cell["B"] <= 20 else ["off1", "pitch1", "inner2"]
    gate = TR._make(cell, PB.r_budget(cell))

    def call(xv, xnv=None):
        y, m = gate.process_batch(xv, xnv, save_mask=True)
        return y, m[:, :, :F]
    try:
        for ln in names:
            tag = "process_batch %s [%s]" % (name, ln)
            lays = [_lay(ln, x)] + ([] if xn is None else [_lay(ln, xn)])
            y, m = _on_views(tag, gate, lays, call)
            assert y.dtype == _tdt(case["dtype"]) and tuple(y.shape) == (cell["B"], gate.output_length(lays[0].view.shape[1]))
            if ln in PB_ORACLE.get(name, ()):
                worst = TR._check_rows(tag, cell, PB.r_oracle(cell), y.cpu().numpy(), m.cpu().numpy())
                print("%s: largest local_error / budget %.2f" % (tag, worst))
                _note("process_batch/%s" % case["dtype"], worst)
    finally:
        gate.close()


# ---- process_batch_backward / process_rows / process_rows_backward (the backward matrix) -------------------------------------
_B_FULL = [i for i, c in enumerate(PB.B_CELLS) if not c.get("lengths")]
_B_ROWS = [i for i, c in enumerate(PB.B_CELLS) if c.get("lengths") and c["n_fft"] in (256, 1024)]
B_ORACLE = {"row-T64": ("off1", "pitch1"), "fast-T65": ("off1",), "reg-512-f64": ("off1",)}


def _b_setup(i):
    from tests import test_gpu_backward_parity as TB
    case = PB.b_case(i)
    cell = case["cell"]
    tdt = _tdt(case["dtype"])
    Lout = PB.adjoint_geometry(case["cfg"], case["L"])[2]
    return TB, case, cell, tdt, Lout


@pytest.mark.parametrize("i", _B_FULL, ids=[PB.b_cell_id(PB.B_CELLS[i]) for i in _B_FULL])
def test_process_batch_backward(i):
    """grad_out on the layouts.  The library is told L, not grad_out's width: ``oddL`` (one more column) is held to the call on
    the aligned (B, Lout) grad_out itself.  Oracle: ``PB.adjoint_check_rows`` (tests/test_gpu_backward_parity.py)."""
    from noisereduce_amd import _ffi
    TB, case, cell, tdt, Lout = _b_setup(i)
    L = case["L"]
    gy = torch.from_numpy(TB._grad_outs(case, Lout, 0.0)[0]).to(tdt)
    with TB._handle_env(cell.get("env", ())):
        tg, gate = _torchgate_handle(case["kw"], PB.T_SR)
        opts = [(getattr(_ffi, "SG_OPT_" + k), v) for k, v in cell.get("opts", ())]
        with gate.lock, gate.with_options(opts):
            _, mask = gate.process_batch(torch.from_numpy(case["x"]).to(tdt).cuda(), save_mask=True)
            gya = gy.cuda()

            def call(gv):
                gx = gate.process_batch_backward(gv, mask, L)
                assert gate.backward_route() == TB._ROUTE[cell["route"]], (cell["name"], gate.backward_route())
                return gx
            for ln in _names(tdt):
                tag = "process_batch_backward %s [%s]" % (cell["name"], ln)
                gx = _on_views(tag, gate, [_lay(ln, gy)], call, aligned=[gya] if ln == "oddL" else None)
                assert gx.dtype == tdt and tuple(gx.shape) == (gy.shape[0], L)
                if ln in B_ORACLE.get(cell["name"], ()):
                    worst = PB.adjoint_check_rows(tag, gx.cpu().numpy(), case["gy"][0], mask.cpu().numpy(), case["cfg"], case["lens"])
                    print("%s: largest local_error / budget %.3f" % (tag, worst))
                    _note("process_batch_backward/%s" % case["dtype"], worst)
        del tg, gate


@pytest.mark.parametrize("i", _B_ROWS, ids=[PB.b_cell_id(PB.B_CELLS[i]) for i in _B_ROWS])
def test_process_rows_and_backward(i):
    """Rows of 2 W, 2 W + 1, 37 H and 37 H + H - 1 samples in a padded batch (NaN behind them: a ragged end inside a 16-byte
    group), x, the noise rows and grad_out on the layouts.  Oracle: the row alone under ``PB.local_check`` (forward,
    tests/test_gpu_stagewise.py::test_torchgate_cell) and ``PB.adjoint_check_rows``."""
    from tests.test_gpu_rows import edge_lengths, make_rows
    TB, case, cell, tdt, Lout = _b_setup(i)
    L, lens, W, H = case["L"], case["lengths"], case["W"], case["H"]
    tg, gate = _torchgate_handle(case["kw"], PB.T_SR)
    F = cell["n_fft"] // 2 + 1
    Ln = max(2 * W, 3000) + 1
    nlens = edge_lengths(W, H, Ln, len(lens), 4)
    xn = make_rows(nlens, Ln, 9, pad=float("nan"))
    names = _names(tdt, copies=("inner2",))
    with gate.lock:
        def fwd(xv, xnv=None):
            y, m = gate.process_rows(xv, lens, xnv, None if xnv is None else nlens, save_mask=True)
            assert gate.rows_batches() == 1
            return y, m[:, :, :F]
        for ln in names:
            tag = "process_rows %s [%s]" % (cell["name"], ln)
            y, m = _on_views(tag, gate, [_lay(ln, case["x"])], fwd)
            if ln in ("off1", "pitch1"):
                got, worst = y.cpu().numpy(), 0.0
                for b, u in enumerate(PB.b_oracle(i)):
                    n = len(u["want"])
                    bad, ratio = PB.local_check(got[b, :n], u)
                    worst = max(worst, ratio)
                    assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                        tag, b, bad[:10].tolist(), ratio)
                    assert np.all(got[b, n:] == 0), (tag, b)
                print("%s: largest local_error / budget %.2f" % (tag, worst))
                _note("process_rows/%s" % case["dtype"], worst)
            if not cell.get("nonstationary"):
                _on_views(tag + " with noise rows", gate, [_lay(ln, case["x"]), _lay(ln, xn)], fwd)
        _, mask = gate.process_rows(torch.from_numpy(case["x"]).cuda(), lens, save_mask=True)
        gy = torch.from_numpy(TB._grad_outs(case, Lout, np.nan)[0]).to(tdt)      # NaN beyond a row's own output: never read
        gya = gy.cuda()

        def bwd(gv):
            gx = gate.process_rows_backward(gv, mask, L, lens)
            assert gate.backward_route() == TB._ROUTE["rows"]
            return gx
        for ln in names:
            tag = "process_rows_backward %s [%s]" % (cell["name"], ln)
            gx = _on_views(tag, gate, [_lay(ln, gy)], bwd, aligned=[gya] if ln == "oddL" else None)
            assert bool(torch.isfinite(gx).all()), tag
            if ln in ("off1", "pitch1"):
                worst = PB.adjoint_check_rows(tag, gx.cpu().numpy(), case["gy"][0], mask.cpu().numpy(), case["cfg"], case["lens"])
                print("%s: largest local_error / budget %.3f" % (tag, worst))
                _note("process_rows_backward/%s" % case["dtype"], worst)
    del tg, gate


# ---- gate_spectrum / gate_features and their backwards ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spec_units(case, variant, dtype):
    x = C.make_x(case, np.dtype(dtype)).astype(np.float64)
    xn = C.make_xn(case, C.VARIANTS[variant][1], np.dtype(dtype))
    us = PB.torchgate_units(x, C.CASES[case]["sr"], xn=None if xn is None else xn.astype(np.float64), window=C.window64(case),
                            **C.gate_kwargs(case, variant))[1]
    for u in us:
        u["emu_spec"] = PB.spectrum_f32(u)
    return us


def _check_spectrum(tag, pairs, mask, units, entry, rows=False):
    """``C.spectrum_check`` per frame, every row, and the mask within the bound of the entry point's own GPU test:
    tests/test_gpu_gated_stft_budget.py's ``_mask_tol``; ``rows``: tests/test_gpu_gated_stft_rows.py's float-tap bound."""
    from tests.test_gpu_gated_stft_budget import _mask_tol
    Y = torch.view_as_complex(pairs.contiguous()).transpose(1, 2).cpu().numpy()       # (B, F, T)
    M = mask.transpose(1, 2).cpu().numpy()
    worst = 0.0
    for b, u in enumerate(units):
        Tb = u["Z"].shape[1]
        bad, ratio = C.spectrum_check(Y[b, :, :Tb], u["Z"], M[b, :, :Tb], u["cfg"], emu=u["emu_spec"])
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: frames %s over their bound (largest error / budget %.2f)" % (tag, b, bad[:12].tolist(), ratio)
        if u["cfg"]["stationary"]:
            cells, w = PB.mask_diff(M[b, :, :Tb], u, bound=PB.mask_bound(u["cfg"], integer_taps=False) if rows else _mask_tol(u["cfg"]))
            assert len(cells) == 0, "%s row %d: mask off by up to %.3g at %d cells" % (tag, b, w, len(cells))
    print("%s: largest local_error / budget %.2f" % (tag, worst))
    _note(entry, worst)


def _grad_pairs(shape, dtype, seed):
    """(B, F, T) complex field of ``dtype``'s precision and its (B, T, F, 2) real pairs."""
    B, T, F = shape
    rng = np.random.default_rng(seed)
    G = (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))).astype(
        np.complex64 if np.dtype(dtype) == np.float32 else np.complex128)
    return G, torch.view_as_real(torch.from_numpy(np.ascontiguousarray(G.transpose(0, 2, 1))))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case,variant", [("a", "plain"), ("a", "xnB"), ("c", "plain"), ("c", "xn1")],
                         ids=["a", "a-xnB", "c", "c-xn1"])
def test_gate_spectrum_and_backward(case, variant, dtype):
    """x and xn on the layouts; the spectrum and the mask into ``flat_off<k>``, the gradient into ``off<k>`` / ``pitch1``,
    inside poison.  Oracle: ``C.spectrum_check`` / ``C.spec_adjoint_check`` (tests/test_gpu_gated_stft_budget.py)."""
    tdt = _tdt(dtype)
    c = C.CASES[case]
    x = C.make_x(case, np.dtype(dtype))
    xn = C.make_xn(case, C.VARIANTS[variant][1], np.dtype(dtype))
    tg, gate = _torchgate_handle(C.gate_kwargs(case, variant), c["sr"])
    B, L = x.shape
    F = c["n_fft"] // 2 + 1
    T = gate.n_frames(L)
    FS = (F + 15) // 16 * 16
    units = _spec_units(case, variant, dtype)
    with gate.lock:
        def fwd(xv, xnv=None):
            Y, m = gate.gate_spectrum(xv, xnv, save_mask=True)
            return Y, m[:, :, :F]
        for ln in _names(tdt):
            tag = "gate_spectrum %s-%s %s [%s]" % (case, variant, dtype, ln)
            lays = [_lay(ln, x)] + ([] if xn is None else [_lay(ln, xn)])
            Y, m = _on_views(tag, gate, lays, fwd)
            if ln in ("off1", "pitch1"):
                _check_spectrum(tag, Y, m, units, "gate_spectrum/%s" % dtype)
        xa = torch.from_numpy(x).cuda()
        xna = None if xn is None else torch.from_numpy(xn).cuda()
        Y0, m0 = gate.gate_spectrum(xa, xna, save_mask=True)
        # ---- output side: out= and mask_out= at a flat offset inside poison
        for k in V.offsets(tdt):
            tag = "gate_spectrum(out=) %s-%s %s [flat_off%d]" % (case, variant, dtype, k)
            so, out = _poison_out((B, T, F, 2), tdt, "flat_off%d" % k)
            sm, mout = _poison_out((B, T, FS), torch.float32, "flat_off%d" % (k % 4 or 1))
            Y1, m1 = gate.gate_spectrum(xa, xna, out=out, mask_out=mout)
            gate.check_errors()
            assert Y1.data_ptr() == out.data_ptr() and m1.data_ptr() == mout.data_ptr()
            _same(tag, (Y1, m1[:, :, :F]), (Y0, m0[:, :, :F]))
            _outside_is_poison(tag, so, out)
            _outside_is_poison(tag + " mask", sm, mout)
            assert bool(V.is_poison(mout[:, :, F:].cpu()).all()), "%s: the padding columns of the mask were written" % tag
        # ---- backward: the gradient field at a flat offset, the result into off<k> / pitch1
        G, pairs = _grad_pairs((B, T, F), dtype, 11)
        pa = pairs.cuda()
        g0 = gate.gate_spectrum_backward(pa, m0, L)

        def bwd(pv):
            return gate.gate_spectrum_backward(pv, m0, L)
        for k in V.offsets(tdt):
            tag = "gate_spectrum_backward %s-%s %s [flat_off%d]" % (case, variant, dtype, k)
            lay, pv = _flat_nd(pairs, k)
            before = V.raw_bytes(lay.store).clone()
            gx = bwd(pv)
            gate.check_errors()
            assert torch.equal(V.raw_bytes(lay.store), before), tag
            _same(tag, gx, g0)
            if k == 1:
                Mn, gn, worst = m0[:, :, :F].transpose(1, 2).cpu().numpy(), gx.cpu().numpy(), 0.0
                for b in range(B):
                    bad, ratio = C.spec_adjoint_check(gn[b], G[b], Mn[b], units[b]["cfg"], L)
                    worst = max(worst, ratio)
                    assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                        tag, b, bad[:10].tolist(), ratio)
                print("%s: largest local_error / budget %.2f" % (tag, worst))
                _note("gate_spectrum_backward/%s" % dtype, worst)
        for ln in ["off%d" % k for k in V.offsets(tdt)] + ["pitch1"]:
            tag = "gate_spectrum_backward(out=) %s-%s %s [%s]" % (case, variant, dtype, ln)
            so, out = _poison_out((B, L), tdt, ln)
            g1 = gate.gate_spectrum_backward(pa, m0, L, out=out)
            gate.check_errors()
            assert g1.data_ptr() == out.data_ptr()
            _same(tag, g1, g0)
            _outside_is_poison(tag, so, out)
    del tg, gate


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case,bname", [("a", "mel80"), ("c", "mel40")], ids=["a-mel80", "c-mel40"])
def test_gate_features_and_backward(case, bname, dtype):
    """Oracle: ``K.feature_check`` per frame and ``K.grad_check`` per hop block (tests/test_gpu_gated_filterbank.py)."""
    tdt = _tdt(dtype)
    c = C.CASES[case]
    x = C.make_x(case, np.dtype(dtype))
    ref = K.reference(case, "plain", np.dtype(dtype).name)
    fb = K.bank(bname, case)
    tg, gate = _torchgate_handle(C.gate_kwargs(case, "plain"), c["sr"])
    B, L = x.shape
    F = c["n_fft"] // 2 + 1
    g = K.upstream(case, bname)                                                   # (B, M, T)
    gt = torch.from_numpy(np.ascontiguousarray(g.transpose(0, 2, 1))).to(tdt)     # (B, T, M)
    g = gt.numpy().astype(np.float64).transpose(0, 2, 1)
    with gate.lock:
        gate.set_filterbank(fb)
        for power, log in ((2, False), (1, True)):
            kw = dict(power=power, log=log, eps=K.EPS)

            def fwd(xv):
                f, m = gate.gate_features(xv, save_mask=True, **kw)
                return f, m[:, :, :F]
            _, m0 = gate.gate_features(torch.from_numpy(x).cuda(), save_mask=True, **kw)
            for ln in _names(tdt):
                tag = "gate_features %s-%s %s power %d log %s [%s]" % (case, bname, dtype, power, log, ln)
                lay = _lay(ln, x)
                f, m = _on_views(tag, gate, [lay], fwd)
                if ln in ("off1", "pitch1") and not log:
                    got, Mk, worst = f.transpose(1, 2).cpu().numpy(), m.transpose(1, 2).cpu().numpy(), 0.0
                    for b in range(B):
                        bad, ratio = K.feature_check(got[b], ref["X"][b], Mk[b], fb, power, ref["emu"][b])
                        worst = max(worst, ratio)
                        assert bad.size == 0, (tag, b, bad, ratio)
                    print("%s: largest local_error / budget %.2f" % (tag, worst))
                    _note("gate_features/%s" % dtype, worst)
                # the backward transforms x again: x on the layout, the upstream gradient at a flat offset
                glay = _lay("flat_off%d" % V.offsets(tdt)[-1], gt.reshape(-1))
                btag = tag.replace("gate_features", "gate_features_backward")
                gx = _on_views(btag, gate, [lay, glay],
                               lambda xv, gv: gate.gate_features_backward(xv, gv.view(gt.shape), m0, **kw))
                if ln in ("off1", "pitch1"):
                    gn, Mk, worst = gx.cpu().numpy(), m0[:, :, :F].transpose(1, 2).cpu().numpy(), 0.0
                    for b in range(B):
                        G64 = K.spectrum_grad(ref["X"][b], Mk[b], fb, g[b], power, log)
                        G32 = K.spectrum_grad32(ref["emu"][b], Mk[b], fb, g[b], power, log)
                        bad, ratio = K.grad_check(gn[b], G64, G32, case, L)
                        worst = max(worst, ratio)
                        assert bad.size == 0, (btag, b, bad, ratio)
                    print("%s: largest local_error / budget %.2f" % (btag, worst))
                    _note("gate_features_backward/%s" % dtype, worst)
    del tg, gate


# ---- the rows (lengths=) spectrum and features ----------------------------------------------------------------------------------
@pytest.mark.parametrize("gkind", R.GATES)
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("cname", ["E-256-256-64", "E-1024-1024-256"])
def test_gate_spectrum_rows_and_backward(cname, dtype, gkind):
    """Rows of 2 W, 2 W + 1, 16 H - 1, 16 H, 18 H - 1 samples and the padded length (odd), NaN behind each.  Oracle: the row
    alone under ``C.spectrum_check`` / ``C.spec_adjoint_check`` (tests/test_gpu_gated_stft_rows.py)."""
    tdt = _tdt(dtype)
    c = R.cell(cname)
    us = R.units(c, gkind, dtype)
    tg, gate = _torchgate_handle(R.gate_kwargs(c, gkind), R.SR)
    x = R.rows(c, dtype, pad=float("nan"))
    lens, L, F = c["lens"], c["L"], c["n_fft"] // 2 + 1
    names = _names(tdt, copies=("inner2",))
    with gate.lock:
        def fwd(xv):
            Y, m = gate.gate_spectrum_rows(xv, lens, save_mask=True)
            return Y, m[:, :, :F]
        for ln in names:
            tag = "gate_spectrum_rows %s %s %s [%s]" % (cname, gkind, dtype, ln)
            Y, m = _on_views(tag, gate, [_lay(ln, x)], fwd)
            if ln in ("off1", "pitch1") and gkind == "stat":
                _check_spectrum(tag, Y, m, us, "gate_spectrum_rows/%s" % dtype, rows=True)
        _, m0 = gate.gate_spectrum_rows(x.cuda(), lens, save_mask=True)
        G = R.grad_fields(c, dtype)["dense"]
        pairs = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(G.transpose(0, 2, 1))))
        g0 = gate.gate_spectrum_rows_backward(pairs.cuda(), m0, L, lens)
        Mn = m0[:, :, :F].transpose(1, 2).cpu().numpy()
        for k in V.offsets(tdt):
            tag = "gate_spectrum_rows_backward %s %s %s [flat_off%d]" % (cname, gkind, dtype, k)
            lay, pv = _flat_nd(pairs, k)
            before = V.raw_bytes(lay.store).clone()
            gx = gate.gate_spectrum_rows_backward(pv, m0, L, lens)
            gate.check_errors()
            assert torch.equal(V.raw_bytes(lay.store), before), tag
            _same(tag, gx, g0)
            if k == 1:
                gn, worst = gx.cpu().numpy(), 0.0
                for i, n in enumerate(lens):
                    Ti = R.frames_of(c)[i]
                    assert not gn[i, n:].any(), (tag, i)
                    bad, ratio = C.spec_adjoint_check(gn[i, :n], G[i, :, :Ti], Mn[i, :, :Ti], us[0]["cfg"], n)
                    worst = max(worst, ratio)
                    assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                        tag, i, bad[:10].tolist(), ratio)
                print("%s: largest local_error / budget %.2f" % (tag, worst))
                _note("gate_spectrum_rows_backward/%s" % dtype, worst)
    del tg, gate


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("cname", ["E-256-256-64", "E-1024-1024-256"])
def test_gate_features_rows_and_backward(cname, dtype):
    """Oracle: ``FR.forward_bad`` (the per-frame rule on every row alone) and ``FR.grad_check``
    (tests/test_gpu_gated_filterbank_rows.py)."""
    tdt = _tdt(dtype)
    c = R.cell(cname)
    us = R.units(c, "stat", dtype)
    tg, gate = _torchgate_handle(R.gate_kwargs(c, "stat"), R.SR)
    fb = FR.bank("mel40", c["n_fft"])
    x = R.rows(c, dtype, pad=float("nan"))
    lens, L, F = c["lens"], c["L"], c["n_fft"] // 2 + 1
    gn = FR.upstream(c, fb.shape[1], dtype)                                       # (B, M, T), NaN beyond a row's own frames
    gt = torch.from_numpy(np.ascontiguousarray(gn.transpose(0, 2, 1)))            # (B, T, M)
    names = _names(tdt, copies=("inner2",))
    with gate.lock:
        gate.set_filterbank(fb)
        for power, log in ((2, False), (1, True)):
            kw = dict(power=power, log=log, eps=FR.EPS)

            def fwd(xv):
                f, m = gate.gate_features_rows(xv, lens, save_mask=True, **kw)
                return f, m[:, :, :F]
            _, m0 = gate.gate_features_rows(x.cuda(), lens, save_mask=True, **kw)
            Mn = m0[:, :, :F].transpose(1, 2).cpu().numpy()
            for ln in names:
                tag = "gate_features_rows %s %s power %d log %s [%s]" % (cname, dtype, power, log, ln)
                lay = _lay(ln, x)
                f, m = _on_views(tag, gate, [lay], fwd)
                if ln in ("off1", "pitch1"):
                    res = FR.forward_bad(c, us, f.transpose(1, 2).cpu().numpy(), m.transpose(1, 2).cpu().numpy(), fb, power, log, dtype)
                    assert all(not bad and dead for bad, dead in res.values()), (tag, res)
                glay = _lay("flat_off%d" % V.offsets(tdt)[-1], gt.reshape(-1))
                btag = tag.replace("gate_features_rows", "gate_features_rows_backward")
                gx = _on_views(btag, gate, [lay, glay],
                               lambda xv, gv: gate.gate_features_rows_backward(xv, gv.view(gt.shape), m0, lens, **kw))
                assert bool(torch.isfinite(gx).all()), btag
                if ln in ("off1", "pitch1"):
                    gxn, worst = gx.cpu().numpy(), 0.0
                    for i, n in enumerate(lens):
                        Ti = R.frames_of(c)[i]
                        unit = FR.grad_unit(us[i], Mn[i][:, :Ti], fb, gn[i][:, :Ti].astype(np.float64), power, log, n)
                        bad, ratio = FR.grad_check(gxn[i, :n], unit)
                        worst = max(worst, ratio)
                        assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
                            btag, i, bad[:10].tolist(), ratio)
                    print("%s: largest local_error / budget %.2f" % (btag, worst))
                    _note("gate_features_rows_backward/%s" % dtype, worst)
    del tg, gate


# ---- variant S: process_chunks (with halos, with out=), filter_padded, stft, noise_stats -----------------------------------------
# one register geometry per size and one general LDS cell, column 1: three channels, a chunk grid with padding, a noise clip
S_CELLS = [c for c in PB.CELLS if c["col"] == 1 and (c["family"] == "register" or (c["family"], c["n_fft"]) == ("lds_pow2", 128))]
I16_SCALE = 12000.0


def _s_case(cell, dtype):
    """The cell's recording and noise clip in ``dtype`` (int16: 12000 x, rounded), as tests/stagewise_checks.py's make_sg
    takes them."""
    case = PB.cell_case(cell)
    if dtype == "int16":
        return dict(case, y=np.rint(case["y"] * I16_SCALE), y_noise=np.rint(case["y_noise"] * I16_SCALE), dtype="int16")
    return dict(case, dtype=dtype)


@pytest.mark.parametrize("dtype", ["float32", "float64", "int16"])
@pytest.mark.parametrize("cell", S_CELLS, ids=PB.cell_id)
def test_stationary_entry_points(cell, dtype):
    """Oracle (float32 / float64 samples, ``off1`` and ``pitch1``): ``SC.check_output`` per hop block for process_chunks,
    the reference's 1e-4 for filter_padded (tests/test_gpu_parity.py::test_do_filter_seam), 1e-13 for the float64 STFT tap
    and 1e-9 dB for the threshold (tests/test_gpu_parity.py::test_stage_taps).  int16: the float64 pipeline; its oracle
    check is ``test_the_floor_sees_the_head_and_the_tail_of_a_unit``."""
    tdt = _tdt(dtype)
    case = _s_case(cell, dtype)
    kw = case["kw"]
    cs, pad = kw["chunk_size"], kw["padding"]
    sg = SC.make_sg(case)
    gate = sg._gate
    y = case["y"].astype(dtype)                      # (3, N)
    Cn, N = y.shape
    fam = PB.kernel_family(cell)
    oracle = dtype != "int16"
    if oracle:
        out, units = PB.cell_oracle(cell)
        emus = [PB.emulate_stages_f32(u) for u in units]
    with gate.lock:
        # ---- process_chunks
        def chunks(v):
            sg._bind()
            return gate.process_chunks(v if v.dim() == 2 else v[None, :], chunked=True)
        y0 = chunks(torch.from_numpy(y).cuda())
        for ln in _names(tdt) + ["flat_off%d" % k for k in V.offsets(tdt)]:
            tag = "process_chunks %s %s [%s]" % (PB.cell_id(cell), dtype, ln)
            got = _on_views(tag, gate, [_lay(ln, y[1] if ln.startswith("flat") else y)], chunks)
            if oracle and ln in ("off1", "pitch1"):
                ratios = {}
                SC.check_output(tag, fam, dict(case, precision=None), got.cpu().numpy(), out, units, emus, "views", ratios)
                _note("process_chunks/%s" % dtype, max(ratios.values()))
        # ---- process_chunks with halos: the pointer itself moves by halo_left elements
        for hl in (1, 3):
            for hr in (0, 2):
                def halo(v):
                    sg._bind()
                    return gate.process_chunks(v, out_dtype=v.dtype, chunked=True, halo_left=hl, halo_right=hr)
                for ln in ["off%d" % k for k in V.offsets(tdt)] + ["pitch1", "inner2"]:
                    tag = "process_chunks %s %s halos (%d, %d) [%s]" % (PB.cell_id(cell), dtype, hl, hr, ln)
                    got = _on_views(tag, gate, [_lay(ln, y)], halo)
                    assert tuple(got.shape) == (Cn, N - hl - hr)
        # ---- process_chunks(out=): into off<k> / pitch1 inside poison
        for ln in ["off%d" % k for k in V.offsets(tdt)] + ["pitch1"]:
            tag = "process_chunks(out=) %s %s [%s]" % (PB.cell_id(cell), dtype, ln)
            so, outv = _poison_out((Cn, N), tdt, ln)
            sg._bind()
            got = gate.process_chunks(torch.from_numpy(y).cuda(), chunked=True, out=outv)
            gate.check_errors()
            assert got.data_ptr() == outv.data_ptr()
            _same(tag, got, y0)
            _outside_is_poison(tag, so, outv)
        # ---- filter_padded: the recording as one padded chunk
        def padded(v):
            sg._bind()
            return gate.filter_padded(v)
        for ln in _names(tdt):
            tag = "filter_padded %s %s [%s]" % (PB.cell_id(cell), dtype, ln)
            got = _on_views(tag, gate, [_lay(ln, y)], padded)
            if oracle and ln in ("off1", "pitch1"):
                cfg = units[0]["cfg"]
                want = O.gate_stationary_S(y.astype(np.float64), units[0]["thresh"], cfg["n_fft"], cfg["W"], cfg["H"], cfg["prop"], cfg["filt"])
                err = O.rel_err(got.cpu().numpy(), want)
                print("%s: rel err %.3g" % (tag, err))
                assert err < 1e-4, (tag, err)
        # ---- stft: the padded window of chunk 1 of every channel
        win = O.read_chunk(y.astype(np.float64), cs - pad, 2 * cs + pad).astype(dtype)
        nch = len(units) // Cn if oracle else 0
        for ln in _names(tdt):
            tag = "stft %s %s [%s]" % (PB.cell_id(cell), dtype, ln)
            Z = _on_views(tag, gate, [_lay(ln, win)], gate.stft)
            if oracle and ln in ("off1", "pitch1"):
                Zn = Z.cpu().numpy()
                for ci in range(Cn):
                    Zo = units[ci * nch + 1]["Z"].T
                    d = float(np.max(np.abs(Zn[ci] - Zo)))
                    assert d <= 1e-13 * max(1.0, float(np.max(np.abs(Zo)))), (tag, ci, d)
        # ---- noise_stats: the clip as one row (the threshold the oracle's units hold), and three channels of the recording
        def stats(v):
            gate.noise_stats(v if v.dim() == 2 else v[None, :])
            return gate.noise_threshold_tensor()
        clip = case["y_noise"].astype(dtype)
        for ln in ["off%d" % k for k in V.offsets(tdt)] + ["flat_off%d" % k for k in V.offsets(tdt)] + ["inner2"]:
            tag = "noise_stats %s %s one row [%s]" % (PB.cell_id(cell), dtype, ln)
            thr = _on_views(tag, gate, [_lay(ln, clip if ln.startswith("flat") else clip[None, :])], stats)
            if oracle and ln in ("off1", "flat_off1"):
                d = float(np.max(np.abs(thr.cpu().numpy() - units[0]["thresh"])))
                print("%s: threshold within %.3g dB of the oracle's" % (tag, d))
                assert d <= 1e-9, (tag, d)
        for ln in _names(tdt):
            tag = "noise_stats %s %s three channels [%s]" % (PB.cell_id(cell), dtype, ln)
            _on_views(tag, gate, [_lay(ln, y[:, :cs])], stats)


# ---- public objects on a device view -----------------------------------------------------------------------------------------
def _sg_of(case, y, y_noise=None):
    """tests/stagewise_checks.py's make_sg with device tensors handed over as they are."""
    from noisereduce_amd.spectralgate.nonstationary import SpectralGateNonStationary
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    kw = case["kw"]
    base = dict(y=y, sr=PB.SR, prop_decrease=kw["prop_decrease"], chunk_size=kw["chunk_size"], padding=kw["padding"],
                n_fft=kw["n_fft"], win_length=kw.get("win_length"), hop_length=kw.get("hop_length"),
                time_constant_s=kw.get("time_constant_s", 2.0),
                freq_mask_smooth_hz=kw.get("freq_mask_smooth_hz", 500), time_mask_smooth_ms=kw.get("time_mask_smooth_ms", 50),
                tmp_folder=None, use_tqdm=False, n_jobs=1, precision=case.get("precision"))
    if kw["stationary"]:
        return SpectralGateStationary(y_noise=y_noise, n_std_thresh_stationary=1.5, clip_noise_stationary=True, **base)
    return SpectralGateNonStationary(thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, **base)


@pytest.mark.parametrize("col", [1, 4], ids=["SpectralGateStationary", "SpectralGateNonStationary"])
def test_spectral_gate_objects_on_a_device_view(col):
    """``SpectralGate*(y=view)`` and, stationary, ``y_noise=view``.  Oracle: ``SC.check_output``."""
    cell = next(c for c in PB.CELLS if (c["family"], c["n_fft"], c["col"]) == ("register", 1024, col))
    case = PB.cell_case(cell)
    out, units = PB.cell_oracle(cell)
    emus = [PB.emulate_stages_f32(u) for u in units]
    y = case["y"].astype(np.float32)
    for ln in ("off1", "pitch1"):
        tag = "%s [%s]" % (PB.cell_id(cell), ln)
        lays = [_lay(ln, y)]
        if case["y_noise"] is not None:
            lays.append(_lay("flat_off1" if ln == "off1" else "flat_off3", case["y_noise"].astype(np.float32)))
        gate = _sg_of(case, *[l.view for l in lays])._gate

        def run(*views):
            sg = _sg_of(case, *views)
            assert sg._gate is gate
            return sg.get_traces()
        got = _on_views(tag, gate, lays, run)
        assert got.dtype == torch.float32 and tuple(got.shape) == y.shape
        ratios = {}
        SC.check_output(tag, "register", case, got.cpu().numpy(), out, units, emus, "views", ratios)
        _note("SpectralGate%sStationary(y=view)" % ("" if col == 1 else "Non"), max(ratios.values()))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_torchgate_on_a_device_view(dtype):
    """``TorchGate.forward`` / ``gated_stft`` / ``gated_filterbank`` with x (and xn) a view, gradients included.  Oracle: the
    project's 1e-4 against ``O.torchgate_T`` for forward (tests/test_gpu_gated_stft.py), ``C.spectrum_check`` and
    ``K.feature_check`` for the other two."""
    from noisereduce_amd.torchgate import TorchGate
    tdt = _tdt(dtype)
    case, variant = "a", "xnB"
    c = C.CASES[case]
    tg = TorchGate(sr=c["sr"], **C.gate_kwargs(case, variant)).cuda()
    gate = tg._gate_for(torch.device("cuda", torch.cuda.current_device()))
    x = C.make_x(case, np.dtype(dtype))
    xn = C.make_xn(case, "batch", np.dtype(dtype))
    fb = K.bank("mel80", case)
    fbt = torch.from_numpy(fb.copy())
    want_y, _ = C.oracle(case, variant, np.dtype(dtype).name)
    units = _spec_units(case, variant, dtype)
    ref = K.reference(case, variant, np.dtype(dtype).name)

    def all_three(xv, xnv):
        xg = xv.detach().requires_grad_()
        outs = []
        y = tg(xg, xnv)
        y.backward(torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(tdt).cuda())
        outs += [y.detach(), xg.grad.clone()]
        xg.grad = None
        Y, M = tg.gated_stft(xg, xnv, return_mask=True)
        R_ = torch.view_as_real(Y)
        (R_ * torch.randn(R_.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64).to(tdt).cuda()).sum().backward()
        outs += [R_.detach(), M.contiguous(), xg.grad.clone()]
        xg.grad = None
        Fm = tg.gated_filterbank(xg, fbt, xnv, power=2.0)
        (Fm * torch.randn(Fm.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(tdt).cuda()).sum().backward()
        outs += [Fm.detach().contiguous(), xg.grad.clone()]
        return tuple(outs)
    for ln in ("off1", "pitch1"):
        tag = "TorchGate %s-%s %s [%s]" % (case, variant, dtype, ln)
        y, gy, Yr, M, gs, Fm, gf = _on_views(tag, gate, [_lay(ln, x), _lay(ln, xn)], all_three)
        err = O.rel_err(y.cpu().numpy(), want_y)
        print("%s: forward rel err %.3g" % (tag, err))
        assert err < 1e-4, (tag, err)
        _check_spectrum(tag + " gated_stft", Yr.transpose(1, 2), M.transpose(1, 2), units, "TorchGate.gated_stft/%s" % dtype)
        got, Mk, worst = Fm.cpu().numpy(), M.cpu().numpy(), 0.0
        for b in range(x.shape[0]):
            bad, ratio = K.feature_check(got[b], ref["X"][b], Mk[b], fb, 2, ref["emu"][b])
            worst = max(worst, ratio)
            assert bad.size == 0, (tag, b, bad, ratio)
        _note("TorchGate.gated_filterbank/%s" % dtype, worst)
        for g in (gy, gs, gf):
            assert bool(torch.isfinite(g).all()) and bool(g.any()), tag


# ---- the floor's unit maximum ------------------------------------------------------------------------------------------------
from tests.test_views_host import U_CELLS  # noqa: E402  (the cells and what makes them mean something: on the oracle alone)


@pytest.mark.parametrize("dtype, where, k", U_CELLS, ids=["%s-%s-k%d" % c for c in U_CELLS])
def test_the_floor_sees_the_head_and_the_tail_of_a_unit(dtype, where, k):
    """Low-level noise and ONE impulse, in the scalar head (tail) ``k_unit_absmax`` reads sample by sample at this offset: only
    the impulse can switch the -top_db floor on.  The default route, and the a-priori floor test forced
    (SG_OPT_FLOOR_TEST 1: ``k_unit_absmax + k_prep_thresh``, asserted from the profile) where the one-pass gate can choose.
    Bits fetched as tests/test_gpu_floor.py fetches them; int16: the output is the truncated float64 oracle's."""
    from noisereduce_amd import _ffi
    from tests.test_gpu_floor import _bits_of
    pos = V.u_position(dtype, where, k)
    y, noise = V.u_recording(dtype, pos)
    out, units = V.u_oracle(dtype, pos)
    ui, f, margin = V.u_named_band(dtype, where, k)
    case = dict(kw=V.u_geometry(dtype)[2], precision=None)
    lay = V.make_flat(y, k, DEV)
    V.assert_claims(lay)
    assert lay.view.data_ptr() % 16 == (k * lay.view.element_size()) % 16 != 0
    before = V.raw_bytes(lay.store).clone()
    noise_t = torch.from_numpy(noise).cuda()
    sg = _sg_of(case, lay.view, noise_t)
    sg_clone = _sg_of(case, V.aligned_clone(lay.view), noise_t)
    gate = sg._gate
    assert sg_clone._gate is gate
    routes = [("default", [])] + ([("floor_test_1", [(_ffi.SG_OPT_FLOOR_TEST, 1)])] if dtype == "float32" else [])
    gate.profile_enable(True)
    try:
        for route, opts in routes:
            tag = "unit maximum %s %s k=%d [%s]" % (dtype, where, k, route)
            with gate.lock, gate.with_options(opts):
                gate.profile_read(reset=True)
                got = sg.get_traces()
                stages = SC.stages_of(gate)
                if route == "floor_test_1" or dtype == "int16":
                    assert any("k_unit_absmax" in s for s in stages), (tag, sorted(stages))
                bits, (d0, d1) = _bits_of(tag, gate, "k_decide" in stages)
                assert bits.shape[0] == len(units), tag
                # the named band of the unit whose head (tail) holds the impulse passes whole, as the oracle says
                assert np.all(units[ui]["raw"][f]), tag
                assert np.all(bits[ui][f, d0:d1]), "%s: unit %d band %d (%.2f dB over its switch in the oracle) is not lifted: " \
                    "%d of %d cells pass -- the maximum missed the impulse at sample %d" % (
                        tag, ui, f, margin, int(bits[ui][f, d0:d1].sum()), d1 - d0, pos)
                for j, u in enumerate(units):
                    cells, left = PB.bit_diff(bits[j], u, frames=(d0, d1))
                    assert left <= PB.LEFT_OUT_CAP
                    assert len(cells) == 0, "%s unit %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                        tag, j, len(cells), cells[:6].tolist())
                got2 = sg_clone.get_traces()
                bits2, _ = _bits_of(tag + " clone", gate, "k_decide" in stages)
                gate.check_errors()
                _same(tag, got, got2)
                assert np.array_equal(bits, bits2), tag
                assert torch.equal(V.raw_bytes(lay.store), before), tag
                if dtype == "int16":
                    assert np.array_equal(got.cpu().numpy(), np.trunc(out).astype(np.int16)), tag
    finally:
        gate.profile_enable(False)


# ---- tensors the ABI takes without strides: refused before anything is launched ---------------------------------------------
def test_wrappers_refuse_a_strided_tensor_before_anything_is_launched():
    """Every wrapper that hands over ``data_ptr()`` alone, with a ``[::2]`` tensor in each such argument: ValueError naming the
    argument, no kernel launched (the profile of the handle stays empty), the handle usable afterwards."""
    from noisereduce_amd import _ffi
    tg, gate = _torchgate_handle(C.gate_kwargs("c", "plain"), 16000)
    x = torch.from_numpy(C.make_x("c", np.float32)).cuda()
    B, L = x.shape
    F, T = 129, gate.n_frames(L)
    fb = K.bank("mel40", "c")
    lens = [L] * B
    s_gate = _ffi.Gate("cuda", variant=_ffi.SG_VARIANT_S, stationary=True, n_fft=1024, win_length=1024, hop_length=256,
                       chunk_size=8192, padding=2048)
    flat = torch.zeros(16384, device="cuda")

    def refused(name, fn):
        with pytest.raises(ValueError, match="^%s must be " % name):
            fn()
    try:
        with gate.lock:
            gate.set_filterbank(fb)
            Y, mask = gate.gate_spectrum(x, save_mask=True)
            mask[:, :, F:] = 0.0          # (the padding columns are never written: whatever the allocation held)
            feat = gate.gate_features(x)
            y = gate.process_batch(x)
            wide = torch.zeros((B, T, 2 * mask.shape[2]), device="cuda")
            wide[:, :, ::2] = mask
            bad = wide[:, :, ::2]
            assert torch.equal(bad, mask) and not bad.is_contiguous()
            gate.profile_enable(True)
            gate.profile_read(reset=True)
            refused("mask", lambda: gate.process_batch_backward(y, bad, L))
            refused("mask", lambda: gate.process_rows_backward(y, bad, L, lens))
            refused("mask", lambda: gate.gate_spectrum_backward(Y, bad, L))
            refused("mask", lambda: gate.gate_spectrum_rows_backward(Y, bad, L, lens))
            refused("mask", lambda: gate.gate_features_backward(x, feat, bad))
            refused("mask", lambda: gate.gate_features_rows_backward(x, feat, bad, lens))
            refused("mask", lambda: gate.process_batch_backward(y, mask.double(), L))
            assert gate.profile_read(reset=True) == {}, "a refused call launched a kernel"
            gate.profile_enable(False)
            assert torch.equal(gate.gate_spectrum_backward(Y, mask, L), gate.gate_spectrum_backward(Y, mask.clone(), L))
        s_gate.profile_enable(True)
        s_gate.profile_read(reset=True)
        half = flat[::2]
        clips = [_ffi.SgClip(x_offset=0, n=4096, x_stride=4096, channels=1, noise=0, out_offset=0, out_stride=4096)]
        srcs = [_ffi.SgNoiseSrc(offset=0, n=4096, stride=4096, channels=1, in_x=1)]
        refused("x", lambda: s_gate.process_clips(half, clips, flat, noise_srcs=srcs))
        refused("out", lambda: s_gate.process_clips(flat, clips, half, noise_srcs=srcs))
        refused("noise", lambda: s_gate.process_clips(flat, clips, flat.clone(), noise=torch.zeros(8192, dtype=torch.float64, device="cuda")[::2],
                                                         noise_srcs=srcs))
        rec = [_ffi.SgStreamRec(slot=0, flush=0, n_samples=1024, in_offset=0, in_stride=1024, out_offset=0, out_stride=1024)]
        srec = [_ffi.SgStreamSpecRec(spec_offset=0, mask_offset=0, stride=513)]
        frec = [_ffi.SgStreamFeatRec(feat_offset=0, feat_stride=40, mask_offset=0, mask_stride=513)]
        cflat = torch.zeros(8192, dtype=torch.complex64, device="cuda")
        # (the layout is looked at before the bank: none is needed to be refused)
        refused("x", lambda: s_gate.stream_push(None, half, flat, rec))
        refused("out", lambda: s_gate.stream_push(None, flat, half, rec))
        refused("x", lambda: s_gate.stream_push_spectrum(None, half, flat, cflat, None, rec, srec))
        refused("out", lambda: s_gate.stream_push_spectrum(None, flat, half, cflat, None, rec, srec))
        refused("spec", lambda: s_gate.stream_push_spectrum(None, flat, flat, cflat[::2], None, rec, srec))
        refused("mask", lambda: s_gate.stream_push_spectrum(None, flat, flat, cflat, half, rec, srec))
        refused("x", lambda: s_gate.stream_push_features(None, half, flat, flat, None, rec, frec, 2, False, 1e-6, 0.0))
        refused("out", lambda: s_gate.stream_push_features(None, flat, half, flat, None, rec, frec, 2, False, 1e-6, 0.0))
        refused("feat", lambda: s_gate.stream_push_features(None, flat, flat, half, None, rec, frec, 2, False, 1e-6, 0.0))
        refused("mask", lambda: s_gate.stream_push_features(None, flat, flat, flat, half, rec, frec, 2, False, 1e-6, 0.0))
        rec2 = flat.view(2, 8192)
        refused("out", lambda: s_gate.process_chunks(rec2, chunked=True, out=torch.zeros((2, 16384), device="cuda")[:, ::2]))
        refused("out", lambda: s_gate.process_chunks(rec2, chunked=True, out=torch.zeros((8192, 2), device="cuda").t()))
        with pytest.raises(ValueError, match="out must be a"):
            s_gate.process_chunks(rec2, chunked=True, out=torch.zeros((2, 8000), device="cuda"))
        refused("t", lambda: s_gate.set_noise_threshold_tensor(torch.zeros(1026, dtype=torch.float64, device="cuda")[::2]))
        assert s_gate.profile_read(reset=True) == {}, "a refused call launched a kernel"
        s_gate.profile_enable(False)
        s_gate.check_errors()
        # the handle still works: a threshold tensor as it should be, then a gate call
        s_gate.set_noise_threshold_tensor(torch.full((513,), -60.0, dtype=torch.float64, device="cuda"))
        assert bool(torch.isfinite(s_gate.process_chunks(torch.randn(2, 8192, device="cuda"), chunked=False)).all())
    finally:
        s_gate.close()
    del tg, gate
