"""Layouts of a caller's samples: unaligned, strided, repeated and overlapping views of a poisoned buffer, for holding a
device-tensor entry point on such a view to the same call on ``view.clone()`` (aligned, contiguous).
tests/test_views_host.py holds the layouts themselves, and what ``_ffi._rows`` does with them, on CPU tensors.

``_ffi._rows`` hands the library ``data_ptr()`` and ``stride(0)`` of any 2-D tensor whose rows are contiguous, and the
kernels pick a 16-byte (8-byte) vector path or a per-sample path by the alignment of a pointer they compute per row or per
tile.  A layout places given samples in a larger buffer filled with poison so that those pointers land in a chosen residue
class of 16 bytes:

==========  ==============================================  =========================================================
off<k>      ``buf(B, P + 64)[:, k:k + L]``                   every row k elements off; P = L rounded up to 8 elements, so the
                                                            pitch keeps the residue (16 bytes: 4 float32, 2 float64, 8 int16)
pitch1      ``buf(B, P + 1)[:, :L]``                         row r is r elements off: aligned and unaligned rows in one launch
oddL        contiguous ``(B, L)`` with L odd                the caller passes L + 1 samples where its own L is even
flat_off    ``buf(L + 64)[k:k + L]``                         one channel, 1-D
inner2      ``buf(B, 2 L)[:, ::2]``                          last stride 2
expand      ``row.expand(B, L)``                            row stride 0
overlap     ``flat.unfold(0, L, L // 2)``                   row stride L // 2 < L
==========  ==============================================  =========================================================

Poison: NaN for floats, alternating +-32767 for int16.  ``MARGIN`` = 32 elements of poison lie before the first row's buffer
and 32 or more behind the last sample of the view; the gaps between rows hold poison too, so an over-read stays inside the
allocation and shows as a difference.  ``expand`` and ``overlap`` cannot hold B independent rows: they take their samples
from row 0 (``Layout.samples`` is what the view holds).

Further down: the recordings of the floor's unit maximum (``k_unit_absmax``: scalar head, aligned middle, scalar tail), in
which only an impulse in the head or in the tail can switch the -top_db floor on.
"""
import collections
import functools

import numpy as np
import torch

from tests import parity_budget as PB

MARGIN = 32
SLACK = 64            # poison columns of the off<k> and flat_off buffers
_TORCH = {"float32": torch.float32, "float64": torch.float64, "int16": torch.int16}

# store: the whole allocation (1-D); view: the tensor handed to the entry point; samples: numpy, what the view holds;
# claims: data_ptr() % 16 of row 0 and row 1 (row 0 alone for one row or a 1-D view) given a 16-byte aligned allocation
Layout = collections.namedtuple("Layout", "name store view samples claims")

ROW_LAYOUTS = ("off1", "off2", "off3", "pitch1", "oddL")
COPY_LAYOUTS = ("inner2", "expand", "overlap")      # _ffi._rows copies these


def poison(n, dtype):
    """(n,) tensor of poison on the CPU."""
    if dtype == torch.int16:
        p = torch.full((n,), 32767, dtype=torch.int16)
        p[1::2] = -32767
        return p
    return torch.full((n,), float("nan"), dtype=dtype)


def is_poison(t):
    """Elementwise: does a (CPU) tensor hold poison?  (int16: either sign of it.)"""
    if t.dtype == torch.int16:
        return t.abs() == 32767
    return torch.isnan(t)


def _up8(n):
    return (n + 7) // 8 * 8


def offsets(dtype):
    """The off<k> / flat_off offsets that cover every residue class of the element size: float32 1, 2, 3 of the 16-byte
    loads; float64 1; int16 1, 2, 3 and 5 -- with 3 + 4 = 7 and 5 the odd classes of the 8-byte loads of ``vec16`` and, with
    2, classes on both sides of every boundary of the 16-byte loads of ``k_unit_absmax``."""
    return {torch.float32: (1, 2, 3), torch.float64: (1,), torch.int16: (1, 2, 3, 5)}[_dtype(dtype)]


def _dtype(dtype):
    return _TORCH[dtype] if isinstance(dtype, str) else dtype


def residue(t, row=0):
    """Byte offset mod 16 of row ``row`` of a view from the start of its allocation (which the caller holds to 16 bytes),
    from storage_offset(), stride() and the element size alone."""
    off = t.storage_offset() + (row * t.stride(0) if t.dim() == 2 else 0)
    return (off * t.element_size()) % 16


def _cpu(a):
    """A contiguous CPU tensor of its own (the case tables hand out read-only arrays)."""
    return torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a.detach().cpu().contiguous()


def make(name, a, device="cpu"):
    """Layout ``name`` of the samples ``a`` ((B, L), or (L,) for flat_off; numpy or tensor) on ``device``."""
    a = _cpu(a)
    dt, es = a.dtype, a.element_size()

    def alloc(n):                        # MARGIN | n elements | MARGIN, all poison
        return poison(MARGIN + n + MARGIN, dt)

    if name.startswith("flat_off"):
        return make_flat(a, int(name[8:]), device)
    B, L = a.shape
    if name.startswith("off"):
        k = int(name[3:])
        # NOT the pitch L + 64 of a plain ``buf(B, L + 64)``: for L no multiple of 4 (PB.R_CELLS: L = 13 mod 256) that pitch
        # would walk the rows through the residues and no row but row 0 would be k elements off.  L is rounded up to 8
        # elements first, so the pitch is a multiple of 16 bytes at every element size; for L a multiple of 8 it IS L + 64
        P = _up8(L) + SLACK
        store = alloc(B * P)
        rows = store[MARGIN:MARGIN + B * P].view(B, P)
        view = rows[:, k:k + L]
        view.copy_(a)
        samples, claims = a, [(k * es) % 16] * min(B, 2)
    elif name == "pitch1":
        # NOT always "a row pitch of L + 1": L rounded up to 8 elements, + 1, so that row r is r elements off whatever L is
        # (with L + 1 and L = 1 mod 4 row r would be 2 r off and the odd residues never met).  For L a multiple of 8, which
        # covers gated_stft_cases' a, c and the recordings of _geometry, the pitch is L + 1; otherwise the gap between rows
        # is up to 8 elements of poison instead of 1
        P = _up8(L) + 1
        store = alloc(B * P)
        view = store[MARGIN:MARGIN + B * P].view(B, P)[:, :L]
        view.copy_(a)
        samples, claims = a, [(r * es) % 16 for r in range(min(B, 2))]
    elif name == "oddL":
        assert L % 2 == 1, "oddL takes an odd row length (pass one more sample of the signal)"
        store = alloc(B * L)
        view = store[MARGIN:MARGIN + B * L].view(B, L)
        view.copy_(a)
        samples, claims = a, [(r * L * es) % 16 for r in range(min(B, 2))]
        assert B < 2 or claims[1] != 0
    elif name == "inner2":
        store = alloc(B * 2 * L)
        view = store[MARGIN:MARGIN + B * 2 * L].view(B, 2 * L)[:, ::2]
        view.copy_(a)
        samples, claims = a, [(r * 2 * L * es) % 16 for r in range(min(B, 2))]
    elif name == "expand":
        store = alloc(L)
        store[MARGIN:MARGIN + L] = a[0]
        view = store[MARGIN:MARGIN + L].unsqueeze(0).expand(B, L)
        samples, claims = a[:1].expand(B, L), [0] * min(B, 2)
    elif name == "overlap":
        step = L // 2
        n = L + (B - 1) * step
        flat = a.reshape(-1)
        flat = flat[:n] if flat.numel() >= n else torch.cat([flat, flat])[:n]
        store = alloc(n)
        store[MARGIN:MARGIN + n] = flat
        view = store[MARGIN:MARGIN + n].unfold(0, L, step)
        assert tuple(view.shape) == (B, L) and view.stride() == (step, 1)
        samples, claims = flat.unfold(0, L, step), [(r * step * es) % 16 for r in range(min(B, 2))]
    else:
        raise KeyError(name)
    return _finish(name, store, view, samples, claims, device)


def make_flat(a, k, device="cpu"):
    """flat_off: ``buf(L + 64)[k:k + L]`` of the 1-D samples ``a``."""
    a = _cpu(a)
    assert a.dim() == 1 and 0 < k <= SLACK - MARGIN
    L = a.shape[0]
    store = poison(MARGIN + L + SLACK, a.dtype)
    view = store[MARGIN + k:MARGIN + k + L]
    view.copy_(a)
    return _finish("flat_off%d" % k, store, view, a, [(k * a.element_size()) % 16], device)


def _finish(name, store, view, samples, claims, device):
    samples = samples.clone().numpy()
    if torch.device(device).type != "cpu":
        dev = store.to(device)
        view = dev.as_strided(tuple(view.shape), view.stride(), view.storage_offset())
        store = dev
    return Layout(name, store, view, samples, claims)


def aligned_clone(view):
    """The same samples in a fresh contiguous allocation (``view.clone()`` keeps the strides of a dense view)."""
    return view.clone(memory_format=torch.contiguous_format)


def assert_claims(lay):
    """The view sits where the layout says: data_ptr() % 16 of row 0 and of row 1 (tests/test_gpu_onepass_plan.py asserts
    the same of its one view)."""
    v = lay.view
    assert lay.store.data_ptr() % 16 == 0, "the allocation itself is not 16-byte aligned"
    got = [v.data_ptr() % 16]
    if v.dim() == 2 and v.shape[0] > 1:
        got.append((v.data_ptr() + v.stride(0) * v.element_size()) % 16)
    assert got == list(lay.claims), "%s: rows at %s mod 16, the layout claims %s" % (lay.name, got, lay.claims)


def raw_bytes(t):
    return t.contiguous().view(torch.uint8)


def odd_rows(a):
    """(B, L) -> (B, L') with L' odd: the rows as they are where L is odd, else with one more sample (each row's last but
    one again: no step the signal does not already hold)."""
    a = np.asarray(a)
    if a.shape[1] % 2 == 1:
        return a
    return np.concatenate([a, a[:, -2:-1]], axis=1)


# ----------------------------------------------------------------------------------------------------------------
# the floor's unit maximum
# ----------------------------------------------------------------------------------------------------------------
# k_unit_absmax (csrc/fused.hpp) bounds every |X[k]| of a unit by max|x| sum|w|: the -top_db floor of _amp_to_db can lift
# a band over its threshold only where 20 log10(max|x|) - 80 exceeds the smallest threshold.  It reads the unit's window
# with 16-byte loads over the aligned middle and sample by sample over a head and a tail of up to 3 float32 (7 int16)
# samples.  The recordings here are the geometry of PB.F_CELLS' register-1024 cells (five units of 56 frames) holding
# low-level noise -- its maximum far under that level -- and ONE impulse, in the head of unit 0 or in the tail of the last
# units, which alone lifts bands: a maximum that misses the head or the tail leaves the floor off and the decision bits
# of the lifted bands wrong.
U_CELL = {"float32": "register-1024", "int16": "register-1024-i16"}
U_PER16 = {"float32": 4, "int16": 8}                     # elements per 16-byte load
U_OFFSETS = {"float32": (1, 2, 3), "int16": (1, 3, 5, 7)}
# float32: the base noise and noise clip of PB._f_build (1e-5 and 3e-5 RMS), an impulse of 64.
# int16: an impulse cannot exceed 32767, (impulse x window / sum w) must clear a switch level that max|rest| stays under --
# a factor of ~600 between them -- so the rest is +-2 LSB and the noise clip a float32 clip of 0.02 LSB RMS (the noise
# statistics take their own dtype).
U_IMPULSE = {"float32": 64.0, "int16": 32000.0}


U_SLACK_DB = 1.0     # how far under the engine's a-priori level the rest must stay (the engine's own slack: 1e-6 dB + an ulp)


def u_top_db():
    """The -top_db of the stationary gate as the engine is given it: read from SpectralGateStationary's handle arguments."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "noisereduce_amd", "spectralgate", "stationary.py")) as f:
        m = re.findall(r"top_db=([0-9.]+)", f.read())
    assert len(m) == 1, m
    return float(m[0])


def u_geometry(dtype):
    cell = PB.f_cell(U_CELL[dtype])
    return cell, PB._f_geometry(cell), PB._f_kw(cell)


def u_head_len(dtype, k):
    """Samples of a row k elements off a 16-byte boundary that precede the first aligned 16-byte load."""
    return (-k) % U_PER16[dtype]


def u_position(dtype, where, k):
    """Row index of the impulse: the last sample of the head (``first``), the last sample of the row (``last``; N is a
    multiple of 8, so a row k elements off ends k samples behind a boundary)."""
    N = u_geometry(dtype)[1][5]
    assert N % 8 == 0 and 0 < k < U_PER16[dtype]
    return u_head_len(dtype, k) - 1 if where == "first" else N - 1


@functools.lru_cache(maxsize=None)
def _u_rest(dtype):
    cell, (n_fft, W, H, cs, pad, N), kw = u_geometry(dtype)
    rng = np.random.default_rng(9900 + (dtype == "int16"))
    if dtype == "int16":
        y = rng.integers(-2, 3, size=N).astype(np.int16)
        noise = (0.02 * rng.standard_normal(40 * H)).astype(np.float32)
    else:
        y = (1e-5 * rng.standard_normal(N)).astype(np.float32)
        noise = (3e-5 * rng.standard_normal(40 * H)).astype(np.float32)
    y.setflags(write=False)
    noise.setflags(write=False)
    return y, noise


def u_recording(dtype, pos=None):
    """``(y, y_noise)``: the rest alone (``pos`` None) or with the impulse at row index ``pos``."""
    y, noise = _u_rest(dtype)
    if pos is None:
        return y, noise
    y = y.copy()
    y[pos] = U_IMPULSE[dtype]
    return y, noise


@functools.lru_cache(maxsize=None)
def u_oracle(dtype, pos=None):
    """``(out, units)`` of the float64 oracle on ``u_recording(dtype, pos)``."""
    y, noise = u_recording(dtype, pos)
    kw = u_geometry(dtype)[2]
    return PB.oracle_units(y.astype(np.float64), PB.SR, y_noise=noise.astype(np.float64), **kw)


def u_named_band(dtype, where, k):
    """``(unit, band, margin dB)``: the band the impulse of cell (``where``, k) lifts furthest over its switch, in the unit
    whose head (``first``: unit 0) or tail (``last``: the last unit) holds it."""
    units = u_oracle(dtype, u_position(dtype, where, k))[1]
    ui = 0 if where == "first" else len(units) - 1
    m = PB.switch_margin(units[ui])
    f = int(np.argmax(m))
    return ui, f, float(m[f])
