"""The layouts of tests/view_cases.py on CPU tensors -- what a comparison of an entry point on a view with the same call on
``view.clone()`` relies on, without a GPU:

* every layout holds the samples it was given, at the residues of 16 bytes it claims (from storage_offset(), stride() and
  the element size), inside at least 32 elements of poison on both sides, with poison in the gaps between its rows;
* the offsets per element size cover the residue classes they are there for;
* ``_ffi._rows`` copies the layouts whose rows are not contiguous or overlap (``inner2``, ``expand``, ``overlap``) and passes
  the others on untouched;
* the recordings of the floor's unit maximum, on the float64 oracle alone: the impulse lifts the named band and changes its
  decision bits, it sits in the scalar head (tail) that ``k_unit_absmax`` reads sample by sample at the view's offset, and
  without it no unit reaches the level at which any band lifts -- so a maximum that misses the impulse decides otherwise.
"""
import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import view_cases as V

DTYPES = ("float32", "float64", "int16")


def _samples(dtype, B, L, seed=0):
    rng = np.random.default_rng(7700 + seed)
    if dtype == "int16":
        return rng.integers(-20000, 20001, size=(B, L)).astype(np.int16)
    return rng.standard_normal((B, L)).astype(dtype)


def _layout_names(dtype):
    return ["off%d" % k for k in V.offsets(dtype)] + ["pitch1", "oddL", "inner2", "expand", "overlap"]


def _span(lay):
    """[first, last] element of the allocation that the view touches."""
    v = lay.view
    lo = v.storage_offset()
    hi = lo + sum((n - 1) * s for n, s in zip(v.shape, v.stride()))
    return lo, hi


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [96, 101, 250])
def test_layouts_hold_their_samples_where_they_claim(dtype, L):
    es = np.dtype(dtype).itemsize
    for name in _layout_names(dtype):
        a = _samples(dtype, 5, L)
        if name == "oddL":
            a = V.odd_rows(a)
        lay = V.make(name, a)
        v = lay.view
        assert v.dtype == V._TORCH[dtype] and tuple(v.shape) == a.shape, name
        assert np.array_equal(v.numpy(), lay.samples), name
        if name not in ("expand", "overlap"):
            assert np.array_equal(lay.samples, a), name
        else:
            assert np.array_equal(lay.samples[0], a[0]), name
        # residues: the view's, and what the layout is there for
        assert [V.residue(v, 0), V.residue(v, 1)] == list(lay.claims), (name, lay.claims)
        assert (V.MARGIN * es) % 16 == 0
        V.assert_claims(lay)                                 # (the same from data_ptr(): the allocation is aligned)
        before = V.raw_bytes(lay.store).clone()
        c = V.aligned_clone(v)
        assert c.is_contiguous() and c.data_ptr() % 16 == 0 and np.array_equal(c.numpy(), lay.samples), name
        assert torch.equal(V.raw_bytes(lay.store), before) and before.numel() == lay.store.numel() * es
        if name.startswith("off"):
            k = int(name[3:])
            assert all(V.residue(v, r) == (k * es) % 16 != 0 for r in range(5)), name
            assert (v.stride(0) * es) % 16 == 0
        if name == "pitch1":
            assert [V.residue(v, r) for r in range(5)] == [(r * es) % 16 for r in range(5)]
            assert V.residue(v, 0) == 0 and V.residue(v, 1) != 0
        if name == "oddL":
            assert v.is_contiguous() and v.shape[1] % 2 == 1 and V.residue(v, 1) != 0
        # margins and gaps
        lo, hi = _span(lay)
        n = lay.store.numel()
        assert lo >= V.MARGIN and n - 1 - hi >= V.MARGIN, (name, lo, n - 1 - hi)
        assert bool(V.is_poison(lay.store[:V.MARGIN]).all()) and bool(V.is_poison(lay.store[hi + 1:]).all()), name
        touched = torch.zeros(n, dtype=torch.bool)
        touched.as_strided(tuple(v.shape), v.stride(), v.storage_offset()).fill_(True)
        if name == "inner2":
            assert int((~touched[lo:hi + 1]).sum()) == 5 * L - 1         # every other element between the samples
        assert bool(V.is_poison(lay.store[~touched]).all()), "%s: an element outside the view holds no poison" % name
        if name in ("off1", "pitch1"):
            gap = lay.store[v.storage_offset() + L:v.storage_offset() + v.stride(0)]
            assert gap.numel() >= 1 and bool(V.is_poison(gap).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_off_and_the_offsets_per_element_size(dtype):
    es = np.dtype(dtype).itemsize
    ks = V.offsets(dtype)
    assert ks == {"float32": (1, 2, 3), "float64": (1,), "int16": (1, 2, 3, 5)}[dtype]
    for k in ks:
        a = _samples(dtype, 1, 203)[0]
        lay = V.make_flat(a, k)
        assert lay.view.dim() == 1 and np.array_equal(lay.view.numpy(), a)
        assert V.residue(lay.view) == (k * es) % 16 == lay.claims[0] != 0
        lo, hi = _span(lay)
        assert lo >= V.MARGIN and lay.store.numel() - 1 - hi >= V.MARGIN
        rest = torch.ones(lay.store.numel(), dtype=torch.bool)
        rest[lo:hi + 1] = False
        assert bool(V.is_poison(lay.store[rest]).all())
    if dtype == "int16":
        # the 8-byte loads of vec16 (4 samples): every class but 0; the 16-byte loads of k_unit_absmax (8 samples): heads of
        # 7, 6, 5 and 3 samples
        assert {k % 4 for k in ks} == {1, 2, 3} and sorted((-k) % 8 for k in ks) == [3, 5, 6, 7]
    if dtype == "float32":
        assert {k % 4 for k in ks} == {1, 2, 3}


def test_poison_is_what_the_kernels_cannot_mistake_for_a_sample():
    assert bool(torch.isnan(V.poison(8, torch.float32)).all()) and bool(torch.isnan(V.poison(8, torch.float64)).all())
    assert V.poison(6, torch.int16).tolist() == [32767, -32767] * 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_copies_what_the_library_cannot_read_and_nothing_else(dtype):
    from noisereduce_amd import _ffi           # importable without a device: the library is loaded by the first Gate
    a = _samples(dtype, 4, 120)
    for name in _layout_names(dtype):
        lay = V.make(name, V.odd_rows(a) if name == "oddL" else a)
        t, stride = _ffi._rows(lay.view)
        copied = t.data_ptr() != lay.view.data_ptr()
        assert copied == (name in V.COPY_LAYOUTS), name         # (by construction: last stride 2, row stride 0, row stride L // 2)
        assert np.array_equal(t.numpy(), lay.samples), name
        assert t.stride(1) == 1 and stride == t.stride(0) >= t.shape[1], name
        if not copied:
            assert t is lay.view and stride == lay.view.stride(0)
        else:
            # what the library is handed for a copied layout is what it is handed for view.clone(): same shape, strides,
            # row stride and samples, a contiguous 16-byte aligned allocation -- it cannot tell the two calls apart
            tc, sc = _ffi._rows(V.aligned_clone(lay.view))
            assert t.is_contiguous() and t.data_ptr() % 16 == 0 and (tuple(t.shape), t.stride(), stride) == (tuple(tc.shape), tc.stride(), sc)
            assert torch.equal(V.raw_bytes(t), V.raw_bytes(tc)), name
    # one row: its stride is never used, the row length goes in its place; a single expanded or strided row
    one = V.make("off1", a[:1])
    t, stride = _ffi._rows(one.view)
    assert t is one.view and stride == a.shape[1]
    t, stride = _ffi._rows(V.make("inner2", a[:1]).view)
    assert t.is_contiguous() and stride == a.shape[1]


# ---- _ffi._dense: the tensors the C ABI takes without strides ---------------------------------------------------------
def _raises_naming(name, fn):
    with pytest.raises(ValueError) as e:
        fn()
    assert str(e.value).startswith(name + " must be"), str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_accepts_what_the_library_reads_as_it_is_and_refuses_the_rest(dtype):
    from noisereduce_amd import _ffi
    tdt = V._TORCH[dtype]
    flat = torch.from_numpy(_samples(dtype, 1, 240)[0])
    cube = flat.view(3, 5, 16)
    # dense, whatever the base address: the tensor itself comes back, nothing is copied
    for t in (flat, flat[7:], flat[:0], flat[3:4], cube, cube[1:], cube[:, :1].expand(3, 1, 16)[:1], flat[::2][:1],
              V.make_flat(flat, 3).view):
        assert _ffi._dense(t, "t") is t
    assert _ffi._dense(cube, "mask", dtype=tdt) is cube
    # not dense: every other element, a transpose, repeated rows, a narrowed last axis, rows at a pitch
    for t in (flat[::2], cube.transpose(1, 2), cube[:, :, :13], cube[:1].expand(3, 5, 16), cube[:, ::2], flat.view(15, 16).t(),
              flat.view(15, 16)[:, :8]):
        assert not t.is_contiguous()
        _raises_naming("mask", lambda: _ffi._dense(t, "mask"))
    other = torch.float64 if tdt != torch.float64 else torch.float32
    _raises_naming("mask", lambda: _ffi._dense(cube, "mask", dtype=other))
    _raises_naming("x", lambda: _ffi._dense(flat.numpy(), "x"))
    _raises_naming("x", lambda: _ffi._dense(None, "x"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_rows_is_the_rule_of_rows_for_an_output(dtype):
    """An output cannot be copied: what ``_rows`` passes on untouched is accepted, what it copies is refused."""
    from noisereduce_amd import _ffi
    a = _samples(dtype, 4, 120)
    for name in _layout_names(dtype):
        lay = V.make(name, V.odd_rows(a) if name == "oddL" else a)
        if name in V.COPY_LAYOUTS:
            _raises_naming("out", lambda: _ffi._dense(lay.view, "out", rows=True))
        else:
            assert _ffi._dense(lay.view, "out", rows=True) is lay.view
            assert _ffi._rows(lay.view)[0] is lay.view
    t = torch.from_numpy(a)
    # a column range of a wider buffer (the pipelined upload's out=), one row of any stride, one column
    for ok in (t[:, 10:50], t[1:2, ::1], t[:1].expand(1, 120), t[:, :1], t[:, ::2][:, :1], t[:0]):
        assert _ffi._dense(ok, "out", rows=True) is ok
    for bad in (t[0], t.view(2, 2, 120), t[:, ::2], t.t(), t[:1, ::3]):
        _raises_naming("out", lambda: _ffi._dense(bad, "out", rows=True))


def test_every_strideless_argument_of_the_wrappers_goes_through_dense():
    """The wrappers named below hand over data_ptr() alone; each checks the tensors it hands over (read from the source:
    the calls themselves need a device and are made by tests/test_gpu_views.py)."""
    import inspect
    from noisereduce_amd import _ffi
    want = {"process_batch_backward": ["mask"], "process_rows_backward": ["mask"], "gate_spectrum_backward": ["mask"],
            "gate_spectrum_rows_backward": ["mask"], "gate_features_backward": ["mask"],
            "gate_features_rows_backward": ["mask"], "process_clips": ["x", "out", "noise"],
            "stream_push": ["x", "out"], "stream_push_spectrum": ["x", "out", "spec", "mask"],
            "stream_push_features": ["x", "out", "feat", "mask"], "process_chunks": ["out"],
            "set_noise_threshold_tensor": ["t"]}
    for fn, names in want.items():
        src = inspect.getsource(getattr(_ffi.Gate, fn))
        for n in names:
            hit = ('_dense(%s, "%s"' % (n, n)) in src or ('("%s", %s)' % (n, n)) in src and "_dense(t, name)" in src or \
                (n == "mask" and "self._saved_mask(mask)" in src)
            assert hit, "%s hands %s to the library unchecked" % (fn, n)
        assert src.index("_dense(") < src.index("self.lib.") if "_dense(" in src else src.index("_saved_mask(") < src.index("self.lib.")
    assert '_dense(mask, "mask", dtype=torch.float32)' in inspect.getsource(_ffi.Gate._saved_mask)


# ---- the floor's unit maximum ------------------------------------------------------------------------------------------
U_CELLS = [(dt, where, k) for dt in ("float32", "int16") for where in ("first", "last") for k in V.U_OFFSETS[dt]]


@pytest.mark.parametrize("dtype, where, k", U_CELLS, ids=["%s-%s-k%d" % c for c in U_CELLS])
def test_only_the_impulse_can_switch_the_floor_on(dtype, where, k):
    cell, (n_fft, W, H, cs, pad, N), kw = V.u_geometry(dtype)
    per = V.U_PER16[dtype]
    pos = V.u_position(dtype, where, k)
    y, noise = V.u_recording(dtype, pos)
    rest, _ = V.u_recording(dtype)
    assert y.dtype == np.dtype(dtype) and np.array_equal(np.delete(y, pos), np.delete(rest, pos))
    # where the impulse sits: in the head of unit 0 (first 3 / 7 samples), or in the tail of the last units
    lay = V.make_flat(y, k)
    first_aligned = next(i for i in range(per + 1) if V.residue(lay.view[i:]) == 0)
    assert first_aligned == V.u_head_len(dtype, k) and 1 <= first_aligned <= per - 1
    if where == "first":
        assert 0 <= pos < first_aligned <= (3 if dtype == "float32" else 7)
    else:
        tail = (k + N) % per                 # samples behind the last 16-byte boundary of the row
        assert tail == k and pos == N - 1 and N - pos <= tail <= (3 if dtype == "float32" else 7)
    # the oracle: the impulse lifts the named band and changes its bits ...
    _, units = V.u_oracle(dtype, pos)
    _, plain = V.u_oracle(dtype)
    ui, f, margin = V.u_named_band(dtype, where, k)
    assert ui == (0 if where == "first" else len(units) - 1)
    assert margin > 1.0, "the named band is %.3f dB over its switch" % margin
    assert PB.switch_margin(plain[ui])[f] < -1.0
    assert np.all(units[ui]["raw"][f]), "a lifted band passes whole"
    changed = int(np.sum(units[ui]["raw"][f] != plain[ui]["raw"][f]))
    assert changed > 0, "removing the impulse leaves the bits of band %d alone" % f
    for u in units:
        assert PB.nearest_margin_db(u) > 1e-7
    # ... and nothing else can: the engine's a-priori test (csrc/fused.hpp: k_prep_thresh) is 20 log10(max|x| sum|w|
    # mag_scale) + 1e-6 - top_db > min thresh, with sum|w| mag_scale = 1 for a non-negative window.  max|x| of the rest,
    # 1 dB of slack added, stays under it for the smallest threshold of all bands -- the named one included
    top_db = V.u_top_db()                    # the engine's, and the one the oracle's margins are taken with
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(np.abs(units[ui]["Z"]) + O.EPS64)
    assert np.array_equal(db.max(axis=1) - top_db - units[ui]["thresh"], PB.switch_margin(units[ui]))
    level = 20.0 * np.log10(float(np.max(np.abs(rest.astype(np.float64)))))
    assert level + V.U_SLACK_DB - top_db < float(np.min(units[ui]["thresh"])) <= float(units[ui]["thresh"][f])
    assert all(float(PB.switch_margin(u).max()) < -V.U_SLACK_DB for u in plain)
    # the units the impulse does not reach lift nothing
    for j, u in enumerate(units):
        reach = (j == 0) if where == "first" else (j >= len(units) - 2)
        assert bool((PB.switch_margin(u) > 0).any()) == reach, j
