"""The feature steps of a stream bank without a GPU (StreamBank.set_filterbank / push_features / flush_features): the
surface, the argument checks (all before any device work), the conditions the float64 model of
tests/stream_features_model.py needs on the oracle alone, and the checks of tests/test_gpu_stream_features.py against
planted defects."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import parity_budget as PB
from tests import stream_features_model as FM
from tests import stream_spectrum_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface():
    from noisereduce_amd import stream
    B, G = stream.StreamBank, stream.StreamGate
    assert list(inspect.signature(B.set_filterbank).parameters) == ["self", "fb"]
    sig = inspect.signature(B.push_features)
    assert list(sig.parameters) == ["self", "blocks", "power", "log", "eps", "scale", "return_mask"]
    assert [sig.parameters[k].default for k in ("power", "log", "eps", "scale", "return_mask")] == [2.0, False, 1e-10, "scipy", False]
    sig = inspect.signature(B.flush_features)
    assert list(sig.parameters) == ["self", "slots", "blocks", "power", "log", "eps", "scale", "return_mask"]
    assert sig.parameters["blocks"].default is None and sig.parameters["eps"].default == 1e-10
    for name in ("set_filterbank", "push_features", "flush_features"):
        assert callable(getattr(G, name))
    assert "1e-6" in B.push_features.__doc__ and "not part of a stream's state" in B.push_features.__doc__


def test_header_prototypes_and_exports_agree_on_the_new_entry_points():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    lib = _ffi.load_library()
    for name, nargs in (("sg_stream_set_filterbank", 3), ("sg_stream_push_features", 16)):
        m = re.search(r"SG_API int %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_ffi._PROTOTYPES[name][1]), name
        assert name in _ffi.exported_symbols() and hasattr(lib, name)
    body = header[header.index("typedef struct sg_stream_feat_rec {"):header.index("} sg_stream_feat_rec;")]
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert fields == [f[0] for f in _ffi.SgStreamFeatRec._fields_] == ["feat_offset", "feat_stride", "mask_offset", "mask_stride"]
    assert ctypes.sizeof(_ffi.SgStreamFeatRec) == 32
    # nothing that was there moved
    assert ctypes.sizeof(_ffi.SgStreamRec) == 48 and ctypes.sizeof(_ffi.SgStreamSpecRec) == 24 and lib.sg_version() == 100
    assert _ffi.SG_STREAM_HEAD_VERSION == 1 and "#define SG_STREAM_HEAD_VERSION 1" in header


def test_arguments_are_checked_before_any_device_work():
    import torch
    from noisereduce_amd import stream
    from noisereduce_amd.torchgate import mel_filterbank
    thr = np.zeros(513)
    z = np.zeros(10, np.float32)
    nobank = stream.StreamBank(48000, 2, thresholds_db=thr, max_block=4800)
    with pytest.raises(ValueError, match="no filterbank set"):
        nobank.push_features({0: z})
    with pytest.raises(ValueError, match="no filterbank set"):
        nobank.flush_features([0])
    assert nobank._bank is None
    bank = stream.StreamBank(48000, 2, thresholds_db=thr, max_block=4800)
    fb = mel_filterbank(48000, 1024, 40)
    bad_fb = [np.zeros((512, 4), np.float32), np.zeros((513, 0), np.float32), np.zeros((513, 1025), np.float32),
              np.zeros(513, np.float32), np.full((513, 3), np.nan, np.float32), np.full((513, 3), np.inf),
              np.zeros((513, 3), np.complex64), torch.zeros(513, 3, requires_grad=True)]
    for i, b in enumerate(bad_fb):      # a refused bank before any is set ...
        with pytest.raises(ValueError):
            bank.set_filterbank(b)
        assert bank._fb is None and bank._bank is None, i
    bank.set_filterbank(fb)
    kept = bank._fb
    assert kept.shape == (513, 40) and kept.dtype == np.float32 and bank._fb_pending and bank._bank is None
    for i, b in enumerate(bad_fb):      # ... and after: the earlier one stays
        with pytest.raises(ValueError):
            bank.set_filterbank(b)
        assert bank._fb is kept, i
    bank.set_filterbank(-fb.double().numpy())      # negative entries, float64, numpy: fine
    assert bank._fb.dtype == np.float32 and np.array_equal(bank._fb, -fb.numpy())
    bad = [lambda: bank.push_features({0: z}, power=3),
           lambda: bank.push_features({0: z}, power=0.5),
           lambda: bank.push_features({0: z}, power=True),
           lambda: bank.push_features({0: z}, eps=float("nan")),
           lambda: bank.push_features({0: z}, scale="librosa"),
           lambda: bank.push_features({0: z}, scale=1.0),
           lambda: bank.flush_features([0], power=4),
           lambda: bank.flush_features([0], {0: np.zeros(2000, np.float32)}, eps=np.nan),
           lambda: bank.flush_features([0], {0: np.zeros(2000, np.float32)}, scale=None),
           # the block handling is push_spectrum's
           lambda: bank.push_features([(0, z), (0, z)]),
           lambda: bank.push_features([(1, z), (np.int64(1), z)], return_mask=True),
           lambda: bank.flush_features([0, 0]),
           lambda: bank.push_features({0: np.zeros(4801, np.float32)}),
           lambda: bank.push_features({0: z, 1: torch.zeros(10)}),
           lambda: bank.push_features({0: torch.zeros(10)}),
           lambda: bank.push_features({0: np.zeros(10, np.int16)}),
           lambda: bank.push_features({2: z}),
           lambda: bank.flush_features([0]),
           lambda: bank.flush_features([0], {0: np.zeros(1023, np.float32)}, log=True),
           lambda: bank.flush_features([5])]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert bank._bank is None, i
    g = stream.StreamGate(48000, thresholds_db=thr, max_block=4800)
    with pytest.raises(ValueError, match="no filterbank set"):
        g.push_features(z)
    g.set_filterbank(fb)
    for f in (lambda: g.push_features(z, power=7), lambda: g.flush_features(), lambda: g.flush_features(z, scale="x")):
        with pytest.raises(ValueError):
            f()
    assert g.bank._bank is None
    nobody = stream.StreamBank(48000, 1)
    nobody.set_filterbank(fb)
    with pytest.raises(ValueError):
        nobody.push_features({0: z})                                                   # no noise profile yet


def test_banks_reach_every_branch_of_the_filter_sum():
    from noisereduce_amd.torchgate.filterbank import check_filterbank, support_tables
    for n_fft in (256, 1024, 4096):
        F = n_fft // 2 + 1
        nt = 64 if n_fft <= 1024 else 256      # threads of a frame's team (tile_core.hpp: tile_nt of n_fft / 2)
        widths = set()
        for name in FM.BANKS:
            fb = check_filterbank(FM.bank(name, n_fft), F)
            kh, _ = support_tables(fb)
            widths.update((kh[:, 1] - kh[:, 0]).tolist())
            if name == "one":
                assert fb.shape[1] == 1 and (fb[kh[0, 0]:kh[0, 1], 0] == 0).any()
            if name == "wide300":
                assert fb.shape[1] > nt and kh[:, 1].max() == F
            if name == "dense_signed":
                assert (kh == (0, F)).all() and (fb < 0).any() and (fb > 0).any()
            if name == "zero_nyq":
                assert kh[1].tolist() == [0, 0] and kh[2].tolist() == [F - 1, F]
        assert {0, 1, 7, 8, 9, 16, 17} <= widths      # no bin, the 8-blocks of the sum and their tails


LOG_CASES = [c for c in FM.CASES if c["log"]]


@pytest.mark.parametrize("case", LOG_CASES, ids=[FM.case_id(c) for c in LOG_CASES])
def test_the_log_bound_is_finite_in_every_cell_of_the_gpu_cases(case):
    """On the oracle alone: E stays under half of lin + eps everywhere, for the float64 and the float32 result."""
    cell = case["cell"]
    units = PB.tile_oracle(cell)[0]
    fb = FM.bank(case["bank"], cell["n_fft"])
    assert (fb >= 0).all()      # (a signed bank has no log)
    for u in units:
        W = u["cfg"]["W"]
        r = FM.scale_ratio(case["scale"], W)
        Y = u["Z"] * u["mask"]
        assert not np.isnan(Y).any()
        E = FM.budget(Y, fb, case["power"], r, FM.frame_bounds(Y, u["Z"], r))
        lin = FM.linear(Y, fb, case["power"], r).astype(np.float64)
        worst = float(np.max(E / (lin + case["eps"])))
        print("%s: largest E / (lin + eps) = %.3g" % (FM.case_id(case), worst))
        assert worst < 0.5
        for dt in (np.float64, np.float32):
            assert np.isfinite(FM.tolerance(lin, E, True, case["eps"], dt)).all()


def _defect_setup():
    cell = next(c for c in PB.TILE_CELLS if c["path"] == "stream-S" and c["n_fft"] == 1024 and c["signal"] == "dc_nyquist")
    u = PB.tile_oracle(cell)[0][0]
    return u, u["cfg"]["W"]


@pytest.mark.parametrize("defect,bankname,power,scale,log", [
    ("hull_short_lo", "mel40", 2, "scipy", True), ("hull_short_hi", "mel40", 1, "scipy", False),
    ("hull_short_lo", "wide300", 1, "torch", True), ("hull_short_hi", "wide300", 2, "torch", False),
    ("nyquist_dropped", "zero_nyq", 2, "scipy", True), ("nyquist_dropped", "dense_signed", 1, "torch", False),
    ("column_plus_one", "mel40", 2, "scipy", True), ("column_plus_one", "dense_signed", 2, "scipy", False),
    ("scale_after_power", "mel40", 2, "torch", True), ("mask_float32", "mel40", 2, "scipy", True),
    ("mask_float32", "one", 1, "torch", False)])
def test_checks_see_a_planted_defect(defect, bankname, power, scale, log):
    """Each defect, planted in the model, is seen by both checks of the GPU test: the oracle bound (check 1) and, where the
    defect lies after Y, the summation-terms bound on the engine's own Y (check 2) -- which the sound result passes."""
    u, W = _defect_setup()
    fb = FM.bank(bankname, 1024)
    Z, mask = u["Z"], u["mask"]
    r = FM.scale_ratio(scale, W)
    args = (fb, power, scale, log, 1e-10, W)
    for dt in (np.float64, np.float32):
        good = FM.features(Z, mask, fb, power, r, log, 1e-10).astype(dt)
        broken = FM.features(Z, mask, fb, power, r, log, 1e-10, defect=defect).astype(dt)
        assert len(FM.check("sound", good, Z, mask, *args)) == 0
        if defect == "mask_float32" and dt == np.float32:
            continue      # (a float32 mask is 6e-8 per bin: under the float32 result's own rounding; the float64 result shows it)
        assert len(FM.check(defect, broken, Z, mask, *args)) > 0
        if defect != "mask_float32":      # (the twin bank's Y would carry the same mask)
            Y = Z * mask
            if scale == "scipy":
                assert len(FM.check("sound, own Y", good, Z, mask, *args, engine_Y=Y)) == 0
            assert len(FM.check(defect + ", own Y", broken, Z, mask, *args, engine_Y=Y)) > 0


def test_the_order_case_sees_a_descending_sum():
    """No rounding bound can tell one order of the same terms from another; partial sums that overflow can.  On the order
    case the ascending sum is +inf for filter 0 and finite for filter 1 on every inside frame, the descending one the
    other way round -- and the gate passes all three bins, so the engine meets exactly these powers."""
    oc = FM.order_case()
    y, n_fft, W, H, k0 = oc["y"], oc["n_fft"], oc["W"], oc["H"], oc["k0"]
    T = SM.frames_total(len(y), W, H)
    gate = SM.stationary_gate(np.zeros(n_fft // 2 + 1), n_fft, W, H, 1.0, 1, 1, False)
    Z, mask = gate(y, T)
    assert np.all(mask[k0 - 1:k0 + 2] == 1.0)
    p = FM.powers(Z * mask, 2, FM.scale_ratio("torch", W)).astype(np.float64)
    assert np.isfinite(p).all()
    asc, desc = FM.lin_sequential(p, oc["fb"]), FM.lin_sequential(p, oc["fb"], descending=True)
    bad, want, inside = FM.order_bad(asc, Z, mask, oc)
    assert inside.sum() >= 15 and len(bad) == 0
    assert np.all(np.isinf(asc[0, inside])) and np.all(np.isfinite(asc[1, inside]))
    assert np.all(np.isfinite(desc[0, inside])) and np.all(np.isinf(desc[1, inside]))
    bad, _, _ = FM.order_bad(desc, Z, mask, oc)
    assert len(bad) == 2 * inside.sum()      # every inside cell of both filters
