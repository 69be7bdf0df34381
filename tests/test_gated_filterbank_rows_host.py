"""``TorchGate.gated_filterbank(x, fb, lengths=...)`` on the native route, without a GPU: the surface (header, exports,
bindings, the route's row), that the numpy model of tests/gated_filterbank_rows_cases.py passes its own checks on every
cell, that every frame of every cell is held (a non-zero budget), and that planted defects are flagged in exactly the
rows and frames they touch.  tests/test_gpu_gated_filterbank_rows.py applies the same checks to the kernels."""
import inspect
import os

import numpy as np
import pytest

from tests import gated_filterbank_cases as K
from tests import gated_filterbank_rows_cases as FR
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the surface ----------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_agree():
    from noisereduce_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    for name, nargs in (("sg_gate_features_rows", 18), ("sg_gate_features_rows_backward", 15)):
        assert "SG_API int %s(" % name in hdr
        assert name in _ffi.exported_symbols() and len(_ffi._PROTOTYPES[name][1]) == nargs
    assert list(inspect.signature(_ffi.Gate.gate_features_rows).parameters) == [
        "self", "x", "lengths", "xn", "xn_lengths", "power", "log", "eps", "save_mask"]
    assert list(inspect.signature(_ffi.Gate.gate_features_rows_backward).parameters) == [
        "self", "x", "grad", "mask", "lengths", "power", "log", "eps"]
    p = inspect.signature(_ffi.Gate.gate_features_rows).parameters
    assert (p["xn"].default, p["xn_lengths"].default, p["power"].default, p["log"].default, p["eps"].default,
            p["save_mask"].default) == (None, None, 2, False, 1e-6, False)
    p = inspect.signature(_ffi.Gate.gate_features_rows_backward).parameters
    assert (p["power"].default, p["log"].default, p["eps"].default) == (2, False, 1e-6)


def test_the_route_is_a_row_of_the_table():
    from noisereduce_amd.torchgate import torchgate as TG
    assert tuple(TG._ROUTES["features_rows"]) == ("gate_features_rows", "gate_features_rows_backward", True, True, True)
    assert callable(getattr(TG.TorchGate, "_filterbank_composed", None))


def test_the_feature_kernels_do_not_change_the_code_of_the_other_rows_kernels():
    """They are a translation unit of their own: rows.hip defines none of them (tests/test_isa_rows_audit.py audits
    rows.hip, tests/test_isa_rows_feat_audit.py the new file)."""
    csrc = os.path.join(ROOT, "noisereduce_amd", "csrc")
    assert "k_rw_feat" not in open(os.path.join(csrc, "rows.hip")).read()
    src = open(os.path.join(csrc, "rows_feat.hip")).read()
    assert "void k_rw_feat(" in src and "void k_rw_feat_bwd(" in src and "atomic" not in src


def test_banks():
    for name, bname in FR.VARIATION + [(c["name"], "mel40") for c in FR.CELLS]:
        c = R.cell(name)
        fb = FR.bank(bname, c["n_fft"])
        assert fb.shape[0] == c["n_fft"] // 2 + 1 and fb.dtype == np.float32 and np.isfinite(fb).all() and fb.any()
    assert FR.bank("mel80", 512).shape[1] > 64 and FR.bank("one", 512).shape[1] == 1
    assert FR.bank("mel1024", 256).shape[1] == FR.bank("mel1024", 4096).shape[1] == 1024
    assert not FR.bank("zero_last", 2048)[:, -1].any() and (FR.bank("neg", 512) < 0).any()
    assert len(FR.BWD_CELLS) == 7


# ---- 2. the model passes its own check; every frame is held -----------------------------------------------------------
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", FR.CELLS, ids=R.cell_id)
def test_the_model_passes_and_every_frame_has_a_budget(c, gate):
    us = R.units(c, gate, "float32")
    fb = FR.bank("mel40", c["n_fft"])
    for power in FR.POWERS:
        for i, u in enumerate(us):
            M32 = u["mask"].astype(np.float32)
            assert M32.min() > 0                                       # R.PROP = 0.5 keeps the mask off 0
            want, bud, allowed = K.feature_budget(u["Z"], M32, fb, power, u["emu_spec"])
            assert want.shape == (40, R.frames_of(c)[i]) and np.all(bud > 0) and np.all(allowed > 0), (c["name"], i)
        for log in (False, True):
            for dtype in R.DTYPES:
                feat, Mk = FR.model_forward(c, us, fb, power, log, dtype, gate=gate)
                assert feat.dtype == (np.float32 if dtype == "float32" else np.float64)
                bad = FR.forward_bad(c, us, feat, Mk, fb, power, log, dtype)
                assert all(v == ([], True) for v in bad.values()), (c["name"], gate, power, log, dtype, bad)


# ---- 3. planted defects -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.E_CELLS, ids=R.cell_id)
def test_planted_defects_are_flagged_where_they_are(c):
    us = R.units(c, "stat", "float32")
    fb = FR.bank("mel40", c["n_fft"])
    short = [i for i, n in enumerate(c["lens"]) if n < c["L"]]
    full = [i for i, n in enumerate(c["lens"]) if n == c["L"]]
    frames = R.frames_of(c)
    assert short and full

    # the features over the mask of the padded row: right given that mask, and the mask is off in every short row only
    feat, Mk = FR.model_forward(c, us, fb, 2, defect="stats_padded")
    assert all(v == ([], True) for v in FR.forward_bad(c, us, feat, Mk, fb, 2).values())
    for i, u in enumerate(us):
        cells, _ = PB.mask_diff(Mk[i, :, :frames[i]], u, bound=PB.mask_bound(u["cfg"], integer_taps=False))
        assert (len(cells) > 0) == (i in short), (c["name"], i, len(cells))

    # frame T_i - 1 transformed from the padding: that frame of every short row, nothing else
    xp = R.rows(c, "float32", pad=0.5).double().numpy()
    for power in FR.POWERS:
        feat, Mk = FR.model_forward(c, us, fb, power, defect="last_frame", x_pad=xp)
        bad = FR.forward_bad(c, us, feat, Mk, fb, power)
        for i in short:
            assert bad[i] == ([frames[i] - 1], True), (c["name"], power, i, bad[i])
        assert all(bad[i] == ([], True) for i in full)

    # dead frames holding ln(eps) where 0 is due, and the reverse: every row that has dead frames, no frame of its own
    for log in (False, True):
        feat, Mk = FR.model_forward(c, us, fb, 2, log, defect="dead_swapped")
        bad = FR.forward_bad(c, us, feat, Mk, fb, 2, log)
        assert all(bad[i] == ([], False) for i in short) and all(bad[i] == ([], True) for i in full), (log, bad)

    # the Nyquist bin left out, under a bank whose one filter weighs that bin alone: in every row, the frames whose
    # Nyquist bin holds more than the frame's allowance (a single bin of noise: most frames, not all), and no other
    ny = np.zeros((c["n_fft"] // 2 + 1, 1), dtype=np.float32)
    ny[-1, 0] = 1.0
    for power in FR.POWERS:
        feat, Mk = FR.model_forward(c, us, ny, power)
        assert all(v == ([], True) for v in FR.forward_bad(c, us, feat, Mk, ny, power).values())
        feat, Mk = FR.model_forward(c, us, ny, power, defect="no_nyquist")
        bad = FR.forward_bad(c, us, feat, Mk, ny, power)
        for i, u in enumerate(us):
            want, _, allowed = K.feature_budget(u["Z"], Mk[i, :, :frames[i]], ny, power, u["emu_spec"])
            assert bad[i] == (np.flatnonzero(np.abs(want[0]) > allowed).tolist(), True), (c["name"], power, i, bad[i])
            assert len(bad[i][0]) > frames[i] // 2, (c["name"], power, i, bad[i])


@pytest.mark.parametrize("name,nt_lanes", [("E-512-512-128", 64), ("E-2048-2048-512", 256)])
def test_a_dropped_last_filter_is_flagged_when_the_bank_is_wider_than_a_team(name, nt_lanes):
    c = R.cell(name)
    us = R.units(c, "stat", "float32")
    frames = R.frames_of(c)
    for bname in ("mel40", "mel80", "mel1024" if nt_lanes == 256 else "mel128"):
        fb = FR.bank(bname, c["n_fft"])
        wider = fb.shape[1] > nt_lanes
        for power in FR.POWERS:
            feat, Mk = FR.model_forward(c, us, fb, power, defect="drop_last_filter", nt_lanes=nt_lanes)
            bad = FR.forward_bad(c, us, feat, Mk, fb, power)
            # filter M - 1 carries every frame's noise above n_fft / 2 - a few bins: far above the frame's allowance
            want = [(list(range(frames[i])) if wider and fb[:, -1].any() else [], True) for i in range(len(us))]
            assert [bad[i] for i in range(len(us))] == want, (name, bname, power, bad)
