"""TorchGate's backward on the CPU: the float64 adjoint of tests/parity_budget.py against torch autograd, the inputs of
the backward matrix (``B_CELLS``: one cell per backward route, for a GPU test to run), and planted defects.

The defects are planted in ``adjoint_f64``'s own stages (no kernel involved), on the ``fast-T65`` cell's first row and on
two grad_out fields: A, ``grad_field`` as the matrix holds it, and B, the same without its impulses (the quiet half
and the row's end are then quiet throughout).  What the suite's older bar, ``max|gx - ref| / max|ref| < 1e-4``, makes of
them, as measured here (error / peak; the local check flags every one of them on both fields):

====================================================  ===============  ===============
defect                                                field A          field B
====================================================  ===============  ===============
(a) last frame's contribution dropped                 3.8e-1 caught    5.0e-4 caught
(b) envelope shifted by one hop                       1.5e-1 caught    9.1e-2 caught
(c) tail [Lq, L) zeroed                               3.1e-2 caught    5.1e-5 MISSED
(d) g_y over the interior envelope at the two ends    1.5e-1 caught    9.1e-2 caught
(e) a quiet-part mask column taken from its neighbour 4.1e-5 MISSED    3.8e-5 MISSED
====================================================  ===============  ===============

(the figures are printed by the tests; `test_what_the_old_bar_misses` asserts the MISSED entries)"""
import numpy as np
import pytest
import torch

from tests import parity_budget as PB

TOL = 1e-4
SHARE = 0.05          # of a row's decisions: at least this share passed and this share gated
CELL = [c["name"] for c in PB.B_CELLS].index("fast-T65")
IDS = [PB.b_cell_id(c) for c in PB.B_CELLS]


def _autograd(x, M, gy, cfg):
    """CPU float64 autograd through torch.stft -> x M -> torch.istft."""
    w = torch.from_numpy(np.asarray(cfg["window"], dtype=np.float64))
    x2 = torch.from_numpy(np.asarray(x, dtype=np.float64))[None].requires_grad_()
    X = torch.stft(x2, cfg["n_fft"], cfg["H"], cfg["W"], window=w, center=True, pad_mode="constant", return_complex=True)
    y = torch.istft(X * torch.from_numpy(M)[None], cfg["n_fft"], cfg["H"], cfg["W"], window=w, center=True)
    assert y.shape[1] == len(gy)
    y.backward(torch.from_numpy(np.asarray(gy, dtype=np.float64))[None])
    return x2.grad[0].numpy()


@pytest.mark.parametrize("i", range(len(PB.B_CELLS)), ids=IDS)
def test_reference_is_torch_autograd_and_inputs_hold_their_conditions(i):
    """Every row of every cell, both grad_out fields, with the oracle's mask of the row."""
    case, units = PB.b_case(i), PB.b_oracle(i)
    cfg, H = case["cfg"], case["H"]
    long_rows = 0
    for b, n in enumerate(case["lens"]):
        u = units[b]
        M = u["mask"]
        p, T, Lq = PB.adjoint_geometry(cfg, n)
        assert M.shape == (cfg["n_fft"] // 2 + 1, T) and len(u["want"]) == Lq
        # the mask has structure: decisions of both kinds, and a final mask that is no constant
        passed = float(np.mean(np.asarray(u["raw"], dtype=np.float64) > 0.5))
        assert passed >= SHARE and 1.0 - passed >= SHARE, (b, passed)
        assert M.max() - M.min() >= 0.2
        for k, gy in enumerate((case["gy"][0][b], case["gy"][1][b])):
            want = PB.adjoint_f64(gy, M, cfg, n)
            assert want.shape == (n,) and np.isfinite(want).all()
            ref = _autograd(case["x"][b, :n], M, gy, cfg)
            err = PB.local_error(want, ref, H)
            ok = PB.F64_REL * np.maximum(PB._blocks(ref, H), 1e-3 * np.max(np.abs(ref)))
            assert np.all(err <= ok), (b, k, float(np.max(err / ok)))
            if n > Lq:
                assert np.max(np.abs(want[Lq:])) > 1e-4 * np.max(np.abs(want)), "the tail [Lq, L) gets no gradient"
            if k == 0 and T >= 16:
                # a row of 9 frames has no block further than two hops from an impulse: no quiet block to speak of
                blk = PB._blocks(want, H)
                live = blk[blk > 0]
                assert 20 * np.log10(live.max() / live.min()) >= 40.0
                long_rows += 1
    assert long_rows or case["cell"]["name"] == "row-T9"


@pytest.mark.parametrize("i", range(len(PB.B_CELLS)), ids=IDS)
def test_dot_product_identity(i):
    """<gy, J v> == <J^T gy, v> with J the oracle's own fixed-mask forward (``regate``), random v.  The two sums are
    compared to 1e-12 of the larger of them, or of ||gy|| ||J v|| where the inner product nearly cancels: each sum
    carries rounding errors of that size whatever its own value, so 1e-12 of a cancelled sum is no bound a correct
    adjoint can be held to."""
    case, units = PB.b_case(i), PB.b_oracle(i)
    rng = np.random.default_rng(i)
    for b, n in enumerate(case["lens"]):
        u = units[b]
        v = rng.standard_normal(n)
        X = PB.O.stft_torch(v[None], case["cfg"]["n_fft"], case["W"], case["H"], case["cfg"]["window"])[0]
        Jv = PB.regate(dict(u, Z=X), mask=u["mask"])
        gy = case["gy"][0][b].astype(np.float64)
        lhs, rhs = float(np.dot(gy, Jv)), float(np.dot(PB.adjoint_f64(gy, u["mask"], case["cfg"], n), v))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), float(np.linalg.norm(gy) * np.linalg.norm(Jv)))


# ---- planted defects --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """{field: (unit, {defect: gradient})} on row 0 of the fast-T65 cell."""
    case, units = PB.b_case(CELL), PB.b_oracle(CELL)
    cfg, H, n = case["cfg"], case["H"], case["lens"][0]
    M = units[0]["mask"]
    p, T, Lq = PB.adjoint_geometry(cfg, n)
    assert n > Lq
    out = {}
    for name, gy in (("A", case["gy"][0][0]), ("B", PB.grad_field(Lq, H, 1, impulses=False))):
        u = PB.adjoint_unit(gy, M, cfg, n)
        env = PB.adjoint_envelope(cfg, n)
        fr = PB.adjoint_frames_f64(gy, M, cfg, n)
        d = {}
        fa = fr.copy()
        fa[T - 1] = 0.0
        d["a"] = PB.adjoint_scatter(fa, cfg, n)
        d["b"] = PB.adjoint_scatter(PB.adjoint_frames_f64(gy, M, cfg, n, env=np.concatenate([env[H:], env[-H:]])), cfg, n)
        d["c"] = u["want"].copy()
        d["c"][Lq:] = 0.0
        d["d"] = PB.adjoint_scatter(PB.adjoint_frames_f64(gy, M, cfg, n, env=np.full(Lq, env[Lq // 2])), cfg, n)
        # in the quiet half of grad_out, clear of its impulses (3/4 Lq, the end), two frames behind x's loud stretch
        # there (B_LOUD: it ends at 0.78): the smoothed mask falls off from column to column
        t = int(0.82 * T)
        assert np.abs(gy[(t - 2) * H:(t + 3) * H]).max() < 0.01
        Me = M.copy()
        Me[:, t] = M[:, t + 1]
        assert np.max(np.abs(Me - M)) > 0.01
        d["e"] = PB.adjoint_f64(gy, Me, cfg, n)
        wf = PB.O._centered_window(cfg["n_fft"], cfg["W"], cfg["window"]).astype(np.float32)
        d["f"] = PB.emulate_adjoint_f32(gy, M, cfg, n, window=np.nextafter(wf, np.float32(2.0)))
        out[name] = (u, d)
    return out


@pytest.mark.parametrize("field", ["A", "B"])
def test_planted_defects_are_flagged(planted, field):
    u, d = planted[field]
    assert not len(PB.local_check(u["want"], u, bud=u["bud"])[0]) and not len(PB.local_check(u["emu"], u, bud=u["bud"])[0])
    for k in "abcde":
        bad, ratio = PB.local_check(d[k], u, bud=u["bud"])
        old = np.max(np.abs(d[k] - u["want"])) / np.max(np.abs(u["want"]))
        print("field %s defect (%s): %d blocks over their bound, largest error / budget %.3g; old bar %.2e" % (
            field, k, len(bad), ratio, old))
        assert len(bad) > 0, k
    bad, ratio = PB.local_check(d["f"], u, bud=u["bud"])
    print("field %s control (f): largest error / budget %.3g" % (field, ratio))
    assert len(bad) == 0 and ratio < PB.FACTOR


def test_adjoint_check_rows_on_a_padded_batch():
    """The batch helper a GPU test hands its gradient to: rows of their own lengths in the (B, T, FS) mask layout the
    engine saves; the emulation passes, the same with one row's tail zeroed is named."""
    i = [c["name"] for c in PB.B_CELLS].index("rows-256")
    case, units = PB.b_case(i), PB.b_oracle(i)
    cfg, lens = case["cfg"], case["lens"]
    F, T = units[0]["mask"].shape
    mask = np.zeros((len(lens), T, F + 7), dtype=np.float32)
    gx = np.zeros(case["x"].shape)
    for b, n in enumerate(lens):
        M = units[b]["mask"].astype(np.float32)
        mask[b, :M.shape[1], :F] = M.T
        gx[b, :n] = PB.emulate_adjoint_f32(case["gy"][0][b], M, cfg, n)
    assert PB.adjoint_check_rows("rows-256", gx, case["gy"][0], mask, cfg, lens) < PB.FACTOR
    gx[4, PB.adjoint_geometry(cfg, lens[4])[2]:] = 0.0
    with pytest.raises(AssertionError, match="row 4"):
        PB.adjoint_check_rows("rows-256", gx, case["gy"][0], mask, cfg, lens)


def test_what_the_old_bar_misses(planted):
    """See the table in the module's docstring."""
    old = {(f, k): np.max(np.abs(d[k] - u["want"])) / np.max(np.abs(u["want"])) for f, (u, d) in planted.items() for k in "abcde"}
    assert old[("A", "e")] < TOL and old[("B", "e")] < TOL and old[("B", "c")] < TOL
    for key in (("A", "a"), ("A", "b"), ("A", "c"), ("A", "d"), ("B", "b"), ("B", "d")):
        assert old[key] > TOL
