"""TorchGate's backward kernels against the float64 adjoint of tests/parity_budget.py per hop block, on the backward
matrix ``B_CELLS``: one cell per route of sg_process_batch_backward / sg_process_rows_backward and per transform family
behind stage_apply_ola.  tests/test_backward_parity_host.py ties that reference to CPU float64 autograd and holds the
conditions on the inputs that keep these checks from being empty.

Per cell: ``tg(x[, lengths=]).backward(gy)`` through autograd, twice -- ``grad_field`` (a loud and a 60 dB quieter half,
impulses on both sides of the first hop seam, at the last hop, the last sample and inside the quiet half), then the two
end impulses alone.  The route is read from the handle (``Gate.backward_route``, sg_debug_backward_route: host
bookkeeping of the last backward call) and the forced options from ``Gate.get_option`` inside the call; the rows cells
run as one sub-batch.  Every row of both gradients goes through ``PB.adjoint_check_rows``: no hop block of ``[0, L)``
over ``FACTOR x`` the float32 emulation's error + 4 eps32 of the local peak, the tail ``[Lq, L)`` included.

The mask the reference is given is the float32 mask the engine saved for that very forward (``y.grad_fn.saved_tensors``).
Which layout each forward route saves, from the code (csrc/api.hip sg_process_batch, csrc/rows.hip):

=====================================================  ==========================================  =============
forward route (what saves the mask)                    cells                                       layout
=====================================================  ==========================================  =============
k_row_gate (1024, stationary, enough rows)             --  (B = 3 stays under its row minimum)     natural
bit-mask path: K16 in lane order, k_k16_to_mask_perm   row-*, fast-T65, fast-norowgate             natural
  writes the saved copy
stage_smooth's float field h->M, copied                fast-ns, reg-*, lds-*, mixed-*, czt-*       natural
rw_process (rows.hip)                                  rows-*                                      natural
=====================================================  ==========================================  =============

The fused apply kernel keeps its OWN mask (uint16 counts) in lane order, but what is saved for the backward is a
natural-order float field on every route, and every backward kernel reads natural order (fastpath.hpp ApplyArgs::Mf).
So no cell needs a second forward under SG_OPT_FORCE_NOFAST to get its mask.  That the saved field really is in natural
order is asserted, not assumed: stationary cells hold it to the oracle's final mask within ``mask_bound`` (``mask_diff``;
the integer-tap bound where the smoothing is integer sums -- n_fft = 1024 without FORCE_NOFAST, and rows.hip -- else the
float-tap bound), which also pins the reference's input to the oracle; the non-stationary cells (fast-ns: the float
field of the same call on the default route; rows-1024-ns) hold it to the float32 emulation's mask by ``_field_rule``.

float64 cells: the kernels compute the adjoint in float32 whatever the container (k_env_scale writes float), so a
float64 gradient is held to the same float32 budget -- asserted only not to be worse than it.

The k_row_backward / k_apply_fast pair (row-T64, fast-norowgate) runs the same input; each is checked against the
reference on its own, there is no third bar between them.  The four-step sizes (n_fft = 16384) are left out: one cell
costs more than the rest of the matrix, and their backward is the stage_apply_ola call of 4096 with another transform
behind it, which the forward matrix holds.

The largest local_error / budget per route goes to the file named by BACKWARD_PARITY_OUT, if set
(profiles/backward_parity.json is the place for that file from an MI355X run; none is committed yet)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_budget as PB

pytestmark = pytest.mark.gpu

_RATIOS = {}
_IDS = [PB.b_cell_id(c) for c in PB.B_CELLS]
_ROUTE = {"row": 1, "fast": 2, "reg": 3, "ola": 4, "rows": 5}       # SG_BWD_* (include/mi355gate_debug.h)


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("BACKWARD_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


def _route_key(cell):
    fam = cell["name"].split("-")[0]
    key = cell["route"] if fam in ("row", "fast", "reg", "rows") else "%s/%s" % (cell["route"], fam)
    return key + ("/nonstationary" if cell.get("nonstationary") else "") + ("/float64" if cell.get("dtype") == "float64" else "")


@contextlib.contextmanager
def _handle_env(pairs):
    """Environment the engine reads when a handle is created; handles are cached, so the cache is emptied around it."""
    from noisereduce_amd import _ffi
    old = {k: os.environ.get(k) for k, _ in pairs}
    if pairs:
        _ffi.clear_gate_cache()
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if pairs:
            _ffi.clear_gate_cache()


def _run(case, gys, env=()):
    """forward once, one backward per grad_out, on a handle created under ``env``.  Returns the saved mask (B, T, FS),
    the gradient per grad_out, the route of every backward and the sub-batches of the last one (rows cells)."""
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    cell = case["cell"]
    tdt = torch.float64 if case["dtype"] == "float64" else torch.float32
    with _handle_env(env):
        tg = TorchGate(sr=PB.T_SR, **case["kw"]).cuda()
        x = torch.from_numpy(case["x"]).to(tdt).cuda().requires_grad_()
        gate = tg._gate_for(x.device)
        opts = [(getattr(_ffi, "SG_OPT_" + k), v) for k, v in cell.get("opts", ())]
        grads, routes = [], []
        with gate.with_options(opts):
            for o, v in opts:
                assert gate.get_option(o) == v
            y = tg(x) if case["lengths"] is None else tg(x, lengths=case["lengths"])
            assert y.dtype == tdt and y.requires_grad
            mask = y.grad_fn.saved_tensors[0].detach().clone()
            for k, gy in enumerate(gys):
                assert tuple(gy.shape) == tuple(y.shape), (gy.shape, y.shape)
                x.grad = None
                y.backward(torch.from_numpy(gy).to(tdt).cuda(), retain_graph=k + 1 < len(gys))
                routes.append(gate.backward_route())
                assert x.grad.dtype == tdt and tuple(x.grad.shape) == tuple(x.shape)
                grads.append(x.grad.detach().cpu().numpy())
        batches = gate.rows_batches() if case["lengths"] is not None else None
        del y, tg, gate
    return mask.cpu().numpy(), grads, routes, batches


def _grad_outs(case, Lout, fill):
    """(B, Lout) per grad_out of the cell: row b's own (Lq_b,) field, ``fill`` beyond it (rows cells)."""
    outs = []
    for per_row in case["gy"]:
        g = np.full((len(case["lens"]), Lout), fill, dtype=np.float32)
        for b, gy in enumerate(per_row):
            g[b, :len(gy)] = gy
        outs.append(g)
    return outs


@pytest.mark.parametrize("i", range(len(PB.B_CELLS)), ids=_IDS)
def test_backward_cell(i):
    case, units = PB.b_case(i), PB.b_oracle(i)
    cell, cfg, lens = case["cell"], case["cfg"], case["lens"]
    tag = PB.b_cell_id(cell)
    F = cfg["n_fft"] // 2 + 1
    Lout = PB.adjoint_geometry(cfg, case["L"])[2]
    rows = case["lengths"] is not None
    gys = _grad_outs(case, Lout, 0.0)
    mask, grads, routes, batches = _run(case, gys + (_grad_outs(case, Lout, np.nan)[:1] if rows else []), cell.get("env", ()))
    assert routes == [_ROUTE[cell["route"]]] * len(routes), "%s: backward routes %s, not %r" % (tag, routes, cell["route"])
    if cell.get("env"):
        # another transform behind the same stage_apply_ola call: not the default handle's gradient bit for bit
        _, other, r2, _ = _run(case, gys[:1])
        assert r2 == routes[:1] and not np.array_equal(other[0], grads[0]), tag
    if rows:
        assert batches == 1
        # a NaN in grad_out beyond a row's own output changes nothing
        assert np.array_equal(grads[2], grads[0]), "%s: grad_out beyond a row's own output reaches the gradient" % tag
    # ---- the mask the reference is given ----
    integer_taps = rows or (cfg["n_fft"] == 1024 and "FORCE_NOFAST" not in dict(cell.get("opts", ())))
    worst_field = 0.0
    for b, u in enumerate(units):
        T = u["mask"].shape[1]
        M = mask[b, :T, :F].T
        assert np.all(mask[b, T:, :F] == 0), "%s row %d: mask rows beyond the row's own frames" % (tag, b)
        if u["cfg"]["stationary"]:
            bound = PB.mask_bound(u["cfg"], integer_taps=integer_taps)
            cells, w = PB.mask_diff(M, u, bound=bound)
            assert len(cells) == 0, "%s row %d: saved mask off the oracle's by up to %.3g (bound %.3g) at %d cells, first " \
                                    "(band, frame) %s" % (tag, b, w, bound, len(cells), cells[:6].tolist())
        else:
            worst_field = max(worst_field, PB._field_rule(M, u["mask"], PB.emulate_stages_f32(u)[2],
                                                          "%s row %d saved mask" % (tag, b)))
    if cell.get("nonstationary"):
        print("%s: largest saved-mask error / the emulation's %.3f" % (tag, worst_field))
    # ---- the gradient ----
    worst = 0.0
    for k, name in enumerate(("field", "ends")):
        gx = grads[k]
        for b, n in enumerate(lens):
            assert np.all(gx[b, n:] == 0), "%s row %d: gradient at or beyond the row's length" % (tag, b)
        r = PB.adjoint_check_rows("%s %s" % (tag, name), gx, case["gy"][k], mask, cfg, lens)
        print("%s %s: largest local_error / budget %.3f" % (tag, name, r))
        worst = max(worst, r)
    key = _route_key(cell)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), worst)
