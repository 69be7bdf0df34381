"""The one-pass gates' host protocol across calls and batches: the handle's running ticket base, its epochs and the second
(REDO) counter.  Not the kernels: every output is compared with the three-kernel route of the same handle, which draws no
tickets.  One handle per frame length takes eighteen interleaved calls of different tile counts, floor-test modes and (at
n_fft = 1024) tile orders: with a single batch per call, with a workspace budget that splits every call into a couple of
batches, and with one unit per batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 1500
STAGE_ONEPASS = 16   # include/mi355gate_debug.h: SG_STAGE_ONEPASS, the first launch of every one-pass batch
STAGE_SMOOTH = 7     # SG_STAGE_SMOOTH: the three-kernel route's mask smoothing (the one-pass gates smooth in the kernel)
UNITS = 6            # units of every call: 2 channels x 3 chunks


def _recordings():
    """Two channels of 66000 samples each: benign noise, and "live" as in test_gpu_onepass._floor_inputs (digital silence next
    to a loud half under a very quiet noise clip: the -top_db floor lifts bands, the in-kernel floor test fires)."""
    rng = np.random.default_rng(4321)
    n = 66000
    benign = (0.05 * rng.standard_normal((2, n))).astype(np.float32)
    live = (0.05 * rng.standard_normal((2, n))).astype(np.float32)
    live[:, : n // 2] = 0.0
    live[:, n // 2:] *= 10.0
    noise = {"benign": (0.05 * rng.standard_normal((1, 30000))).astype(np.float32),
             "live": (1e-7 * rng.standard_normal((1, 30000))).astype(np.float32)}
    return {"benign": benign, "live": live}, noise


def _windows(y, cs):
    """The three chunks of each channel of y[:, :3 * cs] as padded windows [i cs - PAD, (i + 1) cs + PAD), zeros outside
    the recording (what sg_process_chunks cuts; here by hand, so that one handle sees another chunk size)."""
    ext = np.zeros((y.shape[0], 3 * cs + 2 * PAD), dtype=y.dtype)
    ext[:, PAD:PAD + 3 * cs] = y[:, :3 * cs]
    return np.stack([ext[c, i * cs:(i + 1) * cs + 2 * PAD] for c in range(y.shape[0]) for i in range(3)])


@pytest.fixture(scope="module")
def jobs():
    """Four gate calls of 6 units each (2 channels x 3 chunks).  Every one-pass tile is 4096 samples at all four frame
    lengths: the 10000-sample chunks give 3-4 tiles per unit, the 22000-sample ones 7, so the same exchange words and
    tickets mean different tiles from call to call."""
    recs, noise = _recordings()
    out = []
    for kind in ("benign", "live"):
        y = recs[kind]
        # chunks of the handle's own size through sg_process_chunks (the padding is staged by no tile of the unit) ...
        out.append((kind, "chunks", torch.from_numpy(np.ascontiguousarray(y[:, 20000:50000])).cuda()))
        # ... and chunks of 22000 samples as padded windows through sg_filter_padded
        out.append((kind, "padded", torch.from_numpy(_windows(y[:, 0:66000], 22000)).cuda()))
    return out, {k: torch.from_numpy(v).cuda() for k, v in noise.items()}


def _run(gate, job):
    _, how, x = job
    return gate.process_chunks(x, chunked=True) if how == "chunks" else gate.filter_padded(x)


def _last_batch_units(gate):
    import ctypes
    dims = (ctypes.c_int64 * 3)()
    gate._check(gate.lib.sg_debug_dims(gate._h, dims))
    return int(dims[0])


# (job, SG_OPT_FLOOR_TEST, SG_OPT_TILE_ORDER at n_fft = 1024).  Jobs 0 / 1: benign with 3-4 / 7 tiles per unit, 2 / 3: live.
# The forced in-kernel floor test (2) meets both live jobs under every tile order -- six calls whose REDO launch draws tickets
# from the second counter -- and benign jobs in between, whose REDO launch leaves that counter alone; the a-priori (1) and the
# predicted (0) test take turns around them.  Every job follows every other one.
PLAN = [(0, 0, 0), (2, 2, 0), (1, 1, 0), (3, 2, 0), (3, 0, 2), (0, 2, 2), (2, 2, 2), (2, 1, 2), (3, 2, 2), (1, 0, 1),
        (2, 2, 1), (0, 1, 1), (3, 2, 1), (1, 2, 0), (3, 1, 0), (2, 0, 2), (1, 2, 1), (0, 0, 0)]


@pytest.mark.parametrize("budget", [0, 400 << 10, 1], ids=["one_batch", "several_batches", "one_unit_per_batch"])
@pytest.mark.parametrize("n_fft,nf,nt", [(256, 1, 37), (512, 2, 18), (1024, 5, 9), (2048, 10, 4)])
def test_onepass_call_sequence_equals_three_kernel_route(jobs, n_fft, nf, nt, budget):
    from noisereduce_amd import _ffi
    jobs, noise = jobs
    gate = _ffi.Gate("cuda", variant=_ffi.SG_VARIANT_S, stationary=True, n_fft=n_fft, win_length=n_fft,
                     hop_length=n_fft // 4, n_grad_freq=nf, n_grad_time=nt, smooth_mask=True, chunk_size=10000,
                     padding=PAD, n_std_thresh=1.5, top_db=80.0, ddof=0, max_workspace_bytes=budget)
    onepass = gate.lib.sg_stage_name(STAGE_ONEPASS).decode()
    smooth = gate.lib.sg_stage_name(STAGE_SMOOTH).decode()
    try:
        thr = {}
        for kind, clip in noise.items():
            gate.noise_stats(clip)
            thr[kind] = gate.get_noise_threshold()
        # the three-kernel route (SG_OPT_FORCE_SPLIT): no tickets, no exchange buffer
        refs = []
        with gate.with_options([(_ffi.SG_OPT_FORCE_SPLIT, 1)]):
            for job in jobs:
                gate.set_noise_threshold(thr[job[0]])
                refs.append(_run(gate, job).cpu().numpy())
        gate.check_errors()
        assert all(np.isfinite(r).all() for r in refs)

        gate.profile_enable(True)
        try:
            # batches of each job on the one-pass route, one call alone: the first launches booked, checked against the units of
            # the last batch that the handle reports (6 units in batches of ub: ceil(6 / ub) batches, the last one with the rest)
            per_job = []
            gate.profile_read()
            for j, job in enumerate(jobs):
                gate.set_noise_threshold(thr[job[0]])
                assert np.array_equal(_run(gate, job).cpu().numpy(), refs[j]), job[:2]
                b, last = gate.profile_read()[onepass][1], _last_batch_units(gate)
                if budget == 0:
                    assert (b, last) == (1, UNITS)
                elif budget == 1:
                    assert (b, last) == (UNITS, 1)
                else:
                    ub = (UNITS - last) // (b - 1) if b > 1 else 0
                    assert b >= 2 and ub >= last and ub * (b - 1) + last == UNITS and -(-UNITS // ub) == b, (b, last)
                per_job.append(b)

            before = gate.debug_counter(1) + gate.debug_counter(2)
            outs = []
            for it, (j, floor_test, tile_order) in enumerate(PLAN):
                kind = jobs[j][0]
                gate.set_option(_ffi.SG_OPT_FLOOR_TEST, floor_test)
                if n_fft == 1024:
                    gate.set_option(_ffi.SG_OPT_TILE_ORDER, tile_order)
                if it % 2:   # (the threshold's compare constants from the statistics' last kernel, or from k_prep_thresh_lazy)
                    gate.noise_stats(noise[kind])
                else:
                    gate.set_noise_threshold(thr[kind])
                if floor_test != 2:
                    outs.append(_run(gate, jobs[j]))   # no synchronisation after these calls: the next one queues up behind
                    continue
                # in-kernel floor test: sg_debug_counter 3 (it synchronises) is the epoch of the last launch in which a unit's
                # test fired -- it moves with a live recording, whose REDO launch then has units to gate, and only then
                stamp = gate.debug_counter(3)
                outs.append(_run(gate, jobs[j]))
                moved = gate.debug_counter(3) - stamp
                assert (moved > 0) if kind == "live" else (moved == 0), (it, jobs[j][:2], moved)
            gate.check_errors()
            launches = gate.profile_read()
        finally:
            gate.profile_enable(False)
            gate.set_option(_ffi.SG_OPT_FLOOR_TEST, 0)
            gate.set_option(_ffi.SG_OPT_TILE_ORDER, 0)
        for it, (o, (j, _, _)) in enumerate(zip(outs, PLAN)):
            assert np.array_equal(o.cpu().numpy(), refs[j]), (it, jobs[j][:2])
        gate.check_errors()
        # every batch went the one-pass route (no launch of the three-kernel route's smoothing stage), one first launch per
        # batch, and each batch was counted once as lazy or a priori
        assert smooth not in launches
        assert launches[onepass][1] == sum(per_job[j] for j, _, _ in PLAN)
        assert gate.debug_counter(1) + gate.debug_counter(2) - before == launches[onepass][1]
    finally:
        gate.close()
