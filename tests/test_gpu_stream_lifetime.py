"""A stream bank gives back every device buffer it allocated (csrc/stream.hip: every device member of StBank is a DevBuf,
st_destroy is ``delete``; st_set_filterbank hands the old tables to a DevBuf that frees them).

Per kind of bank (fixed, adaptive, non-stationary, each plain and exact): COUNT banks of 2 slots at n_fft = 256, max_block 512
are created and destroyed.  Each takes one feature step of two full blocks -- at hop 16 that is 34 to 38 tiles against the 32
that the table buffer allocated up front holds, so the step grows ``tabs``; the growth path of the scratch ``ws`` is not
exercised, since ``ws`` is sized for max_block up front and no step can outgrow it -- and has its filterbank set twice, so
that the replaced tables are released as well as the last ones.  The device's free memory after is compared with before
(after a warm-up cycle); a figure that moves in the allocator's steps, so a leak of a few KB per bank would not show.

Measured on the MI355X with the library of the parent commit, which freed a hand-kept list of 15 pointers: 0 bytes of growth
for every kind (profiles/stream_plan.txt).  The bound is the parent's growth, so 0: this test is a guard, it never failed.

``python tests/test_gpu_stream_lifetime.py`` prints the figures without asserting (SG_LIB_PATH selects the library)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

COUNT = 200
PARENT_GROWTH_BYTES = 0   # measured with the library of the parent commit (profiles/stream_plan.txt)
KINDS = [(k, ex) for k in ("fixed", "adaptive", "nonstationary") for ex in (False, True)]


def _growth(kind, exact, count=COUNT):
    """Bytes by which the device's free memory shrank over `count` bank lifetimes of one kind."""
    import numpy as np
    import torch
    from noisereduce_amd import _ffi

    g = _ffi.Gate("cuda:0", variant=_ffi.SG_VARIANT_S, stationary=kind != "nonstationary", n_fft=256, win_length=256,
                  hop_length=16, n_grad_freq=2, n_grad_time=2, smooth_mask=True)
    code = {"fixed": _ffi.SG_STREAM_FIXED, "adaptive": _ffi.SG_STREAM_ADAPTIVE, "nonstationary": _ffi.SG_STREAM_NONSTATIONARY}[kind]
    desc = g.stream_desc(2, 1, 512, kind=code, lookahead_frames=3 if kind == "nonstationary" else 0, exact=exact)
    x = torch.zeros(1024, dtype=torch.float32, device="cuda:0")
    out = torch.zeros(1024, dtype=torch.float32, device="cuda:0")
    feat = torch.zeros(2 * 40 * 8, dtype=torch.float32, device="cuda:0")
    recs = [_ffi.SgStreamRec(slot=s, flush=0, n_samples=512, in_offset=512 * s, in_stride=512, out_offset=512 * s, out_stride=512)
            for s in (0, 1)]
    frecs = [_ffi.SgStreamFeatRec(feat_offset=40 * 8 * s, feat_stride=40 * 8, mask_offset=0, mask_stride=0) for s in (0, 1)]
    fbs = [np.ascontiguousarray(np.full((g.n_bins, m), 0.5, dtype=np.float32)) for m in (8, 5)]

    def life():
        b = g.stream_create_ex(desc)
        if kind == "fixed":
            g.stream_set_threshold(b, [0, 1], np.full(g.n_bins, -40.0))
        g.stream_set_filterbank(b, fbs[0])
        g.stream_push_features(b, x, out, feat, None, recs, frecs, 2, 1, 1e-6, 0.0)
        g.stream_set_filterbank(b, fbs[1])
        torch.cuda.synchronize()
        g.stream_destroy(b)

    life()   # warm-up: the runtime's own first-use allocations
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(count):
        life()
    torch.cuda.synchronize()
    grew = free0 - torch.cuda.mem_get_info(0)[0]
    g.close()
    return grew


@pytest.mark.parametrize("kind,exact", KINDS, ids=["%s%s" % (k, "-exact" if ex else "") for k, ex in KINDS])
def test_banks_leak_nothing(kind, exact):
    grew = _growth(kind, exact)
    print(f"[stream lifetime] {kind} exact={exact}: free memory shrank by {grew} bytes over {COUNT} banks "
          f"(the parent commit's library: {PARENT_GROWTH_BYTES})")
    assert grew <= PARENT_GROWTH_BYTES, (grew, PARENT_GROWTH_BYTES)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import time
    for k, ex in KINDS:
        t0 = time.perf_counter()
        print(f"[stream lifetime] lib={os.environ.get('SG_LIB_PATH', 'in-tree')} {k} exact={ex}: grew {_growth(k, ex)} bytes "
              f"over {COUNT} banks in {time.perf_counter() - t0:.1f} s", flush=True)
