"""A handle gives back every device buffer it allocated (csrc/handle.hpp: DevBuf frees its allocation in its destructor;
sg_destroy deletes the handle).

Until the buffers owned themselves, sg_destroy freed a hand-kept list of members, and ``norm64`` -- 2 KB uploaded by
sg_create for the default geometry only (n_fft = win = 1024, hop 256) -- was not on it: every such handle leaked one
allocation.  Per geometry: after a warm-up create / destroy, the device's free memory before and after COUNT create /
destroy pairs.

Measured on the MI355X (COUNT = 2000; profiles/host_split.txt): the library before this change grows by 8388608 bytes
at the default geometry (2000 allocations of one 4 KiB granule, taken from the device in 2 MiB steps) and by 0 at
n_fft = 512 and 1000; this library grows by 0 bytes at all three.  The bound is a quarter of the former's growth
(2 MiB: a single step of the allocator already misses it), for every geometry: the register geometry n_fft = 512 and the
mixed-radix n_fft = 1000 upload other tables (tw512 / invn / regtab; the radix plan's twiddles) and never leaked, so
the same bound holds them to "no table family leaks".

``python tests/test_gpu_handle_lifetime.py`` prints the figures without asserting (SG_LIB_PATH selects the library)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

COUNT = 2000
PARENT_GROWTH_BYTES = 8388608   # measured with the library of the parent commit (profiles/host_split.txt)


def _growth(n_fft, count=COUNT):
    """Bytes by which the device's free memory shrank over `count` create / destroy pairs of one geometry."""
    import torch
    from noisereduce_amd import _ffi

    def pair():
        g = _ffi.Gate("cuda:0", variant=_ffi.SG_VARIANT_S, stationary=True, n_fft=n_fft, win_length=n_fft,
                      hop_length=n_fft // 4, n_grad_freq=2, n_grad_time=4, smooth_mask=True)
        g.close()

    pair()   # warm-up: the runtime's own first-use allocations
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(count):
        pair()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info(0)[0]


def test_default_geometry_handles_leak_nothing():
    grew = _growth(1024)
    print(f"[handle lifetime] n_fft=1024: free memory shrank by {grew} bytes over {COUNT} handles "
          f"(before the buffers owned themselves: {PARENT_GROWTH_BYTES})")
    assert grew < PARENT_GROWTH_BYTES / 4, (grew, PARENT_GROWTH_BYTES)


@pytest.mark.parametrize("n_fft", [512, 1000])
def test_other_table_families_leak_nothing(n_fft):
    grew = _growth(n_fft)
    print(f"[handle lifetime] n_fft={n_fft}: free memory shrank by {grew} bytes over {COUNT} handles")
    assert grew < PARENT_GROWTH_BYTES / 4, (grew, PARENT_GROWTH_BYTES)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import time
    for n in (1024, 512, 1000):
        t0 = time.perf_counter()
        print(f"[handle lifetime] lib={os.environ.get('SG_LIB_PATH', 'in-tree')} n_fft={n}: grew {_growth(n)} bytes "
              f"over {COUNT} handles in {time.perf_counter() - t0:.1f} s", flush=True)
