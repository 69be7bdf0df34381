"""Resource guard for feat.hip (TorchGate.gated_filterbank; no GPU needed: hipcc cross-compiles).  Its whole device code,
built with build()'s flags: no kernel has a private segment -- the frame loop of k_feat_fwd / k_feat_bwd holds the transform's
registers, the filter sums and (with log) a float64 logarithm within four waves per SIMD without spilling."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noisereduce_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_EXTRA  # noqa: E402  (the flags the library is built with)

SHIPPED = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"] + HIPCC_EXTRA


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_kernel_of_feat_hip_has_a_private_segment(tmp_path):
    asm = tmp_path / "feat.s"
    subprocess.run([HIPCC] + SHIPPED + ["-I", CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "feat.hip"), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^\s*\.name:\s*(_Z\w*k_feat_\w+)\s*$", text, re.M)
    # every frame length, both kernels, both sample types, both powers, log off and on
    for k in ("k_feat_fwd", "k_feat_bwd"):
        for N in (128, 256, 512, 1024, 2048):
            got = [nm for nm in names if "%sILi%dE" % (k, N) in nm]
            assert len(got) == 8, (k, N, got)
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(scratch) == len(names) == 80, (len(scratch), len(names))
    assert all(int(v) == 0 for v in scratch), scratch
