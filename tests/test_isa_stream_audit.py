"""ISA-level guard for stream.hip (StreamBank; no GPU needed: hipcc cross-compiles).  From n_fft = 2048 on its
transforms run as 256-thread teams that share one LDS buffer across team_sync barriers -- the hazard class
tools/audit_barrier_waits.py looks for.  Its whole device code, built with build()'s flags."""
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
KERNELS = ("k_st_thresh", "k_st_decide", "k_st_fsmooth", "k_st_apply", "k_st_finish")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_barrier_of_the_stream_kernels_is_reached_with_an_unwaited_lds_write(tmp_path):
    asm = tmp_path / "stream.s"
    subprocess.run([HIPCC] + SHIPPED + ["-I", CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "stream.hip"), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^(_Z\w*k_st_\w+):", text, re.M)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_barrier_waits.py"), str(asm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "barriers flagged: 0" in out, out
    audited = re.search(r"(\d+) kernels audited", out)
    assert names and audited and int(audited.group(1)) >= len(names), out
    for k in KERNELS:
        assert any(k in nm for nm in names), (k, names)
    for k in ("k_st_decide", "k_st_apply"):
        for N in (128, 256, 512, 1024, 2048):
            assert any("%sILi%dE" % (k, N) in nm for nm in names), (k, N, names)
    # no kernel of the file spills: private segment (scratch) size 0 everywhere
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert scratch and all(int(v) == 0 for v in scratch), scratch
