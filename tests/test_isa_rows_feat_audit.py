"""ISA-level guard for rows_feat.hip (TorchGate.gated_filterbank lengths=; no GPU needed: hipcc cross-compiles), after
tests/test_isa_rows_audit.py: the two feature kernels share one LDS buffer (and the backward its g' and p rows) across
team_sync barriers -- the hazard class tools/audit_barrier_waits.py looks for.  Built with
build()'s flags; no kernel of the file may use scratch, and the forward keeps k_rw_spec's waves per SIMD."""
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
SIZES = (128, 256, 512, 1024, 2048)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_barrier_of_the_feature_kernels_is_reached_with_an_unwaited_lds_write(tmp_path):
    asm = tmp_path / "rows_feat.s"
    subprocess.run([HIPCC] + SHIPPED + ["-I", CSRC, "--cuda-device-only", "-S", os.path.join(CSRC, "rows_feat.hip"), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^(_Z\w*k_rw_\w+):", text, re.M)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_barrier_waits.py"), str(asm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "barriers flagged: 0" in out, out
    audited = re.search(r"(\d+) kernels audited", out)
    assert len(names) == 10 and audited and int(audited.group(1)) >= len(names), out
    for k in ("9k_rw_feat", "13k_rw_feat_bwd"):
        for N in SIZES:
            assert any("%sILi%dE" % (k, N) in nm for nm in names), (k, N, names)
    # no kernel of the file spills: private segment (scratch) size 0 everywhere
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(scratch) == 10 and all(int(v) == 0 for v in scratch), scratch
    # the forward fits k_rw_spec's waves per SIMD (profiles/rows_kernel_resources.txt): 3 up to n_fft = 1024 (at most 168
    # VGPRs of the 512 a SIMD lane has), 2 from n_fft = 2048 on (at most 256)
    for N in SIZES:
        m = re.search(r"\.name:\s+_ZN2sg9k_rw_featILi%dE.*?\.vgpr_count:\s*(\d+)" % N, text, re.S)
        assert m and int(m.group(1)) <= (168 if N <= 512 else 256), (N, m and m.group(1))
