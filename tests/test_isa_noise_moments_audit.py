"""ISA-level guard for the two-launch noise statistics (no GPU needed: hipcc cross-compiles).  k_noise_moments reuses
its teams' transform buffers twice across workgroup barriers (the frames' {P, dB} rows, then the frame groups'
partials) and, at n_fft = 2048, runs its transforms as 256-thread teams over team_sync barriers -- the hazard class
tools/audit_barrier_waits.py looks for.  The four instantiations api.hip launches and the
16-band k_colstats1_final, built with build()'s flags; none of them may spill."""
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
SHAPES = [(128, 16, 64), (256, 32, 32), (512, 64, 16), (1024, 256, 4)]     # N, threads per frame, teams (launch_noise_moments_n)

TU = """#include <hip/hip_runtime.h>
#include <cstdint>
#include "kernels.hpp"
%s
template __global__ void sg::k_colstats1_final<4, true, 16, 16>(const double*, const double*, sg::Geom, int, double, double, double, int,
                                                         double*, double*, sg::GateConsts, int);
""" % "\n".join("template __global__ void sg::k_noise_moments<%d, %d, %d>(sg::View, sg::Geom, const sg::cx<double>*, const double*, "
                "double*, double, double*, sg::DbFast, unsigned*, int);" % s for s in SHAPES)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_barrier_of_the_noise_moment_kernels_is_reached_with_an_unwaited_lds_write(tmp_path):
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert "constexpr int NT = nm_team_threads<N>(), TEAMS = 1024 / NT;" in api and "k_colstats1_final<NM_TG, true, NM_BW, NM_MAXS>" in api
    src = tmp_path / "tu.hip"
    src.write_text(TU)
    asm = tmp_path / "tu.s"
    subprocess.run([HIPCC] + SHIPPED + ["-I", CSRC, "--cuda-device-only", "-S", str(src), "-o", str(asm)], check=True,
                   capture_output=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^(_Z\w*(?:k_noise_moments|k_colstats1_final)\w+):", text, re.M)
    for s in SHAPES:
        assert any("k_noise_momentsILi%dELi%dELi%dE" % s in nm for nm in names), (s, names)
    assert any("k_colstats1_finalILi4ELb1ELi16ELi16E" in nm for nm in names), names
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_barrier_waits.py"), str(asm)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "barriers flagged: 0" in out, out
    audited = re.search(r"(\d+) kernels audited", out)
    assert audited and int(audited.group(1)) >= len(SHAPES) + 1, out
    scratch = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
    assert len(scratch) >= len(SHAPES) + 1 and all(int(v) == 0 for v in scratch), scratch
