"""ISA-level guard (no GPU needed: hipcc cross-compiles) of the launch plan in the persistent one-pass gate (DESIGN.md section 3,
profiles/onepass_tile_plan.txt).  Per persistent instantiation, from the listing the shipped flags give:

  * 168 VGPRs, no spilled VGPR, no scratch: the plan must not cost the kernel its three workgroups per CU;
  * at most RCP_KEPT expansions of a 32-bit integer division (one v_rcp_iflag_f32 each).  The parent's listing holds 17 per
    persistent instantiation: the loop top, the publish stage, prefetch_next, seam_where (three copies), the epilogue, and the
    cold paths.  The loop top, prefetch_next and the epilogue take their quotients from the plan (a multiply-high and two
    shifts); what is left is the publish stage and seam_issue (ceilings below 1 % of a step: left alone), the general
    evaluation a unit at a row's edge falls back to inside prefetch_next, and the cold paths -- 11 in the finished build's
    listing."""
import os
import re
import shutil

import pytest

from tests.test_isa_audit import HIPCC, TU, _compile
from tests.test_isa_onepass_waits import PERSISTENT, _instructions

RCP_PARENT = 17
RCP_KEPT = 11

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists(HIPCC)), reason="hipcc not found")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    d = tmp_path_factory.mktemp("onepass_plan_isa")
    src, asm = d / "tu.hip", d / "tu.s"
    src.write_text(TU % "")
    _compile(src, asm)
    return asm.read_text()


def _meta(text, name, key):
    """A field of the kernel's entry in the code object's metadata (amdhsa.kernels)."""
    for blk in text.split("  - .agpr_count:")[1:]:
        if re.search(r"\.name:\s+%s\s" % re.escape(name), blk):
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    raise AssertionError("no metadata for " + name)


@pytest.mark.parametrize("tag", sorted(PERSISTENT))
def test_registers_and_scratch(listing, tag):
    name = PERSISTENT[tag]
    assert _meta(listing, name, "vgpr_count") == 168
    assert _meta(listing, name, "vgpr_spill_count") == 0
    assert _meta(listing, name, "private_segment_fixed_size") == 0


@pytest.mark.parametrize("tag", sorted(PERSISTENT))
def test_division_expansions(listing, tag):
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(PERSISTENT[tag]), listing, re.M | re.S)
    assert m, tag
    n = sum(1 for s in _instructions(m.group(1)) if s.startswith("v_rcp_iflag_f32"))
    assert 0 < n <= RCP_KEPT < RCP_PARENT, n
