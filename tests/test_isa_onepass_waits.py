"""ISA-level guard (no GPU needed: hipcc cross-compiles): the three places of the persistent one-pass gate's per-tile chain at
which the compiler used to wait vmcnt(0) although the result did not need it there (profiles/
onepass_chain.txt section D).  While a FLAT access is pending every wait the gfx9 wait-count insertion emits is a zero wait,
and a zero wait also waits for the write-through acknowledgements of the inline-asm sc1 stores and for every load issued
after the value that is needed.  Per persistent instantiation:

  (a) between the next-ticket atomic of an interior tile and the first MFMA behind it no s_waitcnt names vmcnt;
  (b) the wait in front of the first multiply by 1 / envelope in the tile_fast epilogue is not vmcnt(0);
  (c) between the bits' publish store and the smoothing stage's closing barrier there is no flat_ instruction.

tests/golden/onepass_waits_parent_isa.txt is the same stretch of the kernel before the change: every assertion fails on it."""
import os
import re
import shutil

import pytest

from tests.test_isa_audit import HIPCC, TU, _compile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tests", "golden", "onepass_waits_parent_isa.txt")
PERSISTENT = {"plain": "_ZN2sg4fast14k_gate_onepassILi4ELb0ELb0ELb0ELb1EEEvNS0_11OnePassArgsE",
              "prop": "_ZN2sg4fast14k_gate_onepassILi4ELb1ELb0ELb0ELb1EEEvNS0_11OnePassArgsE"}

pytestmark = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists(HIPCC)), reason="hipcc not found")


def _instructions(text):
    """Instruction lines of an assembly listing, in layout order: no labels, directives or comments."""
    out = []
    for ln in text.split("\n"):
        t = ln.strip()
        if not t or t.startswith(";") or t.startswith(".") or re.match(r"^[\w.$]+:", t):
            continue
        out.append(t.split(";")[0].strip())
    return out


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    d = tmp_path_factory.mktemp("onepass_waits")
    src, asm = d / "tu.hip", d / "tu.s"
    src.write_text(TU % "")
    _compile(src, asm)
    text = asm.read_text()
    out = {}
    for tag, name in PERSISTENT.items():
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.M | re.S)
        assert m, name
        out[tag] = _instructions(m.group(1))
    return out


@pytest.fixture(scope="module")
def parent():
    return _instructions(open(PARENT).read())


def _is(ins, prefix):
    return ins.startswith(prefix)


def _names_vmcnt(ins):
    return ins.startswith("s_waitcnt") and "vmcnt" in ins


def _mfmas(body):
    idx = [i for i, s in enumerate(body) if _is(s, "v_mfma")]
    assert idx, "no MFMA in the kernel"
    return idx


def waits_between_draw_and_mfma(body):
    """(a): the interior tile's draw is the last returning atomic add of the kernel (before it: the first ticket in the
    prologue and a halo tile's draw, both consumed at once)."""
    draws = [i for i, s in enumerate(body) if re.match(r"(flat|global)_atomic_add\b.*\bsc0\b", s)]
    assert draws, "no returning atomic add"
    d = draws[-1]
    m = next(i for i in _mfmas(body) if i > d)
    return [s for s in body[d + 1:m] if _names_vmcnt(s)]


def wait_before_first_envelope_multiply(body):
    """(b): the tile_fast epilogue begins with the trailing partial hops' two sc1 stores (the first pair of 16-byte sc1 stores
    behind the smoothing stage); the first multiply behind them is the first finished hop's."""
    last = _mfmas(body)[-1]
    sc1 = [i for i, s in enumerate(body) if i > last and re.match(r"global_store_dwordx4 .*\bsc1\b", s)]
    assert len(sc1) >= 2 and sc1[1] - sc1[0] < 16, "no pair of sc1 stores behind the smoothing stage"
    mul = next(i for i in range(sc1[1], len(body)) if _is(body[i], "v_mul_f32"))
    bar = max(i for i in range(mul) if _is(body[i], "s_barrier"))
    waits = [s for s in body[bar:mul] if _names_vmcnt(s)]
    return waits[-1] if waits else None


def flats_in_the_smoothing_stage(body):
    """(c): from the bits' publish (the last sc1 store in front of the first MFMA) to the first barrier behind the last MFMA."""
    mf = _mfmas(body)
    pub = max(i for i in range(mf[0]) if re.match(r"global_store_dwordx4 .*\bsc1\b", body[i]))
    end = next(i for i in range(mf[-1], len(body)) if _is(body[i], "s_barrier"))
    return [s for s in body[pub:end] if _is(s, "flat_")]


@pytest.mark.parametrize("tag", sorted(PERSISTENT))
def test_no_vmcnt_wait_between_the_ticket_draw_and_the_matrix_cores(bodies, tag):
    waits = waits_between_draw_and_mfma(bodies[tag])
    assert not waits, waits


@pytest.mark.parametrize("tag", sorted(PERSISTENT))
def test_the_epilogue_waits_for_the_envelope_with_a_partial_vmcnt(bodies, tag):
    w = wait_before_first_envelope_multiply(bodies[tag])
    assert w is not None, "no wait that names vmcnt between the epilogue's barrier and its first multiply"
    assert "vmcnt(0)" not in w, w


@pytest.mark.parametrize("tag", sorted(PERSISTENT))
def test_no_flat_access_in_the_smoothing_stage(bodies, tag):
    flats = flats_in_the_smoothing_stage(bodies[tag])
    assert not flats, flats


def test_every_assertion_fails_on_the_parents_code(parent):
    waits = waits_between_draw_and_mfma(parent)
    assert waits and all("vmcnt(0)" in s for s in waits), waits
    assert "vmcnt(0)" in wait_before_first_envelope_multiply(parent)
    flats = flats_in_the_smoothing_stage(parent)
    assert any(_is(s, "flat_atomic_add") for s in flats) and sum(_is(s, "flat_load_dwordx2") for s in flats) == 3, flats
