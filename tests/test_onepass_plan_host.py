"""The launch plan of the n_fft = 1024 one-pass gate (noisereduce_amd/csrc/onepass_plan.hpp) on the host: for every ticket of
a launch, what the kernel gets by evaluating the ticket against the plan equals the plain evaluation -- integer divisions and
the clause chains of `blk_vec` / `tile_fast` / the floor-test slice as k_gate_onepass writes them field by field, restated here.

The header's functions are `__host__ __device__`; tests/onepass_plan_host.cpp is a stand-alone program around them (built here
with the host compiler and -fsanitize=address,undefined where the compiler has them).  Contract of the plan: u, jt, row, chunk
and the granule offsets for EVERY ticket; for a unit the plan calls interior, both flags for every tile of the unit, and the
source / output / slice addresses wherever a flag holds.  A unit that is not interior is the kernel's own evaluation's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "onepass_plan_host.cpp")
from tests.test_isa_audit import HIPCC

# a host C++ compiler: the system's, else the clang++ that hipcc drives (next to it, or under the ROCm tree's llvm/bin)
_ROCM = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
CXX = (shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or
       next((p for p in (os.path.join(_ROCM, "llvm", "bin", "clang++"), os.path.join(_ROCM, "lib", "llvm", "bin", "clang++"),
                         os.path.join(os.path.dirname(HIPCC), "clang++")) if os.path.exists(p)), None))


def test_a_host_compiler_is_there():
    assert CXX is not None, "no host C++ compiler: neither g++ / c++ / clang++ on PATH nor the clang++ of %s" % HIPCC

NF, SPAN, TILE, HOP, PADL, SCAN_MAX, TILE_WORDS = 16, 4864, 4096, 256, 512, 1280, 288
FIELDS = ("x out in_dtype out_dtype normalize stride lo hi cs pad Lp c0 unit0 n_chunks ostride p0 p1 g_step g0 g_lo g_hi padL "
          "T Lout h_begin h_end n_tiles scan_q").split()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onepass_plan") / "plan_host")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizer runtimes)
        subprocess.run(base, check=True)
    return exe


def geometry(N, rows=1, cs=600000, pad=30000, start=0, end=None, dtype=0, odtype=None, x=1 << 20, out=1 << 30, halo=(0, 0),
             stride=None, unit0=0, units=None):
    """The launch sg_process_chunks + onepass_run set up for a chunked call (api.hip), as plain numbers."""
    end = N if end is None else end
    ich1, ich2 = start // cs, (end - 1) // cs
    g = dict(x=x, out=out, in_dtype=dtype, out_dtype=dtype if odtype is None else odtype, normalize=1,
             stride=N if stride is None else stride, lo=-halo[0], hi=N + halo[1], cs=cs, pad=pad, Lp=cs + 2 * pad, c0=ich1, unit0=unit0,
             n_chunks=ich2 - ich1 + 1, ostride=N if stride is None else stride, p0=pad, p1=pad + cs, g_step=cs, g0=start, g_lo=start,
             g_hi=end, padL=PADL)
    g["T"] = g["Lp"] // HOP + 1
    g["Lout"] = (g["T"] - 1) * HOP
    g["h_begin"] = (g["p0"] + PADL) // HOP
    g["h_end"] = (g["p1"] - 1 + PADL) // HOP + 1
    g["n_tiles"] = (g["h_end"] - g["h_begin"] + 3 + NF - 1) // NF
    ntt = g["n_tiles"] + 2
    sp0 = (g["h_begin"] - 3 - NF) * HOP - PADL
    sp1 = (g["h_begin"] - 3 + g["n_tiles"] * NF) * HOP - PADL + SPAN
    inside = max(0, min(g["Lp"], sp1) - max(0, sp0))
    g["scan_q"] = (g["Lp"] - inside + ntt - 1) // ntt
    g["units"] = rows * g["n_chunks"] - unit0 if units is None else units
    return g


def plain(g, t):
    """k_gate_onepass's own evaluation of ticket t (loop top, tile_src, epilogue), field by field."""
    ntt = g["n_tiles"] + 2
    u, jt = t // ntt, t % ntt - 1
    gu = g["unit0"] + u
    row, chunk = gu // g["n_chunks"], g["c0"] + gu % g["n_chunks"]
    tf = g["h_begin"] - 3 + jt * NF
    s0b = tf * HOP - g["padL"]
    g0c = chunk * g["cs"] - g["pad"]
    gb = g0c + s0b
    sp = g["x"] + 4 * (row * g["stride"] + gb)
    blk_vec = (g["in_dtype"] == 0 and tf >= 0 and tf + NF <= g["T"] and s0b >= 0 and s0b + SPAN <= g["Lp"] and gb >= g["lo"] and
               gb + SPAN <= g["hi"] and sp % 16 == 0)
    gi00 = chunk * g["g_step"] + (s0b - g["p0"])
    dbase = g["out"] + 4 * (row * g["ostride"] + gi00 - g["g0"])
    tile_fast = (g["out_dtype"] == 0 and g["normalize"] != 0 and tf >= 3 and tf + NF + 2 < g["T"] and tf >= g["h_begin"] and
                 tf + NF + 2 < g["h_end"] and s0b >= g["p0"] and s0b + TILE <= g["p1"] and s0b + TILE <= g["Lout"] and
                 gi00 >= g["g_lo"] and gi00 + TILE <= g["g_hi"] and dbase % 16 == 0)
    # the floor-test slice (tile_src, test == true)
    s_lo, s_hi = max(0, g["lo"] - g0c), min(g["Lp"], g["hi"] - g0c)
    sp0 = (g["h_begin"] - 3 - NF) * HOP - g["padL"]
    sp1 = (g["h_begin"] - 3 + g["n_tiles"] * NF) * HOP - g["padL"] + SPAN
    first = min(s_hi, max(s_lo, sp0))
    last = max(s_lo, min(s_hi, sp1))
    lenA = first - s_lo
    c0 = (jt + 1) * g["scan_q"]
    c1 = min(c0 + g["scan_q"], lenA + (s_hi - last))
    sc_base = None
    if g["in_dtype"] == 0 and c1 > c0 and c1 - c0 <= SCAN_MAX and (c1 <= lenA or c0 >= lenA):
        sc_base = g["x"] + 4 * (row * g["stride"] + g0c + (s_lo + c0 if c1 <= lenA else last + (c0 - lenA)))
    return dict(u=u, jt=jt, row=row, chunk=chunk, blk_vec=blk_vec, tile_fast=tile_fast, sp=sp, dbase=dbase,
                xbits=(u * ntt + jt + 1) * TILE_WORDS, part2=(u * g["n_tiles"] + jt) * 3 * 256, c0=c0, c1=c1, sc_base=sc_base)


def run_plan(prog, g, first, count):
    args = [prog, "plan"] + [str(g[f]) for f in FIELDS] + [str(first), str(count)]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.split("\n")
    head = [int(v) for v in lines[0].split()]
    rows = [[int(v) for v in ln.split()] for ln in lines[1:] if ln]
    assert len(rows) == count
    return dict(zip("k0 k1 bv0 bv1 tf0 tf1 src dst".split(), head)), rows


def check(prog, g, grid=8):
    """Every ticket of the launch (and the `grid` tickets past its end, which only the quotients see) against plain()."""
    ntt = g["n_tiles"] + 2
    total = g["units"] * ntt
    P, rows = run_plan(prog, g, 0, total + grid)
    interior_units = 0
    for t, r in enumerate(rows):
        u, jt, row, k, interior, bv, fast, src_off, dst_off, xbits, part2, c0, c1, has, sc_off = r
        w = plain(g, t)
        assert (u, jt, row, g["c0"] + k) == (w["u"], w["jt"], w["row"], w["chunk"]), (t, r, w)
        assert (xbits, part2) == (w["xbits"], w["part2"]), (t, r, w)
        if t >= total:
            continue
        if not interior:
            assert not bv and not fast, (t, r)   # the plan claims nothing about this unit: the kernel evaluates it itself
            continue
        interior_units += jt == 0
        assert (bool(bv), bool(fast)) == (w["blk_vec"], w["tile_fast"]), (t, r, w)
        if bv:
            assert P["src"] + 4 * src_off == w["sp"], (t, r, w)
            assert (c0, c1) == (w["c0"], w["c1"]) and bool(has) == (w["sc_base"] is not None), (t, r, w)
            if has:
                assert P["src"] + 4 * sc_off == w["sc_base"], (t, r, w)
        if fast:
            assert P["dst"] + 4 * dst_off == w["dbase"], (t, r, w)
    return P, interior_units


N48 = 48 * 600000


def test_benchmark_geometry_interior_units_and_ranges(prog):
    """configs[1]: 48 chunks of 147 tiles + 2 halo tiles; every chunk but the first and the last is interior, every tile of
    those is blk_vec and tiles 1 .. 145 are tile_fast."""
    g = geometry(N48)
    assert (g["n_tiles"], g["n_chunks"], g["scan_q"]) == (147, 48, 329)
    P, n = check(prog, g, grid=768)
    assert (P["k0"], P["k1"], P["bv0"], P["bv1"], P["tf0"], P["tf1"]) == (1, 46, -1, 147, 1, 145) and n == 46


@pytest.mark.parametrize("cs, n_tiles", [(4096, 2), (8192, 3), (606720, 149)])
@pytest.mark.parametrize("n_chunks", [1, 3, 7, 48])
def test_tiles_per_unit_and_chunks_per_row(prog, cs, n_tiles, n_chunks):
    if n_tiles == 149 and n_chunks == 48:
        n_chunks = 9   # (the 48-chunk launch of long units is the benchmark geometry above)
    N = n_chunks * cs
    g = geometry(N, cs=cs, pad=2048)
    assert g["n_tiles"] == n_tiles and g["n_chunks"] == n_chunks
    P, n = check(prog, g)
    assert n == max(0, n_chunks - 2), (P, n)   # the first and the last chunk of the row read its edge


@pytest.mark.parametrize("kw, interior", [
    (dict(rows=3), 3 * 5),                                      # three rows
    (dict(rows=3, unit0=9, units=12), 4 + 5),                   # a batch that starts inside row 1: its chunks 2 .. 6, then row 2
    (dict(N=7 * 8192 - 3000), 5),                               # ragged last chunk: chunk 5's window still ends inside the row
    (dict(N=7 * 8192 - 4), 5),
    (dict(N=7 * 8192 - 1), 0),                                  # ... a row length that does not keep the rows' alignment
    (dict(start=8192 + 100, end=5 * 8192 + 17), 4),             # a sub-range: chunks 1 .. 5; the kept range's end cuts chunk 5's
                                                                # tile_fast tile, its start only chunk 1's tile 0 (never tile_fast)
    (dict(rows=3, start=2 * 8192, end=6 * 8192), 3 * 4),        # ... on chunk boundaries: only the row's own edges bind
    (dict(x=(1 << 20) + 4), 0),                                 # a row base one sample off a 16-byte boundary
    (dict(rows=3, stride=7 * 8192 + 2), 0),                     # rows that do not keep the alignment
    (dict(dtype=2), 0),                                         # int16 input
    (dict(odtype=1), 0),
    (dict(halo=(2048, 2048)), 7),                               # the caller holds halos: no chunk reads past the range
])
def test_edges_subranges_alignment_and_sample_types(prog, kw, interior):
    kw = dict(kw)
    N = kw.pop("N", 7 * 8192)
    g = geometry(N, cs=8192, pad=2048, **kw)
    P, n = check(prog, g)
    assert n == interior, (P, n)


@pytest.mark.parametrize("d", [3, 4, 5, 48, 149, 151, 1 << 16, (1 << 31) + 1, (1 << 32) - 1])
def test_magic_quotients(prog, d):
    """ticket / d by multiply-high and shifts against //.  At the listed geometries check() above compares u, jt, row and chunk
    for EVERY ticket below total_tiles + grid.  At the largest total_tiles the driver admits (its counters are 32-bit:
    total_tiles + grid < 2^32) every ticket is 4 G quotients per divisor: SAMPLED here, five windows of 4 096 dividends per
    divisor -- the start of the range, around d, around 1000 d, around the last multiple of d, and the last 4 096 values below
    2^32.  (The round-up multiplier is exact for every 32-bit dividend by construction: Granlund & Montgomery 1994, section 4.)"""
    top = (1 << 32) - 1
    for first in (0, d - 2, 1000 * d - 3, (top // d) * d - 3, top - 4095):
        first = max(0, min(first, top - 4095))
        out = subprocess.run([prog, "magic", str(d), str(first), "4096"], capture_output=True, text=True, check=True).stdout.split()
        assert [int(v) for v in out] == [n // d for n in range(first, first + 4096)], (d, first)
