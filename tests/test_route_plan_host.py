"""The route table of the gate engine (noisereduce_amd/csrc/route.hpp: plan_S, plan_T, workspace_S) on the host.
tests/route_plan_host.cpp is a stand-alone program around the header (built with the host compiler, -fsanitize=address,undefined
where the compiler has them); it prints the plan of every caps / shape tuple it reads.  No GPU and no Python extension.

Every field of the plan is compared with a restatement of the rules as api.hip wrote them against the handle BEFORE route.hpp
existed (``parent_S`` / ``parent_T`` below: clause by clause, each with the line of that api.hip -- the commit before
route.hpp -- in a comment), over a lattice of

* every routing option on and off, SG_OPT_FORCE_NOROWGATE 0 / 1 / 2, SG_OPT_TILE_ORDER 0 / 1 / 2;
* both variants, both gates, prop_decrease 1 and 0.8, every geometry class (default 1024, register 512 / 256 / 2048, other
  power of two, mixed radix, chirp-z, long frames), with and without each table;
* smoothing off, on, and at widths just inside and outside each kernel's limits (max_nf / max_nt of each OnePassGeom,
  NS_MAX_NF, the ns_iir_nt_ok set, NS_BOX_MAX_NT, RG_NFMAX / RG_NTMAX, ktot 65535 / 65536);
* hop counts giving 0, 1 and 2 one-pass tiles, T = 64 / 65 (row gate) and 128 / 129 (row-fused decide), 159 / 160 rows,
  float32 / int16 / float64 in, float32 / int16 out, field sink or not, noise rows none / one / one per row.

The axes are too many for one product (about 10^12 points), so the lattice is the union of full products over the axes that
interact (``LATTICES``) and a seeded sample of the whole product.  A debug fact the parent did not write on a route (the value
of the batch before stayed, and no tap could read it) is not compared.

Invariants of every plan: one pipeline and one apply stage; ``lean`` only on routes that never touch P, raw, M or seg; the
workspace figure covers units_per_batch x unit_bytes of the plan's own route plus the exchange buffers that route ensures."""
import itertools
import os
import random
import subprocess
from types import SimpleNamespace as NS

import pytest

from tests.test_onepass_plan_host import CXX, ROOT

SRC = os.path.join(ROOT, "tests", "route_plan_host.cpp")
S, T = 0, 1
F32, F64, I16, I32 = 0, 1, 2, 3
# enumerations of route.hpp, in declaration order
EXACT_FUSED, EXACT, ONEPASS, ONEPASS_REG, BITS3, FUSED, UNFUSED = range(7)
D_NONE, D_FAST, D_REG, D_LDS, D_F64 = range(5)
NS_NONE, NS_SMOOTHED, NS_CHAIN, NS_RAW, NS_BOX = range(5)
(A_NONE, A_FAST64_K, A_FAST64_M, A_X_OLA, A_FAST_K, A_FAST_M, A_REG_K, A_REG_M, A_OLA_K, A_OLA_M, A_FIELD) = range(11)
R_KEEP, R_ALL, R_WINDOW, R_TILES = range(4)
TH_NONE, TH_SHARED, TH_PER_ROW, TH_SELF = range(4)
# limits of the kernel headers
NS_TT, NS_MAX_NF, NS_IIR_MAX_NT, NS_BOX_MAX_NT, NS_BOX_KB = 64, 24, 20, 12, 20
RG_FRAMES, RG_NFMAX, RG_NTMAX, RG_MIN_ROWS = 64, 30, 16, 160


def ns_iir_nt_ok(nt):
    return 1 <= nt <= NS_IIR_MAX_NT or nt in (25, 34, 37)


def opg(hop, NF, NH, tile_words, xw, max_nf, max_nt, F, extra):
    return NS(hop=hop, NF=NF, NH=NH, tile_words=tile_words, xw=xw, max_nf=max_nf, max_nt=max_nt, F=F, extra=extra,
              tiles=lambda nh: (nh + extra + NH - 1) // NH)


OP1024 = opg(256, 16, 16, 288, 9, 8, 16, 513, 3)
REGS = [NS(op=opg(128, 32, 29, 320, 5, 8, 24, 257, 0), op_seam=opg(128, 32, 32, 320, 5, 8, 24, 257, 3), abut=False, frames=32, hop=128),
        NS(op=opg(64, 64, 61, 384, 3, 8, 40, 129, 0), op_seam=opg(64, 64, 64, 384, 3, 8, 40, 129, 3), abut=False, frames=64, hop=64),
        NS(op=opg(512, 8, 8, 272, 17, 24, 8, 1025, 3), op_seam=opg(512, 8, 8, 272, 17, 24, 8, 1025, 3), abut=True, frames=8, hop=512)]
# (geom, reg_sel) -> n_fft, F, FS and the handle's geometry members as sg_create sets them
GEOMS = {(0, 0): (1024, 513, 528), (1, 0): (512, 257, 272), (1, 1): (256, 129, 144), (1, 2): (2048, 1025, 1040),
         (2, 0): (4096, 2049, 2064), (3, 0): (1000, 501, 512), (4, 0): (1022, 512, 512), (5, 0): (16384, 8193, 8208)}
OPTS = ("force_unfused force_nofast force_f64_decide force_noseam force_nolean force_split fast_integer force_exact "
        "exact_materialised").split()


def handle(c):
    """The members of sg_handle that the parent's routing read, for a caps tuple."""
    h = NS(**vars(c))
    h.fast_ok = c.geom == 0
    h.reg = REGS[c.reg_sel] if c.geom == 1 else None
    h.big_M = 65536 if c.geom == 5 else 0
    h.czt_M = 2048 if c.geom in (3, 4) else 0
    h.mr_ok = c.geom == 3
    return h


def pw(b, rows):
    return (1.0 - b) ** float(rows)


# ---------------------------------------------------------------------------------------------------------------------
# the parent's rules (line numbers: noisereduce_amd/csrc/api.hip of the commit before route.hpp)
# ---------------------------------------------------------------------------------------------------------------------
def nonstat2_chain_ok(h, s):
    if h.variant != S or h.stationary or h.force_unfused:                                  # 1173
        return False
    if not (0.0 < h.iir_b < 1.0):                                                          # 1175
        return False
    return pw(h.iir_b, NS_TT + 2 * NS_IIR_MAX_NT) >= 1e-3 and s.T >= 1                     # 1177


def nonstat2_ok(h, s):
    if not nonstat2_chain_ok(h, s) or not h.smooth_mask:                                   # 1180
        return False
    if h.nt > NS_IIR_MAX_NT and not (pw(h.iir_b, NS_TT + 2 * h.nt) >= 1e-3):               # 1182
        return False
    return h.nf <= NS_MAX_NF and ns_iir_nt_ok(h.nt)                                        # 1183


def onepass_ok(h, s):
    g = OP1024                                                                             # 1619
    if h.force_split or h.force_f64_decide or h.force_noseam or h.force_nolean:            # 1620
        return False
    if not h.smooth_mask or h.nf > g.max_nf or h.nt > g.max_nt or not h.ftab3 or not h.optab:   # 1621
        return False
    if s.F != g.F:                                                                         # 1622
        return False
    return g.tiles(s.nh) >= 2                                                              # 1623


def onepass_reg_ok(h, r, s):
    if r.abut and h.force_noseam:                                                          # 1108
        return False
    g = r.op
    if h.force_nofast or h.force_split or h.force_f64_decide or h.force_unfused or not h.fused_ok:   # 1101
        return False
    if h.variant != S or not h.stationary or not h.smooth_mask:                            # 1102
        return False
    if h.nf > g.max_nf or h.nt > g.max_nt or s.F != g.F or not h.regtab:                   # 1103
        return False
    if h.tile_order == 1:                                                                  # 1104
        return False
    return s.nh > 0                                                                        # 1105


def exact_fused_ok(h, s):
    return (h.stationary and h.fused_ok and not h.force_unfused and h.fast_ok and not h.force_nofast and       # 1780
            not h.force_f64_decide and s.F == 513 and h.norm64 and not h.exact_materialised)                  # 1781


def k16_apply_geom(h):
    return not h.big_M and (not h.czt_M or h.mr_ok)                                        # 539


def parent_S(h, s):
    p = NS(pipe=None, decide=D_NONE, ns=NS_NONE, smooth_stage=False, k16_to_mask=False, apply=A_NONE, seam=False,
           exact_tiled=False, lean=False, f32_copy=False)
    f = NS(keeps=True, has_P=None, has_raw=None, fused=None, fast=None, k16_only=None, rg=None, range=R_KEEP)
    p.facts = f
    geom_fast = h.fast_ok and not h.force_nofast                                           # 2021
    r = None if h.force_nofast else h.reg                                                  # 195, 1992
    p.fast, p.reg = geom_fast, r is not None
    if h.force_exact or (s.out_dtype in (I16, I32) and not h.fast_integer):                # 1987
        if exact_fused_ok(h, s):                                                           # 1988
            p.pipe, p.lean = EXACT_FUSED, True                                             # 1786
            p.decide, p.apply = D_FAST, A_FAST64_K                                         # 1797 (fast = true), 1482, 1798
            f.has_P, f.fused, f.fast, f.range = False, True, True, R_WINDOW                # 1799, 1464
        else:
            p.pipe = EXACT
            p.exact_tiled = not h.exact_materialised                                       # 1900, 1933
            apply64 = geom_fast and s.F == 513 and h.norm64 and not h.exact_materialised   # 1877
            p.apply = A_FAST64_M if apply64 else A_X_OLA                                   # 1957, 1964
            f.keeps = False                                                                # 1959, 1973
        return p
    fused = h.fused_ok and not h.force_unfused                                             # 2020
    onepass = fused and geom_fast and onepass_ok(h, s)                                     # 1991
    onepass_r = r is not None and onepass_reg_ok(h, r, s)                                  # 1993
    full = h.prop_decrease == 1.0
    p.lean = bool(onepass or onepass_r or (fused and geom_fast and full))                  # 1994
    p.f32_copy = bool(s.in_dtype != F32 and                                                # 2003
                      ((geom_fast and (onepass or (not h.stationary and nonstat2_ok(h, s)))) or onepass_r))
    fast = fused and geom_fast and full                                                    # 2022
    if onepass:                                                                            # 2023
        p.pipe, p.seam = ONEPASS, True
        f.has_P, f.fused, f.fast, f.range = False, True, True, R_TILES                     # 2027, 1090
        return p
    if onepass_r:                                                                          # 2030
        p.pipe, p.seam = ONEPASS_REG, bool(r.abut or not h.force_noseam)                   # 1117
        f.has_P, f.fused, f.fast, f.k16_only, f.range = False, True, True, False, R_TILES  # 2034, 1090
        return p
    if fast:                                                                               # 2037
        p.pipe, p.apply = BITS3, A_FAST_K                                                  # 2041, 2042
        p.decide = D_FAST if not h.force_f64_decide else D_F64                             # 1482, 1510
        f.has_P, f.fused, f.fast = False, True, True                                       # 2043
        f.range = R_WINDOW if not h.force_f64_decide else R_ALL                            # 1464
        return p
    f.fast = bool(geom_fast or (fused and r is not None and full))                         # 2047
    if fused:                                                                              # 2048
        p.pipe = FUSED
        rr = r if not h.force_f64_decide else None                                         # 1474 (fast = false)
        p.decide = D_REG if rr else (D_LDS if not h.force_f64_decide else D_F64)           # 1504, 1506, 1510
        f.range = R_ALL                                                                    # 1464, 1465
        k16_only = False
        if r is not None and full:                                                         # 1528
            pass
        else:
            k16_only = bool(k16_apply_geom(h) and full)                                    # 1531
            f.k16_only = k16_only
            p.k16_to_mask = not k16_only                                                   # 1533, 1534
    else:
        p.pipe = UNFUSED
        if h.stationary:                                                                   # 2051
            pass
        elif nonstat2_ok(h, s):                                                            # 2054
            p.ns = NS_SMOOTHED
        elif nonstat2_chain_ok(h, s):                                                      # 2056
            p.ns = NS_CHAIN
        else:
            p.ns = NS_RAW                                                                  # 2059
        p.smooth_stage = bool(h.stationary or not (nonstat2_ok(h, s) or (nonstat2_chain_ok(h, s) and not h.smooth_mask)))   # 2061
    if geom_fast:                                                                          # 2064
        p.apply = A_FAST_M
    elif r is not None:                                                                    # 2066
        p.apply = A_REG_K if (fused and full) else A_REG_M                                 # 2067
    elif fused and k16_only:                                                               # 2069
        p.apply = A_OLA_K
    else:
        p.apply = A_OLA_M                                                                  # 2072
    f.has_P = bool(h.stationary and not fused)                                             # 2076
    if not fused:   # (a fused batch: no tap reads has_raw, debug.hip fetch field 0 fails on `fused` first)
        f.has_raw = bool(h.stationary or not nonstat2_chain_ok(h, s) or (not nonstat2_ok(h, s) and h.smooth_mask))   # 2077
    f.fused = fused                                                                        # 2078
    return p


def box_mask_ok(h):
    if h.variant != T or h.stationary or h.force_unfused or h.n_movemean != NS_BOX_KB:     # 1271
        return False
    if not h.smooth_mask:                                                                  # 1272
        return True
    return h.nf <= NS_MAX_NF and 1 <= h.nt <= NS_BOX_MAX_NT                                # 1273


def rowgate_ok(h, s):
    if h.rowgate_mode == 1 or (h.rowgate_mode == 0 and s.units < RG_MIN_ROWS):             # 2091
        return False
    return bool(h.fast_ok and not h.force_nofast and not h.force_unfused and h.stationary and h.prop_decrease == 1.0 and   # 2092
                h.smooth_mask and h.ktot <= 65535 and s.F == 513 and 1 <= s.T <= RG_FRAMES and                          # 2093
                1 <= h.nf <= RG_NFMAX and 1 <= h.nt <= RG_NTMAX)                                                        # 2094


def bits_path_ok(h):
    return bool(h.fast_ok and not h.force_nofast and not h.force_unfused and h.prop_decrease == 1.0 and h.ktot <= 65535 and   # 2401
                (not h.smooth_mask or (h.nt <= 96 and h.t_sm2_ok)))                                                          # 2402


def parent_T(h, s):
    p = NS(rowgate=False, bits_path=False, to_raw=False, row_fused=False, thresh=TH_NONE, ns=NS_NONE, smooths=False, apply=A_NONE)
    geom_fast = h.fast_ok and not h.force_nofast                                           # 2501
    r = None if h.force_nofast else h.reg                                                  # 2556
    p.fast, p.reg = geom_fast, r is not None
    smooths = bool(h.stationary or not box_mask_ok(h))                                     # 2502
    sink = A_FIELD if s.field else (A_FAST_M if geom_fast else (A_REG_M if r is not None else A_OLA_M))   # 2549 .. 2559
    general = NS(keeps=True, has_P=bool(h.stationary), has_raw=smooths, fused=False, fast=geom_fast, k16_only=None, rg=False,   # 2561, 2562, 2484
                 range=R_KEEP)
    p.smooths, p.apply, p.facts = smooths, sink, general
    if h.stationary:                                                                       # 2510
        if not s.field and not s.noise_rows and rowgate_ok(h, s):                          # 2511
            p.rowgate, p.smooths, p.apply = True, False, A_NONE                            # 2513
            p.facts = NS(keeps=True, has_P=False, has_raw=False, fused=True, fast=True, k16_only=None, rg=True, range=R_ALL)   # 2514 .. 2516
            return p
        p.bits_path = bits_path_ok(h)                                                      # 2519
        p.to_raw = bool(s.field)                                                           # 2520
        p.thresh = TH_SHARED if s.noise_rows == 1 else (TH_PER_ROW if s.noise_rows else TH_SELF)   # 2415, 2417, 2421
        p.row_fused = bool(p.bits_path and s.T * 64 * 8 <= 64 * 1024)                      # 2425, 2426
        if p.bits_path and not s.field:                                                    # 2521
            p.smooths, p.apply = False, A_FAST_K                                           # 2523, 2529
            p.facts = NS(keeps=True, has_P=True, has_raw=None, fused=True, fast=True, k16_only=None, rg=False, range=R_ALL)    # 2530, 2531
    elif box_mask_ok(h):                                                                   # 2534
        p.ns = NS_BOX
    else:
        p.ns = NS_RAW                                                                      # 2538
    return p


def unit_bytes(s, lean):
    cells = s.T * s.FS
    if lean:                                                                               # 579
        return s.T * ((s.F + 63) // 64) * 8 + cells * 2 + s.FS * 16 + 64 + (s.T // 16 + 2) * 6 * 256 * 4
    return (cells * 18 + s.T * s.n * 4 + s.FS * 16 + (s.T // NS_TT + 1) * 2 * s.FS * 8 * 2 +    # 581, 582
            (s.T // 8 + 1) * 2 * s.FS * 8)                                                      # 583


def exact_unit_bytes(s):
    return s.T * s.FS * 32 + s.T * s.n * 8 + s.FS * 16 + (s.T // 32 + 2) * s.FS * 32       # 1860


def parent_workspace(h, s, p):
    """Units per batch, bytes per unit and the exchange buffers that the route's stages ensure, at the parent."""
    unit = exact_unit_bytes(s) if p.pipe == EXACT else unit_bytes(s, p.lean)               # 1863, 587, 1786, 1996
    ub = min(max(1, min(h.ws_budget // unit, 32768)), s.units)                             # 588, 589
    r = None if h.force_nofast else h.reg
    frames, hop = (16, 256) if h.fast_ok else ((r.frames, r.hop) if r else (0, 0))
    abut = (s.nh + 3 + frames - 1) // frames if frames else 0                              # 153
    ex = 0
    if p.pipe == ONEPASS:
        tiles = OP1024.tiles(s.nh)
        ex = ub * (tiles + 2) * OP1024.tile_words * 8 + ub * tiles * 3 * 256 * 8           # 1039, 1647
    elif p.pipe == ONEPASS_REG:
        g = r.op_seam if p.seam else r.op                                                  # 1120
        ex = ub * (g.tiles(s.nh) + 2) * g.tile_words * 8                                   # 1039
        if p.seam:
            ex += ub * abut * 6 * r.hop * 4                                                # 920
    elif p.apply in (A_FAST_K, A_FAST_M) and s.nh > 0 and abut >= 2 and not h.force_noseam:     # 1562, 1567
        ex = ub * abut * 3 * 256 * 8 + (ub * 64 if not h.force_nolean else 0)              # 1578, 1586, 1589
    elif p.apply in (A_REG_K, A_REG_M) and s.nh > 0 and abut >= 2 and not h.force_noseam:  # 941, 944
        ex = ub * abut * 6 * hop * 4                                                       # 920
    return ub, unit, ex


# ---------------------------------------------------------------------------------------------------------------------
# the lattice
# ---------------------------------------------------------------------------------------------------------------------
CAPS_FIELDS = ("variant stationary smooth_mask prop_decrease iir_b nf nt n_movemean ktot fused_ok t_sm2_ok geom reg_sel ftab3 optab "
               "regtab norm64 " + " ".join(OPTS) + " rowgate_mode tile_order ws_budget").split()
SHAPE_FIELDS = "F FS n T nh in_dtype out_dtype units field noise_rows".split()
BASE = dict(variant=S, stationary=1, smooth_mask=1, prop_decrease=1.0, iir_b=0.05, nf=2, nt=4, n_movemean=20, ktot=None, fused_ok=1,
            t_sm2_ok=1, geom=0, reg_sel=0, ftab3=1, optab=1, regtab=1, norm64=1, rowgate_mode=0, tile_order=0, ws_budget=8 << 30,
            T=300, nh=200, in_dtype=F32, out_dtype=F32, units=6, field=0, noise_rows=0, **{o: 0 for o in OPTS})
GEOM_AXIS = [dict(geom=g, reg_sel=r) for g, r in GEOMS]
GATES = [dict(variant=v, stationary=st, prop_decrease=p) for v in (S, T) for st in (1, 0) for p in (1.0, 0.8)]
WIDTHS = ([dict(smooth_mask=0)] +
          [dict(nf=nf, nt=nt) for nf in (1, 2, 8, 9, 24, 25, 30, 31) for nt in (4, 16)] +
          [dict(nf=2, nt=nt) for nt in (1, 8, 9, 12, 13, 17, 20, 21, 24, 25, 26, 34, 37, 38, 40, 41, 96, 97)] +
          [dict(nf=1, nt=nt) for nt in (96, 97)] +       # (ktot = 4 (nt + 1)^2 stays below 65536: the nt <= 96 edge of the bit paths alone)
          [dict(nf=2, nt=4, ktot=k) for k in (65535, 65536)])
SINGLE_OPTS = ([{}] + [{o: 1} for o in OPTS] + [dict(rowgate_mode=1), dict(rowgate_mode=2), dict(tile_order=1), dict(tile_order=2),
                                                dict(fused_ok=0), dict(t_sm2_ok=0), dict(ftab3=0), dict(optab=0), dict(regtab=0),
                                                dict(norm64=0), dict(iir_b=0.0), dict(iir_b=0.2), dict(iir_b=1.0), dict(iir_b=0.01),
                                                dict(n_movemean=21), dict(ws_budget=3 << 20)])
ALL_OPTS = [dict(zip(OPTS, bits)) for bits in itertools.product((0, 1), repeat=len(OPTS))]
S_SHAPES = [dict(nh=nh, T=nh + 6, in_dtype=i, out_dtype=o) for nh in (0, 1, 13, 14, 29, 30, 61, 62, 200) for i in (F32, I16, F64)
            for o in (F32, I16)]
T_SHAPES = [dict(variant=T, T=t, units=rows, field=fl, noise_rows=nr, in_dtype=i)
            for t in (64, 65, 128, 129) for rows in (159, 160) for fl in (0, 1) for nr in (0, 1, rows) for i in (F32, F64)]
LATTICES = {
    "options x gates x geometries x smoothing on / off": (ALL_OPTS, GATES, GEOM_AXIS, [{}, dict(smooth_mask=0)]),
    "widths x gates x geometries x single options": (WIDTHS, GATES, GEOM_AXIS, SINGLE_OPTS),
    "S shapes x gates x geometries x single options": (S_SHAPES, [g for g in GATES if g["variant"] == S], GEOM_AXIS, SINGLE_OPTS),
    "T shapes x gates x geometries x single options": (T_SHAPES, [dict(stationary=st, prop_decrease=p) for st in (1, 0) for p in (1.0, 0.8)],
                                                       GEOM_AXIS, SINGLE_OPTS),
}


def point(*parts):
    d = dict(BASE)
    for part in parts:
        d.update(part)
    if d["ktot"] is None:
        d["ktot"] = (d["nf"] + 1) ** 2 * (d["nt"] + 1) ** 2 if d["smooth_mask"] else 1
    d["n"], d["F"], d["FS"] = GEOMS[(d["geom"], d["reg_sel"])]
    return d


def sampled(n, seed=20260101):
    rnd = random.Random(seed)
    axes = (ALL_OPTS, GATES, GEOM_AXIS, WIDTHS, SINGLE_OPTS, SINGLE_OPTS, S_SHAPES,
            [{k: v for k, v in t.items() if k != "variant"} for t in T_SHAPES])
    for _ in range(n):
        yield point(*(rnd.choice(a) for a in axes))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    assert CXX is not None
    exe = str(tmp_path_factory.mktemp("route_plan") / "route_plan_host")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizer runtimes)
        subprocess.run(base, check=True)
    return exe


def run(prog, points):
    text = "".join(" ".join(repr(d[k]) for k in CAPS_FIELDS + SHAPE_FIELDS) + "\n" for d in points)
    out = subprocess.run([prog], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[int(v) for v in line.split()] for line in out if line]
    assert len(rows) == len(points)
    return rows


FACTS = "keeps has_P has_raw fused fast k16_only rg range".split()
S_FIELDS = "pipe decide ns smooth_stage k16_to_mask apply seam exact_tiled lean f32_copy fast reg".split()
T_FIELDS = "rowgate bits_path to_raw row_fused thresh ns smooths apply fast reg".split()


def check(d, row):
    c = NS(**d)
    h = handle(c)
    it = iter(row)
    got_S = NS(**{k: next(it) for k in S_FIELDS}, facts=NS(**{k: next(it) for k in FACTS}))
    got_T = NS(**{k: next(it) for k in T_FIELDS}, facts=NS(**{k: next(it) for k in FACTS}))
    ub, unit, exchange = next(it), next(it), next(it)

    def same(got, want, fields, who):
        for k in fields:
            assert getattr(got, k) == int(getattr(want, k)), (who, k, getattr(got, k), getattr(want, k), d)
        assert got.facts.keeps == int(want.facts.keeps), (who, "keeps", d)
        if want.facts.keeps:
            for k in FACTS[1:]:
                w = getattr(want.facts, k)
                if w is not None:   # (None: the parent wrote nothing on this route, and no tap could read the field)
                    assert getattr(got.facts, k) == int(w), (who, "facts." + k, getattr(got.facts, k), w, d)

    want_S, want_T = parent_S(h, c), parent_T(h, c)
    same(got_S, want_S, S_FIELDS, "plan_S")
    same(got_T, want_T, T_FIELDS, "plan_T")
    # invariants: one pipeline, one apply stage (none where the gate applies itself); lean routes never touch P, raw, M, seg
    assert 0 <= got_S.pipe <= UNFUSED and A_NONE <= got_S.apply < A_FIELD
    assert (got_S.apply == A_NONE) == (got_S.pipe in (ONEPASS, ONEPASS_REG)), d
    assert (got_T.apply == A_NONE) == bool(got_T.rowgate), d
    if got_S.lean:
        assert got_S.pipe in (EXACT_FUSED, ONEPASS, ONEPASS_REG, BITS3) and got_S.ns == NS_NONE and not got_S.k16_to_mask and \
            not got_S.smooth_stage and got_S.apply in (A_NONE, A_FAST64_K, A_FAST_K), d
    # the workspace figure covers the route's own fields and the exchange buffers its stages ensure
    w_ub, w_unit, w_ex = parent_workspace(h, c, want_S)
    assert (ub, unit) == (w_ub, w_unit), (ub, unit, w_ub, w_unit, d)
    assert ub * unit + exchange >= w_ub * w_unit + w_ex, (exchange, w_ex, d)


@pytest.mark.parametrize("name", list(LATTICES))
def test_lattice(prog, name):
    points = [point(*parts) for parts in itertools.product(*LATTICES[name])]
    for d, row in zip(points, run(prog, points)):
        check(d, row)


def test_sample_of_the_whole_product(prog):
    points = list(sampled(40000))
    for d, row in zip(points, run(prog, points)):
        check(d, row)


def test_one_tuple_on_the_command_line(prog):
    """The benchmark's call: default geometry, stationary, 48 units of 2579 frames, 2348 hops -> the one-pass gate, lean."""
    d = point(dict(T=2579, nh=2348, units=48))
    out = subprocess.run([prog] + [repr(d[k]) for k in CAPS_FIELDS + SHAPE_FIELDS], check=True, capture_output=True, text=True).stdout
    row = [int(v) for v in out.split()]
    check(d, row)
    assert row[0] == ONEPASS and row[8] == 1 and row[S_FIELDS.index("apply")] == A_NONE


def test_every_pipeline_and_apply_stage_is_reached(prog):
    """The lattice is not vacuous: each pipeline, decide kernel, mask form and apply stage occurs in it."""
    points = [point(*parts) for name in LATTICES for parts in itertools.product(*LATTICES[name])][::7]
    rows = run(prog, points)
    assert {r[0] for r in rows} == set(range(7))
    assert {r[1] for r in rows} == set(range(5))
    assert {r[2] for r in rows} == {NS_NONE, NS_SMOOTHED, NS_CHAIN, NS_RAW}
    assert {r[5] for r in rows} == set(range(A_FIELD))
    off = len(S_FIELDS) + len(FACTS)
    assert {r[off + 5] for r in rows} == {NS_NONE, NS_RAW, NS_BOX} and {r[off + 7] for r in rows} == {A_NONE, A_FAST_K, A_FAST_M, A_REG_M, A_OLA_M, A_FIELD}
    assert {r[off + 4] for r in rows} == set(range(4)) and {r[off]for r in rows} == {0, 1}
