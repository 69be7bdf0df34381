"""The host arithmetic of a stream bank (noisereduce_amd/csrc/stream_plan.hpp: st_counters_at, st_layout, st_check_step, st_plan_step,
st_payload_words) on the host.  tests/stream_plan_host.cpp is a stand-alone program around the header (built with the host
compiler, -fsanitize=address,undefined where the compiler has them); it answers commands on stdin.  No GPU, no Python extension.

Everything the program prints is compared with a restatement of the rules as stream.hip's st_push, st_create and st_state_bytes
wrote them BEFORE the header existed (``Parent`` below: the slot keeps td, ts, ta and E and advances them incrementally, as the
parent's StSlot did), and with noisereduce_amd/stream.py's own arithmetic (t_decided / emitted / frames_applied / state_bytes /
state_payload_bytes), over

* (n_fft, W, H) = (256, 200, 80), (512, 400, 160), (1024, 1024, 256) and (256, 201, 67) (odd W, a hop that divides nothing);
* nt 0 / 1 / 4; lookahead 0 / 3; fixed, adaptive and non-stationary banks, plain and exact; 1 and 2 channels;
* blocks of 0, 1 and max_block samples, a block across several hops, a flush with and without a final block, a stream restarted
  after its flush, push / spectrum / feature steps mixed, several slots per step.

The planner states the counters as functions of n; the parent advanced them step by step.  ``test_closed_form_*`` hold the two
equal after every step of random block splits (with the equality of every StUnit member, that is the ground on which StSlot
dropped td / ts / ta / E).  Every rejection of st_check_step is asserted by code and exact text."""
import itertools
import os
import random
import subprocess

import pytest

from tests.test_onepass_plan_host import CXX, ROOT

SRC = os.path.join(ROOT, "tests", "stream_plan_host.cpp")
F32, F64, I16, I32 = 0, 1, 2, 3
FIXED, NONSTAT, ADAPT = 0, 1, 2
E_INVALID, E_STATE = -1, -5
PUSH, SPEC, FEAT, BOTH = 0, 1, 2, 3
WHO = {PUSH: "sg_stream_push", SPEC: "sg_stream_push_spectrum", FEAT: "sg_stream_push_features", BOTH: "sg_stream_push_features"}
ST_OLA, ST_APPEND, ST_CLEAR = 0, 1, 2
FPT, RPT, WS_PREALLOC = 2, 16, 256 << 20
UNBOUNDED = 1 << 60
SIZEOF_UNIT, SIZEOF_TILE, SIZEOF_SPEC = 19 * 8 + 4 * 4, 24, 16

GEOMS = [(256, 200, 80), (512, 400, 160), (1024, 1024, 256), (256, 201, 67)]
KINDS = [(FIXED, 0), (ADAPT, 0), (NONSTAT, 0), (NONSTAT, 3)]


def align256(b):
    return (b + 255) // 256 * 256


def cdiv_trunc(a, b):
    """C's a / b on int64 (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


class Prog:
    def __init__(self, exe):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        out = []
        while True:
            ln = self.p.stdout.readline()
            assert ln, "stream_plan_host ended (exit %r) on: %s" % (self.p.poll(), line)
            ln = ln.rstrip("\n")
            if ln == "end":
                return out
            out.append(ln)

    def close(self):
        self.p.stdin.close()
        assert self.p.wait(timeout=60) == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_host")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", path]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizer runtimes)
        subprocess.run(base, check=True)
    return path


@pytest.fixture()
def prog(exe):
    p = Prog(exe)
    yield p
    p.close()


# ---------------------------------------------------------------------------------------------------------------------
# the parent's rules (stream.hip of the commit before stream_plan.hpp: st_tdec, st_bank_frames, st_state_bytes, st_create, st_push)
# ---------------------------------------------------------------------------------------------------------------------
class Slot:
    def __init__(self, has_thr):
        self.n, self.td, self.ts, self.ta, self.E, self.par, self.has_thr = 0, -1, -1, -1, 0, 0, has_thr


class Parent:
    """A bank as the parent's StBank held it on the host."""

    def __init__(self, n_fft, W, H, nt, L, C, kind, exact, n_slots, max_block, M, has_thr):
        self.n_fft, self.W, self.H, self.nt, self.C, self.kind, self.exact = n_fft, W, H, nt, C, kind, exact
        self.ns, self.ad = kind == NONSTAT, kind == ADAPT
        self.L = L if self.ns else 0
        self.F = n_fft // 2 + 1
        self.FS = (self.F + 15) // 16 * 16
        self.wpr = (self.F + 63) // 64
        self.n_slots, self.max_block, self.M = n_slots, max_block, M
        self.RC = W + (nt + self.L + 1) * H
        self.slots = [Slot(has_thr) for _ in range(n_slots)]

    def line(self, has_thr):
        return "bank %d %d %d %d %d %d %d %d %d %d %d %d" % (self.n_fft, self.W, self.H, self.nt, self.L, self.C, self.kind,
                                                            self.exact, self.n_slots, self.max_block, self.M, has_thr)

    def tdec(self, n):
        a = n + self.W // 2 - self.W
        return -1 if a < 0 else a // self.H

    def bank_frames(self, n):
        return max(0, self.tdec(n) - self.nt - self.L + 1)

    def layout(self):
        """st_create's take(...) list and st_state_bytes, as the parent spelt them (twice)."""
        nu = self.n_slots * self.C
        mf = (self.max_block + self.W // 2) // self.H + 3
        RB = 2 * self.nt + 1 + self.L + mf
        RF = self.L + 1 + mf
        FS, ex = self.FS, self.exact
        y = dict(ring=nu * self.RC * 8, carry=nu * 2 * self.W * 8, fst=0, fa=0, mk=0, rmax=0, bits=0, nst=0, thr=0, T2=0, stage=0)
        if self.ns:
            y.update(fst=nu * FS * 8, fa=nu * RF * 2 * FS * 8, mk=nu * RB * FS * (8 if ex else 4))
        else:
            y.update(rmax=nu * FS * 8, bits=nu * RB * self.wpr * 8)
            if self.ad:
                y.update(nst=nu * 3 * FS * 8)
            else:
                y.update(thr=self.n_slots * FS * 8, T2=self.n_slots * FS * 8, stage=FS * 8)
        y["slot_list"] = self.n_slots * 4
        y["tabs"] = align256(nu * SIZEOF_UNIT) + align256(nu * 16 * SIZEOF_TILE) + align256(nu * SIZEOF_SPEC)
        per_unit = align256((mf + 2 * self.nt) * FS * (8 if ex and self.ns else 4)) + align256(mf * self.n_fft * (8 if ex else 4))
        y["ws"] = min(WS_PREALLOC, nu * per_unit)
        # st_state_bytes
        per = self.RC * 8 + 2 * self.W * 8
        if self.ns:
            per += FS * 8 + (self.L + 1 + mf) * 2 * FS * 8 + RB * FS * (8 if ex else 4)
        else:
            per += FS * 8 + RB * self.wpr * 8
        if self.ad:
            per += 3 * FS * 8
        return [self.RC, RB, RF, mf] + [y[k] for k in "ring carry fst fa mk rmax bits nst thr T2 stage slot_list tabs ws".split()] + [
            nu * per, min(RB, 2 ** 31 - 1), 0 if self.ns else nu * min(RB, 2 ** 31 - 1) * self.wpr * 8]   # (take(bits): the clamped b->RB)

    def check(self, mode, in_dtype, out_dtype, recs, so=None, fo=None):
        """st_push's checks, in its order.  recs: dicts; so / fo: dicts with dtype, buf, recs (bool), mask and fo's switches."""
        who, W, C = WHO[mode], self.W, self.C
        h = W // 2

        def dtype_ok(d):
            return d in (F32, F64) or (self.exact and d in (I16, I32))
        if not dtype_ok(in_dtype) or not dtype_ok(out_dtype):
            return E_INVALID, who + ": bad argument (float32 / float64 buffers)"
        if so and (so["dtype"] not in (F32, F64) or (len(recs) > 0 and (not so["buf"] or not so["recs"]))):
            return E_INVALID, who + ": bad argument (spec_dev and spec_recs are needed; spec_dtype is SG_F32 or SG_F64)"
        if fo:
            if so:
                return E_INVALID, who + ": bad argument (a step stores the spectrum or the features)"
            if fo["dtype"] not in (F32, F64) or (len(recs) > 0 and (not fo["buf"] or not fo["recs"])):
                return E_INVALID, who + ": bad argument (feat_dev and feat_recs are needed; feat_dtype is SG_F32 or SG_F64)"
            if fo["power"] not in (1, 2):
                return E_INVALID, who + ": power must be 1 or 2"
            if fo["eps"] != fo["eps"]:
                return E_INVALID, who + ": eps is NaN"
            if not (0.0 <= fo["scale"] <= 1.79769313486231570e308):
                return E_INVALID, who + ": scale must be finite and not negative (0: the bank's 1 / sum(window))"
            if not self.M:
                return E_INVALID, who + ": no filterbank set (sg_stream_set_filterbank)"
        seen = set()
        for i, r in enumerate(recs):
            s = r["slot"]
            if s < 0 or s >= self.n_slots:
                return E_INVALID, "%s: record %d: unknown slot %d (the bank has %d)" % (who, i, s, self.n_slots)
            if s in seen:
                return E_INVALID, "%s: slot %d appears twice in one step" % (who, s)
            seen.add(s)
            if r["n"] < 0 or r["n"] > self.max_block:
                return E_INVALID, "%s: slot %d: block of %d samples (max_block is %d)" % (who, s, r["n"], self.max_block)
            if r["in_off"] < 0 or r["out_off"] < 0 or (C > 1 and (r["in_stride"] < r["n"] or r["out_stride"] < 0)):
                return E_INVALID, "%s: slot %d: bad offsets / strides" % (who, s)
            S = self.slots[s]
            if not S.has_thr:
                return E_STATE, "%s: slot %d has no noise threshold yet" % (who, s)
            if r["flush"] and S.n + r["n"] < W:
                return E_INVALID, "%s: slot %d: a stream of %d samples is shorter than win_length=%d" % (who, s, S.n + r["n"], W)
            n1 = S.n + r["n"]
            ta1 = cdiv_trunc(n1 + 2 * h - W, self.H) if r["flush"] else max(S.ta, self.bank_frames(n1) - 1)
            if so:
                if r["spec_off"] < 0 or (so["mask"] and r["smask_off"] < 0) or (C > 1 and r["sstride"] < (ta1 - S.ta) * self.F):
                    return E_INVALID, "%s: slot %d: bad spectrum offsets / stride" % (who, s)
            if fo:
                if (r["feat_off"] < 0 or (fo["mask"] and r["fmask_off"] < 0) or
                        (C > 1 and (r["feat_stride"] < (ta1 - S.ta) * self.M or (fo["mask"] and r["fmask_stride"] < (ta1 - S.ta) * self.F)))):
                    return E_INVALID, "%s: slot %d: bad feature offsets / strides" % (who, s)
        return None

    def frames(self, r):
        """Frames a record reports (what a caller sizes its spectrum / feature rows with)."""
        S = self.slots[r["slot"]]
        n1 = S.n + r["n"]
        return (cdiv_trunc(n1 + 2 * (self.W // 2) - self.W, self.H) if r["flush"] else max(S.ta, self.bank_frames(n1) - 1)) - S.ta

    def plan(self, mode, recs):
        """st_push's plan: the incremental counters, the unit table, the four tile lists; commits the slots as st_push does."""
        W, H, nt, L, C = self.W, self.H, self.nt, self.L, self.C
        h = W // 2
        units, third, after = [], [], []
        mrows = sframes = 0
        for r in recs:
            S = self.slots[r["slot"]]
            U = dict(n0=S.n, n1=S.n + r["n"], td0=S.td, ts0=S.ts, ta0=S.ta, E0=S.E, flush=1 if r["flush"] else 0, r0=0, r1=0)
            if r["flush"]:
                T = cdiv_trunc(U["n1"] + 2 * h - W, H) + 1
                U.update(Tend=T, Lout=(T - 1) * H + W - 2 * h, td1=T - 1, ts1=T - 1, ta1=T - 1, E1=U["n1"])
            else:
                td1 = max(U["td0"], self.tdec(U["n1"]))
                ts1 = max(U["ts0"], td1 - L)
                ta1 = max(U["ta0"], ts1 - nt)
                U.update(Tend=UNBOUNDED, Lout=UNBOUNDED, td1=td1, ts1=ts1, ta1=ta1, E1=max(0, (ta1 + 1) * H - h))
            U["cov0"] = U["ta0"] * H - h + W if U["ta0"] >= 0 else 0
            if U["ta1"] > U["ta0"]:
                U["r0"] = max(0, U["ta0"] + 1 - nt)
                U["r1"] = min(U["Tend"], U["ta1"] + nt + 1)
            U["slot"], U["par"] = r["slot"], S.par
            for ch in range(C):
                V = dict(U, state=r["slot"] * C + ch, in_off=r["in_off"] + ch * r["in_stride"], out_off=r["out_off"] + ch * r["out_stride"],
                         mrow=mrows, srow=sframes)
                mrows += V["r1"] - V["r0"]
                sframes += V["ta1"] - V["ta0"]
                units.append(V)
                if mode == SPEC:
                    third.append((r["spec_off"] + ch * r["sstride"], r["smask_off"] + ch * r["sstride"]))
                if mode == FEAT:
                    third.append((r["feat_off"] + ch * r["feat_stride"], r["fmask_off"] + ch * r["fmask_stride"]))
            N = Slot(True)
            if not r["flush"]:
                N.n, N.td, N.ts, N.ta, N.E = U["n1"], U["td1"], U["ts1"], U["ta1"], U["E1"]
                N.par = S.par ^ 1 if U["ta1"] > U["ta0"] else S.par
            after.append(N)
        tiles = []

        def ranges(u, lo, hi, step, kind=0):
            a = lo
            while a < hi:
                tiles.append((u, kind, a, min(hi, a + step)))
                a += step
        t_dec = len(tiles)
        for u, U in enumerate(units):
            if U["td1"] > U["td0"] or U["ts1"] > U["ts0"]:
                tiles.append((u, 0, U["td0"] + 1, U["td1"] + 1))
        t_fs = len(tiles)
        for u, U in enumerate(units):
            ranges(u, U["r0"], U["r1"], RPT)
        t_ap = len(tiles)
        for u, U in enumerate(units):
            ranges(u, U["ta0"] + 1, U["ta1"] + 1, FPT)
        t_fin = len(tiles)
        for u, U in enumerate(units):
            if U["ta1"] > U["ta0"] or U["flush"]:
                ranges(u, U["E0"], U["E1"] if U["flush"] else max(U["E1"], U["ta1"] * H - h + W), 256, ST_OLA)
            if not U["flush"]:
                ranges(u, max(U["n0"], U["n1"] - self.RC), U["n1"], 256, ST_APPEND)
            elif not self.ns:
                tiles.append((u, ST_CLEAR, 0, 0))
        head = [mrows, sframes, t_dec, t_fs - t_dec, t_fs, t_ap - t_fs, t_ap, t_fin - t_ap, t_fin, len(tiles) - t_fin]
        for r, N in zip(recs, after):
            self.slots[r["slot"]] = N
        return head, units, third, tiles, after


UNIT_FIELDS = "in_off out_off n0 n1 td0 td1 ts0 ts1 ta0 ta1 Tend Lout E0 E1 cov0 r0 r1 mrow srow state slot par flush".split()


def rec(slot, flush, n, C=1, **kw):
    r = dict(slot=slot, flush=flush, n=n, in_off=1000 * slot + 3, in_stride=n + 5, out_off=2000 * slot + 1, out_stride=5000,
             spec_off=10 ** 6 * slot, smask_off=10 ** 6 * slot + 11, sstride=0, feat_off=10 ** 5 * slot, feat_stride=0,
             fmask_off=10 ** 5 * slot + 7, fmask_stride=0)
    r.update(kw)
    return r


def step_line(mode, in_dtype, out_dtype, recs, so=None, fo=None):
    parts = ["step", mode, in_dtype, out_dtype, len(recs)]
    if mode in (SPEC, BOTH):
        parts += [so["dtype"], int(so["buf"]), int(so["recs"]), int(so["mask"])]
    if mode in (FEAT, BOTH):
        parts += [fo["dtype"], int(fo["buf"]), int(fo["recs"]), int(fo["mask"]), fo["power"], fo["take_log"], repr(fo["eps"]), repr(fo["scale"])]
    for r in recs:
        parts += [r["slot"], int(r["flush"]), r["n"], r["in_off"], r["in_stride"], r["out_off"], r["out_stride"]]
        if mode in (SPEC, BOTH):
            parts += [r["spec_off"], r["smask_off"], r["sstride"]]
        if mode in (FEAT, BOTH):
            parts += [r["feat_off"], r["feat_stride"], r["fmask_off"], r["fmask_stride"]]
    return " ".join(str(x) for x in parts)


SO = dict(dtype=F32, buf=True, recs=True, mask=True)
FO = dict(dtype=F64, buf=True, recs=True, mask=True, power=2, take_log=1, eps=1e-6, scale=0.0)


def run_step(prog, bank, mode, recs, in_dtype=F32, out_dtype=F32, so=None, fo=None):
    """One step through the program and through the parent's rules; every printed value compared.  Returns the verdict."""
    so = so if so is not None else (dict(SO) if mode in (SPEC, BOTH) else None)
    fo = fo if fo is not None else (dict(FO) if mode in (FEAT, BOTH) else None)
    for r in recs:   # rows wide enough for what the record reports, as a caller sizes them
        if 0 <= r["slot"] < bank.n_slots and r.get("auto", True):
            fr = max(0, bank.frames(r))
            r["sstride"] = r["sstride"] or fr * bank.F + 3
            r["feat_stride"] = r["feat_stride"] or fr * bank.M + 1
            r["fmask_stride"] = r["fmask_stride"] or fr * bank.F + 2
    got = prog.ask(step_line(mode, in_dtype, out_dtype, recs, so, fo))
    bad = bank.check(mode, in_dtype, out_dtype, recs, so, fo)
    if bad:
        assert got == ["err %d %s" % bad]
        return bad
    head, units, third, tiles, after = bank.plan(mode, recs)
    want = ["plan " + " ".join(map(str, head))]
    want += ["unit " + " ".join(str(U[k]) for k in UNIT_FIELDS) for U in units]
    want += ["third %d %d" % t for t in third]
    want += ["tile %d %d %d %d" % t for t in tiles]
    want += ["slot %d %d %d %d" % (r["slot"], N.n, N.par, 1) for r, N in zip(recs, after)]
    assert got == want
    return None


def closed_form(bank, n):
    """(td, ts, ta, E) of n samples from stream.py's own functions."""
    from noisereduce_amd import stream
    td = stream.t_decided(n, bank.W, bank.H)
    ta = stream.frames_applied(n, bank.W, bank.H, bank.nt + bank.L) - 1
    return td, max(-1, td - bank.L), ta, stream.emitted(n, bank.W, bank.H, bank.nt + bank.L)


def assert_closed_form(prog, bank):
    for S in bank.slots:
        want = closed_form(bank, S.n)
        assert (S.td, S.ts, S.ta, S.E) == want, (S.n, vars(bank))
        assert prog.ask("counters %d" % S.n) == ["counters %d %d %d %d" % want]


LATTICE = [(g, nt, k, ex, C) for g in GEOMS for nt in (0, 1, 4) for k in KINDS for ex in (0, 1) for C in (1, 2)]


def make_bank(prog, g, nt, kind_L, exact, C, n_slots=3, max_block=None, M=40, has_thr=1):
    n_fft, W, H = g
    kind, L = kind_L
    bank = Parent(n_fft, W, H, nt, L, C, kind, exact, n_slots, max_block or 4 * H + 5, M, bool(has_thr))
    got = prog.ask(bank.line(has_thr))
    return bank, [int(x) for x in got[0].split()[1:]]


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: "%dx%dx%d" % g)
def test_layout_and_payload(prog, g):
    """StLayout: every buffer as st_create's take(...) list had it, the sum as st_state_bytes had it and as stream.state_bytes has
    it; st_payload_words x 8 == stream.state_payload_bytes for n across every counter's steps."""
    from noisereduce_amd import stream
    n_fft, W, H = g
    for _, nt, kL, ex, C in (q for q in LATTICE if q[0] == g):
        for n_slots, mb in ((1, 1), (3, 4 * H + 5), (2, 512), (5, 100000), (1, 2 ** 40)):   # (the last: RB beyond INT32_MAX)
            bank, got = make_bank(prog, g, nt, kL, ex, C, n_slots=n_slots, max_block=mb)
            want = bank.layout()
            assert got == want
            assert got[18] == sum(got[4:12])
            assert got[20] == got[10] or (got[1] > 2 ** 31 - 1 and got[20] < got[10])
            assert got[18] == stream.state_bytes(n_slots * C, n_fft, W, H, nt, bank.L, mb, not bank.ns, noise_from_stream=bank.ad,
                                                 exact=bool(ex))
        kind = ("fixed", "nonstationary", "adaptive")[kL[0]]
        for n in sorted(set([0, 1, W // 2 - 1, W // 2, W // 2 + 1, W - 1, W, W + 1, bank.RC - 1, bank.RC, bank.RC + 1] +
                            [W // 2 + k * H + d for k in range(0, nt + kL[1] + 8) for d in (-1, 0, 1)] + [10 ** 6 + 7, 2 ** 33 + 5])):
            assert prog.ask("payload %d" % n) == ["payload %d" % stream.state_payload_bytes(n, n_fft, W, H, nt, bank.L, C, kind, bool(ex))]
            assert prog.ask("counters %d" % n) == ["counters %d %d %d %d" % closed_form(bank, n)]


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: "%dx%dx%d" % g)
def test_steps_equal_the_parents_plan(prog, g):
    """A fixed scenario per lattice point: every block length that takes another path, every kind of step, several slots per step."""
    n_fft, W, H = g
    for _, nt, kL, ex, C in (q for q in LATTICE if q[0] == g):
        bank, _ = make_bank(prog, g, nt, kL, ex, C)
        MB = bank.max_block
        dt = (I16, I32) if ex else (F32, F64)
        scenario = [
            (PUSH, [rec(0, 0, 0), rec(1, 0, 1)]),                              # an empty block and one sample
            (SPEC, [rec(0, 0, MB), rec(1, 0, 1), rec(2, 0, MB)]),             # exactly max_block
            (FEAT, [rec(0, 0, 3 * H + 1), rec(2, 0, 0)]),                     # across several hops
            (PUSH, [rec(1, 0, MB), rec(0, 0, MB)]),
            (SPEC, [rec(2, 0, H - 1), rec(1, 0, H), rec(0, 0, H + 1)]),
            (FEAT, [rec(1, 0, MB), rec(2, 0, MB)]),
            (PUSH, [rec(0, 0, 0), rec(1, 0, 0), rec(2, 0, 0)]),               # nothing new anywhere
            (FEAT, [rec(0, 1, 7), rec(1, 0, 2 * H)]),                         # a flush with a final block
            (SPEC, [rec(1, 1, 0), rec(0, 0, 1)]),                             # a flush without one; slot 0 starts again
            (PUSH, [rec(0, 0, MB), rec(2, 1, MB)]),
            (SPEC, [rec(0, 1, MB)]),                                          # the restarted stream, flushed with a full block
            (PUSH, []),                                                       # a step without records
        ]
        for mode, recs in scenario:
            for r in recs:
                r["in_stride"] = r["n"] + 5
            assert run_step(prog, bank, mode, recs, in_dtype=dt[0], out_dtype=dt[1]) is None
            assert_closed_form(prog, bank)


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_equals_incremental_for_random_splits(prog, seed):
    """One stream per slot, split at random (blocks 0 .. max_block, biased to the short ones and to hop multiples): after every step
    the incrementally advanced counters of the parent are the closed form at n, and the next step's StUnit (planned from n alone)
    equals the parent's (planned from the stored counters).  Ends with a flush and a second stream on the same slot."""
    rng = random.Random(1000 + seed)
    for g, nt, kL, C in itertools.product(GEOMS, (0, 1, 4), KINDS, (1, 2)):
        if rng.random() < 0.5:
            continue
        H = g[2]
        MB = rng.choice((1, H - 1, H, 2 * H + 3, 7 * H + 1))
        bank, _ = make_bank(prog, g, nt, kL, rng.randrange(2), C, n_slots=2, max_block=MB)
        for _ in range(40):
            recs = []
            for s in rng.sample((0, 1), rng.choice((1, 2))):
                n = rng.choice((0, 1, MB, rng.randrange(MB + 1), min(MB, H), min(MB, rng.randrange(1, 4) * H)))
                flush = bank.slots[s].n + n >= g[1] and rng.random() < 0.08
                recs.append(rec(s, int(flush), n))
            assert run_step(prog, bank, rng.choice((PUSH, SPEC, FEAT)), recs) is None
            assert_closed_form(prog, bank)


def test_every_rejection_by_code_and_text(prog):
    g = GEOMS[0]
    n_fft, W, H = g
    F = n_fft // 2 + 1

    def refused(bank, mode, recs, code, text, **kw):
        before = [vars(S).copy() for S in bank.slots]
        assert run_step(prog, bank, mode, recs, **kw) == (code, text)   # (program == parent inside; parent == the literal here)
        assert [vars(S) for S in bank.slots] == before
    # ---- dtype per bank kind
    for kL in KINDS:
        bank, _ = make_bank(prog, g, 1, kL, 0, 1)
        for dts in ((I16, F32), (F32, I32), (4, F32), (F32, -1)):
            refused(bank, PUSH, [rec(0, 0, 5)], E_INVALID, "sg_stream_push: bad argument (float32 / float64 buffers)", in_dtype=dts[0], out_dtype=dts[1])
        bank, _ = make_bank(prog, g, 1, kL, 1, 1)
        assert run_step(prog, bank, PUSH, [rec(0, 0, 5)], in_dtype=I16, out_dtype=I32) is None
        refused(bank, SPEC, [rec(0, 0, 5)], E_INVALID, "sg_stream_push_spectrum: bad argument (float32 / float64 buffers)", in_dtype=4, out_dtype=F32)
        # (the dtype comes before the records: an unknown slot does not hide it)
        refused(bank, FEAT, [rec(9, 0, 5)], E_INVALID, "sg_stream_push_features: bad argument (float32 / float64 buffers)", in_dtype=F32, out_dtype=7)
    bank, _ = make_bank(prog, g, 1, KINDS[0], 0, 2)
    MB = bank.max_block
    # ---- spectrum / feature buffers
    spec_msg = "sg_stream_push_spectrum: bad argument (spec_dev and spec_recs are needed; spec_dtype is SG_F32 or SG_F64)"
    refused(bank, SPEC, [rec(0, 0, 5)], E_INVALID, spec_msg, so=dict(SO, buf=False))
    refused(bank, SPEC, [rec(0, 0, 5)], E_INVALID, spec_msg, so=dict(SO, recs=False))
    refused(bank, SPEC, [rec(0, 0, 5)], E_INVALID, spec_msg, so=dict(SO, dtype=I16))
    refused(bank, SPEC, [], E_INVALID, spec_msg, so=dict(SO, dtype=I32, buf=False, recs=False))
    assert run_step(prog, bank, SPEC, [], so=dict(SO, buf=False, recs=False)) is None     # no records: no buffers needed
    feat_msg = "sg_stream_push_features: bad argument (feat_dev and feat_recs are needed; feat_dtype is SG_F32 or SG_F64)"
    refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID, feat_msg, fo=dict(FO, buf=False))
    refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID, feat_msg, fo=dict(FO, recs=False))
    refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID, feat_msg, fo=dict(FO, dtype=I16))
    refused(bank, BOTH, [rec(0, 0, 5)], E_INVALID, "sg_stream_push_features: bad argument (a step stores the spectrum or the features)")
    # ---- power, eps, scale, filterbank
    for p in (0, 3, -1):
        refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID, "sg_stream_push_features: power must be 1 or 2", fo=dict(FO, power=p))
    refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID, "sg_stream_push_features: eps is NaN", fo=dict(FO, eps=float("nan")))
    for sc in (-1e-300, float("inf"), float("nan")):
        refused(bank, FEAT, [rec(0, 0, 5)], E_INVALID,
                "sg_stream_push_features: scale must be finite and not negative (0: the bank's 1 / sum(window))", fo=dict(FO, scale=sc))
    assert run_step(prog, bank, FEAT, [rec(0, 0, 5)], fo=dict(FO, power=1, eps=float("-inf"), scale=1.7e308)) is None
    nofb, _ = make_bank(prog, g, 1, KINDS[0], 0, 2, M=0)
    refused(nofb, FEAT, [rec(0, 0, 5)], E_INVALID, "sg_stream_push_features: no filterbank set (sg_stream_set_filterbank)")
    assert run_step(prog, nofb, SPEC, [rec(0, 0, 5)]) is None
    bank, _ = make_bank(prog, g, 1, KINDS[0], 0, 2)
    # ---- records
    refused(bank, PUSH, [rec(0, 0, 5), rec(3, 0, 5)], E_INVALID, "sg_stream_push: record 1: unknown slot 3 (the bank has 3)")
    refused(bank, SPEC, [rec(-1, 0, 5)], E_INVALID, "sg_stream_push_spectrum: record 0: unknown slot -1 (the bank has 3)")
    refused(bank, FEAT, [rec(1, 0, 5), rec(2, 0, 5), rec(1, 0, 0)], E_INVALID, "sg_stream_push_features: slot 1 appears twice in one step")
    refused(bank, PUSH, [rec(2, 0, MB + 1)], E_INVALID, "sg_stream_push: slot 2: block of %d samples (max_block is %d)" % (MB + 1, MB))
    refused(bank, PUSH, [rec(2, 0, -1)], E_INVALID, "sg_stream_push: slot 2: block of -1 samples (max_block is %d)" % MB)
    bad = "sg_stream_push: slot 1: bad offsets / strides"
    refused(bank, PUSH, [rec(1, 0, 5, in_off=-1)], E_INVALID, bad)
    refused(bank, PUSH, [rec(1, 0, 5, out_off=-1)], E_INVALID, bad)
    refused(bank, PUSH, [rec(1, 0, 5, in_stride=4)], E_INVALID, bad)
    refused(bank, PUSH, [rec(1, 0, 5, out_stride=-1)], E_INVALID, bad)
    refused(bank, PUSH, [rec(9, 0, MB + 1)], E_INVALID, "sg_stream_push: record 0: unknown slot 9 (the bank has 3)")   # the order
    mono, _ = make_bank(prog, g, 1, KINDS[0], 0, 1)
    assert run_step(prog, mono, PUSH, [rec(1, 0, 5, in_stride=0, out_stride=-3)]) is None   # one channel: the strides are not read
    # ---- no threshold: a fixed bank only
    cold, _ = make_bank(prog, g, 1, KINDS[0], 0, 2, has_thr=0)
    refused(cold, PUSH, [rec(0, 0, 5)], E_STATE, "sg_stream_push: slot 0 has no noise threshold yet")
    prog.ask("thr 0 1")
    cold.slots[0].has_thr = True
    assert run_step(prog, cold, PUSH, [rec(0, 0, 5)]) is None
    refused(cold, SPEC, [rec(0, 0, 5), rec(2, 0, 5)], E_STATE, "sg_stream_push_spectrum: slot 2 has no noise threshold yet")
    # ---- a flush of a stream shorter than win_length  (the program holds one bank at a time: a fresh one from here on)
    bank, _ = make_bank(prog, g, 1, KINDS[0], 0, 2)
    refused(bank, PUSH, [rec(0, 1, 0)], E_INVALID, "sg_stream_push: slot 0: a stream of 0 samples is shorter than win_length=200")
    assert run_step(prog, bank, PUSH, [rec(0, 0, W - 6)]) is None
    refused(bank, FEAT, [rec(0, 1, 5)], E_INVALID, "sg_stream_push_features: slot 0: a stream of 199 samples is shorter than win_length=200")
    assert run_step(prog, bank, FEAT, [rec(0, 1, 6)]) is None
    # ---- spectrum / feature rows of a 2-channel bank: one element short of the frames the record reports
    assert run_step(prog, bank, PUSH, [rec(1, 0, MB)]) is None
    fr = bank.frames(rec(1, 0, MB))
    assert fr >= 2
    smsg = "sg_stream_push_spectrum: slot 1: bad spectrum offsets / stride"
    refused(bank, SPEC, [rec(1, 0, MB, sstride=fr * F - 1)], E_INVALID, smsg)
    refused(bank, SPEC, [rec(1, 0, MB, spec_off=-1)], E_INVALID, smsg)
    refused(bank, SPEC, [rec(1, 0, MB, smask_off=-1)], E_INVALID, smsg)
    assert run_step(prog, bank, SPEC, [rec(1, 0, 0, smask_off=-1)], so=dict(SO, mask=False)) is None   # no mask buffer: offset ignored
    fmsg = "sg_stream_push_features: slot 1: bad feature offsets / strides"
    fr = bank.frames(rec(1, 0, MB))
    refused(bank, FEAT, [rec(1, 0, MB, feat_stride=fr * bank.M - 1)], E_INVALID, fmsg)
    refused(bank, FEAT, [rec(1, 0, MB, fmask_stride=fr * F - 1)], E_INVALID, fmsg)
    refused(bank, FEAT, [rec(1, 0, MB, feat_off=-1)], E_INVALID, fmsg)
    refused(bank, FEAT, [rec(1, 0, MB, fmask_off=-1)], E_INVALID, fmsg)
    assert run_step(prog, bank, FEAT, [rec(1, 0, MB, feat_stride=fr * bank.M, fmask_stride=1)], fo=dict(FO, mask=False)) is None
    # ... and of a flush, whose frames are the stream's remaining ones
    fr = bank.frames(rec(1, 1, 3))
    assert fr > bank.frames(rec(1, 0, 3))
    refused(bank, SPEC, [rec(1, 1, 3, sstride=fr * F - 1)], E_INVALID, smsg)
    assert run_step(prog, bank, SPEC, [rec(1, 1, 3, sstride=fr * F)]) is None
    assert_closed_form(prog, bank)
