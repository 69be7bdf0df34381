"""The common tail of the register geometries' kernels (fastpath.hpp: store_partial_hop, finish_hop) -- k_gate_onepass512 / 256 /
2048 and k_apply_fast512 / 256 / 2048 -- on a recording of two tiles plus five hops, (2 NF + 5) hop samples, float32:

* as ONE unit without padding: the first and last hops read frames outside [0, T) (the normalisation sums the squared windows
  of the frames that exist), every other hop takes the precomputed 1 / envelope and the aligned float4 store;
* as THREE units (chunk_size a multiple of 4, padding = hop + 2) read back through get_traces(3, N - 2): every destination is
  odd, so every hop falls through from the float4 store to the per-sample path, and the unit seams cut through hops.

Routes: the one-pass gate on abutting tiles (default: the three hops that straddle two tiles leave as partial sums), the same on
overlapping tiles (SG_OPT_FORCE_NOSEAM; n_fft = 2048 has abutting tiles only and is left out) and decide + smooth + apply
(SG_OPT_FORCE_SPLIT).  Per route: the kernels the route names ran and the others did not (the seam kernel on the default route,
not under SG_OPT_FORCE_NOSEAM), every hop block of every unit within FACTOR x the float32 budget of the float64 oracle
(tests/parity_budget.py), decision bits equal to the oracle's inside debug_range(), a second call on the same handle bitwise
equal.

int16: api.hip routes integer samples to these kernels under SG_OPT_FAST_INTEGER (the output map's dtype reaches store_sample);
DESIGN.md section 2 sets the bar: at most 1 LSB from the truncated float64 result.

The conditions the inputs meet on the oracle's side alone (no GPU): test_the_oracle_side_is_sound."""
import functools

import numpy as np
import pytest

from tests import parity_budget as PB

NF = {256: 64, 512: 32, 2048: 8}      # frames per tile
SEED = {256: 11, 512: 12, 2048: 13}
LAYOUTS = ("one_unit", "three_units")


def _geometry(n_fft, layout):
    H = n_fft // 4
    N = (2 * NF[n_fft] + 5) * H        # 8 512, 8 832, 10 752
    if layout == "one_unit":
        return dict(N=N, H=H, cs=N, pad=0, sub=None)
    cs = 4 * (-(-N // 12))             # three chunks, every chunk start a multiple of 4
    assert 2 * cs < N <= 3 * cs
    return dict(N=N, H=H, cs=cs, pad=H + 2, sub=(3, N - 2))


@functools.lru_cache(maxsize=None)
def _case(n_fft, layout):
    """Input, keyword arguments and the float64 oracle's units (computed once, shared by the routes; nobody writes to them)."""
    geo = _geometry(n_fft, layout)
    y = PB.signals.dc_nyquist(geo["N"], PB.SR, SEED[n_fft])
    kw = dict(stationary=True, n_fft=n_fft, chunk_size=geo["cs"], padding=geo["pad"], prop_decrease=1.0)
    out, units = PB.oracle_units(y.astype(np.float64), PB.SR, **kw)
    return geo, y, kw, out, units


def _make_sg(y, kw):
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    return SpectralGateStationary(y=y, sr=PB.SR, y_noise=None, n_std_thresh_stationary=1.5, clip_noise_stationary=True,
                                  prop_decrease=kw["prop_decrease"], chunk_size=kw["chunk_size"], padding=kw["padding"],
                                  n_fft=kw["n_fft"], win_length=None, hop_length=None, time_constant_s=2.0,
                                  freq_mask_smooth_hz=500, time_mask_smooth_ms=50, tmp_folder=None, use_tqdm=False, n_jobs=1)


def _routes(n_fft):
    """(name, options, kernels that must have run, kernels that must not).  The seam kernel k_ola_seam is booked under the
    k_apply_fast stage: on the one-pass routes that stage is there exactly when the straddling hops left as partial sums
    (store_partial_hop) and k_ola_seam finished them."""
    from noisereduce_amd import _ffi
    routes = [("default", [], {"k_gate_onepass", "k_apply_fast"}, {"k_decide_fast"}),
              ("force_split", [(_ffi.SG_OPT_FORCE_SPLIT, 1)], {"k_decide_fast", "k_apply_fast"}, {"k_gate_onepass"})]
    if n_fft != 2048:
        routes.append(("force_noseam", [(_ffi.SG_OPT_FORCE_NOSEAM, 1)], {"k_gate_onepass"}, {"k_apply_fast", "k_decide_fast"}))
    return routes


def _cut(u, sub):
    """The part of a unit that get_traces(*sub) returns: (unit restricted to it, where it lies in the returned array)."""
    s0, e0 = u["dst"]
    a, b = (s0, e0) if sub is None else (max(s0, sub[0]), min(e0, sub[1]))
    k0 = u["keep"][0]
    cut = dict(u, want=u["want"][a - s0:b - s0], keep=(k0 + a - s0, k0 + b - s0), dst=(a, b))
    off = 0 if sub is None else sub[0]
    return cut, (a - off, b - off)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_fft", sorted(NF))
def test_the_oracle_side_is_sound(n_fft, layout):
    """No cell within 1e-7 dB of its threshold, a mask that passes between 1 % and 99 % of the cells, and the hops the layouts
    are there for: frames outside [0, T) under the first and last kept hop of the single unit, none but odd destinations and
    three units in the other."""
    geo, y, kw, out, units = _case(n_fft, layout)
    H = geo["H"]
    assert len(units) == (1 if layout == "one_unit" else 3)
    for u in units:
        assert PB.nearest_margin_db(u) > 1e-7
        assert 0.01 < float(np.mean(u["raw"])) < 0.99
        T, padL = u["raw"].shape[1], n_fft // 2
        k0, k1 = u["keep"]
        h0, h1 = (k0 + padL) // H, (k1 - 1 + padL) // H      # first and last hop block (frame coordinates) of the kept range
        if layout == "one_unit":
            assert h0 - 3 < 0 and h1 >= T and h0 + 3 < h1 - 3  # both edges sum the squared windows, the hops between do not
            assert (u["dst"][0] + h0 * H - padL - k0) % 4 == 0
        else:
            cut, (a, _) = _cut(u, geo["sub"])
            # sample p of the unit lands at returned index a + (p - keep[0]): hop starts are multiples of 4 in p + padL
            assert (a - cut["keep"][0] - padL) % 2 == 1
    if layout == "three_units":
        assert geo["sub"][0] % 2 == 1 and geo["sub"][1] - geo["sub"][0] > geo["cs"] and geo["pad"] % 4 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_fft", sorted(NF))
def test_the_tail_of_the_register_kernels(n_fft, layout):
    geo, y, kw, out, units = _case(n_fft, layout)
    sub = geo["sub"]
    args = {} if sub is None else dict(start_frame=sub[0], end_frame=sub[1])
    emus = [PB.emulate_stages_f32(u)[0] for u in units]
    sg = _make_sg(y, kw)
    gate = sg._gate
    gate.profile_enable(True)
    try:
        for name, opts, kernels, absent in _routes(n_fft):
            tag = "n_fft %d %s [%s]" % (n_fft, layout, name)
            with gate.lock, gate.with_options(opts):
                gate.profile_read(reset=True)
                got = sg.get_traces(**args)
                stages = {k.split(" ")[0] for k in gate.profile_read(reset=True)}
                bits = np.swapaxes(gate.debug_field(3), 1, 2)
                d0, d1 = gate.debug_range()
                again = sg.get_traces(**args)
            assert kernels <= stages and not (absent & stages), (tag, sorted(stages))
            assert got.dtype == np.float32 and got.shape == ((geo["N"],) if sub is None else (sub[1] - sub[0],)), tag
            worst = 0.0
            for ui, u in enumerate(units):
                cut, (a, b) = _cut(u, sub)
                bad, ratio = PB.local_check(got[a:b], cut, bud=PB.budget(cut, emus[ui]))
                worst = max(worst, ratio)
                assert len(bad) == 0, "%s unit %d: hop blocks %s over their bound, largest error / budget %.2f" % (
                    tag, ui, bad[:10].tolist(), ratio)
            print("%s: largest local_error / budget %.2f" % (tag, worst))
            assert bits.shape[0] == len(units) and 0 <= d0 < d1 <= bits.shape[2], (tag, bits.shape, d0, d1)
            for ui, u in enumerate(units):
                cells, left = PB.bit_diff(bits[ui], u, frames=(d0, d1))
                assert left <= PB.LEFT_OUT_CAP and len(cells) == 0, "%s unit %d: decision bits differ at %s" % (
                    tag, ui, cells[:6].tolist())
            assert np.array_equal(got, again), tag
    finally:
        gate.profile_enable(False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft", sorted(NF))
def test_int16_samples_through_the_one_pass_gate(n_fft):
    """SG_OPT_FAST_INTEGER: int16 in, int16 out of k_gate_onepass512 / 256 / 2048 (three units, odd destinations: the per-sample
    path with the integer conversion of store_sample), at most 1 LSB from the truncated float64 result."""
    from noisereduce_amd import _ffi
    geo = _geometry(n_fft, "three_units")
    y = np.round(PB.signals.dc_nyquist(geo["N"], PB.SR, SEED[n_fft]) * 20000.0).astype(np.int16)
    kw = dict(stationary=True, n_fft=n_fft, chunk_size=geo["cs"], padding=geo["pad"], prop_decrease=1.0)
    out, _ = PB.oracle_units(y.astype(np.float64), PB.SR, **kw)
    want = out.astype(np.int16)                      # (the reference truncates its float64 result)
    sg = _make_sg(y, kw)
    gate = sg._gate
    gate.profile_enable(True)
    try:
        with gate.lock, gate.with_options([(_ffi.SG_OPT_FAST_INTEGER, 1)]):
            gate.profile_read(reset=True)
            got = sg.get_traces(start_frame=geo["sub"][0], end_frame=geo["sub"][1])
            stages = {k.split(" ")[0] for k in gate.profile_read(reset=True)}
    finally:
        gate.profile_enable(False)
    assert "k_gate_onepass" in stages, sorted(stages)
    assert got.dtype == np.int16 and got.shape == (geo["sub"][1] - geo["sub"][0],)
    d = np.abs(got.astype(np.int32) - want[geo["sub"][0]:geo["sub"][1]].astype(np.int32))
    print("n_fft %d int16: %d of %d samples 1 LSB off" % (n_fft, int(np.sum(d == 1)), d.size))
    assert d.max() <= 1
