"""What the clips of tests/noise_moments_cases.py do, held on the float64 oracle (no GPU):

* the slice lengths and route bounds the cases are built around are the ones csrc/api.hip routes by;
* every (n_fft, T) cell lies on the two-launch route, with a last slice that is partial wherever the cell says so;
* zero-power runs sit where stated: exactly zero power on every band of their frames, none in the frames next to them,
  and the run lies inside one slice / across a slice boundary / at the clip's end as its name says;
* the -80 dB floor is live where it should be: on every band of a zero-power frame, and in the tone's band on cells
  between the bursts;
* no threshold lies near a tie.  The engine's threshold differs from the oracle's by summation order only as long as
  both floor the same cells and take the same branch for the compare constant, so: no cell within 1e-7 dB of its band's
  floor, and no threshold within 1e-7 dB of the dB of a zero cell (where T2 switches to "every cell passes")."""
import os
import re

import numpy as np
import pytest

from tests import noise_moments_cases as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slices_and_bounds_match_the_sources():
    api = open(os.path.join(ROOT, "noisereduce_amd", "csrc", "api.hip")).read()
    assert "constexpr int nm_frames_per_slice() { return 1024 / nm_team_threads<N>() - 1; }" in api
    assert "constexpr int nm_team_threads() { return N >= 1024 ? 256 : team_threads<N>(); }" in api
    assert "return N >= SG_TEAM_N ? 256 : (!SG_SHORT_TEAMS ? 64 : (N <= 128 ? 16 : (N == 256 ? 32 : 64)));" in api
    threads = {256: 16, 512: 32, 1024: 64, 2048: 256}     # per frame, from the two expressions above (N = n_fft / 2)
    assert NM.FPS == {n: 1024 // t - 1 for n, t in threads.items()}
    assert int(re.search(r"constexpr int NM_MIN_FRAMES = (\d+);", api).group(1)) == NM.MIN_FRAMES
    tg, bw, maxs = (int(re.search(r"constexpr int NM_%s = (\d+);" % k, api).group(1)) for k in ("TG", "BW", "MAXS"))
    assert "<= NM_TG * (64 / NM_BW) * NM_MAXS;" in api
    assert tg * (64 // bw) * maxs == NM.MAX_SLICES


def test_cells_lie_on_the_route():
    partial = {(1024, 512): 2, (1024, 513): 3, (1024, 525): 0, (1024, 527): 2, (1024, 1041): 6, (256, 512): 8, (512, 512): 16,
               (2048, 512): 2}
    for n_fft, T in NM.GEOMS:
        fps = NM.FPS[n_fft]
        assert T >= NM.MIN_FRAMES and -(-T // fps) <= NM.MAX_SLICES
        assert T % fps == partial[(n_fft, T)]
    assert {n for n, _ in NM.GEOMS} == {256, 512, 1024, 2048}
    for n_fft in (256, 512, 2048):     # the smallest T >= 512 that is no multiple of the slice
        assert [T for n, T in NM.GEOMS if n == n_fft] == [next(T for T in range(512, 600) if T % NM.FPS[n_fft])]


@pytest.mark.parametrize("case", NM.case_ids(), ids=NM.case_name)
def test_case_does_what_it_claims(case):
    n_fft, T, kind = case
    clip = NM.build(n_fft, T, kind)
    assert clip.shape == (2 if kind == "stereo" else 1, (T - 1) * (n_fft // 4) + 3)
    assert clip.dtype == {"int16": np.int16, "float64": np.float64}.get(kind, np.float32)
    thr, db, floor, Z = NM.oracle(n_fft, clip)
    assert db.shape == (n_fft // 2 + 1, T)
    if kind == "nan":
        assert np.isnan(thr).all()      # the NaN frames put a NaN into every band's moments
        return
    assert np.isfinite(thr).all()
    live = db < floor
    fps = NM.FPS[n_fft]
    run = NM.zero_run(n_fft, T, kind)
    if run is not None:
        t0, t1 = run
        assert 0 <= t0 <= t1 < T
        assert (Z[:, t0:t1 + 1] == 0.0).all() and live[:, t0:t1 + 1].all()
        outside = np.ones(T, bool)
        outside[t0:t1 + 1] = False
        assert (Z[:, outside] > 0.0).any(axis=0).all()      # no other frame is silent
        assert (Z[:, max(0, t0 - 1)] > 0).all() or t0 == 0
        assert t1 == T - 1 or (Z[:, t1 + 1] > 0).all()
        if kind == "zeros_inside":
            assert t0 // fps == t1 // fps and t0 % fps > 0 and (t1 + 1) % fps > 0
        if kind == "zeros_straddle":
            assert t1 // fps == t0 // fps + 1 and t0 % fps == fps - 1
        if kind == "zeros_last5":
            assert (t0, t1) == (T - 5, T - 1)
    if kind == "tone":
        f = NM.tone_band(n_fft)
        assert live[f].any() and not live[f].all()
        # the band's maximum is the tone: some 80 dB over the band's median cell between the bursts
        assert 70.0 < db[f].max() - np.median(db[f][live[f]]) < 110.0
    # no tie: every cell clear of its band's floor, every threshold clear of a zero cell's dB
    assert np.min(np.abs(db - floor)) > 1e-7
    assert np.min(np.abs(thr - 20.0 * np.log10(2.220446049250313e-16))) > 1e-7
