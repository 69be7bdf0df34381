"""The two-launch noise statistics (k_noise_moments + k_colstats1_final over its slices; csrc/api.hip: stage_stats)
against the float64 oracle and against the three-launch route it replaces for one long noise clip.

Clips: tests/noise_moments_cases.py (tests/test_noise_moments_host.py holds on the oracle what each one does).  Per clip:

* ``stats_route()`` says the two-launch form ran, and the profile books one scope per launch group -- the transform
  with its slice partials, and the final stage (plus the channel mean of a two-channel clip) -- as sg_noise_stats
  books all its kernels under one stage, the route word is what tells k_noise_moments from k_stft<double> + k_colstats1;
* the threshold lies within 1e-9 dB of ``O.noise_threshold_S`` on every band (NaN where the oracle's is NaN);
* the gate's compare constants equal those of the forced three-launch route (SG_OPT_STATS_THREE_LAUNCH) on the same clip
  within the same 1e-9 dB: T2 as 10 log10 of the power, the floor test's bounds as 20 log10 of the amplitude; the
  sentinels (every cell passes / none does) agree exactly.  (The bounds are float32 roundings of a float64 value: a
  differing rounding would show as 5e-7 dB);
* a second run gives the same bits in threshold and constants."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import noise_moments_cases as NM

pytestmark = pytest.mark.gpu

BOUND_DB = 1e-9


def _gate(n_fft):
    from noisereduce_amd import _ffi
    H = n_fft // 4
    nf, nt, smooth = O.mask_smoothing_widths(NM.SR, n_fft, H, 500, 50)
    return _ffi.cached_gate("cuda:0", slot=1907, variant=_ffi.SG_VARIANT_S, stationary=True, n_std_thresh=1.5, top_db=80.0,
                            ddof=0, n_fft=n_fft, win_length=n_fft, hop_length=H, n_grad_freq=nf, n_grad_time=nt,
                            smooth_mask=smooth, chunk_size=600000, padding=30000, prop_decrease=1.0, exact=False)


def _stats(gate, x):
    gate.profile_read(reset=True)
    gate.noise_stats(x)
    thr = gate.get_noise_threshold()
    t2, alim = gate.gate_consts()
    launches = {k.split(" ")[0]: v[1] for k, v in gate.profile_read(reset=True).items() if v[1] > 0}
    return thr, t2, alim, gate.stats_route(), launches


def _db_gap(a, b, scale):
    """Largest |scale log10(a / b)| over the entries that are positive and finite in both; the others must be equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num = (a > 0) & (b > 0) & np.isfinite(a) & np.isfinite(b) & (a < 1e299) & (b < 1e299)
    assert np.array_equal(a[~num], b[~num], equal_nan=True), (a[~num], b[~num])
    return float(np.max(np.abs(scale * np.log10(a[num] / b[num])))) if num.any() else 0.0


@pytest.mark.parametrize("case", NM.case_ids(), ids=NM.case_name)
def test_two_launch_statistics(case):
    import torch
    from noisereduce_amd import _ffi
    n_fft, T, kind = case
    clip = NM.build(n_fft, T, kind)
    want, _, _, _ = NM.oracle(n_fft, clip)
    gate = _gate(n_fft)
    x = torch.from_numpy(clip).to("cuda:0")
    with gate.lock:
        gate.profile_enable(True)
        try:
            thr, t2, alim, route, launches = _stats(gate, x)
            thr_b, t2_b, alim_b, route_b, _ = _stats(gate, x)
            with gate.with_options([(_ffi.SG_OPT_STATS_THREE_LAUNCH, 1)]):
                thr_3, t2_3, alim_3, route_3, launches_3 = _stats(gate, x)
        finally:
            gate.profile_enable(False)
    name = NM.case_name(case)
    scopes = 2 + (clip.shape[0] > 1)
    print("%s: route %d launched %s; forced route %d launched %s" % (name, route, launches, route_3, launches_3))
    assert (route, route_b, route_3) == (2, 2, 1)
    assert launches == {"noise": scopes} and launches_3 == {"noise": scopes}, (launches, launches_3)
    if kind == "nan":
        assert np.isnan(want).all() and np.isnan(thr).all() and np.isnan(thr_3).all()
    else:
        d = np.abs(thr - want)
        d3 = np.abs(thr_3 - want)
        f = int(np.argmax(d))
        print("%s: threshold within %.3g dB of the oracle's (band %d); three-launch route within %.3g dB"
              % (name, d[f], f, d3.max()))
        assert d[f] <= BOUND_DB, "%s: band %d off by %.3g dB" % (name, f, d[f])
    g_t2, g_alim = _db_gap(t2, t2_3, 10.0), _db_gap(alim, alim_3, 20.0)
    print("%s: compare constants within %.3g dB (T2) and %.3g dB (floor-test bounds) of the three-launch route's"
          % (name, g_t2, g_alim))
    assert g_t2 <= BOUND_DB and g_alim <= BOUND_DB
    assert thr.tobytes() == thr_b.tobytes() and t2.tobytes() == t2_b.tobytes() and alim.tobytes() == alim_b.tobytes()
