"""The exact stream banks (StreamBank(precision="float64")) without a GPU: argument checks that touch no device, the
byte counts and the descriptor's layout by hand, and the inputs of tests/test_gpu_stream_exact.py held to their conditions
against the float64 models alone."""
import ctypes

import numpy as np
import pytest

from noisereduce_amd import _ffi, stream
from tests import stream_exact_cases as X


def _bank(**kw):
    return stream.StreamBank(16000, 2, thresholds_db=np.zeros(257), n_fft=512, win_length=400, hop_length=160,
                             max_block=4800, **kw)


@pytest.mark.parametrize("bad", ["float16", "double", 64, "exact", ""])
def test_a_bad_precision_is_refused(bad):
    with pytest.raises(ValueError):
        _bank(precision=bad)
    with pytest.raises(ValueError):
        stream.StreamGate(16000, thresholds_db=np.zeros(257), n_fft=512, precision=bad)


def test_block_types_are_checked_before_any_device_work():
    exact = _bank(precision="float64")
    assert exact.exact and exact._bank is None
    for dt in (np.uint8, np.float16, np.bool_, np.int64, np.uint16):
        with pytest.raises(ValueError):
            exact.push({0: np.zeros(10, dt)})
    assert exact._bank is None
    for precision in (None, "float32"):
        default = _bank(precision=precision)
        assert not default.exact
        with pytest.raises(ValueError, match="float64"):
            default.push({0: np.zeros(10, np.int16)})
        with pytest.raises(ValueError):
            default.push({0: np.zeros(10, np.int32)})
        assert default._bank is None


def test_state_bytes_by_hand():
    # stationary, n_fft 512 / 400 / 160 at 16 kHz (nt = 5), max_block 4800, 6 units: the exact bank's state is unchanged
    F, FS, W, H, nt = 257, 272, 400, 160, 5
    mf = (4800 + 200) // 160 + 3
    RB = 2 * nt + 1 + mf
    per = (W + (nt + 1) * H) * 8 + 2 * W * 8 + FS * 8 + RB * 5 * 8
    assert mf == 34 and RB == 45 and per == 21256
    for exact in (False, True):
        assert stream.state_bytes(6, 512, W, H, nt, 0, 4800, True, exact=exact) == 6 * per
    assert stream.state_bytes(6, 512, W, H, nt, 0, 4800, True, noise_from_stream=True, exact=True) == 6 * (per + 3 * FS * 8)
    # non-stationary with L = 7: + RB * FS * 4 per unit for the float64 sigmoid rows
    L = 7
    RB = 2 * nt + 1 + L + mf
    per = (W + (nt + L + 1) * H) * 8 + 2 * W * 8 + FS * 8 + (L + 1 + mf) * 2 * FS * 8 + RB * FS * 4
    assert RB == 52 and per == 267776
    assert stream.state_bytes(6, 512, W, H, nt, L, 4800, False) == 6 * per
    assert stream.state_bytes(6, 512, W, H, nt, L, 4800, False, exact=True) == 6 * (per + RB * FS * 4)
    bank = stream.StreamBank(16000, 3, channels=2, stationary=False, lookahead_ms=75.0, n_fft=512, win_length=400,
                             hop_length=160, max_block=4800, precision="float64")
    assert bank.lookahead_frames == L and bank.state_bytes == 6 * (per + RB * FS * 4) and bank._bank is None
    with pytest.raises(ValueError, match="max_state_bytes"):
        stream.StreamBank(16000, 3, channels=2, stationary=False, lookahead_ms=75.0, n_fft=512, win_length=400,
                          hop_length=160, max_block=4800, precision="float64", max_state_bytes=6 * (per + RB * FS * 4) - 1)


def test_the_descriptor_has_the_headers_layout():
    # int32 n_slots, channels; int64 max_block; int32 kind, lookahead_frames; double forget; int64 learn_frames; int32 exact
    D = _ffi.SgStreamDesc
    want = dict(n_slots=0, channels=4, max_block=8, kind=16, lookahead_frames=20, forget=24, learn_frames=32, exact=40)
    assert [n for n, _ in D._fields_] == list(want)
    for name, off in want.items():
        assert getattr(D, name).offset == off, name
    assert ctypes.sizeof(D) == 48 and ctypes.alignment(D) == 8
    assert (_ffi.SG_STREAM_FIXED, _ffi.SG_STREAM_NONSTATIONARY, _ffi.SG_STREAM_ADAPTIVE) == (0, 1, 2)
    d = _ffi.Gate.stream_desc(3, 2, 4800, _ffi.SG_STREAM_ADAPTIVE, forget=0.5, learn_frames=9, exact=True)
    assert (d.n_slots, d.channels, d.max_block, d.kind, d.forget, d.learn_frames, d.exact) == (3, 2, 4800, 2, 0.5, 9, 1)
    for name in ("sg_stream_create_ex", "sg_stream_state_bytes_ex"):
        assert name in _ffi._PROTOTYPES


def _check_integer_input(geom, kind, dt, y, want64):
    assert y.dtype == dt and np.max(np.abs(y.astype(np.float64))) < 0.8 * np.iinfo(dt).max
    finite = np.isfinite(want64)
    assert finite.all() and np.max(np.abs(want64)) < np.iinfo(dt).max
    share = np.count_nonzero(X.decided(want64, dt)) / want64.size
    nonzero = np.count_nonzero(X.trunc(want64, dt)) / want64.size
    print(f"[exact-host] {geom} {kind} {dt}: decided {share:.4f}, non-zero {nonzero:.3f}")
    assert share > X.DECIDED_SHARE, share
    assert nonzero > 0.5, nonzero


@pytest.mark.parametrize("i", range(len(X.INT_CASES)), ids=lambda i: "%s-%s-%s" % (X.INT_CASES[i][1], X.INT_CASES[i][2], X.INT_CASES[i][3]))
def test_integer_inputs_are_decided_and_not_silent(i):
    geom, kind, dt, p, y, want64, info = X.int_case(i)
    _, _, W, H = X.resolve(geom)
    assert W + 5 <= len(y) <= 6 * W + 20 * H
    _check_integer_input(geom, kind, dt, y, want64)
    if kind == "fixed":
        assert info["live"] is False      # the causal floor is not live: the offline claim may be checked on these


@pytest.mark.parametrize("i", range(len(X.LARGE_CASES)))
def test_large_tile_inputs_are_decided_and_not_silent(i):
    geom, kind, dt, p, y, want64, info = X.int_case(i, large=True)
    assert len(y) == 2 * X.resolve(geom)[2] + 3 and info["live"] is False
    _check_integer_input(geom, kind, dt, y, want64)


def test_silence_input_has_nan_and_decided_parts():
    y = X.silence_signal()
    want64, _ = X.model(X.GEOMS[0], "nonstationary", y, direct=True)
    nan = np.isnan(want64)
    assert 1000 < np.count_nonzero(nan) < len(y) - 2000
    ok = ~nan
    share = np.count_nonzero(X.decided(want64[ok], np.int16)) / np.count_nonzero(ok)
    print(f"[exact-host] silence: {np.count_nonzero(nan)} NaN samples, decided {share:.4f} of the rest")
    assert share > X.DECIDED_SHARE


@pytest.mark.parametrize("i", range(len(X.F64_CASES)), ids=lambda i: "%s-%d" % (X.F64_CASES[i][1], X.F64_CASES[i][0][1]))
def test_no_cell_of_the_float64_cases_lies_on_its_threshold(i):
    geom, kind, streams = X.f64_case(i)
    for y, want64, info64, want32, info32 in streams:       # the float64 stream and its float32-valued twin
        for want, info in ((want64, info64), (want32, info32)):
            assert np.isfinite(want).all() and np.max(np.abs(want)) > 1e-3
            if kind == "fixed":
                assert info["live"] is False
            if kind != "nonstationary":       # (the sigmoid has no hard threshold)
                print(f"[exact-host] {geom} {kind}: nearest cell {info['margin_db']:.2e} dB from its threshold")
                assert info["margin_db"] > X.THRESHOLD_MARGIN_DB, info["margin_db"]
