"""State transfer of stream banks, the part that needs no GPU: the new C symbols and the header struct, the payload
arithmetic against its Python restatement, StreamState's bytes form and every rejection path of restore."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(n_fft=512, win_length=400, hop_length=160)
NEW = ("sg_stream_export_bytes", "sg_stream_head_bytes", "sg_stream_export", "sg_stream_import")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    return _ffi, _ffi.load_library()


def _bank(kind="fixed", **over):
    from noisereduce_amd import stream
    kw = dict(KW)
    if kind == "fixed":
        kw.update(thresholds_db=np.zeros(kw["n_fft"] // 2 + 1))
    elif kind == "nonstationary":
        kw.update(stationary=False, lookahead_ms=35.0, time_constant_s=0.1)
    else:
        kw.update(noise_from_stream=True, noise_memory_s=0.25, noise_learn_s=0.3)
    kw.update(over)
    if kw.get("n_fft") != 512 and "thresholds_db" in kw:
        kw["thresholds_db"] = np.zeros(kw["n_fft"] // 2 + 1)
    return stream.StreamBank(16000, 3, **kw)


def _head(bank, n):
    """The header sg_stream_export would write for a stream of `bank` that has received n samples."""
    from noisereduce_amd import _ffi, stream
    sig = bank._signature()
    W, H, L = bank.win_length, bank.hop_length, bank.lookahead_frames
    td = stream.t_decided(n, W, H)
    ts = max(-1, td - L)
    ta = max(-1, ts - bank.nt)
    E = max(0, (ta + 1) * H - W // 2)
    assert E == stream.emitted(n, W, H, bank.nt + L)
    hd = _ffi.SgStreamHead(magic=_ffi.SG_STREAM_HEAD_MAGIC, version=_ffi.SG_STREAM_HEAD_VERSION, n=n, td=td, ts=ts, ta=ta, E=E,
                           par=1, has_thr=1, client0=0, client1=1, client2=1, **sig)
    hd.payload_bytes = stream.state_payload_bytes(n, bank.n_fft, W, H, bank.nt, L, bank.channels,
                                                  ("fixed", "nonstationary", "adaptive")[sig["kind"]], bank.exact)
    return hd


def _state(bank, n, seed=0):
    from noisereduce_amd import stream
    hd = _head(bank, n)
    payload = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, hd.payload_bytes, dtype=np.uint8))
    return stream.StreamState(hd, payload)


def test_new_symbols_are_declared_exported_and_bound():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    debug = open(os.path.join(ROOT, "include", "mi355gate_debug.h")).read()
    exports = open(os.path.join(ROOT, "noisereduce_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*sg_\*;", exports)
    for name in NEW:
        assert re.search(r"SG_API int %s\(" % name, header), name
        assert name in _ffi.exported_symbols()
        assert hasattr(lib, name)
    assert lib.sg_version() == 100
    # the two profiling stages lie beyond the 27 that sg_profile_read's earlier callers read
    assert int(re.search(r"#define SG_STAGE_ST_EXPORT (\d+)", debug).group(1)) == 27
    assert int(re.search(r"#define SG_STAGE_ST_IMPORT (\d+)", debug).group(1)) == 28
    assert int(re.search(r"#define SG_N_STAGES_ALL (\d+)", debug).group(1)) == _ffi.SG_N_STAGES_ALL == 29
    assert lib.sg_stage_name(27).startswith(b"k_st_export") and lib.sg_stage_name(28).startswith(b"k_st_import")
    assert lib.sg_stage_name(29) == b"?"
    import noisereduce_amd as nr
    assert nr.StreamState is not None and "StreamState" in nr.__all__
    assert hasattr(nr.StreamBank, "snapshot") and hasattr(nr.StreamBank, "restore")
    assert hasattr(nr.StreamGate, "snapshot") and hasattr(nr.StreamGate, "restore")


def test_head_struct_matches_the_header_field_by_field():
    _ffi, _ = _lib()
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    body = header[header.index("typedef struct sg_stream_head {"):header.index("} sg_stream_head;")]
    fields = re.findall(r"^\s*(int32_t|int64_t|double)\s+(\w+);", body, flags=re.M)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    assert [(f[1], ctype[f[0]]) for f in fields] == list(_ffi.SgStreamHead._fields_)
    size = ctypes.sizeof(_ffi.SgStreamHead)
    assert size == 184 == sum(ctypes.sizeof(t) for _, t in _ffi.SgStreamHead._fields_)      # no padding anywhere
    names = [f[1] for f in fields]
    assert tuple(names[2:2 + len(_ffi.STREAM_SIGNATURE)]) == _ffi.STREAM_SIGNATURE
    assert int(re.search(r"#define SG_STREAM_HEAD_MAGIC (0x[0-9a-fA-F]+)", header).group(1), 16) == _ffi.SG_STREAM_HEAD_MAGIC
    assert int(re.search(r"#define SG_STREAM_HEAD_VERSION (\d+)", header).group(1)) == _ffi.SG_STREAM_HEAD_VERSION
    assert _ffi.SG_STREAM_HEAD_MAGIC.to_bytes(4, "little") == b"SGST"


def _layout_bytes(n, n_fft, W, H, nt, L, C, kind, exact):
    """The layout table of DESIGN section 13d, written out field by field from the frame ranges (not from stream.py)."""
    F = n_fft // 2 + 1
    FS, wpr, h = -(-F // 16) * 16, -(-F // 64), W // 2
    if kind != "nonstationary":
        L = 0
    td = (n + h - W) // H if n + h - W >= 0 else -1
    ts = td - L if td - L >= 0 else -1
    ta = ts - nt if ts - nt >= 0 else -1
    E = max(0, (ta + 1) * H - h)
    ring = len(range(max(0, n - (W + (nt + L + 1) * H)), n))
    carry = len(range(E, ta * H - h + W)) if ta >= 0 else 0
    rows_lo = max(0, ta + 1 - nt)
    unit = 8 * (ring + carry)
    if kind == "nonstationary":
        unit += 8 * FS + len(range(ts + 1, td + 1)) * 2 * FS * 8 + len(range(rows_lo, ts + 1)) * FS * (8 if exact else 4)
    else:
        unit += 8 * FS + len(range(rows_lo, td + 1)) * wpr * 8
        if kind == "adaptive":
            unit += 3 * FS * 8
    return (2 * FS * 8 if kind == "fixed" else 0) + C * unit


def test_payload_bytes_equal_the_layout_arithmetic_over_counters_and_geometries():
    _ffi, lib = _lib()
    from noisereduce_amd import stream
    rng = np.random.default_rng(13)
    seen = 0
    for n_fft, W, H in ((512, 400, 160), (256, 256, 64), (1024, 1024, 256), (4096, 3000, 333), (2048, 2048, 2048)):
        for kind in ("fixed", "nonstationary", "adaptive"):
            for nt, L, C, exact in ((0, 0, 1, False), (5, 3, 2, False), (9, 40, 1, True), (1, 0, 3, True)):
                edge = 3 * H - W // 2 + W          # the sample that completes frame 3
                ns = [0, 1, W // 2 - 1, W // 2, W - 1, W, edge - 1, edge, edge + 1, W + (nt + L + 1) * H, 10 * W + 3]
                ns += [int(v) for v in rng.integers(0, 40 * W, 12)] + [(1 << 40) + 12345]
                for n in ns:
                    want = _layout_bytes(n, n_fft, W, H, nt, L, C, kind, exact)
                    assert stream.state_payload_bytes(n, n_fft, W, H, nt, L, C, kind, exact) == want
                    hd = _ffi.SgStreamHead(magic=_ffi.SG_STREAM_HEAD_MAGIC, version=1, n_fft=n_fft, win_length=W, hop_length=H,
                                           channels=C, kind=("fixed", "nonstationary", "adaptive").index(kind),
                                           n_grad_freq=2, n_grad_time=max(nt, 1), smooth_mask=int(nt > 0),
                                           lookahead_frames=L, exact=int(exact), n=n)
                    got = ctypes.c_int64(-1)
                    assert lib.sg_stream_head_bytes(ctypes.byref(hd), ctypes.byref(got)) == 0
                    assert got.value == want and want % 8 == 0, (n_fft, W, H, kind, nt, L, C, exact, n)
                    seen += 1
    assert seen > 1000
    # a payload never grows past the live window: it does not depend on how long the stream has run
    a = stream.state_payload_bytes(10 ** 6, 512, 400, 160, 5, 3, 2, "nonstationary")
    assert a == stream.state_payload_bytes(10 ** 9 + 160 * 7, 512, 400, 160, 5, 3, 2, "nonstationary")
    # signatures no bank can have
    bad = [dict(n_fft=500), dict(n_fft=8192), dict(win_length=513), dict(win_length=1), dict(hop_length=0), dict(channels=0),
           dict(kind=3), dict(kind=1, lookahead_frames=-1), dict(kind=1, lookahead_frames=4097), dict(n=-1)]
    for b in bad:
        f = dict(n_fft=512, win_length=400, hop_length=160, channels=1, kind=0, n_grad_time=1, n=0)
        f.update(b)
        got = ctypes.c_int64(-1)
        assert lib.sg_stream_head_bytes(ctypes.byref(_ffi.SgStreamHead(**f)), ctypes.byref(got)) == _ffi.SG_E_INVALID, b
    assert lib.sg_stream_head_bytes(None, ctypes.byref(got)) == _ffi.SG_E_INVALID


def test_bank_arithmetic_is_the_modules():
    from noisereduce_amd import stream
    for kind in ("fixed", "nonstationary", "adaptive"):
        bank = _bank(kind, channels=2)
        assert bank.state_bytes_of(1) == stream.state_payload_bytes(0, 512, 400, 160, bank.nt, bank.lookahead_frames, 2, kind)
        assert bank._bank is None


def test_bytes_round_trip_a_hand_made_state():
    from noisereduce_amd import _ffi, stream
    for kind, n in (("fixed", 0), ("fixed", 5000), ("nonstationary", 1234), ("adaptive", 399)):
        bank = _bank(kind, channels=2)
        st = _state(bank, n, seed=n)
        blob = st.to_bytes()
        assert isinstance(blob, bytes) and len(blob) == 184 + st.head.payload_bytes
        assert blob[:4] == b"SGST"
        back = stream.StreamState.from_bytes(blob)
        assert bytes(back.head) == bytes(st.head)
        assert back.payload.dtype == torch.uint8 and torch.equal(back.payload, st.payload)
        assert (back.received, back.emitted) == (n, st.head.E) == (st.received, st.emitted)
        assert back.emitted == stream.emitted(n, 400, 160, bank.nt + bank.lookahead_frames)
        assert stream.StreamState.from_bytes(bytearray(blob)).to_bytes() == blob
        for f in _ffi.STREAM_SIGNATURE:
            assert getattr(back.head, f) == bank._signature()[f]


def test_from_bytes_rejects_wrong_magic_version_and_length():
    from noisereduce_amd import stream
    blob = _state(_bank("adaptive"), 3000).to_bytes()
    ok = stream.StreamState.from_bytes(blob)
    assert ok.received == 3000
    with pytest.raises(ValueError, match="magic"):
        stream.StreamState.from_bytes(b"XGST" + blob[4:])
    with pytest.raises(ValueError, match="version"):
        stream.StreamState.from_bytes(blob[:4] + (2).to_bytes(4, "little") + blob[8:])
    for cut in (0, 10, 183, 184, len(blob) - 1):
        with pytest.raises(ValueError):
            stream.StreamState.from_bytes(blob[:cut])
    with pytest.raises(ValueError):
        stream.StreamState.from_bytes(blob + b"\0")


def test_restore_checks_every_argument_before_any_device_work():
    from noisereduce_amd import _ffi, stream
    other = dict(n_fft=dict(n_fft=1024, win_length=400), win_length=dict(win_length=320), hop_length=dict(hop_length=100),
                 channels=dict(channels=2), n_grad_freq=dict(freq_mask_smooth_hz=200), n_grad_time=dict(time_mask_smooth_ms=80),
                 exact=dict(precision="float64"),
                 prop_decrease=dict(prop_decrease=0.5), n_std_thresh=dict(n_std_thresh_stationary=2.0))
    ns_other = dict(kind=None, lookahead_frames=dict(lookahead_ms=95.0), iir_b=dict(time_constant_s=0.5),
                    nonstat_thresh=dict(thresh_n_mult_nonstationary=3), nonstat_slope=dict(sigmoid_slope_nonstationary=7))
    ad_other = dict(noise_forget=dict(noise_memory_s=0.5), noise_learn_frames=dict(noise_learn_s=0.6))
    covered = set()
    for kind, table in (("fixed", other), ("nonstationary", ns_other), ("adaptive", ad_other)):
        bank = _bank(kind)
        for field, over in table.items():
            src = _bank("fixed") if over is None else _bank(kind, **over)
            diff = [f for f in _ffi.STREAM_SIGNATURE if src._signature()[f] != bank._signature()[f]]
            assert diff and diff[0] == field, (field, diff)           # the case isolates the field, or names it first
            with pytest.raises(ValueError, match=r": %s is " % field):
                bank.restore({1: _state(src, 2000)})
            covered.add(field)
        assert bank._bank is None and bank.received(1) == 0
    # top_db is not an argument of StreamBank, and smoothing on / off always moves the widths too: headers that differ
    # there alone
    bank = _bank("fixed")
    for field, value in (("top_db", 40.0), ("smooth_mask", 0)):
        st = _state(bank, 2000)
        setattr(st.head, field, value)
        with pytest.raises(ValueError, match=": %s is " % field):
            bank.restore({0: st})
        covered.add(field)
    with pytest.raises(ValueError, match=": n_grad_freq is "):
        bank.restore({0: _state(_bank("fixed", freq_mask_smooth_hz=None, time_mask_smooth_ms=None), 2000)})
    assert covered == set(_ffi.STREAM_SIGNATURE)
    good = _state(bank, 2000)
    with pytest.raises(ValueError, match="unknown slot"):
        bank.restore({3: good})
    with pytest.raises(ValueError, match="unknown slot"):
        bank.restore({-1: good})
    with pytest.raises(ValueError, match="twice"):
        bank.restore([(1, good), (2, good), (1, good)])
    with pytest.raises(ValueError, match="StreamState"):
        bank.restore({0: good.to_bytes()})
    for field, value in (("magic", 7), ("version", 2)):
        st = _state(bank, 2000)
        setattr(st.head, field, value)
        with pytest.raises(ValueError, match="format version"):
            bank.restore({0: st})
    st = _state(bank, 2000)
    st.payload = st.payload[:-8]
    with pytest.raises(ValueError, match="payload"):
        bank.restore({0: st})
    st = _state(bank, 2000)
    st.head.n = 2001                      # the same payload size, but E, td, ... are those of n = 2000 ...
    st.head.E += 1
    with pytest.raises(ValueError, match="counters"):
        bank.restore({0: st})
    st = _state(bank, 2000)
    st.head.n = -5
    with pytest.raises(ValueError, match="counters"):
        bank.restore({0: st})
    with pytest.raises(ValueError, match="twice"):
        bank.snapshot([1, 1])
    with pytest.raises(ValueError, match="unknown slot"):
        bank.snapshot([5])
    assert bank._bank is None and [bank.received(s) for s in range(3)] == [0, 0, 0]
    bank.restore({})                      # nothing to do: no device either
    assert bank._bank is None
