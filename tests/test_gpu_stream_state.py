"""StreamBank.snapshot / restore on the GPU: a stream that is snapshotted anywhere and continued in its own slot, another
slot, another bank or another process's bytes gives, bit for bit, what the uninterrupted stream gives; the other streams
of the target bank do not notice; one launch per call; no host wait; no write outside a payload."""
import functools

import numpy as np
import pytest
import torch

import noisereduce_amd as nr
from noisereduce_amd import _ffi, stream
from oracle import spectralgate_oracle as O
from tests import stream_adaptive_model as MA
from tests import stream_exact_cases as X
from tests import stream_model as M
from tests.test_gpu_stream import ORACLE_TOL

pytestmark = pytest.mark.gpu

ADAPTIVE = dict(noise_memory_s=MA.MEMORY_S[1], noise_learn_s=MA.LEARN_S[1])      # 0.25 s of memory, 0.3 s of learning
CONFIGS = [(g, kind, prec, C) for g in X.GEOMS for kind in X.KINDS for prec in (None, "float64") for C in (1, 2)]


def _id(cfg):
    g, kind, prec, C = cfg
    return "%d-%s-%s-%dch" % (g[1], kind, prec or "default", C)


def _kw(geom, kind, prec):
    kw = X.bank_kw(geom, kind)
    if kind == "adaptive":
        kw.update(ADAPTIVE)
    if prec:
        kw["precision"] = prec
    return kw


def _signal(geom, C, dtype, seed, N=None):
    _, _, W, H = X.resolve(geom)
    N = 6 * W + 20 * H if N is None else N
    y = np.stack([X.signal(geom, seed + c, dtype, N=N) for c in range(C)])
    return y if C > 1 else y[0]


def _noise(geom, kind, dtype):
    return X.noise_clip(geom[0], X.scale_of(dtype)) if kind == "fixed" else None


def _feed(bank, slots, y, cuts):
    """Push y's blocks (split at `cuts`; equal cuts give 0-sample blocks) to every slot of `slots` in the same steps."""
    outs = {s: [] for s in slots}
    for blk in np.split(y, cuts, axis=-1):
        for s, o in bank.push({s: blk for s in slots}).items():
            outs[s].append(o)
    return outs


def _cat(parts, like):
    return np.concatenate(parts, axis=-1) if parts else like[..., :0]


def _chunks(lo, hi, step):
    return list(range(lo + step, hi, step))


@functools.lru_cache(maxsize=None)
def _whole(cfg, seed=0):
    """(y, out, tail, noise) of the uninterrupted stream: one push, one flush, alone in a bank.  Computed once."""
    geom, kind, prec, C = cfg
    dtype = np.int16 if prec else np.float32
    y = _signal(geom, C, dtype, 40 + seed)
    noise = _noise(geom, kind, dtype)
    bank = stream.StreamBank(geom[0], 1, channels=C, y_noise=noise, max_block=y.shape[-1], **_kw(geom, kind, prec))
    out = bank.push({0: y})[0]
    tail = bank.flush([0])[0]
    bank.close()
    for a in (y, out, tail):
        a.setflags(write=False)
    return y, out, tail, noise


def _cut_points(geom, kind, rng):
    """(n, ends with a 0-sample push) for the cuts the stream is snapshotted at."""
    sr, n_fft, W, H = X.resolve(geom)
    nt = M.geometry(sr, n_fft, W, H, 500, 50)[4]
    N = 6 * W + 20 * H
    k = nt + (X.LOOKAHEAD if kind == "nonstationary" else 0) + 2      # a frame late enough for samples to have come out
    e = k * H - W // 2 + W                                             # the sample count that completes frame k
    assert stream.t_decided(e, W, H) == k and stream.t_decided(e - 1, W, H) == k - 1 and e + 2 < N
    return [(0, False), (W - W // 2 - 1, False), (e, False), (e - 1, False), (int(rng.integers(e + 1, N)), False),
            (int(rng.integers(W, N)), True), (N, False)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_a_snapshot_continues_bitwise_wherever_it_is_restored(cfg):
    geom, kind, prec, C = cfg
    sr, n_fft, W, H = X.resolve(geom)
    y, out, tail, noise = _whole(cfg)
    N = y.shape[-1]
    kw = _kw(geom, kind, prec)
    rng = np.random.default_rng(CONFIGS.index(cfg))
    small = 2 * H + 7                                       # the other bank's max_block: its RB and RF differ
    A = stream.StreamBank(sr, 3, channels=C, y_noise=noise, max_block=N, **kw)
    B = stream.StreamBank(sr, 5, channels=C, max_block=small, **kw)          # (a fixed bank: no profile of its own)
    D = stream.StreamBank(sr, 2, channels=C, max_block=N, **kw)
    lag = A.nt + A.lookahead_frames
    for n, zero_last in _cut_points(geom, kind, rng):
        A.reset([0])
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, 3)) + ([n] if zero_last else [])
        pre = _feed(A, [0], y[..., :n], cuts)[0] if n or zero_last else []
        snap = A.snapshot([0])[0]
        assert (snap.received, snap.emitted) == (n, stream.emitted(n, W, H, lag))
        assert snap.payload.is_cuda and snap.payload.numel() == A.state_bytes_of(0)
        A.restore({2: snap})
        B.restore({4: snap})
        D.restore({1: nr.StreamState.from_bytes(snap.to_bytes())})
        for bank, s in ((A, 2), (B, 4), (D, 1)):
            assert bank.received(s) == n
            assert bank.gate.stream_counters(bank._bank, s) == (n, stream.emitted(n, W, H, lag))
        rest = y[..., n:]
        r = N - n
        post = _feed(A, [0, 2], rest, sorted((min(r, 1), r // 3, r // 3, min(r, 2 * r // 3 + 5))))      # one 0-sample block
        post.update({4: _feed(B, [4], rest, _chunks(0, r, small))[4], 1: _feed(D, [1], rest, [])[1]})
        places = {"own slot": (A, 0), "other slot": (A, 2), "other bank": (B, 4), "bytes": (D, 1)}
        for name, (bank, s) in places.items():
            assert bank.received(s) == N, (name, n)
            assert bank.gate.stream_counters(bank._bank, s) == (N, stream.emitted(N, W, H, lag)), (name, n)
            got = _cat(pre + post[s], out)
            t = bank.flush([s])[s]
            assert got.dtype == out.dtype and got.shape == out.shape, (name, n)
            assert np.array_equal(got, out), (name, n)
            assert t.dtype == tail.dtype and np.array_equal(t, tail), (name, n)
            assert bank.received(s) == 0
    for bank in (A, B, D):
        bank.close()


def test_the_other_bank_is_held_to_the_float64_model():
    cfg = (X.GEOMS[0], "fixed", None, 1)
    sr, n_fft, W, H = X.resolve(cfg[0])
    y, out, tail, noise = _whole(cfg)
    thr = X.fixed_threshold(cfg[0])
    _, _, _, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H, 500, 50)
    model = np.concatenate(M.stream_model([y.astype(np.float64)], thr, n_fft, W, H, 1.0, nf, nt, smooth)[0])
    A = stream.StreamBank(sr, 1, y_noise=noise, max_block=len(y), **_kw(cfg[0], "fixed", None))
    B = stream.StreamBank(sr, 4, max_block=2 * H + 7, **_kw(cfg[0], "fixed", None))
    n = 2777
    pre = A.push({0: y[:n]})[0]
    B.restore({3: A.snapshot([0])[0]})
    post = _feed(B, [3], y[n:], _chunks(0, len(y) - n, 2 * H + 7))[3]
    got = np.concatenate([pre] + post + [B.flush([3])[3]])
    err = np.max(np.abs(got - model)) / np.max(np.abs(model))
    print(f"[stream state] restored into another bank at n = {n}: {err:.2e} of peak from the float64 model")
    assert err <= ORACLE_TOL


def _launches(gate, fn):
    gate.profile_enable(True)
    gate.profile_read(reset=True)
    res = fn()
    counts = {k.split(" ")[0]: v[1] for k, v in gate.profile_read(reset=True).items()}
    gate.profile_enable(False)
    return res, counts


def test_40_states_into_a_busy_bank_in_one_launch_and_nobody_notices():
    geom = X.GEOMS[0]
    sr, n_fft, W, H = X.resolve(geom)
    kw = _kw(geom, "fixed", None)
    noise = X.noise_clip(sr)
    rng = np.random.default_rng(64)
    lens = [int(v) for v in rng.integers(W + 5, 3000, 64)]
    ys = [X.signal(geom, 300 + s, np.float32, N=lens[s]) for s in range(64)]
    ref = stream.StreamBank(sr, 64, y_noise=noise, max_block=3000, **kw)
    want = ref.push({s: ys[s] for s in range(64)})
    want_tail = ref.flush(range(64))
    ref.close()
    src = stream.StreamBank(sr, 40, y_noise=noise, max_block=3000, **kw)
    dst = stream.StreamBank(sr, 64, y_noise=X.noise_clip(sr, seed=8), max_block=1500, **kw)      # another profile: it is replaced
    cut = [int(rng.integers(0, lens[s] + 1)) for s in range(64)]
    cut[0], cut[1] = 0, lens[1]
    pre = src.push({s: ys[s][:cut[s]] for s in range(40)})
    dst.set_noise(range(40, 64), y_noise=noise)
    pre.update(dst.push({s: ys[s][:min(cut[s], 1500)] for s in range(40, 64)}))
    cut[40:] = [min(c, 1500) for c in cut[40:]]
    one, counts = _launches(src.gate, lambda: src.snapshot([7]))
    assert counts == {"k_st_export": 1}, counts
    states, counts = _launches(src.gate, lambda: src.snapshot(range(40)))
    assert counts == {"k_st_export": 1}, counts
    assert torch.equal(one[7].payload, states[7].payload) and bytes(one[7].head) == bytes(states[7].head)
    assert len({st.payload.untyped_storage().data_ptr() for st in states.values()}) == 1      # one allocation per call
    # 40 states in one call, slot s -> slot 39 - s, while slots 40 .. 63 are mid-stream
    _, counts = _launches(dst.gate, lambda: dst.restore({39 - s: states[s] for s in range(40)}))
    assert counts == {"k_st_import": 1}, counts
    _, counts = _launches(dst.gate, lambda: dst.restore({39 - 7: one[7]}))
    assert counts == {"k_st_import": 1}, counts
    where = {s: (39 - s if s < 40 else s) for s in range(64)}
    post = {s: [] for s in range(64)}
    for i in range(2):            # the rest in two steps of at most max_block samples
        step = {where[s]: ys[s][cut[s] + i * 1500:cut[s] + (i + 1) * 1500] for s in range(64)}
        got = dst.push(step)
        for s in range(64):
            post[s].append(got[where[s]])
    tails = dst.flush(range(64))
    for s in range(64):
        whole = np.concatenate([pre[s]] + post[s])
        assert np.array_equal(whole, want[s]), ("restored" if s < 40 else "untouched", s, cut[s])
        assert np.array_equal(tails[where[s]], want_tail[s]), s
    # the source went on undisturbed as well
    rest = src.push({s: ys[s][cut[s]:] for s in range(40)})
    for s in range(40):
        assert np.array_equal(np.concatenate([pre[s], rest[s]]), want[s]), s
    src.close()
    dst.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_nan_stays_gated_across_a_restore():
    geom = X.GEOMS[0]
    sr = geom[0]
    kw, noise = _kw(geom, "fixed", None), X.noise_clip(geom[0])
    y = O.synth_signal(8000, sr=sr, seed=3, dtype=np.float32)
    y[2500] = np.nan
    A = stream.StreamBank(sr, 1, y_noise=noise, max_block=8000, **kw)
    want = np.concatenate([A.push({0: y})[0], A.flush([0])[0]])
    B = stream.StreamBank(sr, 2, max_block=8000, **kw)
    pre = A.push({0: y[:3000]})[0]
    B.restore({1: A.snapshot([0])[0]})
    got = np.concatenate([pre, B.push({1: y[3000:6001]})[1], B.flush([1], {1: y[6001:]})[1]])
    assert np.isnan(want).sum() >= 400 and np.max(np.abs(want[5000:])) == 0.0      # gated from the NaN's first frame on
    assert np.array_equal(_bits(got), _bits(want))
    # the restored slot is clean after the flush, and a reset drops a restored state
    clean = y.copy()
    clean[2500] = 0.0
    A.reset([0])
    ref = np.concatenate([A.push({0: clean})[0], A.flush([0])[0]])
    assert np.array_equal(np.concatenate([B.push({1: clean})[1], B.flush([1])[1]]), ref)
    A.push({0: y[:3000]})
    B.restore({0: A.snapshot([0])[0]})
    B.reset([0])
    assert B.received(0) == 0 and B.gate.stream_counters(B._bank, 0) == (0, 0)
    assert np.array_equal(np.concatenate([B.push({0: clean})[0], B.flush([0])[0]]), ref)


def test_a_learn_window_goes_on_across_a_restore():
    geom = X.GEOMS[0]
    sr, n_fft, W, H = X.resolve(geom)
    kw = _kw(geom, "adaptive", None)
    y = np.stack([MA.swell(9000, sr, 21 + c) for c in range(2)])
    A = stream.StreamBank(sr, 1, channels=2, max_block=9000, **kw)
    assert A.noise_learn_frames == 30
    A.push({0: y})
    want = A.noise_profile(0)
    A.reset([0])
    n = 12 * H + 3                                         # frames 0 .. 10 learnt from so far, 19 to go
    A.push({0: y[:, :n]})
    B = stream.StreamBank(sr, 3, channels=2, max_block=4000, **kw)
    B.restore({2: A.snapshot([0])[0]})
    assert np.array_equal(B.noise_profile(2), A.noise_profile(0))
    B.push({2: y[:, n:n + 4000]})
    B.push({2: y[:, n + 4000:]})
    got = B.noise_profile(2)
    assert np.isfinite(want).all() and np.array_equal(got, want)
    # a state of a slot that received nothing restores as a reset
    B.restore({2: A.snapshot([0])[0], 1: B.snapshot([0])[0]})
    assert B.received(1) == 0 and np.isnan(B.noise_profile(1)).all()
    assert np.array_equal(B.noise_profile(2), A.noise_profile(0))


def test_snapshot_and_restore_of_device_states_do_not_wait_for_the_device():
    geom = X.GEOMS[0]
    sr = geom[0]
    kw, noise = _kw(geom, "nonstationary", None), None
    S, n = 64, 4000
    A = stream.StreamBank(sr, S, max_block=n, **kw)
    B = stream.StreamBank(sr, S, max_block=n, **kw)
    x = {s: torch.from_numpy(X.signal(geom, 500 + s, np.float32, N=2 * n)).cuda() for s in range(S)}
    A.push({s: v[:n] for s, v in x.items()})
    B.restore(A.snapshot(range(S)))                         # (tables, allocator: nothing left to grow in the timed part)
    busy = torch.zeros(1 << 26, device="cuda")
    torch.cuda.synchronize()
    for _ in range(400):                                    # tens of milliseconds of work ahead of the two calls
        busy.add_(1.0)
    done = torch.cuda.Event()
    states = A.snapshot(range(S))
    B.restore(states)
    done.record()
    pending = not done.query()                              # both calls returned with the stream's earlier work still running
    assert all(st.payload.is_cuda and st.received == n for st in states.values())
    torch.cuda.synchronize()
    assert pending
    assert float(busy[0]) == 400.0
    a = A.push({s: v[n:] for s, v in x.items()})
    b = B.push({s: v[n:] for s, v in x.items()})
    assert all(torch.equal(a[s], b[s]) for s in range(S))
    one = nr.StreamGate(sr, max_block=2 * n, **kw)
    head = one.push(x[5][:n].cpu().numpy())
    two = nr.StreamGate(sr, max_block=2 * n, **kw)
    two.restore(one.snapshot())
    assert np.array_equal(two.push(x[5][n:].cpu().numpy()), b[5].cpu().numpy())
    assert len(head) == stream.emitted(n, 400, 160, A.nt + A.lookahead_frames)


@pytest.mark.parametrize("kind", X.KINDS)
def test_export_and_import_stay_inside_the_payloads(kind):
    geom = X.GEOMS[0]
    sr = geom[0]
    kw = _kw(geom, kind, "float64" if kind == "nonstationary" else None)
    A = stream.StreamBank(sr, 4, channels=2, y_noise=_noise(geom, kind, np.float32), max_block=5000, **kw)
    ys = {s: _signal(geom, 2, np.float32, 600 + s, N=5000) for s in (0, 1, 3)}
    cut = {0: 0, 1: 1813, 3: 4999}
    A.push({s: ys[s][:, :cut[s]] for s in cut})
    g, b = A.gate, A._bank
    slots = [3, 0, 1]
    sizes = [g.stream_export_bytes(b, s) for s in slots]
    assert sizes == [A.state_bytes_of(s) for s in slots] and all(v % 8 == 0 for v in sizes)
    offsets, total = [], 512
    for v in sizes:
        offsets.append(total)
        total += (v + 255) // 256 * 256 + 256
    blob = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    heads = g.stream_export(b, slots, blob, offsets)
    host = blob.cpu().numpy()
    inside = np.zeros(total, dtype=bool)
    for o, v, hd, s in zip(offsets, sizes, heads, slots):
        inside[o:o + v] = True
        assert (hd.n, hd.payload_bytes, hd.channels) == (cut[s], v, 2)
    assert np.all(host[~inside] == 0xA5)
    assert not np.all(host[inside] == 0xA5)
    for bad in ([3, 0, 3], [3, 0, 9]):
        with pytest.raises(ValueError):
            g.stream_export(b, bad, blob, offsets)
    with pytest.raises(ValueError):
        g.stream_export(b, slots, blob, [offsets[0], offsets[1], offsets[2] + 8])
    with pytest.raises(ValueError):
        g.stream_export(b, slots, blob, [offsets[0], offsets[0], offsets[2]])      # payloads that overlap
    # the import reads the payloads where they lie and writes nothing but the slots' state: the streams go on
    B = stream.StreamBank(sr, 3, channels=2, max_block=5000, **kw)
    B._ensure()
    bad = _ffi.SgStreamHead.from_buffer_copy(bytes(heads[0]))
    bad.n += 1
    with pytest.raises(ValueError, match="counters"):
        B.gate.stream_import(B._bank, [0], blob, offsets[:1], [bad])
    bad = _ffi.SgStreamHead.from_buffer_copy(bytes(heads[0]))
    bad.hop_length += 1
    with pytest.raises(ValueError, match="hop_length differs"):
        B.gate.stream_import(B._bank, [0], blob, offsets[:1], [bad])
    assert B.gate.stream_counters(B._bank, 0) == (0, 0)
    B.gate.stream_import(B._bank, [2, 1, 0], blob, offsets, heads)
    assert np.array_equal(blob.cpu().numpy(), host)
    for s, t in zip(slots, (2, 1, 0)):
        assert B.gate.stream_counters(B._bank, t) == A.gate.stream_counters(A._bank, s)
        B._n[t], B._e[t] = B.gate.stream_counters(B._bank, t)      # (the raw call went past the Python mirrors)
        B._has_noise[t] = True
    a = A.push({s: ys[s][:, cut[s]:] for s in cut})
    c = B.push({t: ys[s][:, cut[s]:] for s, t in zip(slots, (2, 1, 0))})
    ta, tc = A.flush(slots), B.flush([2, 1, 0])
    for s, t in zip(slots, (2, 1, 0)):
        assert np.array_equal(a[s], c[t]) and np.array_equal(ta[s], tc[t]), s


def test_states_of_several_snapshots_and_of_bytes_restore_in_one_call_and_a_state_forks():
    geom = X.GEOMS[1]
    sr, n_fft, W, H = X.resolve(geom)
    kw, noise = _kw(geom, "fixed", None), X.noise_clip(geom[0])
    N = 6 * W + 20 * H
    ys = [X.signal(geom, 800 + s, np.float32, N=N) for s in range(3)]
    cut = [1000, 1717, 2303]
    A = stream.StreamBank(sr, 3, y_noise=noise, max_block=N, **kw)
    A.push({s: ys[s][:cut[s]] for s in range(3)})
    s0 = A.snapshot([0])[0]
    s1 = A.snapshot([1])[1]                                             # another call: another allocation
    s2 = nr.StreamState.from_bytes(A.snapshot([2])[2].to_bytes())
    assert s0.payload.untyped_storage().data_ptr() != s1.payload.untyped_storage().data_ptr() and not s2.payload.is_cuda
    B = stream.StreamBank(sr, 4, max_block=N, **kw)
    _, counts = _launches(B.gate, lambda: B.restore({3: s1, 0: s0, 2: s0}))       # two buffers; slot 2 forks slot 0's stream
    assert counts == {"k_st_import": 1}, counts
    C = stream.StreamBank(sr, 2, max_block=N, **kw)
    _, counts = _launches(C.gate, lambda: C.restore({1: s0, 0: s2}))              # a device state and a host state
    assert counts == {"k_st_import": 1}, counts
    want = A.push({s: ys[s][cut[s]:] for s in range(3)})
    want_tail = A.flush(range(3))
    got = B.push({0: ys[0][cut[0]:], 2: ys[0][cut[0]:], 3: ys[1][cut[1]:]})
    tail = B.flush([0, 2, 3])
    for slot, s in ((0, 0), (2, 0), (3, 1)):
        assert np.array_equal(got[slot], want[s]) and np.array_equal(tail[slot], want_tail[s]), slot
    got = C.push({1: ys[0][cut[0]:], 0: ys[2][cut[2]:]})
    tail = C.flush([0, 1])
    for slot, s in ((1, 0), (0, 2)):
        assert np.array_equal(got[slot], want[s]) and np.array_equal(tail[slot], want_tail[s]), slot
