"""The exact stream banks (StreamBank(precision="float64"), sg_stream_create_ex) on the GPU, against the float64 host
models (tests/stream_exact_cases.py holds the inputs; tests/test_stream_exact_host.py holds them to their conditions):
float64 accuracy, integers bit for bit, bitwise invariance, mixed steps, the 256-thread tiles, flush / reuse, the NaN rule,
the C ABI and the launch count."""
import numpy as np
import pytest
import torch

from noisereduce_amd import _ffi, stream
from oracle import spectralgate_oracle as O
from tests import stream_exact_cases as X

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12        # of peak: the project's bar for its float64 pipeline (tests/test_gpu_dtypes.py::test_force_exact_float64)


def _run(bank, plans, as_tensor=False):
    """plans: {slot: (signal (N,) or (C, N), cuts)}.  Step i pushes every stream's i-th block; then all are flushed."""
    blocks = {s: np.split(np.asarray(y), c, axis=-1) for s, (y, c) in plans.items()}
    outs = {s: [] for s in plans}
    for i in range(max(len(b) for b in blocks.values())):
        step = {s: b[i] for s, b in blocks.items() if i < len(b)}
        if as_tensor:
            step = {s: torch.from_numpy(np.array(v)).cuda() for s, v in step.items()}
        for s, o in bank.push(step).items():
            outs[s].append(o.cpu().numpy() if as_tensor else o)
    for s, o in bank.flush(list(plans)).items():
        outs[s].append(o.cpu().numpy() if as_tensor else o)
    return {s: np.concatenate(v, axis=-1) for s, v in outs.items()}


def _bank(geom, kind, n_slots, p=1.0, scale=1.0, channels=1, precision="float64", L=X.LOOKAHEAD, max_block=None):
    sr, _, W, H = X.resolve(geom)
    kw = X.bank_kw(geom, kind, p, L)
    if kind == "fixed":
        kw["y_noise"] = X.noise_clip(sr, scale)
    return stream.StreamBank(sr, n_slots, channels=channels, max_block=max_block or 6 * W + 20 * H, precision=precision, **kw)


def _four_plans(geom, y, seed):
    _, _, W, H = X.resolve(geom)
    rng = np.random.default_rng(seed)
    return {s + 1: (y, X.cuts(kind, y.shape[-1], W, H, rng)) for s, kind in enumerate(X.PLANS)}


def _check_integers(got, y, want64, tag):
    """tests/test_gpu_dtypes.py::test_integer_recordings_are_bit_exact's criterion, against the model (NaN -> 0)."""
    dt = y.dtype
    assert got.dtype == dt and got.shape == y.shape, (tag, got.dtype, got.shape)
    diff = got.astype(np.int64) - X.trunc(want64, dt).astype(np.int64)
    decided = X.decided(want64, dt) | np.isnan(want64)
    print(f"[exact] {tag}: max |diff| {np.max(np.abs(diff))}, {np.count_nonzero(diff)} differ, "
          f"{np.count_nonzero(diff[decided])} of them decided, decided share {np.count_nonzero(decided) / decided.size:.4f}")
    assert np.max(np.abs(diff)) <= 1 and np.count_nonzero(diff[decided]) == 0, (tag, np.count_nonzero(diff[decided]))
    assert np.count_nonzero(decided) > X.DECIDED_SHARE * decided.size


# ---- 1. float64 accuracy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(X.F64_CASES)), ids=lambda i: "%s-%d" % (X.F64_CASES[i][1], X.F64_CASES[i][0][1]))
def test_float64_blocks_come_back_float64_accurate(i):
    geom, kind, streams = X.f64_case(i)
    sr, n_fft, W, H = X.resolve(geom)
    C = 1 + i % 2          # (the gate is odd in the signal, exactly: channel 1 carries -y and must give -model)
    rng = np.random.default_rng(i)
    plans = {}
    for s, ((y, *_), plan) in enumerate(zip(streams, X.PLANS)):
        plans[s + 1] = (np.stack([y, -y]) if C == 2 else y, X.cuts(plan, len(y), W, H, rng))
    exact = _run(_bank(geom, kind, 5, channels=C), plans, as_tensor=bool(i % 3 == 0))
    default = _run(_bank(geom, kind, 5, channels=C, precision=None), plans)
    plans32 = {s: (y.astype(np.float32), c) for s, (y, c) in plans.items()}
    exact32 = _run(_bank(geom, kind, 5, channels=C), plans32)
    for s, (y, want, _, want32, _) in enumerate(streams):
        g, d, g32 = (np.atleast_2d(a[s + 1]) for a in (exact, default, exact32))
        assert exact[s + 1].dtype == np.float64 and exact[s + 1].shape == plans[s + 1][0].shape
        assert exact32[s + 1].dtype == np.float32
        for c in range(C):
            sign = -1.0 if c else 1.0
            e_exact, e_default = O.rel_err(g[c], sign * want), O.rel_err(d[c], sign * want)
            print(f"[exact] {geom} {kind} slot {s + 1} ch {c}: exact bank {e_exact:.2e}, default bank {e_default:.2e} of peak")
            assert e_exact <= F64_TOL, (s, c, e_exact)
            assert e_default > 1e-9, (s, c, e_default)       # the test sees the difference
        # float32 blocks: the float64 result of the float32-valued stream, rounded once
        assert O.rel_err(g32[0], want32) <= 1e-6
        r = want32.astype(np.float32)
        off = np.flatnonzero(g32[0] != r)
        # ... except where the model lies within 1e-12 of peak of the boundary between two neighbouring float32 values
        lo, hi = np.minimum(g32[0][off], r[off]), np.maximum(g32[0][off], r[off])
        assert np.array_equal(np.nextafter(lo, np.float32(np.inf)), hi), (s, off[:8])
        mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
        assert np.all(np.abs(want32[off] - mid) <= F64_TOL * np.max(np.abs(want32))), (s, off[:8])
        print(f"[exact] {geom} {kind} slot {s + 1}: float32 blocks: {len(off)} of {len(r)} samples on a rounding boundary")
        if kind == "fixed":      # the causal floor is not live (host test): the stream is the offline gate
            off64 = O.reduce_noise_S(np.asarray(y), sr, stationary=True, y_noise=X.noise_clip(sr), chunk_size=None,
                                     padding=0, n_fft=n_fft, win_length=W, hop_length=H)
            assert O.rel_err(g[0], off64) <= F64_TOL


@pytest.mark.parametrize("geom", X.GEOMS, ids=lambda g: str(g[1]))
def test_nonstationary_with_the_lookahead_over_the_stream_is_the_offline_gate(geom):
    sr, n_fft, W, H = X.resolve(geom)
    y = X.signal(geom, 777, np.float64, N=3 * W + 7 * H + 5)
    T = (len(y) + 2 * (W // 2) - W) // H + 1
    bank = _bank(geom, "nonstationary", 2, L=T)
    assert bank.lookahead_frames >= T - 1
    got = _run(bank, {1: (y, X.cuts("random", len(y), W, H, np.random.default_rng(5)))})[1]
    want = O.reduce_noise_S(y, sr, stationary=False, chunk_size=None, padding=0, n_fft=n_fft, win_length=W, hop_length=H,
                            time_constant_s=X.TC)
    model, _ = X.model(geom, "nonstationary", y, L=T)
    e_off, e_mod = O.rel_err(got, want), O.rel_err(got, model)
    print(f"[exact] {geom} non-stationary, L = {T}: offline {e_off:.2e}, model {e_mod:.2e} of peak")
    assert e_off <= F64_TOL and e_mod <= F64_TOL


# ---- 2. integers, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(X.INT_CASES)),
                         ids=lambda i: "%s-%s-%s" % (X.INT_CASES[i][1], X.INT_CASES[i][2], X.INT_CASES[i][3]))
def test_integer_blocks_are_the_truncated_float64_result(i):
    geom, kind, dt, p, y, want64, _ = X.int_case(i)
    sr, n_fft, W, H = X.resolve(geom)
    bank = _bank(geom, kind, 5, p=p, scale=X.scale_of(dt))
    plans = _four_plans(geom, y, i)
    host = _run(bank, plans)
    dev = _run(bank, {4: plans[2], 0: plans[3]}, as_tensor=True)
    for s in plans:
        _check_integers(host[s], y, want64, f"{geom} {kind} {dt} p={p} slot {s}")
    _check_integers(dev[4], y, want64, f"{geom} {kind} {dt} p={p} tensors")
    # one result, bitwise, whatever the block plan, the slot and the kind of buffer
    for g in (host[2], host[3], host[4], dev[4], dev[0]):
        assert np.array_equal(g, host[1])
    if i == 0:       # a fixed-profile case whose causal floor is not live: the offline integer claim
        off64 = O.reduce_noise_S(y.astype(np.float64), sr, stationary=True, y_noise=X.noise_clip(sr, X.scale_of(dt)),
                                 chunk_size=None, padding=0, prop_decrease=p, n_fft=n_fft, win_length=W, hop_length=H)
        decided = X.decided(off64, dt)
        assert np.count_nonzero(decided) > X.DECIDED_SHARE * decided.size
        assert np.array_equal(host[1][decided], off64.astype(dt)[decided])


# ---- 3. bitwise invariance: alone against next to other streams, float64 as well ----------------------------------------
@pytest.mark.parametrize("k", range(len(X.KINDS)), ids=X.KINDS)
def test_a_stream_does_not_depend_on_its_plan_its_slot_or_its_neighbours(k):
    kind = X.KINDS[k]
    geom, _, dt, p, yi, _, _ = X.int_case(4 * k)
    _, _, streams = X.f64_case(2 * k + X.GEOMS.index(geom))
    yf = streams[0][0]
    _, _, W, H = X.resolve(geom)
    rng = np.random.default_rng(30 + k)
    for y, scale in ((yi, X.scale_of(dt)), (yf, 1.0)):
        alone = _run(_bank(geom, kind, 1, p=p, scale=scale), {0: (y, [])})[0]
        assert alone.dtype == y.dtype
        crowd = _bank(geom, kind, 5, p=p, scale=scale)
        other = y[::-1].copy()
        got = _run(crowd, {3: (y, X.cuts("small", len(y), W, H, rng)), 0: (other, [17]), 4: (other[: W + 9], [])})
        assert np.array_equal(got[3], alone)
        got = _run(crowd, {1: (y, X.cuts("edge", len(y), W, H, rng)), 3: (other, X.cuts("random", len(y), W, H, rng))},
                   as_tensor=True)
        assert np.array_equal(got[1], alone)


# ---- 4. a step of mixed sample types ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "tensor"])
def test_a_mixed_step_gives_every_slot_its_own_streams_samples(kind, as_tensor):
    geom = X.GEOMS[0]
    sr, _, W, H = X.resolve(geom)
    N = 3 * W + 11 * H + 3
    ys = {0: X.signal(geom, 41, np.int16, N=N), 1: X.signal(geom, 42, np.float64, N=N) * 20000.0,
          2: (X.signal(geom, 43, np.float32, N=N) * np.float32(20000.0)).astype(np.float32), 3: X.signal(geom, 44, np.int32, N=N)}
    cuts = X.cuts("random", N, W, H, np.random.default_rng(4)) + [N, N]
    mixed = _run(_bank(geom, kind, 4, scale=20000.0), {s: (y, cuts[s:]) for s, y in ys.items()}, as_tensor=as_tensor)
    bank = _bank(geom, kind, 4, scale=20000.0)
    for s, y in ys.items():
        alone = _run(bank, {s: (y, [])}, as_tensor=as_tensor)[s]      # a single-type step
        assert mixed[s].dtype == y.dtype and np.array_equal(mixed[s], alone), s
    assert np.count_nonzero(mixed[0]) > 0.5 * N


# ---- 5. the 256-thread tiles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(X.LARGE_CASES)), ids=lambda i: str(X.LARGE_CASES[i][0][1]))
def test_large_tiles(i):
    geom, kind, dt, p, y, want64, _ = X.int_case(i, large=True)
    _, _, W, H = X.resolve(geom)
    bank = _bank(geom, kind, 2, p=p, scale=X.scale_of(dt), max_block=len(y))
    got = _run(bank, {1: (y, [W + H // 2 + 1])})[1]
    _check_integers(got, y, want64, f"{geom} {kind} {dt} two blocks")


# ---- 6. flush and reuse -----------------------------------------------------------------------------------------------
def test_flush_tail_reuse_and_reset():
    geom = X.GEOMS[0]
    sr, _, W, H = X.resolve(geom)
    N = 5 * W + 77                                      # (N - W + 2 h) % H != 0: the inverse transform ends before the stream
    T = (N + 2 * (W // 2) - W) // H + 1
    Lout = (T - 1) * H + W - 2 * (W // 2)
    assert Lout < N
    y16, y32 = X.signal(geom, 61, np.int16, N=N), X.signal(geom, 62, np.int32, N=N)
    want16, _ = X.model(geom, "fixed", y16)
    bank = _bank(geom, "fixed", 2, scale=20000.0)
    got16 = _run(bank, {1: (y16, [1000, 1001])})[1]
    _check_integers(got16, y16, want16, "flush tail int16")
    assert got16.dtype == np.int16 and np.all(got16[Lout:] == 0) and np.all(want16[Lout:] == 0.0)
    # a flush without a last block returns the type the stream was last fed with
    head = bank.push({1: y16[:1500]})[1]
    tail = bank.flush([1])[1]
    assert head.dtype == tail.dtype == np.int16 and len(head) + len(tail) == 1500
    # the slot fed again with another sample type gives what a fresh bank gives
    fresh = _run(_bank(geom, "fixed", 2, scale=20000.0), {1: (y32, [])})[1]
    again = _run(bank, {1: (y32, [999])})[1]
    assert again.dtype == np.int32 and np.array_equal(again, fresh)
    # and so after a reset in mid-stream
    bank.push({1: y16[:2000]})
    bank.reset([1])
    assert np.array_equal(_run(bank, {1: (y32, [4, 2000])})[1], fresh)


# ---- 7. the NaN rule --------------------------------------------------------------------------------------------------
def test_nan_becomes_integer_zero():
    geom = X.GEOMS[0]
    _, _, W, H = X.resolve(geom)
    y = X.silence_signal()
    want64, _ = X.model(geom, "nonstationary", y, direct=True)
    nan = np.isnan(want64)
    assert nan.any()
    bank = _bank(geom, "nonstationary", 2, max_block=len(y))
    got = _run(bank, {0: (y, [500, 2499, 2501, 4000])})[0]
    assert np.all(got[nan] == 0)
    _check_integers(got, y, want64, "silence then signal")
    dev = _run(bank, {1: (y, [3000])}, as_tensor=True)[1]
    assert np.array_equal(dev, got)
    # the mixed route converts on arrival with the same rule
    mixed = _run(bank, {0: (y, [3000]), 1: (y.astype(np.float64), [3000])})
    assert np.array_equal(mixed[0], got) and np.array_equal(np.isnan(mixed[1]), nan)


# ---- 8. the C ABI -----------------------------------------------------------------------------------------------------
def test_c_abi_is_additive():
    geom = X.GEOMS[0]
    sr, n_fft, W, H = X.resolve(geom)
    y = X.signal(geom, 81, np.float32, N=3000)
    classic = _bank(geom, "fixed", 2, precision=None, max_block=4000)
    classic._ensure()
    g, b = classic.gate, classic._bank
    # integer codes on a classic bank: SG_E_INVALID, nothing changes
    x16 = torch.zeros(3000, dtype=torch.int16, device="cuda")
    xf = torch.from_numpy(y).cuda()
    out = torch.full((3000,), -7.0, device="cuda")
    out16 = torch.zeros(3000, dtype=torch.int16, device="cuda")
    k = stream.emitted(3000, W, H, classic.nt)
    rec = [_ffi.SgStreamRec(slot=1, flush=0, n_samples=3000, in_offset=0, in_stride=3000, out_offset=0, out_stride=k)]
    for xi, oi in ((x16, out), (xf, out16)):
        rc = g.lib.sg_stream_push(b, xi.data_ptr(), _ffi._sg_dtype(xi), oi.data_ptr(), _ffi._sg_dtype(oi),
                                  (_ffi.SgStreamRec * 1)(*rec), 1, g._stream())
        assert rc == _ffi.SG_E_INVALID
        assert b"float32 / float64 buffers" in g.lib.sg_last_error(g._h)
        assert g.stream_counters(b, 1) == (0, 0)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0)
    g.stream_push(b, xf, out, rec)
    ref = out[:k].cpu().numpy()
    assert g.stream_counters(b, 1) == (3000, k)
    # sg_stream_create_ex with exact = 0 is the classic create call
    for kind, code in (("fixed", _ffi.SG_STREAM_FIXED), ("nonstationary", _ffi.SG_STREAM_NONSTATIONARY),
                       ("adaptive", _ffi.SG_STREAM_ADAPTIVE)):
        bank = _bank(geom, kind, 2, precision=None, max_block=4000)
        bank._ensure()
        gg = bank.gate
        desc = _ffi.Gate.stream_desc(2, 1, 4000, code, bank.lookahead_frames, bank.noise_forget, bank.noise_learn_frames)
        b2 = gg.stream_create_ex(desc)
        if kind == "fixed":
            gg.stream_set_threshold(b2, [0, 1], bank.thresholds())
        kk = stream.emitted(3000, W, H, bank._lag)
        rec2 = [_ffi.SgStreamRec(slot=1, flush=0, n_samples=3000, in_offset=0, in_stride=3000, out_offset=0, out_stride=kk)]
        o1, o2 = torch.zeros(3000, device="cuda"), torch.ones(3000, device="cuda")
        gg.stream_push(bank._bank, xf, o1, rec2)
        gg.stream_push(b2, xf, o2, rec2)
        assert kk > 0 and torch.equal(o1[:kk], o2[:kk])
        rc = gg.lib.sg_stream_push(b2, x16.data_ptr(), _ffi.SG_I16, o2.data_ptr(), _ffi.SG_F32, (_ffi.SgStreamRec * 1)(*rec2), 1,
                                   gg._stream())
        assert rc == _ffi.SG_E_INVALID
        # sg_stream_state_bytes_ex is Python's state_bytes, exact or not
        for exact in (False, True):
            desc.exact = int(exact)
            assert gg.stream_state_bytes_ex(desc) == stream.state_bytes(2, n_fft, W, H, bank.nt, bank.lookahead_frames, 4000,
                                                                         kind != "nonstationary", kind == "adaptive", exact)
        desc.exact = 0
        assert gg.stream_state_bytes_ex(desc) == gg.stream_state_bytes(2, 1, 4000, bank.lookahead_frames, kind == "adaptive")
        gg.stream_destroy(b2)
    assert np.array_equal(ref, _run(_bank(geom, "fixed", 2, precision=None, max_block=4000), {0: (y, [])})[0][:k])


# ---- 9. launches per step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", X.KINDS)
def test_a_step_of_an_exact_bank_is_four_launches(kind):
    geom = X.GEOMS[0]
    counts = []
    for S, n, dt in ((3, 1, np.int16), (40, 4000, np.int16), (3, 4000, np.float64)):
        bank = _bank(geom, kind, S, scale=20000.0, max_block=4000)
        x = {s: torch.from_numpy(X.signal(geom, s, dt, N=n)).cuda() for s in range(S)}
        bank.push(x)
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        bank.push(x)
        counts.append({k: v[1] for k, v in g.profile_read(reset=True).items()})
        g.profile_enable(False)
    assert all(c == counts[0] for c in counts), counts
    assert sum(counts[0].values()) == 4
