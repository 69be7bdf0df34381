"""``reduce_noise_batch`` -- many recordings of any length gated in one call.

Each recording gets exactly what ``reduce_noise(ys[i], sr, y_noise=<its noise>, **kw)`` computes for it (the reference's
chunk grid, base.py:144-226, per recording; its own noise threshold, stationary.py:47-81), with a fixed number of kernel
launches per call however many recordings there are (sg_process_clips, include/mi355gate.h).

``plan`` is the pure-Python planner: which clips take the batched HIP path, and the unit table the library builds for
them.  It needs no GPU.
"""
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from noisereduce_amd import _ffi
from noisereduce_amd.spectralgate.nonstationary import iir_coefficient

BATCHED, FALLBACK = "batched", "fallback"
_NONE_CHUNK = 1 << 62       # chunk_size=None: one window per clip whatever its length (base.py:222)
_BATCH_SLOT = 7301          # the batch's own cached engine handles (a live gate object's threshold is never touched)
_FAST_DTYPES = (np.dtype(np.float32), np.dtype(np.float64))
_INT_DTYPES = (np.dtype(np.int16), np.dtype(np.int32))


@dataclass
class Unit:
    """One padded window the reference gates as one piece (base.py:144-150): one channel of one chunk of one clip."""
    clip: int
    channel: int
    chunk: int
    win0: int      # clip sample index of window sample 0 (chunk * chunk_size - padding)
    Lp: int        # window length
    T: int         # frames of the window (n_frames_for)
    k0: int        # first kept window position (= padding)
    k1: int        # end of the kept positions
    out0: int      # clip sample index of kept position k0
    noise: int     # noise source (stationary)


@dataclass
class BatchPlan:
    routes: list = field(default_factory=list)      # per clip: "batched" | "fallback"
    reasons: list = field(default_factory=list)     # per clip: why it falls back ("" when batched)
    units: list = field(default_factory=list)       # Unit rows of the batched clips, in clip order
    n_fft: int = 1024
    win_length: int = 1024
    hop_length: int = 256
    chunk_size: int = None
    padding: int = 0


def _resolve(n_fft, win_length, hop_length):
    W = n_fft if win_length is None else win_length
    H = W // 4 if hop_length is None else hop_length
    return int(n_fft), int(W), int(H)


def _shape_of(y):
    if isinstance(y, torch.Tensor):
        return tuple(y.shape), np.dtype(str(y.dtype).replace("torch.", ""))
    a = np.asarray(y)
    return a.shape, a.dtype


def _route(dtype, n_fft, precision, fast_int):
    if precision is None:
        precision = "float64" if os.environ.get("NOISEREDUCE_AMD_EXACT", "0") == "1" else "float32"
    if precision == "float64":
        return FALLBACK, "precision='float64' (float64 pipeline)"
    if n_fft not in (256, 512, 1024, 2048, 4096):
        return FALLBACK, "n_fft outside the batched kernels' sizes (powers of two 256..4096)"
    if dtype in _FAST_DTYPES:
        return BATCHED, ""
    if dtype in _INT_DTYPES:
        return (BATCHED, "") if fast_int else (FALLBACK, "integer samples without NOISEREDUCE_AMD_FAST_INT=1 (bit-exact pipeline)")
    return FALLBACK, f"sample type {dtype}"


def clip_units(i, n, channels, chunk_size, padding, W, H, noise=0):
    """Units of one clip (base.py:167-226): the chunk grid when n > chunk_size, else one window."""
    chunked = chunk_size is not None and n > chunk_size
    nch = -(-n // chunk_size) if chunked else 1
    out = []
    for c in range(channels):
        for k in range(nch):
            Lp = chunk_size + 2 * padding if chunked else n + 2 * padding
            T = (Lp + 2 * (W // 2) - W) // H + 1
            k1 = padding + (min(chunk_size, n - k * chunk_size) if chunked else n)
            out.append(Unit(clip=i, channel=c, chunk=k, win0=(k * chunk_size if chunked else 0) - padding, Lp=Lp, T=T,
                            k0=padding, k1=k1, out0=k * chunk_size if chunked else 0, noise=noise))
    return out


def plan(ys, sr, stationary=False, y_noise=None, chunk_size=600000, padding=30000, n_fft=1024, win_length=None,
         hop_length=None, precision=None, fast_int=None, **_ignored):
    """Route every clip and build the unit table of the batched ones (no GPU involved)."""
    if fast_int is None:
        fast_int = os.environ.get("NOISEREDUCE_AMD_FAST_INT", "0") == "1"
    n_fft, W, H = _resolve(n_fft, win_length, hop_length)
    p = BatchPlan(n_fft=n_fft, win_length=W, hop_length=H, chunk_size=chunk_size, padding=int(padding or 0))
    noise_idx = _noise_indices(ys, y_noise) if stationary else [0] * len(ys)
    for i, y in enumerate(ys):
        shape, dtype = _shape_of(y)
        if len(shape) > 2 or len(shape) == 0:
            raise ValueError(f"clip {i}: Waveform must be in shape (# frames, # channels)")
        C, n = (1, shape[0]) if len(shape) == 1 else shape
        route, why = _route(dtype, n_fft, precision, fast_int)
        p.routes.append(route)
        p.reasons.append(why)
        if route == BATCHED:
            if n < 1 or C < 1:
                raise ValueError(f"clip {i}: empty recording")
            units = clip_units(i, int(n), int(C), chunk_size, p.padding, W, H, noise_idx[i])
            if units[0].Lp < W:
                raise ValueError(f"clip {i}: chunk window of {units[0].Lp} samples is shorter than win_length={W}")
            p.units.extend(units)
    return p


def _per_clip_noise(y_noise, n_clips):
    """A Python list is per-clip noise (one entry per clip: array, tensor or None); anything else -- an array, a tensor,
    a tuple -- is one noise clip shared by every clip.  (A shared multichannel noise given as a list of per-channel
    arrays would be ambiguous: pass it as one (C, n) array.)"""
    if isinstance(y_noise, list):
        if len(y_noise) != n_clips:
            raise ValueError(f"y_noise: a list is per-clip noise and needs one entry per clip ({len(y_noise)} for "
                             f"{n_clips} clips); pass a shared noise clip as one array or tensor")
        return list(y_noise)
    return None


def _noise_indices(ys, y_noise):
    """Noise source of every clip: own clip (None), 0 (one shared array) or its list entry."""
    lst = _per_clip_noise(y_noise, len(ys))
    if lst is not None:
        return list(range(len(ys)))
    if y_noise is None:
        return list(range(len(ys)))
    return [0] * len(ys)


def _as_2d(a):
    return a[None, :] if a.ndim == 1 else a


def reduce_noise_batch(ys, sr, stationary=False, y_noise=None, prop_decrease=1.0, time_constant_s=2.0,
                       freq_mask_smooth_hz=500, time_mask_smooth_ms=50, thresh_n_mult_nonstationary=2,
                       sigmoid_slope_nonstationary=10, n_std_thresh_stationary=1.5, tmp_folder=None,
                       chunk_size=600000, padding=30000, n_fft=1024, win_length=None, hop_length=None,
                       clip_noise_stationary=True, use_tqdm=False, n_jobs=1, use_torch=False, device="cuda",
                       precision=None, max_workspace_bytes=0):
    """``[reduce_noise(y, sr, ...) for y in ys]`` in one batched call (see the module docstring).

    ``y_noise``: None (each clip is its own noise source), one array or tensor (shared by every clip; its threshold is
    computed once per sub-batch), or a Python list of ``len(ys)`` entries, each an array, a tensor or None.  A list is
    always read as per-clip noise: a shared multichannel noise clip goes in as one (C, n) array.

    ``max_workspace_bytes``: device memory budget of one sub-batch (0: 4 GiB); a call whose clips need more is processed
    in several sub-batches (``workspace_bytes`` gives what one sub-batch of all clips would take).  The workspace stays
    allocated in the batch's cached engine handle -- one per distinct parameter set -- for the next call;
    ``noisereduce_amd._ffi.clear_gate_cache()`` releases it.

    Device-tensor results are views into one output buffer of the whole batch: keeping any one of them keeps that
    buffer alive (``.clone()`` a result to keep it on its own)."""
    from noisereduce_amd.noisereduce import reduce_noise
    ys, kw, tensor_io, p, noise_list, noise_of = _setup(
        ys, sr, stationary, y_noise, dict(
            prop_decrease=prop_decrease, time_constant_s=time_constant_s, freq_mask_smooth_hz=freq_mask_smooth_hz,
            time_mask_smooth_ms=time_mask_smooth_ms, thresh_n_mult_nonstationary=thresh_n_mult_nonstationary,
            sigmoid_slope_nonstationary=sigmoid_slope_nonstationary, n_std_thresh_stationary=n_std_thresh_stationary,
            tmp_folder=tmp_folder, chunk_size=chunk_size, padding=padding, n_fft=n_fft, win_length=win_length,
            hop_length=hop_length, clip_noise_stationary=clip_noise_stationary, use_tqdm=use_tqdm, n_jobs=n_jobs,
            device=device, precision=precision), use_torch)
    if not ys:
        return []
    outs = [None] * len(ys)
    batched = [i for i, r in enumerate(p.routes) if r == BATCHED]
    for i, r in enumerate(p.routes):
        if r == FALLBACK:
            try:
                outs[i] = reduce_noise(ys[i], sr, stationary=stationary, y_noise=noise_of(i), **kw)
            except (ValueError, NotImplementedError) as e:
                raise type(e)(f"clip {i}: {e}") from None
    if batched:
        res = _run_batched(ys, batched, sr, stationary, noise_of, y_noise, noise_list, tensor_io, p, kw,
                           max_workspace_bytes)
        for i, o in zip(batched, res):
            outs[i] = o
    return outs


_KW_NAMES = ("prop_decrease", "time_constant_s", "freq_mask_smooth_hz", "time_mask_smooth_ms",
             "thresh_n_mult_nonstationary", "sigmoid_slope_nonstationary", "n_std_thresh_stationary", "tmp_folder",
             "chunk_size", "padding", "n_fft", "win_length", "hop_length", "clip_noise_stationary", "use_tqdm", "n_jobs",
             "device", "precision")


def _setup(ys, sr, stationary, y_noise, kw, use_torch):
    """Argument checks, plan and noise lookup shared by reduce_noise_batch and workspace_bytes."""
    if use_torch:
        raise ValueError("reduce_noise_batch evaluates the spectralgate algorithm; TorchGate is the batched torchgate API "
                         "(equal-length rows)")
    if kw["precision"] not in (None, "float32", "float64"):
        raise ValueError("precision must be None, 'float32' or 'float64'")
    ys = list(ys)
    tensor_io = bool(ys) and isinstance(ys[0], torch.Tensor)
    if any(isinstance(y, torch.Tensor) != tensor_io for y in ys):
        raise ValueError("reduce_noise_batch: all clips must be numpy-like or all device tensors")
    p = plan(ys, sr, stationary=stationary, y_noise=y_noise, chunk_size=kw["chunk_size"], padding=kw["padding"],
             n_fft=kw["n_fft"], win_length=kw["win_length"], hop_length=kw["hop_length"], precision=kw["precision"])
    noise_list = _per_clip_noise(y_noise, len(ys)) if stationary else None

    def noise_of(i):
        if not stationary:
            return None
        if noise_list is not None:
            return noise_list[i]
        return y_noise
    return ys, kw, tensor_io, p, noise_list, noise_of


def workspace_bytes(ys, sr, stationary=False, y_noise=None, **kwargs):
    """Device workspace (bytes) that ``reduce_noise_batch(ys, sr, ...)`` with the same arguments needs to gate its batched
    clips in ONE sub-batch (sg_clips_workspace_bytes): ``max_workspace_bytes`` at least this large means one sub-batch.
    Host arithmetic only (the engine handle is created on the device, no sample is read)."""
    import inspect
    args = inspect.signature(reduce_noise_batch).bind(ys, sr, stationary, y_noise, **kwargs)
    args.apply_defaults()
    a = args.arguments
    ys, kw, tensor_io, p, noise_list, noise_of = _setup(ys, sr, stationary, y_noise, {k: a[k] for k in _KW_NAMES},
                                                        a["use_torch"])
    idx = [i for i, r in enumerate(p.routes) if r == BATCHED]
    if not idx:
        return 0
    clips, noise_srcs = _tables(ys, idx, stationary, noise_of, noise_list, tensor_io, p, kw)[6:8]
    dev = ys[idx[0]].device if tensor_io else _ffi.resolve_device(kw["device"])
    return _gate_for(sr, stationary, p, kw, dev).clips_workspace_bytes(clips, noise_srcs)


def _gate_for(sr, stationary, p, kw, dev):
    n_grad_freq, n_grad_time, smooth = 1, 1, True
    fhz, tms = kw["freq_mask_smooth_hz"], kw["time_mask_smooth_ms"]
    if fhz is None and tms is None:
        smooth = False
    else:
        # base.py:99-128 (same errors as SpectralGate._generate_mask_smoothing_filter)
        if fhz is not None:
            n_grad_freq = int(fhz / (sr / (p.n_fft / 2)))
            if n_grad_freq < 1:
                raise ValueError("freq_mask_smooth_hz needs to be at least {}Hz".format(int((sr / (p.n_fft / 2)))))
        if tms is not None:
            n_grad_time = int(tms / ((p.hop_length / sr) * 1000))
            if n_grad_time < 1:
                raise ValueError("time_mask_smooth_ms needs to be at least {}ms".format(int((p.hop_length / sr) * 1000)))
        if n_grad_time == 1 and n_grad_freq == 1:
            smooth = False
    cs = _NONE_CHUNK if kw["chunk_size"] is None else int(kw["chunk_size"])
    common = dict(variant=_ffi.SG_VARIANT_S, n_fft=p.n_fft, win_length=p.win_length, hop_length=p.hop_length,
                  n_grad_freq=n_grad_freq if smooth else 1, n_grad_time=n_grad_time if smooth else 1,
                  smooth_mask=smooth, chunk_size=cs, padding=p.padding, prop_decrease=kw["prop_decrease"], exact=False)
    if stationary:
        return _ffi.cached_gate(dev, slot=_BATCH_SLOT, stationary=True, n_std_thresh=kw["n_std_thresh_stationary"],
                                top_db=80.0, ddof=0, **common)
    b = iir_coefficient(kw["time_constant_s"], sr, p.hop_length)
    return _ffi.cached_gate(dev, slot=_BATCH_SLOT, stationary=False, iir_b=b,
                            nonstat_thresh=kw["thresh_n_mult_nonstationary"],
                            nonstat_slope=kw["sigmoid_slope_nonstationary"], **common)


def _torch_dtype_of(dt):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32}[np.dtype(dt)]


def _tables(ys, idx, stationary, noise_of, noise_list, tensor_io, p, kw):
    """Clip and noise tables of the batched clips (sg_clip / sg_noise_src rows) and the packing offsets."""
    arrs = [ys[i] if tensor_io else np.asarray(ys[i]) for i in idx]
    shapes = [tuple(a.shape) for a in arrs]
    dtypes = [np.dtype(str(a.dtype).replace("torch.", "")) if tensor_io else a.dtype for a in arrs]
    # the statistics read int32 / float64 samples at their own precision: such a batch travels as float64
    wide = any(d in (np.dtype(np.float64), np.dtype(np.int32)) for d in dtypes)
    sizes = [int(np.prod(s)) for s in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1])
    clips = []
    chunk_size = kw["chunk_size"]
    clip_noise = kw["clip_noise_stationary"] and chunk_size is not None
    noise_srcs, noise_parts, noise_off = [], [], 0
    shared = None
    for j, (i, s) in enumerate(zip(idx, shapes)):
        C, n = (1, s[0]) if len(s) == 1 else s
        noise = 0
        if stationary:
            yn = noise_of(i)
            if yn is None:      # the clip is its own noise source (stationary.py:47-64)
                nn = min(n, chunk_size) if clip_noise else n
                if nn < p.win_length:
                    raise ValueError(f"clip {i}: noise clip of {nn} samples is shorter than win_length={p.win_length}")
                noise_srcs.append(_ffi.SgNoiseSrc(offset=int(offs[j]), n=int(nn), stride=int(n), channels=int(C), in_x=1))
                noise = len(noise_srcs) - 1
            elif noise_list is None and shared is not None:
                noise = shared
            else:
                a = yn.detach() if isinstance(yn, torch.Tensor) else np.asarray(yn)
                if a.ndim > 2 or a.ndim == 0:
                    raise ValueError(f"clip {i}: noise waveform must be in shape (# frames, # channels)")
                a = _as_2d(a)
                if clip_noise:
                    a = a[:, :chunk_size]
                Cn, nn = a.shape
                if nn < p.win_length:
                    raise ValueError(f"clip {i}: noise clip of {nn} samples is shorter than win_length={p.win_length}")
                noise_parts.append(a)
                noise_srcs.append(_ffi.SgNoiseSrc(offset=noise_off, n=int(nn), stride=int(nn), channels=int(Cn), in_x=0))
                noise_off += int(Cn) * int(nn)
                noise = len(noise_srcs) - 1
                if noise_list is None:
                    shared = noise
        clips.append(_ffi.SgClip(x_offset=int(offs[j]), n=int(n), x_stride=int(n), channels=int(C), noise=noise,
                                 out_offset=int(offs[j]), out_stride=int(n)))
    return arrs, shapes, dtypes, wide, offs, total, clips, noise_srcs, noise_parts


def _run_batched(ys, idx, sr, stationary, noise_of, y_noise, noise_list, tensor_io, p, kw, max_ws):
    dev = _ffi.resolve_device(kw["device"])
    if tensor_io:
        devs = {y.device for y in (ys[i] for i in idx)}
        if len(devs) != 1:
            raise ValueError("reduce_noise_batch: all device tensors must be on one device")
        dev = next(iter(devs))
        if dev.type != "cuda":
            raise ValueError("reduce_noise_batch: tensors must live on the GPU")
    arrs, shapes, dtypes, wide, offs, total, clips, noise_srcs, noise_parts = _tables(
        ys, idx, stationary, noise_of, noise_list, tensor_io, p, kw)
    g = _gate_for(sr, stationary, p, kw, dev)
    tdt = torch.float64 if wide else torch.float32
    with torch.cuda.device(dev):
        if tensor_io:
            x = torch.cat([a.reshape(-1).to(tdt) for a in arrs]) if total else torch.empty(0, dtype=tdt, device=dev)
        else:
            xh = torch.empty(total, dtype=tdt, pin_memory=True)
            xn_ = xh.numpy()
            for j, a in enumerate(arrs):
                xn_[offs[j]:offs[j + 1]] = a.reshape(-1)
            x = xh.to(dev, non_blocking=True)
        noise_t = None
        if noise_parts:
            if all(isinstance(a, torch.Tensor) for a in noise_parts):
                noise_t = torch.cat([a.to(dev, torch.float64).reshape(-1) for a in noise_parts])
            else:
                noise_t = torch.from_numpy(np.concatenate(
                    [np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(-1)
                     for a in noise_parts])).to(dev)
        out = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        with g.lock:
            g.process_clips(x, clips, out, noise=noise_t, noise_srcs=noise_srcs, max_workspace_bytes=max_ws)
        res = []
        if tensor_io:
            for j, (s, d) in enumerate(zip(shapes, dtypes)):
                o = out[offs[j]:offs[j + 1]].view(s)
                res.append(o if d == np.float32 else o.to(_torch_dtype_of(d)))
            return res
        oh = torch.empty(max(total, 1), dtype=torch.float32, pin_memory=True)
        oh.copy_(out)
        on = oh.numpy()
        for j, (s, d) in enumerate(zip(shapes, dtypes)):
            res.append(on[offs[j]:offs[j + 1]].reshape(s).astype(d, copy=True))
        return res
