"""ctypes binding of libmi355gate.so (C ABI: include/mi355gate.h; stage taps, development options and
per-kernel timing: include/mi355gate_debug.h).

PyTorch-ROCm tensors are only the I/O container: this module passes
``tensor.data_ptr()`` and the current HIP stream to the library.  There is no CPU
fallback: if the shared library is missing, or no MI355X/HIP device is visible, the
calls raise.
"""
import contextlib
import ctypes
import os
import threading
import weakref
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_int, c_int32,
                    c_int64, c_void_p)

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355gate.so")

SG_F32, SG_F64, SG_I16, SG_I32 = 0, 1, 2, 3
SG_VARIANT_S, SG_VARIANT_T = 0, 1
SG_E_INVALID, SG_E_UNSUPPORTED, SG_E_HIP, SG_E_NOMEM, SG_E_STATE, SG_E_HANDOFF = -1, -2, -3, -4, -5, -6
SG_N_STAGES = 27
SG_N_STAGES_ALL = 29      # with the state-transfer stages of stream banks (SG_STAGE_ST_EXPORT / SG_STAGE_ST_IMPORT)
SG_OPT_FORCE_F64_DECIDE = 3
SG_OPT_FORCE_NOSEAM = 4
SG_OPT_FORCE_NOLEAN = 5
SG_OPT_FORCE_SPLIT = 6
SG_OPT_INJECT_HANDOFF_FAULT = 7
SG_OPT_FAST_INTEGER = 8
SG_OPT_FORCE_EXACT = 9
SG_OPT_FORCE_NOROWGATE = 10
SG_OPT_ROWGATE_TAP = 11
SG_OPT_ROWGATE_SHAPE = 12
SG_OPT_FLOOR_TEST = 13
SG_OPT_TILE_ORDER = 15
SG_OPT_EXACT_MATERIALISED = 16
SG_OPT_STATS_THREE_LAUNCH = 17
SG_OPT_FLOOR_TWO_LAUNCH = 18
SG_OPT_FORCE_UNFUSED = 1
SG_OPT_FORCE_NOFAST = 2
SG_BWD_ROW, SG_BWD_FAST, SG_BWD_REG, SG_BWD_OLA, SG_BWD_ROWS = 1, 2, 3, 4, 5
# sg_debug_counter(17): the smoothing kernel of the last gate call (include/mi355gate_debug.h)
SG_SMOOTH_NAMES = {0: "none", 1: "off", 2: "k_smooth_tiled", 3: "k_smooth_f+k_smooth_t", 4: "k_smooth_bits2", 5: "k_smooth_bits",
                   6: "k_gate_onepass", 7: "k_gate_onepass_reg", 8: "k_row_gate", 9: "k_iir_mask<nt>", 10: "k_box_mask",
                   11: "kx_smooth_tiled", 12: "kx_smooth_f+kx_smooth_t"}
# sg_debug_counter(18): SG_SPEC_* of include/mi355gate_debug.h, the decide branch of the last sg_gate_spectrum call
SG_SPEC_NAMES = {0: "none", 1: "k_row_decide", 2: "k_t2_rows+k_decide_bits_t2", 3: "stage_decide", 4: "stage_box_mask",
                 5: "stage_nonstat_raw"}

_TORCH_DTYPES = {torch.float32: SG_F32, torch.float64: SG_F64, torch.int16: SG_I16,
                 torch.int32: SG_I32}


class HandoffTimeout(RuntimeError):
    """SG_E_HANDOFF: a bounded inter-workgroup wait of a fused kernel timed out (the device was preempted for
    about a second); the outputs of the calls enqueued since the last check are invalid and must be re-run."""


class SgParams(Structure):
    """struct sg_params (include/mi355gate.h)."""
    _fields_ = [
        ("variant", c_int32), ("stationary", c_int32), ("n_fft", c_int32),
        ("win_length", c_int32), ("hop_length", c_int32), ("n_grad_freq", c_int32),
        ("n_grad_time", c_int32), ("smooth_mask", c_int32), ("chunk_size", c_int64),
        ("padding", c_int64), ("prop_decrease", c_double), ("n_std_thresh", c_double),
        ("top_db", c_double), ("ddof", c_int32), ("n_movemean", c_int32),
        ("nonstat_thresh", c_double), ("nonstat_slope", c_double), ("iir_b", c_double),
        ("max_workspace_bytes", c_int64),
    ]


class SgClip(Structure):
    """struct sg_clip (include/mi355gate.h)."""
    _fields_ = [("x_offset", c_int64), ("n", c_int64), ("x_stride", c_int64), ("channels", c_int32),
                ("noise", c_int32), ("out_offset", c_int64), ("out_stride", c_int64)]


class SgNoiseSrc(Structure):
    """struct sg_noise_src (include/mi355gate.h)."""
    _fields_ = [("offset", c_int64), ("n", c_int64), ("stride", c_int64), ("channels", c_int32), ("in_x", c_int32)]


class SgStreamRec(Structure):
    """struct sg_stream_rec (include/mi355gate.h)."""
    _fields_ = [("slot", c_int32), ("flush", c_int32), ("n_samples", c_int64), ("in_offset", c_int64),
                ("in_stride", c_int64), ("out_offset", c_int64), ("out_stride", c_int64)]


class SgStreamSpecRec(Structure):
    """struct sg_stream_spec_rec (include/mi355gate.h): where one record's newly applied frames go."""
    _fields_ = [("spec_offset", c_int64), ("mask_offset", c_int64), ("stride", c_int64)]


class SgStreamFeatRec(Structure):
    """struct sg_stream_feat_rec (include/mi355gate.h): where one record's feature rows and mask rows go."""
    _fields_ = [("feat_offset", c_int64), ("feat_stride", c_int64), ("mask_offset", c_int64), ("mask_stride", c_int64)]


SG_STREAM_FIXED, SG_STREAM_NONSTATIONARY, SG_STREAM_ADAPTIVE = 0, 1, 2


class SgStreamDesc(Structure):
    """struct sg_stream_desc (include/mi355gate.h)."""
    _fields_ = [("n_slots", c_int32), ("channels", c_int32), ("max_block", c_int64), ("kind", c_int32),
                ("lookahead_frames", c_int32), ("forget", c_double), ("learn_frames", c_int64), ("exact", c_int32)]


SG_STREAM_HEAD_MAGIC, SG_STREAM_HEAD_VERSION = 0x54534753, 1


class SgStreamHead(Structure):
    """struct sg_stream_head (include/mi355gate.h): signature, counters and payload size of one stream's state."""
    _fields_ = [("magic", c_int32), ("version", c_int32), ("n_fft", c_int32), ("win_length", c_int32),
                ("hop_length", c_int32), ("channels", c_int32), ("kind", c_int32), ("n_grad_freq", c_int32),
                ("n_grad_time", c_int32), ("smooth_mask", c_int32), ("lookahead_frames", c_int32), ("exact", c_int32),
                ("prop_decrease", c_double), ("n_std_thresh", c_double), ("top_db", c_double), ("iir_b", c_double),
                ("nonstat_thresh", c_double), ("nonstat_slope", c_double), ("noise_forget", c_double),
                ("noise_learn_frames", c_int64), ("n", c_int64), ("td", c_int64), ("ts", c_int64), ("ta", c_int64),
                ("E", c_int64), ("par", c_int32), ("has_thr", c_int32), ("payload_bytes", c_int64),
                ("client0", c_int32), ("client1", c_int32), ("client2", c_int32), ("client3", c_int32)]


# the fields two banks must share for a state to move between them, in the order they are compared
STREAM_SIGNATURE = ("n_fft", "win_length", "hop_length", "channels", "kind", "n_grad_freq", "n_grad_time", "smooth_mask",
                    "lookahead_frames", "exact", "prop_decrease", "n_std_thresh", "top_db", "iir_b", "nonstat_thresh",
                    "nonstat_slope", "noise_forget", "noise_learn_frames")

# every symbol include/mi355gate.h and include/mi355gate_debug.h declare: name -> (restype, argtypes)
_PROTOTYPES = {
    "sg_version": (c_int, []),
    "sg_last_error": (c_char_p, [c_void_p]),
    "sg_create": (c_int, [POINTER(SgParams), POINTER(c_double), POINTER(c_void_p)]),
    "sg_destroy": (c_int, [c_void_p]),
    "sg_n_frames": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "sg_output_length": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "sg_workspace_bytes": (c_int, [c_void_p, c_int64, c_int64, c_int32, POINTER(c_int64)]),
    "sg_noise_stats": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p]),
    "sg_get_noise_threshold": (c_int, [c_void_p, POINTER(c_double), c_int32, c_void_p]),
    "sg_set_noise_threshold": (c_int, [c_void_p, POINTER(c_double), c_int32, c_void_p]),
    "sg_get_noise_threshold_dev": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "sg_set_noise_threshold_dev": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "sg_process_chunks": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int64,
                                  c_int64, c_int64, c_int64, c_int64, c_int32, c_int64, c_int64,
                                  c_void_p]),
    "sg_filter_padded": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int64, c_int64,
                                 c_int64, c_int64, c_void_p]),
    "sg_process_batch": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p,
                                 c_int64, c_int64, c_int64, c_void_p, c_int, c_int64, c_void_p,
                                 c_void_p]),
    "sg_process_batch_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64,
                                          c_void_p, c_void_p, c_int64, c_void_p]),
    "sg_gate_spectrum": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                 c_int64, c_void_p, c_void_p, c_void_p]),
    "sg_gate_spectrum_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                          c_void_p]),
    "sg_set_filterbank": (c_int, [c_void_p, c_void_p, c_int32]),
    "sg_gate_features": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                 c_int64, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "sg_gate_features_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                          c_int32, c_int32, c_double, c_void_p, c_int64, c_void_p]),
    "sg_process_rows": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                c_int64, c_int64, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "sg_process_rows_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_void_p, c_int64, c_void_p]),
    "sg_gate_spectrum_rows": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                      c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sg_gate_spectrum_rows_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                               c_void_p, c_int64, c_void_p]),
    "sg_gate_features_rows": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                      c_int64, c_int64, c_void_p, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p]),
    "sg_gate_features_rows_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                               c_void_p, c_int32, c_int32, c_double, c_void_p, c_int64, c_void_p]),
    "sg_debug_rows_batches": (c_int, [c_void_p, POINTER(c_int64)]),
    "sg_debug_backward_route": (c_int, [c_void_p, POINTER(c_int64)]),
    "sg_stft": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "sg_clips_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, POINTER(c_int64)]),
    "sg_process_clips": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int32, c_void_p, c_int64,
                                 c_void_p, c_int, c_int64, c_void_p]),
    "sg_debug_clip_thresholds": (c_int, [c_void_p, POINTER(c_double), c_int32, c_int32, c_void_p]),
    "sg_debug_clip_batches": (c_int, [c_void_p, POINTER(c_int64)]),
    "sg_stream_create": (c_int, [c_void_p, c_int32, c_int32, c_int64, POINTER(c_void_p)]),
    "sg_stream_destroy": (c_int, [c_void_p]),
    "sg_stream_set_threshold": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p]),
    "sg_stream_push": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int32, c_void_p]),
    "sg_stream_push_spectrum": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                        c_void_p, c_int32, c_void_p]),
    "sg_stream_bank_frames": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "sg_stream_set_filterbank": (c_int, [c_void_p, c_void_p, c_int32]),
    "sg_stream_push_features": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int32,
                                        c_int32, c_double, c_double, c_void_p, c_void_p, c_int32, c_void_p]),
    "sg_stream_reset": (c_int, [c_void_p, c_void_p, c_int32, c_void_p]),
    "sg_stream_emitted": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "sg_stream_counters": (c_int, [c_void_p, c_int32, POINTER(c_int64), POINTER(c_int64)]),
    "sg_stream_create_nonstationary": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int32, POINTER(c_void_p)]),
    "sg_stream_state_bytes": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int32, POINTER(c_int64)]),
    "sg_stream_bank_emitted": (c_int, [c_void_p, c_int64, POINTER(c_int64)]),
    "sg_stream_create_adaptive": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_double, c_int64, POINTER(c_void_p)]),
    "sg_stream_noise_profile": (c_int, [c_void_p, c_int32, POINTER(c_double), c_int32, c_void_p]),
    "sg_stream_state_bytes_adaptive": (c_int, [c_void_p, c_int32, c_int32, c_int64, POINTER(c_int64)]),
    "sg_stream_create_ex": (c_int, [c_void_p, POINTER(SgStreamDesc), POINTER(c_void_p)]),
    "sg_stream_state_bytes_ex": (c_int, [c_void_p, POINTER(SgStreamDesc), POINTER(c_int64)]),
    "sg_stream_export_bytes": (c_int, [c_void_p, c_int32, POINTER(c_int64)]),
    "sg_stream_head_bytes": (c_int, [POINTER(SgStreamHead), POINTER(c_int64)]),
    "sg_stream_export": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, POINTER(SgStreamHead), c_void_p]),
    "sg_stream_import": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, POINTER(SgStreamHead), c_void_p]),
    "sg_set_option": (c_int, [c_void_p, c_int32, c_int64]),
    "sg_get_option": (c_int, [c_void_p, c_int32, POINTER(c_int64)]),
    "sg_check_errors": (c_int, [c_void_p, c_void_p]),
    "sg_profile_enable": (c_int, [c_void_p, c_int32]),
    "sg_profile_select": (c_int, [c_void_p, c_int64]),
    "sg_profile_read": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64), c_int32, c_int32]),
    "sg_stage_name": (c_char_p, [c_int32]),
    "sg_debug_dims": (c_int, [c_void_p, POINTER(c_int64)]),
    "sg_debug_range": (c_int, [c_void_p, POINTER(c_int64)]),
    "sg_debug_counter": (c_int, [c_void_p, c_int32, POINTER(c_int64), c_void_p]),
    "sg_debug_fetch": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p]),
}

_lib = None


def load_library():
    """dlopen libmi355gate.so and bind every declared symbol.  Loading needs the HIP
    runtime but no GPU; calling compute entry points does."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SG_LIB_PATH", LIB_PATH)   # development: A/B builds (tools/ablate.sh)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  noisereduce_amd has no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_PROTOTYPES)


def resolve_device(device="cuda"):
    """Return a torch.device on an AMD GPU or raise -- never falls back to CPU."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            "noisereduce_amd needs a HIP device (MI355X / gfx950): torch.cuda.is_available() is "
            "False and there is no CPU fallback.")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"noisereduce_amd only runs on the GPU (got device={device!r})")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _sg_dtype(t):
    try:
        return _TORCH_DTYPES[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported device sample dtype {t.dtype}") from None


def _rows(t):
    """(tensor, row_stride) for the C ABI: a 2-D tensor whose rows are contiguous and do not overlap goes as it is (any
    base address, any row pitch >= the row length); a non-unit last stride, and rows that overlap or repeat (row stride
    below the row length: ``expand``, ``unfold``), are copied -- the entry points disagree about such rows
    (sg_process_batch takes any stride, sg_process_rows and sg_gate_features_backward refuse one below L)."""
    assert t.dim() == 2
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _dense(t, name, rows=False, dtype=None):
    """``t`` for an argument of the C ABI that carries no strides of its own: the library reads (writes) ``numel()``
    elements from ``data_ptr()`` on, so the tensor must be contiguous -- a ``[::2]`` view, a transpose or an ``expand`` would be
    taken for other samples without anybody noticing.  ``rows=True``: an output the ABI takes with a row stride
    (sg_process_chunks' ``out``): 2-D, unit stride inside a row, rows that do not overlap; any base address and any pitch
    >= the row length go as they are (``_rows`` is the same rule for inputs, which it may copy; an output cannot be
    copied).  ``dtype``: the one element type the ABI reads there.  Raises ValueError naming the argument; never copies.
    Works on CPU tensors: no device is touched."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor (got {type(t).__name__})")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if rows:
        ok = t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
        what = "a 2-D tensor whose rows are contiguous and do not overlap"
    else:
        ok = t.is_contiguous()
        what = "contiguous"
    if not ok:
        raise ValueError(f"{name} must be {what}: the library reads it from data_ptr() on as dense memory (got shape "
                         f"{tuple(t.shape)} with strides {tuple(t.stride())})")
    return t


class Gate:
    """One sg_handle bound to one device (and used on that device's current stream)."""

    def __init__(self, device, *, variant, stationary, n_fft, win_length, hop_length,
                 n_grad_freq=1, n_grad_time=1, smooth_mask=False, chunk_size=600000,
                 padding=30000, prop_decrease=1.0, n_std_thresh=1.5, top_db=80.0, ddof=0,
                 n_movemean=20, nonstat_thresh=2.0, nonstat_slope=10.0, iir_b=0.0,
                 window=None, max_workspace_bytes=0, fast_integer=False, exact=False):
        self.lib = load_library()
        self.device = resolve_device(device)
        p = SgParams(variant=variant, stationary=int(bool(stationary)), n_fft=int(n_fft),
                     win_length=int(win_length), hop_length=int(hop_length),
                     n_grad_freq=int(n_grad_freq), n_grad_time=int(n_grad_time),
                     smooth_mask=int(bool(smooth_mask)), chunk_size=int(chunk_size or 1),
                     padding=int(padding or 0), prop_decrease=float(prop_decrease),
                     n_std_thresh=float(n_std_thresh), top_db=float(top_db), ddof=int(ddof),
                     n_movemean=int(n_movemean), nonstat_thresh=float(nonstat_thresh),
                     nonstat_slope=float(nonstat_slope), iir_b=float(iir_b),
                     max_workspace_bytes=int(max_workspace_bytes))
        self.params = p
        self.n_bins = int(n_fft) // 2 + 1
        # A handle carries per-call state (workspace, the stationary threshold h->thresh): callers that
        # share a cached handle serialise on `lock`, and `thresh_owner` names the object whose threshold
        # the handle currently holds (None: unknown) -- see SpectralGateStationary._bind().
        self.lock = threading.RLock()
        self.fb_key, self.n_filters = None, 0   # the filterbank the handle holds (set_filterbank)
        self.thresh_owner = None
        self._thresh_owner_ref = None    # weak reference to the owning object while its only copy is the handle's (claim_threshold)
        self._thr_stream = None          # stream the handle's current threshold was written on (noise_stats / set_noise_threshold*)
        wptr = None
        if window is not None:
            w = np.ascontiguousarray(np.asarray(window, dtype=np.float64))
            if w.shape != (int(win_length),):
                raise ValueError("window must have win_length entries")
            wptr = w.ctypes.data_as(POINTER(c_double))
        self._h = c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.sg_create(byref(p), wptr, byref(self._h))
        if rc != 0:
            msg = self.lib.sg_last_error(None).decode()
            self._h = c_void_p()
            self._raise(rc, msg)
        if fast_integer:   # integer outputs from the fused float32 kernels (<= 1 LSB off) instead of the float64 pipeline
            self.set_option(SG_OPT_FAST_INTEGER, 1)
        if exact:          # float64 pipeline for every sample type (precision="float64": float64-accurate results)
            self.set_option(SG_OPT_FORCE_EXACT, 1)

    # -- plumbing --------------------------------------------------------------------
    @staticmethod
    def _raise(rc, msg):
        if rc == SG_E_INVALID:
            raise ValueError(msg)
        if rc == SG_E_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == SG_E_NOMEM:
            raise MemoryError(msg)
        if rc == SG_E_HANDOFF:
            raise HandoffTimeout(msg)
        raise RuntimeError(f"libmi355gate error {rc}: {msg}")

    def _check(self, rc):
        if rc != 0:
            self._raise(rc, self.lib.sg_last_error(self._h).decode())

    def _stream(self):
        return c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            with torch.cuda.device(self.device):
                self.lib.sg_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _on_device(self, t):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"expected a tensor on {self.device}")

    # -- geometry --------------------------------------------------------------------
    def n_frames(self, L):
        out = c_int64()
        self._check(self.lib.sg_n_frames(self._h, int(L), byref(out)))
        return out.value

    def output_length(self, L):
        out = c_int64()
        self._check(self.lib.sg_output_length(self._h, int(L), byref(out)))
        return out.value

    def workspace_bytes(self, C, N, chunked=True):
        """HBM the handle will own after process_chunks on a (C, N) recording (host arithmetic only)."""
        out = c_int64()
        self._check(self.lib.sg_workspace_bytes(self._h, int(C), int(N), int(bool(chunked)), byref(out)))
        return out.value

    # -- variant S -------------------------------------------------------------------
    # The threshold belongs to the object that computed it (stationary.py:79-81), the handle is shared.  An object leaves its
    # threshold IN the handle and takes a device copy only when somebody else is about to overwrite it (evict_threshold):
    # the usual life -- one object, statistics, gate, gone -- never copies (a 4 KB device copy is a 4.8 us slot in the
    # stream of a 0.29 ms call).
    def claim_threshold(self, obj, token):
        """`obj` (with attributes _token, _thr_dev) owns the threshold the handle holds now.  Caller holds the lock."""
        self.thresh_owner = token
        self._thresh_owner_ref = weakref.ref(obj)

    def evict_threshold(self):
        """Before the handle's threshold is overwritten: its owner, if still alive and without a copy, saves one."""
        with self.lock:
            ref, self._thresh_owner_ref = self._thresh_owner_ref, None
            obj = ref() if ref is not None else None
            if obj is not None and obj._thr_dev is None and self.thresh_owner is obj._token:
                # The copy runs on the EVICTING caller's stream; the threshold was written on the owner's.  One stream (the
                # usual case): ordered by the stream, nothing to do.  Two: the copy waits for the writer's stream, the
                # owner's stream -- which will read the copy later -- waits for the copy, and the caching allocator is told
                # (costs nothing on the single-stream path)
                with torch.cuda.device(self.device):
                    cur, src = torch.cuda.current_stream(self.device), self._thr_stream
                    if src is not None and src != cur:
                        cur.wait_stream(src)
                    obj._thr_dev = self.noise_threshold_tensor()
                    if src is not None and src != cur:
                        src.wait_stream(cur)
                        obj._thr_dev.record_stream(src)
            self.thresh_owner = None

    def noise_stats(self, noise):
        self.evict_threshold()
        self._on_device(noise)
        noise, stride = _rows(noise)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_noise_stats(self._h, noise.data_ptr(), _sg_dtype(noise),
                                                noise.shape[0], noise.shape[1], stride,
                                                self._stream()))
            self._thr_stream = torch.cuda.current_stream(self.device)

    def get_noise_threshold(self):
        out = np.empty(self.n_bins, dtype=np.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_get_noise_threshold(
                self._h, out.ctypes.data_as(POINTER(c_double)), self.n_bins, self._stream()))
        return out

    def set_noise_threshold(self, thresh):
        self.evict_threshold()
        t = np.ascontiguousarray(np.asarray(thresh, dtype=np.float64))
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_set_noise_threshold(
                self._h, t.ctypes.data_as(POINTER(c_double)), int(t.shape[0]), self._stream()))
            self._thr_stream = torch.cuda.current_stream(self.device)

    def noise_threshold_tensor(self):
        """The threshold as a float64 device tensor (no host synchronisation)."""
        t = torch.empty(self.n_bins, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_get_noise_threshold_dev(self._h, t.data_ptr(), self.n_bins,
                                                            self._stream()))
        return t

    def set_noise_threshold_tensor(self, t):
        self.evict_threshold()
        self._on_device(t)
        t = _dense(t, "t").to(torch.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_set_noise_threshold_dev(self._h, t.data_ptr(), int(t.numel()),
                                                            self._stream()))
            self._thr_stream = torch.cuda.current_stream(self.device)

    def process_chunks(self, x, out_dtype=None, start_frame=0, end_frame=None, chunked=True,
                       out=None, halo_left=0, halo_right=0):
        """x: (C, N) tensor, or -- with halos -- a (C, halo_left + N + halo_right) tensor whose
        columns [halo_left, halo_left + N) are this shard's samples."""
        self._on_device(x)
        x, stride = _rows(x)
        C = x.shape[0]
        N = x.shape[1] - halo_left - halo_right
        x_ptr = x.data_ptr() + halo_left * x.element_size()
        end_frame = N if end_frame is None else int(end_frame)
        n_out = end_frame if not chunked else end_frame - int(start_frame)
        if out is None:
            out = torch.empty((C, n_out), dtype=out_dtype or x.dtype, device=self.device)
        elif tuple(_dense(out, "out", rows=True).shape) != (C, n_out):
            raise ValueError(f"out must be a (C, n) = {(C, n_out)} tensor, got {tuple(out.shape)}")
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_chunks(
                self._h, x_ptr, _sg_dtype(x), out.data_ptr(), _sg_dtype(out), C, N, stride,
                out.stride(0) if C > 1 else n_out, int(start_frame), end_frame, int(bool(chunked)),
                int(halo_left), int(halo_right), self._stream()))
        return out

    def filter_padded(self, chunk, out_dtype=None):
        self._on_device(chunk)
        chunk, stride = _rows(chunk)
        C, Lp = chunk.shape
        out = torch.empty((C, Lp), dtype=out_dtype or chunk.dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_filter_padded(self._h, chunk.data_ptr(), _sg_dtype(chunk),
                                                  out.data_ptr(), _sg_dtype(out), C, Lp, stride, Lp,
                                                  self._stream()))
        return out

    # -- variant T -------------------------------------------------------------------
    # Every wrapper below is marshalling (_noise, _mask, _grad_x, _lengths) and one library call.
    def _noise(self, x, xn):
        """The noise rows for the C ABI, in x's dtype: the tensor to keep alive and (ptr, Bn, Ln, stride)."""
        if xn is None:
            return None, (None, 0, 0, 0)
        self._on_device(xn)
        if xn.dtype != x.dtype:
            xn = xn.to(x.dtype)
        xn, xns = _rows(xn)
        return xn, (xn.data_ptr(), xn.shape[0], xn.shape[1], xns)

    def _mask(self, B, T, save_mask, mask_out=None):
        """The final mask (B, T, FS) float32, natural bin order: None unless asked for, mask_out (validated) when given."""
        if not save_mask and mask_out is None:
            return None
        FS = (self.n_bins + 15) // 16 * 16
        mask = mask_out if mask_out is not None else torch.empty((B, T, FS), dtype=torch.float32, device=self.device)
        if mask.shape != (B, T, FS) or mask.dtype != torch.float32 or not mask.is_contiguous():
            raise ValueError("mask_out must be a contiguous (B, T, FS) float32 tensor")
        return mask

    def _saved_mask(self, mask):
        """The mask a backward call is given: the library reads B x T x FS float32 from its data_ptr()."""
        self._on_device(mask)
        return _dense(mask, "mask", dtype=torch.float32)

    def _grad_x(self, B, L, dtype):
        return torch.empty((B, L), dtype=dtype, device=self.device)

    @staticmethod
    def _lengths(lengths, count):
        """Host int64 array for the C ABI (None stays None: every row full)."""
        if lengths is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        if a.shape[0] != count:
            raise ValueError(f"expected {count} lengths, got {a.shape[0]}")
        return a, a.ctypes.data_as(c_void_p)

    def process_batch(self, x, xn=None, out_dtype=None, save_mask=False):
        """TorchGate.forward.  With save_mask=True also returns the final mask
        (B, T, FS) float32 needed by process_batch_backward."""
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        Lout = self.output_length(L)
        out = torch.empty((B, Lout), dtype=out_dtype or x.dtype, device=self.device)
        mask = self._mask(B, self.n_frames(L), save_mask) if save_mask else None
        xn, noise = self._noise(x, xn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_batch(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, *noise, out.data_ptr(), _sg_dtype(out), Lout,
                None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if save_mask else out

    def process_batch_backward(self, grad_out, mask, L):
        """Adjoint of process_batch with the mask fixed: (B, Lout) -> (B, L)."""
        self._on_device(grad_out)
        self._saved_mask(mask)
        grad_out, gs = _rows(grad_out)
        B = grad_out.shape[0]
        gx = self._grad_x(B, L, grad_out.dtype)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_batch_backward(
                self._h, grad_out.data_ptr(), _sg_dtype(grad_out), B, L, gs, mask.data_ptr(),
                gx.data_ptr(), L, self._stream()))
        return gx

    # -- variant T: the gated spectrogram (sg_gate_spectrum) ---------------------------------------
    def gate_spectrum(self, x, xn=None, save_mask=False, out=None, mask_out=None):
        """TorchGate.gated_stft: x (B, L) float32 / float64 -> (B, T, F, 2) real pairs of x.dtype, torch.stft's storage
        (``torch.view_as_complex(Y).transpose(1, 2)`` is the (B, F, T) spectrogram).  With save_mask=True also the final
        mask (B, T, FS) float32, natural bin order.  out / mask_out: contiguous tensors of those shapes to write into."""
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        T = self.n_frames(L)
        if out is None:
            out = torch.empty((B, T, self.n_bins, 2), dtype=x.dtype, device=self.device)
        elif out.shape != (B, T, self.n_bins, 2) or out.dtype != x.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous (B, T, F, 2) tensor of x.dtype")
        mask = self._mask(B, T, save_mask, mask_out)
        xn, noise = self._noise(x, xn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_spectrum(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, *noise, out.data_ptr(),
                None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if mask is not None else out

    def gate_spectrum_backward(self, grad, mask, L, out=None):
        """Adjoint of gate_spectrum with the mask fixed: grad (B, T, F, 2) real pairs -> (B, L) of grad.dtype.
        out: a (B, L) tensor (rows may be strided) to write into."""
        self._on_device(grad)
        self._saved_mask(mask)
        grad = grad.contiguous()
        B = grad.shape[0]
        if out is None:
            out = self._grad_x(B, L, grad.dtype)
        elif out.shape != (B, L) or out.dtype != grad.dtype or (L > 1 and out.stride(1) != 1):
            raise ValueError("out must be a (B, L) tensor of grad.dtype with contiguous rows")
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_spectrum_backward(
                self._h, grad.data_ptr(), _sg_dtype(grad), B, L, mask.data_ptr(), out.data_ptr(),
                out.stride(0) if B > 1 else L, self._stream()))
        return out

    # -- variant T: gated filterbank features (sg_set_filterbank / sg_gate_features) ------------------
    def set_filterbank(self, fb, key=None):
        """The handle's filterbank: fb (F, M) float32, C-contiguous host array.  ``key`` is remembered as ``fb_key`` so
        that callers sharing a cached handle can tell whose bank it holds.  Synchronises the device when it replaces a
        bank."""
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        if fb.ndim != 2 or fb.shape[0] != self.n_bins:
            raise ValueError(f"filterbank must be ({self.n_bins}, M), got {fb.shape}")
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_set_filterbank(self._h, fb.ctypes.data, fb.shape[1]))   # a refused bank leaves the earlier one
        self.fb_key, self.n_filters = key, fb.shape[1]

    def gate_features(self, x, xn=None, power=2, log=False, eps=1e-6, save_mask=False):
        """TorchGate.gated_filterbank: x (B, L) float32 / float64 -> (B, T, M) of x.dtype, the filters contiguous
        (``.transpose(1, 2)`` is the (B, M, T) feature map).  With save_mask=True also the final mask (B, T, FS) float32,
        natural bin order, for gate_features_backward."""
        if not self.n_filters:
            raise RuntimeError("no filterbank set (set_filterbank)")
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        T = self.n_frames(L)
        out = torch.empty((B, T, self.n_filters), dtype=x.dtype, device=self.device)
        mask = self._mask(B, T, save_mask)
        xn, noise = self._noise(x, xn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_features(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, *noise, int(power), int(bool(log)), float(eps),
                out.data_ptr(), None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if save_mask else out

    def gate_features_backward(self, x, grad, mask, power=2, log=False, eps=1e-6):
        """Adjoint of gate_features w.r.t. x with the mask and the bank fixed: grad (B, T, M) -> (B, L) of x.dtype.  x,
        power, log, eps: the forward call's."""
        if not self.n_filters:
            raise RuntimeError("no filterbank set (set_filterbank)")
        self._on_device(x)
        self._on_device(grad)
        self._saved_mask(mask)
        x, xs = _rows(x)
        B, L = x.shape
        grad = grad.to(x.dtype).contiguous()
        if grad.shape != (B, self.n_frames(L), self.n_filters):
            raise ValueError(f"grad must be (B, T, M) = {(B, self.n_frames(L), self.n_filters)}, got {tuple(grad.shape)}")
        out = self._grad_x(B, L, x.dtype)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_features_backward(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, grad.data_ptr(), mask.data_ptr(), int(power),
                int(bool(log)), float(eps), out.data_ptr(), L, self._stream()))
        return out

    # -- variant T: padded batches of different-length rows (sg_process_rows) ------------------------
    def process_rows(self, x, lengths, xn=None, xn_lengths=None, out_dtype=None, save_mask=False):
        """TorchGate.forward on a padded batch: row i holds lengths[i] samples (host integers) and padding after
        them.  Returns (B, output_length(L)); row i is the gate of x[i, :lengths[i]] alone, zeros beyond
        hop * (lengths[i] // hop).  With save_mask=True also the (B, T, FS) float32 mask (natural bin order, frames
        beyond the row's own zero) for process_rows_backward."""
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        Lout = self.output_length(L)
        out = torch.empty((B, Lout), dtype=out_dtype or x.dtype, device=self.device)
        mask = self._mask(B, self.n_frames(L), save_mask) if save_mask else None
        xn, (xn_ptr, Bn, Ln, xns) = self._noise(x, xn)
        la, lp = self._lengths(lengths, B)
        na, np_ = self._lengths(xn_lengths if xn is not None else None, Bn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_rows(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, lp, xn_ptr, Bn, Ln, xns, np_, out.data_ptr(),
                _sg_dtype(out), Lout, None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if save_mask else out

    def process_rows_backward(self, grad_out, mask, L, lengths):
        """Adjoint of process_rows with the mask fixed: (B, Lout) -> (B, L), zero at and beyond lengths[i]."""
        self._on_device(grad_out)
        self._saved_mask(mask)
        grad_out, gs = _rows(grad_out)
        B = grad_out.shape[0]
        gx = self._grad_x(B, L, grad_out.dtype)
        la, lp = self._lengths(lengths, B)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_rows_backward(
                self._h, grad_out.data_ptr(), _sg_dtype(grad_out), B, L, gs, lp, mask.data_ptr(),
                gx.data_ptr(), L, self._stream()))
        return gx

    def gate_spectrum_rows(self, x, lengths, xn=None, xn_lengths=None, save_mask=False):
        """TorchGate.gated_stft on a padded batch (sg_gate_spectrum_rows): row i holds lengths[i] samples (host integers)
        and padding after them.  Returns (B, T, F, 2) real pairs of x.dtype, torch.stft's storage; frames
        [0, 1 + lengths[i] // hop) of row i are the gated spectrum of x[i, :lengths[i]] alone, the frames after them
        zero.  With save_mask=True also the (B, T, FS) float32 mask process_rows returns (natural bin order, frames
        beyond the row's own zero) for gate_spectrum_rows_backward."""
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        T = self.n_frames(L)
        out = torch.empty((B, T, self.n_bins, 2), dtype=x.dtype, device=self.device)
        mask = self._mask(B, T, save_mask)
        xn, (xn_ptr, Bn, Ln, xns) = self._noise(x, xn)
        la, lp = self._lengths(lengths, B)
        na, np_ = self._lengths(xn_lengths if xn is not None else None, Bn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_spectrum_rows(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, lp, xn_ptr, Bn, Ln, xns, np_, out.data_ptr(),
                None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if save_mask else out

    def gate_spectrum_rows_backward(self, grad, mask, L, lengths):
        """Adjoint of gate_spectrum_rows with the mask fixed: grad (B, T, F, 2) real pairs -> (B, L) of grad.dtype, zero
        at and beyond lengths[i]; grad[i, 1 + lengths[i] // hop:] is never read."""
        self._on_device(grad)
        self._saved_mask(mask)
        grad = grad.contiguous()
        B = grad.shape[0]
        gx = self._grad_x(B, L, grad.dtype)
        la, lp = self._lengths(lengths, B)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_spectrum_rows_backward(
                self._h, grad.data_ptr(), _sg_dtype(grad), B, L, lp, mask.data_ptr(), gx.data_ptr(), L,
                self._stream()))
        return gx

    def gate_features_rows(self, x, lengths, xn=None, xn_lengths=None, power=2, log=False, eps=1e-6, save_mask=False):
        """TorchGate.gated_filterbank on a padded batch (sg_gate_features_rows): row i holds lengths[i] samples (host
        integers) and padding after them.  Returns (B, T, M) of x.dtype, the filters contiguous; frames
        [0, 1 + lengths[i] // hop) of row i are the features of x[i, :lengths[i]] alone, the frames after them 0 (ln(eps)
        with log).  With save_mask=True also the (B, T, FS) float32 mask gate_spectrum_rows returns, for
        gate_features_rows_backward."""
        if not self.n_filters:
            raise RuntimeError("no filterbank set (set_filterbank)")
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        T = self.n_frames(L)
        out = torch.empty((B, T, self.n_filters), dtype=x.dtype, device=self.device)
        mask = self._mask(B, T, save_mask)
        xn, (xn_ptr, Bn, Ln, xns) = self._noise(x, xn)
        la, lp = self._lengths(lengths, B)
        na, np_ = self._lengths(xn_lengths if xn is not None else None, Bn)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_features_rows(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, lp, xn_ptr, Bn, Ln, xns, np_, int(power), int(bool(log)),
                float(eps), out.data_ptr(), None if mask is None else mask.data_ptr(), self._stream()))
        return (out, mask) if save_mask else out

    def gate_features_rows_backward(self, x, grad, mask, lengths, power=2, log=False, eps=1e-6):
        """Adjoint of gate_features_rows w.r.t. x with the mask and the bank fixed: grad (B, T, M) -> (B, L) of x.dtype,
        zero at and beyond lengths[i]; grad[i, 1 + lengths[i] // hop:] is never read.  x, lengths, power, log, eps: the
        forward call's."""
        if not self.n_filters:
            raise RuntimeError("no filterbank set (set_filterbank)")
        self._on_device(x)
        self._on_device(grad)
        self._saved_mask(mask)
        x, xs = _rows(x)
        B, L = x.shape
        grad = grad.to(x.dtype).contiguous()
        if grad.shape != (B, self.n_frames(L), self.n_filters):
            raise ValueError(f"grad must be (B, T, M) = {(B, self.n_frames(L), self.n_filters)}, got {tuple(grad.shape)}")
        gx = self._grad_x(B, L, x.dtype)
        la, lp = self._lengths(lengths, B)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_gate_features_rows_backward(
                self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, lp, grad.data_ptr(), mask.data_ptr(), int(power),
                int(bool(log)), float(eps), gx.data_ptr(), L, self._stream()))
        return gx

    def rows_batches(self):
        v = c_int64()
        self._check(self.lib.sg_debug_rows_batches(self._h, byref(v)))
        return int(v.value)

    def backward_route(self):
        """SG_BWD_* (include/mi355gate_debug.h) of the last backward call on this handle: 1 k_row_backward, 2 tiled
        k_apply_fast, 3 register apply kernels, 4 k_apply_istft + k_ola, 5 rw_backward; 0 before any."""
        v = c_int64()
        self._check(self.lib.sg_debug_backward_route(self._h, byref(v)))
        return int(v.value)

    # -- ragged batches (sg_process_clips) ---------------------------------------------------------
    def process_clips(self, x, clips, out, noise=None, noise_srcs=(), max_workspace_bytes=0):
        """x, out: 1-D device tensors holding every clip (offsets / strides in `clips`, a sequence of SgClip);
        noise: 1-D device tensor or None; noise_srcs: sequence of SgNoiseSrc."""
        self._on_device(x)
        self._on_device(out)
        _dense(x, "x")
        _dense(out, "out")
        n_clips = len(clips)
        carr = (SgClip * max(1, n_clips))(*clips)
        narr = (SgNoiseSrc * max(1, len(noise_srcs)))(*noise_srcs)
        if noise is not None:
            self._on_device(noise)
            _dense(noise, "noise")
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_process_clips(
                self._h, x.data_ptr(), _sg_dtype(x), None if noise is None else noise.data_ptr(),
                SG_F64 if noise is None else _sg_dtype(noise), narr, len(noise_srcs), carr, n_clips, out.data_ptr(),
                _sg_dtype(out), int(max_workspace_bytes), self._stream()))
        return out

    def clips_workspace_bytes(self, clips, noise_srcs=()):
        """Workspace bytes process_clips needs for `clips` in one sub-batch (what max_workspace_bytes is compared with)."""
        carr = (SgClip * max(1, len(clips)))(*clips)
        narr = (SgNoiseSrc * max(1, len(noise_srcs)))(*noise_srcs)
        out = c_int64()
        self._check(self.lib.sg_clips_workspace_bytes(self._h, narr, len(noise_srcs), carr, len(clips), byref(out)))
        return out.value

    def clip_thresholds(self, n_noise):
        """(n_noise, F) float64 thresholds of the last process_clips call (synchronises)."""
        out = np.empty((int(n_noise), self.n_bins), dtype=np.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_debug_clip_thresholds(self._h, out.ctypes.data_as(POINTER(c_double)), int(n_noise),
                                                          self.n_bins, self._stream()))
        return out

    def clip_batches(self):
        v = c_int64()
        self._check(self.lib.sg_debug_clip_batches(self._h, byref(v)))
        return int(v.value)

    # -- banks of live streams (sg_stream_*) --------------------------------------------------------
    def stream_create(self, n_slots, channels, max_block):
        b = c_void_p()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_create(self._h, int(n_slots), int(channels), int(max_block), byref(b)))
        return b

    def stream_create_nonstationary(self, n_slots, channels, max_block, lookahead_frames):
        b = c_void_p()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_create_nonstationary(self._h, int(n_slots), int(channels), int(max_block),
                                                                int(lookahead_frames), byref(b)))
        return b

    def stream_create_adaptive(self, n_slots, channels, max_block, forget, learn_frames):
        """forget: per-frame factor in (0, 1]; learn_frames: >= 1, or negative for unlimited."""
        b = c_void_p()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_create_adaptive(self._h, int(n_slots), int(channels), int(max_block),
                                                           float(forget), int(learn_frames), byref(b)))
        return b

    @staticmethod
    def stream_desc(n_slots, channels, max_block, kind=SG_STREAM_FIXED, lookahead_frames=0, forget=1.0, learn_frames=-1,
                    exact=False):
        return SgStreamDesc(n_slots=int(n_slots), channels=int(channels), max_block=int(max_block), kind=int(kind),
                            lookahead_frames=int(lookahead_frames), forget=float(forget), learn_frames=int(learn_frames),
                            exact=int(bool(exact)))

    def stream_create_ex(self, desc):
        """desc: SgStreamDesc (stream_desc(...)).  exact=True: a bank that takes and returns every sample type exactly."""
        b = c_void_p()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_create_ex(self._h, byref(desc), byref(b)))
        return b

    def stream_state_bytes_ex(self, desc):
        v = c_int64()
        self._check(self.lib.sg_stream_state_bytes_ex(self._h, byref(desc), byref(v)))
        return int(v.value)

    def stream_noise_profile(self, bank, slot, channels):
        """(channels, n_bins) float64 dB thresholds of an adaptive bank's slot (synchronises the current stream)."""
        out = np.empty((int(channels), self.n_bins), dtype=np.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_noise_profile(bank, int(slot), out.ctypes.data_as(POINTER(c_double)),
                                                         self.n_bins, self._stream()))
        return out

    def stream_state_bytes(self, n_slots, channels, max_block, lookahead_frames=0, adaptive=False):
        v = c_int64()
        if adaptive:
            self._check(self.lib.sg_stream_state_bytes_adaptive(self._h, int(n_slots), int(channels), int(max_block),
                                                                byref(v)))
            return int(v.value)
        self._check(self.lib.sg_stream_state_bytes(self._h, int(n_slots), int(channels), int(max_block),
                                                   int(lookahead_frames), byref(v)))
        return int(v.value)

    def stream_bank_emitted(self, bank, n):
        v = c_int64()
        self._check(self.lib.sg_stream_bank_emitted(bank, int(n), byref(v)))
        return int(v.value)

    def stream_destroy(self, bank):
        if bank is not None and bank.value and self._h.value:
            with torch.cuda.device(self.device):
                self.lib.sg_stream_destroy(bank)

    def stream_set_threshold(self, bank, slots, thresh=None):
        """thresh: n_bins dB values (host), or None for the handle's current threshold on the device."""
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        tp, t = None, None
        if thresh is not None:
            t = np.ascontiguousarray(np.asarray(thresh, dtype=np.float64).reshape(-1))
            if t.shape[0] != self.n_bins:
                raise ValueError(f"thresholds_db must hold n_fft // 2 + 1 = {self.n_bins} values")
            tp = t.ctypes.data_as(c_void_p)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_set_threshold(bank, sl.ctypes.data_as(c_void_p), int(sl.shape[0]), tp,
                                                         self.n_bins, self._stream()))

    def stream_push(self, bank, x, out, recs):
        """x, out: 1-D float32 / float64 device tensors (an exact bank: int16 / int32 too); recs: sequence of SgStreamRec.
        Enqueues only."""
        self._on_device(x)
        self._on_device(out)
        _dense(x, "x")
        _dense(out, "out")
        arr = (SgStreamRec * max(1, len(recs)))(*recs)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_push(bank, x.data_ptr(), _sg_dtype(x), out.data_ptr(), _sg_dtype(out), arr,
                                                len(recs), self._stream()))

    def stream_push_spectrum(self, bank, x, out, spec, mask, recs, spec_recs):
        """stream_push that also stores every newly applied frame's gated spectrum: spec a 1-D complex64 / complex128
        device tensor, mask None or a 1-D real tensor of spec's real type, spec_recs a sequence of SgStreamSpecRec
        parallel to recs.  Enqueues only."""
        if spec.dtype not in (torch.complex64, torch.complex128):
            raise TypeError(f"stream_push_spectrum: spec is complex64 or complex128 (got {spec.dtype})")
        real = torch.float32 if spec.dtype == torch.complex64 else torch.float64
        if mask is not None and mask.dtype != real:
            raise TypeError(f"stream_push_spectrum: mask must be {real} next to a {spec.dtype} spec (got {mask.dtype})")
        if len(spec_recs) != len(recs):
            raise ValueError("stream_push_spectrum: recs and spec_recs must have the same length")
        for name, t in (("x", x), ("out", out), ("spec", spec)) + (() if mask is None else (("mask", mask),)):
            self._on_device(t)
            _dense(t, name)
        arr = (SgStreamRec * max(1, len(recs)))(*recs)
        sarr = (SgStreamSpecRec * max(1, len(spec_recs)))(*spec_recs)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_push_spectrum(
                bank, x.data_ptr(), _sg_dtype(x), out.data_ptr(), _sg_dtype(out), spec.data_ptr(),
                _TORCH_DTYPES[real], None if mask is None else mask.data_ptr(), arr, sarr, len(recs), self._stream()))

    def stream_set_filterbank(self, bank, fb):
        """fb: C-contiguous (n_bins, M) float32 numpy array (torchgate.filterbank.check_filterbank's result).  Replacing a
        filterbank synchronises the device."""
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_set_filterbank(bank, fb.ctypes.data_as(c_void_p), int(fb.shape[1])))

    def stream_push_features(self, bank, x, out, feat, mask, recs, feat_recs, power, take_log, eps, scale):
        """stream_push that also stores every newly applied frame's filterbank features: feat a 1-D float32 / float64
        device tensor, mask None or a 1-D tensor of feat's type, feat_recs a sequence of SgStreamFeatRec parallel to recs;
        scale 0.0: the bank's own 1 / sum(window).  Enqueues only."""
        if feat.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"stream_push_features: feat is float32 or float64 (got {feat.dtype})")
        if mask is not None and mask.dtype != feat.dtype:
            raise TypeError(f"stream_push_features: mask must be {feat.dtype} next to such a feat (got {mask.dtype})")
        if len(feat_recs) != len(recs):
            raise ValueError("stream_push_features: recs and feat_recs must have the same length")
        for name, t in (("x", x), ("out", out), ("feat", feat)) + (() if mask is None else (("mask", mask),)):
            self._on_device(t)
            _dense(t, name)
        arr = (SgStreamRec * max(1, len(recs)))(*recs)
        farr = (SgStreamFeatRec * max(1, len(feat_recs)))(*feat_recs)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_push_features(
                bank, x.data_ptr(), _sg_dtype(x), out.data_ptr(), _sg_dtype(out), feat.data_ptr(), _TORCH_DTYPES[feat.dtype],
                None if mask is None else mask.data_ptr(), int(power), int(bool(take_log)), float(eps), float(scale),
                arr, farr, len(recs), self._stream()))

    def stream_bank_frames(self, bank, n):
        v = c_int64(0)
        self._check(self.lib.sg_stream_bank_frames(bank, int(n), byref(v)))
        return v.value

    def stream_reset(self, bank, slots):
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_reset(bank, sl.ctypes.data_as(c_void_p), int(sl.shape[0]), self._stream()))

    def stream_emitted(self, n):
        v = c_int64()
        self._check(self.lib.sg_stream_emitted(self._h, int(n), byref(v)))
        return int(v.value)

    def stream_counters(self, bank, slot):
        n, e = c_int64(), c_int64()
        self._check(self.lib.sg_stream_counters(bank, int(slot), byref(n), byref(e)))
        return int(n.value), int(e.value)

    def stream_export_bytes(self, bank, slot):
        """Bytes of the slot's state payload right now (host arithmetic from its counters)."""
        v = c_int64()
        self._check(self.lib.sg_stream_export_bytes(bank, int(slot), byref(v)))
        return int(v.value)

    def stream_export(self, bank, slots, blob, offsets):
        """blob: 1-D uint8 device tensor; slot i's payload goes to byte offsets[i] (multiples of 256).  Returns the
        SgStreamHead of every slot.  One launch; enqueues only."""
        self._on_device(blob)
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        heads = (SgStreamHead * max(1, sl.shape[0]))()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_export(bank, sl.ctypes.data_as(c_void_p), int(sl.shape[0]), blob.data_ptr(),
                                                  off.ctypes.data_as(c_void_p), heads, self._stream()))
        return [heads[i] for i in range(sl.shape[0])]

    def stream_import(self, bank, slots, blob, offsets, heads):
        """The reverse of stream_export into `slots` of a compatible bank.  One launch; enqueues only."""
        self._on_device(blob)
        sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).reshape(-1))
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        arr = (SgStreamHead * max(1, len(heads)))(*heads)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stream_import(bank, sl.ctypes.data_as(c_void_p), int(sl.shape[0]), blob.data_ptr(),
                                                  off.ctypes.data_as(c_void_p), arr, self._stream()))

    def set_option(self, option, value):
        self._check(self.lib.sg_set_option(self._h, int(option), int(value)))

    def get_option(self, option):
        """The option's current value on this (shared, cached) handle, read from the handle itself (sg_get_option):
        the library's default if it was never set -- not every default is 0 (SG_OPT_ROWGATE_SHAPE: 16)."""
        v = c_int64(0)
        rc = self.lib.sg_get_option(self._h, int(option), byref(v))
        if rc != 0:   # (the handle is const in sg_get_option: the library leaves no message of its own)
            raise ValueError(f"sg_get_option: unknown option {int(option)} (rc {rc})")
        return int(v.value)

    @contextlib.contextmanager
    def with_options(self, pairs):
        """`with g.with_options([(SG_OPT_X, 1), ...]):` -- sets the options and RESTORES their previous values (the
        handle is shared between objects: a user's or a test's setting must survive somebody else's retry)."""
        prev = [(o, self.get_option(o)) for o, _ in pairs]
        try:
            for o, v in pairs:
                self.set_option(o, v)
            yield self
        finally:
            for o, v in prev:
                self.set_option(o, v)

    def check_errors(self):
        """Synchronise the current stream and raise HandoffTimeout if a launch enqueued on this handle since the
        last check lost an in-launch hand-off (include/mi355gate.h: sg_check_errors)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_check_errors(self._h, self._stream()))

    def run_checked(self, fn):
        """fn() -> device tensor, then check_errors(); a call that lost a hand-off is re-run ONCE on the kernels
        without in-launch hand-offs (three-kernel gate, apply + seam kernel).  For callers that synchronise
        anyway (host arrays out); holds the handle's lock."""
        with self.lock:
            # an error left behind by an EARLIER unchecked (tensor-in / tensor-out) call on this shared handle belongs to
            # that call: report it as such instead of "fixing" it with a retry of this one
            try:
                self.check_errors()
            except HandoffTimeout as e:
                raise HandoffTimeout("an earlier, unchecked call on this engine handle lost a tile hand-off (its output "
                                     "is invalid); this call has not run: " + str(e)) from None
            try:
                out = fn()
                self.check_errors()
                return out
            except HandoffTimeout:
                with self.with_options([(SG_OPT_FORCE_SPLIT, 1), (SG_OPT_FORCE_NOLEAN, 1)]):
                    out = fn()
                    self.check_errors()
                    return out

    # -- per-kernel timing -----------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.sg_profile_enable(self._h, int(bool(on))))

    def profile_select(self, stage_names=None):
        """Time only the named stages (names as returned by profile_read); None = all."""
        mask = 0
        if stage_names:
            names = [self.lib.sg_stage_name(i).decode() for i in range(SG_N_STAGES_ALL)]
            for n in stage_names:
                mask |= 1 << names.index(n)
        self._check(self.lib.sg_profile_select(self._h, mask))

    def profile_read(self, reset=True):
        """{stage name: (total ms, launches)} accumulated since the last reset (synchronises)."""
        ms = (c_double * SG_N_STAGES_ALL)()
        cnt = (c_int64 * SG_N_STAGES_ALL)()
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_profile_read(self._h, ms, cnt, SG_N_STAGES_ALL, int(bool(reset))))
        return {self.lib.sg_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(SG_N_STAGES_ALL)
                if cnt[i]}

    # -- stage taps ------------------------------------------------------------------
    def stft(self, x):
        """(B, L) -> complex128 (B, T, F), scaled like the variant's reference STFT."""
        self._on_device(x)
        x, xs = _rows(x)
        B, L = x.shape
        T = self.n_frames(L)
        z = torch.empty((B, T, self.n_bins, 2), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_stft(self._h, x.data_ptr(), _sg_dtype(x), B, L, xs, z.data_ptr(),
                                         self._stream()))
        return torch.view_as_complex(z)

    def debug_range(self):
        r = (c_int64 * 2)()
        self._check(self.lib.sg_debug_range(self._h, r))
        return int(r[0]), int(r[1])

    def debug_counter(self, which=0, value=0):
        """0: (row, band) pairs the row gate re-evaluated in float64 since the handle was created; 1 / 2: batches of the
        one-pass gate that took the in-kernel / the a-priori floor test (SG_OPT_FLOOR_TEST); 3: launch epoch of the last gate
        call in which a chunk's floor test fired."""
        v = c_int64(int(value))   # (in: an argument of the development counters; 0 for the documented ones)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_debug_counter(self._h, int(which), ctypes.byref(v), self._stream()))
        return int(v.value)

    def stats_route(self):
        """The form of the last noise statistics of fewer than 16 units on this handle: 1 = k_stft<double> + k_colstats1 +
        k_colstats1_final, 2 = k_noise_moments + k_colstats1_final, 0 = none yet -- sg_debug_counter(19), host bookkeeping only."""
        return self.debug_counter(19)

    def floor_route(self):
        """The floor fix-up of the last one-pass gate call on this handle: 1 = one launch (k_floor_fix), 2 = two launches
        (k_stft_bits<max> + the gate's REDO instantiation, SG_OPT_FLOOR_TWO_LAUNCH), 0 = that call took the a-priori floor
        test, or none yet -- sg_debug_counter(20), host bookkeeping only."""
        return self.debug_counter(20)

    def gate_consts(self):
        """``(T2, alim)`` of the last noise_stats call: the power-domain compare constant per band (n_bins,) float64 and the
        float32 bounds on max|x| of the floor test per block of 64 bands -- sg_debug_fetch(5)."""
        host = np.empty(self.n_bins * 8 + 256, dtype=np.uint8)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_debug_fetch(self._h, 5, host.ctypes.data_as(c_void_p), host.nbytes, self._stream()))
        t2 = host[:self.n_bins * 8].view(np.float64).copy()
        words = host[self.n_bins * 8:].view(np.uint32)
        return t2, words[2:2 + (self.n_bins + 63) // 64].view(np.float32).copy()

    def smooth_route(self):
        """The mask smoothing of the last gate call on this handle: ``(kernel name, bytes of the cell it sums in, output
        frames per tile)`` -- sg_debug_counter(17), host bookkeeping only."""
        v = self.debug_counter(17)
        return SG_SMOOTH_NAMES[v & 0xff], (v >> 8) & 0xff, v >> 16

    def spectrum_route(self):
        """The route of the last gate_spectrum call on this handle: ``(decide branch, through k_spec_bits_to_raw, smoothed
        straight into the caller's mask, sub-batches)`` -- sg_debug_counter(18), host bookkeeping only.  ("none", False,
        False, 0): the call failed before its first spectrum launch."""
        v = self.debug_counter(18)
        return SG_SPEC_NAMES[v & 0xff], bool(v & 0x100), bool(v & 0x200), v >> 16

    def debug_field(self, what):
        """0: raw mask, 1: final mask (float32); 2: power (float64) of the last unit batch,
        as (units, T, F) numpy arrays."""
        dims = (c_int64 * 3)()
        self._check(self.lib.sg_debug_dims(self._h, dims))
        units, T, FS = dims[0], dims[1], dims[2]
        if what == 4:  # row gate: float32 power tile (4 |X|^2) of pass 1, (units, 64, 528); rows >= T are scratch
            host = np.empty((units, 64, 528), dtype=np.float32)
            with torch.cuda.device(self.device):
                self._check(self.lib.sg_debug_fetch(self._h, 4, host.ctypes.data_as(c_void_p), host.nbytes,
                                                    self._stream()))
            return host[:, :T, :self.n_bins]
        if what == 3:  # bit field -> boolean (units, T, F)
            wpr = (self.n_bins + 63) // 64
            words = np.empty((units, T, wpr), dtype=np.uint64)
            with torch.cuda.device(self.device):
                self._check(self.lib.sg_debug_fetch(self._h, 3, words.ctypes.data_as(c_void_p),
                                                    words.nbytes, self._stream()))
            b = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
            return b[:, :, :self.n_bins].astype(bool)
        dt = np.float64 if what == 2 else np.float32
        host = np.empty((units, T, FS), dtype=dt)
        with torch.cuda.device(self.device):
            self._check(self.lib.sg_debug_fetch(self._h, int(what), host.ctypes.data_as(c_void_p),
                                                host.nbytes, self._stream()))
        return host[:, :, :self.n_bins]


# Handles are cached per (device, parameters): a handle owns its twiddle/window tables and a
# grown-on-demand workspace, so repeated reduce_noise()/TorchGate calls with the same settings
# reuse them instead of paying hipMalloc/hipFree per call.  The cache itself is guarded by
# _CACHE_LOCK; a handle is NOT re-entrant: users hold Gate.lock around a call sequence that depends on
# handle state (noise statistics -> filter).  The stationary threshold is per OBJECT (reference
# stationary.py:79-81), never per handle: objects re-load theirs when Gate.thresh_owner is not them.
_GATE_CACHE = {}
_CACHE_LOCK = threading.Lock()


def cached_gate(device, slot=0, **kw):
    """`slot` distinguishes handles with identical parameters: calls that are in flight at the same time
    on different streams must not share a handle (its workspace is per call)."""
    dev = resolve_device(device)
    # integer recordings: the reference truncates a float64 result (base.py:217-226) -> float64 pipeline by default;
    # NOISEREDUCE_AMD_FAST_INT=1 keeps the fused float32 kernels (<= 1 LSB off on ~1 % of the samples)
    kw.setdefault("fast_integer", os.environ.get("NOISEREDUCE_AMD_FAST_INT", "0") == "1")
    # precision="float64" / NOISEREDUCE_AMD_EXACT=1: the float64 pipeline for every sample type -- a float64 recording then
    # gets float64-accurate results like the reference's (base.py:140 computes every dtype in float64) instead of
    # float32-accurate ones in a float64 container (the default: 14 x faster, 2e-7 of peak off)
    if kw.get("exact") is None:
        kw["exact"] = os.environ.get("NOISEREDUCE_AMD_EXACT", "0") == "1"

    def norm(v):
        if isinstance(v, np.ndarray):
            return ("nd", v.shape, v.tobytes())
        if isinstance(v, (bool, np.bool_)):
            return bool(v)
        if isinstance(v, (int, np.integer)):
            return int(v)
        if isinstance(v, (float, np.floating)):
            return float(v)
        return v
    key = (dev.index, int(slot)) + tuple(sorted((k, norm(v)) for k, v in kw.items()))
    with _CACHE_LOCK:
        g = _GATE_CACHE.get(key)
        if g is None:
            if len(_GATE_CACHE) >= 8:  # bound the number of cached workspaces
                # dropped, not closed: an object that still holds the evicted gate keeps it alive, and
                # Gate.__del__ frees the handle with the last reference
                _GATE_CACHE.pop(next(iter(_GATE_CACHE)))
            g = Gate(dev, **kw)
            _GATE_CACHE[key] = g
        return g


def clear_gate_cache():
    with _CACHE_LOCK:
        while _GATE_CACHE:
            _GATE_CACHE.popitem()[1].close()
