"""``TorchGate`` -- nn.Module with the constructor, buffer and forward contract of
/root/reference/noisereduce/torchgate/torchgate.py:7-264, evaluated by the HIP engine
(sg_process_batch).  0 parameters, one buffer ``smoothing_filter`` of shape
(1, 1, 2*n_grad_freq+1, 2*n_grad_time+1) (or None), so state_dicts round-trip with the
reference's.  The mask is computed without gradient (torchgate.py:126,167) and the output
is differentiable w.r.t. ``x`` through STFT -> (x mask) -> ISTFT.

``forward``, ``gated_stft`` and ``gated_filterbank`` share one call path.  ``TorchGate._prepare`` validates and normalises
every call (the errors and their order, the dtype promotion, the noise rows, the host lengths, whether the rows are in fact
all full), and ``_NativeFunction`` is the one ``autograd.Function`` of the native routes, driven by a row of ``_ROUTES``
(which ``_ffi.Gate`` methods, whether lengths ride along, whether the mask is an output, whether x is saved).  A further
native output is a row of that table and a kernel.  The fallbacks for an n_fft without native kernels -- the per-row loops,
the composed ``torch.stft * mask`` and the composed filterbank matmul -- take their inputs from the same ``_prepare``.
"""
import collections
import hashlib
import math
import weakref
from typing import Optional, Union

import torch

from noisereduce_amd import _ffi
from noisereduce_amd.torchgate import filterbank as _fbank
from noisereduce_amd.torchgate import rows as _rows
from noisereduce_amd.torchgate.utils import linspace


# How a native route is called (_ffi.Gate): the forward and backward methods, whether the host lengths ride along, whether
# the mask is an output of the call (else it is kept for the backward only), and whether the backward needs x again.
_Route = collections.namedtuple("_Route", "fwd bwd lengths mask_out save_x")
_ROUTES = {
    "waveform": _Route("process_batch", "process_batch_backward", False, False, False),
    "waveform_rows": _Route("process_rows", "process_rows_backward", True, False, False),        # csrc/rows.hip
    "spectrum": _Route("gate_spectrum", "gate_spectrum_backward", False, True, False),           # csrc/spec.hip
    "spectrum_rows": _Route("gate_spectrum_rows", "gate_spectrum_rows_backward", True, True, False),
    "features": _Route("gate_features", "gate_features_backward", False, True, True),            # csrc/feat.hip
    "features_rows": _Route("gate_features_rows", "gate_features_rows_backward", True, True, True),   # csrc/rows_feat.hip
}

_NO_KW = {}   # (the routes without keyword arguments)


def _bind_bank(gate, bank):
    """The handle holds this bank (handles are shared between modules of equal parameters: the caller holds gate.lock)."""
    if gate.fb_key != bank["digest"]:
        gate.set_filterbank(bank["host"], key=bank["digest"])


def _engine(gate, bank, method, args, kw):
    """One call into the engine; with a bank (the features route) under gate.lock, the bank bound again first."""
    if bank is None:
        return getattr(gate, method)(*args, **kw)
    with gate.lock:
        _bind_bank(gate, bank)
        return getattr(gate, method)(*args, **kw)


class _NativeFunction(torch.autograd.Function):
    """Every native route of forward, gated_stft and gated_filterbank.  ``call`` is one tuple (autograd's apply costs a
    quarter of a microsecond per argument): the module, ``route`` (a row of _ROUTES), ``lengths`` / ``xn_lengths`` (host
    int64 arrays or None; the backward gets the same lengths), ``bank`` (the entry of TorchGate._bank, host array and
    digest, or None) and ``kw`` (the power / log / eps of the features route, {} otherwise).

    The waveform routes return y and ask for the mask only when x needs a gradient: the call without one does not write
    it.  The spectrum and feature routes always return the mask, which carries no gradient: the real pairs (B, T, F, 2)
    -- torch.view_as_complex is applied outside, so the complex autograd convention stays torch's -- or the features
    (B, T, M).  The features route saves x and the mask: its backward transforms the frames again, so nothing of size
    B x T x F is kept but the mask."""

    @staticmethod
    def forward(ctx, x, xn, call):
        module, route, lengths, xn_lengths, bank, kw = call
        gate = module._gate_for(x.device)
        args = (x, lengths, xn, xn_lengths) if route.lengths else (x, xn)
        if not (route.mask_out or ctx.needs_input_grad[0]):
            return _engine(gate, bank, route.fwd, args, kw)
        out, mask = _engine(gate, bank, route.fwd, args, dict(kw, save_mask=True))
        ctx.gate, ctx.route, ctx.L, ctx.lengths, ctx.bank, ctx.kw = gate, route, x.shape[-1], lengths, bank, kw
        ctx.save_for_backward(*((x, mask) if route.save_x else (mask,)))
        if not route.mask_out:
            return out
        ctx.mark_non_differentiable(mask)
        return out, mask

    @staticmethod
    def backward(ctx, grad, _grad_mask=None):
        *x, mask = ctx.saved_tensors
        route = ctx.route
        args = (x[0].detach(), grad.contiguous(), mask) if route.save_x else (grad.contiguous(), mask, ctx.L)
        if route.lengths:
            args += (ctx.lengths,)
        return _engine(ctx.gate, ctx.bank, route.bwd, args, ctx.kw), None, None


class TorchGate(torch.nn.Module):
    """A PyTorch module that applies a spectral gate to an input signal (see the reference
    docstring, torchgate.py:8-29, for the arguments)."""

    @torch.no_grad()
    def __init__(self, sr: int, nonstationary: bool = False, n_std_thresh_stationary: float = 1.5,
                 n_thresh_nonstationary: float = 1.3, temp_coeff_nonstationary: float = 0.1,
                 n_movemean_nonstationary: int = 20, prop_decrease: float = 1.0, n_fft: int = 1024,
                 win_length: int = None, hop_length: int = None, freq_mask_smooth_hz: float = 500,
                 time_mask_smooth_ms: float = 50):
        super().__init__()
        self.sr = sr
        self.nonstationary = nonstationary
        assert 0.0 <= prop_decrease <= 1.0
        self.prop_decrease = prop_decrease
        self.n_fft = n_fft
        self.win_length = self.n_fft if win_length is None else win_length
        self.hop_length = self.win_length // 4 if hop_length is None else hop_length
        self.n_std_thresh_stationary = n_std_thresh_stationary
        self.temp_coeff_nonstationary = temp_coeff_nonstationary
        self.n_movemean_nonstationary = n_movemean_nonstationary
        self.n_thresh_nonstationary = n_thresh_nonstationary
        self.freq_mask_smooth_hz = freq_mask_smooth_hz
        self.time_mask_smooth_ms = time_mask_smooth_ms
        self._n_grad = (1, 1)
        self.register_buffer("smoothing_filter", self._generate_mask_smoothing_filter())
        self._gates = {}
        self._banks = {}

    @torch.no_grad()
    def _generate_mask_smoothing_filter(self) -> Union[torch.Tensor, None]:
        """(torchgate.py:73-124).  The reference's error path for a too-small
        freq_mask_smooth_hz dereferences a missing attribute (torchgate.py:94); here it
        raises the ValueError it meant to."""
        if self.freq_mask_smooth_hz is None and self.time_mask_smooth_ms is None:
            return None
        n_grad_freq = (1 if self.freq_mask_smooth_hz is None
                       else int(self.freq_mask_smooth_hz / (self.sr / (self.n_fft / 2))))
        if n_grad_freq < 1:
            raise ValueError(
                f"freq_mask_smooth_hz needs to be at least {int((self.sr / (self.n_fft / 2)))} Hz")
        n_grad_time = (1 if self.time_mask_smooth_ms is None
                       else int(self.time_mask_smooth_ms / ((self.hop_length / self.sr) * 1000)))
        if n_grad_time < 1:
            raise ValueError(
                f"time_mask_smooth_ms needs to be at least {int((self.hop_length / self.sr) * 1000)} ms")
        if n_grad_time == 1 and n_grad_freq == 1:
            return None
        self._n_grad = (n_grad_freq, n_grad_time)
        v_f = torch.cat([linspace(0, 1, n_grad_freq + 1, endpoint=False),
                         linspace(1, 0, n_grad_freq + 2)])[1:-1]
        v_t = torch.cat([linspace(0, 1, n_grad_time + 1, endpoint=False),
                         linspace(1, 0, n_grad_time + 2)])[1:-1]
        smoothing_filter = torch.outer(v_f, v_t).unsqueeze(0).unsqueeze(0)
        return smoothing_filter / smoothing_filter.sum()

    def _gate_for(self, device):
        key = (device.type, device.index)
        g = self._gates.get(key)
        if g is None:
            # The reference builds its Hann window in float32 whatever the input dtype
            # (torchgate.py:150,231,261); hand the engine the same table.
            window = torch.hann_window(self.win_length).double().numpy()
            nf, nt = self._n_grad
            g = _ffi.cached_gate(device, variant=_ffi.SG_VARIANT_T, stationary=not self.nonstationary,
                          n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length,
                          n_grad_freq=nf, n_grad_time=nt,
                          smooth_mask=self.smoothing_filter is not None,
                          prop_decrease=self.prop_decrease,
                          n_std_thresh=self.n_std_thresh_stationary, top_db=40.0, ddof=1,
                          n_movemean=self.n_movemean_nonstationary,
                          nonstat_thresh=self.n_thresh_nonstationary,
                          nonstat_slope=1.0 / self.temp_coeff_nonstationary, window=window)
            self._gates[key] = g
        return g

    def forward(self, x: torch.Tensor, xn: Optional[torch.Tensor] = None, lengths=None,
                xn_lengths=None) -> torch.Tensor:
        """x: (batch, signal_length); xn: optional noise signal(s) for the stationary
        statistics.  Returns (batch, hop*(signal_length//hop)) in x.dtype
        (torchgate.py:200-264).

        lengths: None, or one integer per row (sequence, numpy array, CPU or device tensor -- a device tensor is
        copied to the host, which synchronises) for a zero-padded batch: row i holds ``lengths[i]`` samples,
        ``2 * win_length <= lengths[i] <= signal_length``.  ``y[i, :hop * (lengths[i] // hop)]`` is then what
        ``forward(x[i:i+1, :lengths[i]], xn_i)`` returns -- band statistics, moving mean, mask smoothing and window
        envelope over the row's own frames -- and the rest of the row is 0.  ``x[i, lengths[i]:]`` is never read, a
        row does not depend on the other rows, and the gradient is 0 beyond ``lengths[i]``.  xn_lengths: the same
        for the rows of ``xn`` (1 or batch integers).  When every length equals the padded length the call takes
        the full-length path and is bitwise ``forward(x, xn)``.  Power-of-two n_fft from 256 to 4096 gate the whole
        batch in a fixed number of launches (csrc/rows.hip); any other n_fft loops over the rows through the
        full-length path (correct, one call per row)."""
        assert x.ndim == 2
        xf, dtype, xnf, lengths, xn_lengths, full = self._prepare(x, xn, lengths, xn_lengths, xn_rows=False)
        if not full and not _rows.native(self.n_fft):
            B, L = x.shape
            H = self.hop_length
            y = x.new_zeros((B, H * (L // H)))
            for i in range(B):
                n = L if lengths is None else int(lengths[i])
                y[i, :H * (n // H)] = self.forward(x[i:i + 1, :n], self._noise_of_row(xn, xn_lengths, i))[0]
            return y
        route = _ROUTES["waveform" if full else "waveform_rows"]
        return _NativeFunction.apply(xf, xnf, (self, route, lengths, xn_lengths, None, _NO_KW)).to(dtype=dtype)

    def stft_lengths(self, lengths):
        """Frames each row of a padded batch owns, ``1 + lengths // hop_length`` (``torch.stft(center=True)`` on the row
        alone): the frames of ``gated_stft(x, lengths=lengths)`` that carry the row, the rest being zero.  A tensor
        gives an int64 tensor on its device; a sequence or numpy array gives an int64 numpy array."""
        if isinstance(lengths, torch.Tensor):
            return 1 + torch.div(lengths.to(torch.int64), self.hop_length, rounding_mode="floor")
        return 1 + _rows.as_lengths(lengths, len(lengths)) // int(self.hop_length)

    def gated_stft(self, x: torch.Tensor, xn: Optional[torch.Tensor] = None, return_mask: bool = False, lengths=None,
                   xn_lengths=None):
        """The gated spectrogram ``Y = X * sig_mask`` that the reference multiplies on the line before its ``torch.istft``
        (torchgate.py:223-252) -- for log-mel features, spectral losses or an enhancement front end, without the inverse
        transform of ``forward`` and a further STFT.

        x: (batch, signal_length), xn: as in ``forward``.  Returns Y (batch, n_fft // 2 + 1, frames) complex, where
        ``X = torch.stft(x, n_fft, hop_length, win_length, window=hann_window(win_length), center=True,
        pad_mode="constant", return_complex=True)`` (unscaled) and ``torch.istft(Y, ...)`` with the same arguments is
        ``forward(x, xn)``.  float32 input gives complex64, float64 complex128, other dtypes go through ``.float()``.
        The memory layout is ``torch.stft``'s: storage (batch, frames, bins) with the bins contiguous, returned as the
        ``.transpose(1, 2)`` view.  With ``return_mask=True`` also the final mask (smoothed, prop_decrease applied) as a
        float32 (batch, bins, frames) view of the engine's buffer.  Differentiable w.r.t. ``x`` with the mask detached,
        like ``forward``; the mask carries no gradient.

        Power-of-two n_fft from 256 to 4096 run on the native kernels (sg_gate_spectrum, csrc/spec.hip).  Any other
        n_fft takes the composed, slow route: ``torch.stft(x) * mask`` with the mask of the full-length path and torch
        autograd for the backward.

        lengths / xn_lengths: as in ``forward``, for a zero-padded batch.  With ``T_i = 1 + lengths[i] // hop_length``
        (``stft_lengths``), ``Y[i, :, :T_i]`` is what ``gated_stft(x[i:i+1, :lengths[i]], xn_i)`` returns -- band
        statistics, moving mean, mask smoothing and the -top_db floor over the row's own frames, a frame seeing zeros
        at and beyond ``lengths[i]`` -- and ``Y[i, :, T_i:]`` (and the mask there) is 0.  The padding is never read, a
        row does not depend on the other rows, the gradient is that of the row alone up to ``lengths[i]`` and 0 after
        it, and the gradient of ``Y[i, :, T_i:]`` is ignored.  When every length equals the padded length the call is
        bitwise ``gated_stft(x, xn)``.  Power-of-two n_fft from 256 to 4096 gate the whole batch in a fixed number of
        launches (sg_gate_spectrum_rows, csrc/rows.hip: float64 transforms, so complex128 is stored unrounded and
        complex64 rounded once); any other n_fft makes one ``gated_stft`` call per row (correct, slow)."""
        assert x.ndim == 2
        x, _, xnf, lengths, xn_lengths, full = self._prepare(x, xn, lengths, xn_lengths, xn_rows=True)
        F = self.n_fft // 2 + 1
        if not full and not _rows.native(self.n_fft):
            B, L = x.shape
            T = 1 + L // self.hop_length
            Yt = torch.zeros((B, T, F), dtype=torch.complex64 if x.dtype == torch.float32 else torch.complex128,
                             device=x.device)
            mask = torch.zeros((B, T, F), dtype=torch.float32, device=x.device)
            for i in range(B):
                n = L if lengths is None else int(lengths[i])
                Yi, Mi = self.gated_stft(x[i:i + 1, :n], self._noise_of_row(xn, xn_lengths, i), return_mask=True)
                Yt[i, :Yi.shape[-1]] = Yi[0].transpose(0, 1)
                mask[i, :Mi.shape[-1]] = Mi[0].transpose(0, 1)
        elif _rows.native(self.n_fft):
            route = _ROUTES["spectrum" if full else "spectrum_rows"]
            pairs, mask = _NativeFunction.apply(x, xnf, (self, route, lengths, xn_lengths, None, _NO_KW))
            Yt = torch.view_as_complex(pairs)
        else:
            with torch.no_grad():
                _, mask = self._gate_for(x.device).process_batch(x.detach(), xnf, save_mask=True)
            window = torch.hann_window(self.win_length, device=x.device).to(x.dtype)  # the float32 table, as _gate_for
            X = torch.stft(x, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length, window=window,
                           center=True, pad_mode="constant", return_complex=True)
            Yt = X.transpose(1, 2).contiguous() * mask[:, :, :F].to(x.dtype)
        Y = Yt.transpose(1, 2)
        return (Y, mask[:, :, :F].transpose(1, 2)) if return_mask else Y

    def _bank(self, fb):
        """The validated host copy of a filterbank (``filterbank.check_filterbank``) and its digest, cached per
        ``(data_ptr, _version, shape, device)`` of a tensor -- an in-place edit bumps ``_version`` and is seen; the entry
        also remembers the tensor itself (weakly), so an address that a later tensor reuses is not mistaken for it.  Any
        other array is converted on every call.  A device tensor is copied to the host once per entry, which
        synchronises."""
        F = self.n_fft // 2 + 1
        key = None
        if isinstance(fb, torch.Tensor):
            if fb.requires_grad:
                raise ValueError("the filterbank is a constant: fb.requires_grad must be False")
            key = (fb.data_ptr(), fb._version, tuple(fb.shape), tuple(fb.stride()), fb.dtype, str(fb.device))
            hit = self._banks.get(key)
            if hit is not None and hit["ref"]() is fb:
                return hit
        host = _fbank.check_filterbank(fb, F)
        bank = dict(host=host, digest=hashlib.sha1(host.tobytes()).hexdigest() + "/%d" % host.shape[1], dev={})
        if key is not None:
            bank["ref"] = weakref.ref(fb)
            if len(self._banks) >= 8:
                self._banks.clear()
            self._banks[key] = bank
        return bank

    def gated_filterbank(self, x: torch.Tensor, fb, xn: Optional[torch.Tensor] = None, power: float = 2.0,
                         log: bool = False, eps: float = 1e-6, return_mask: bool = False, lengths=None, xn_lengths=None):
        """Filterbank features of the gated spectrogram -- gated log-mel features with ``fb = mel_filterbank(...)`` and
        ``log=True`` -- without the (batch, bins, frames) spectrogram in memory.

        With ``Y = gated_stft(x, xn)``: ``lin[b, m, t] = sum_k fb[k, m] * |Y[b, k, t]| ** power``, returned as it is
        (``log=False``) or as ``ln(lin + eps)``.  Returns (batch, M, frames): float32 for float32 input, float64 for
        float64 (the transforms are float32 as in ``gated_stft``, the sums over the bins run in the output type), other
        dtypes go through ``.float()``.  Storage is (batch, frames, M) with the filters contiguous, returned as the
        ``.transpose(1, 2)`` view, the way ``gated_stft`` returns Y.  ``return_mask=True`` adds the (batch, bins, frames)
        float32 mask view exactly as ``gated_stft`` returns it.

        fb: any real (n_fft // 2 + 1, M) array or tensor, 1 <= M <= 1024, finite; a constant (``fb.requires_grad`` raises
        ValueError).  Entries may be negative when ``log=False``.  The uploaded tables are cached per
        ``(data_ptr, _version, shape, device)`` of a tensor; a device tensor is copied to the host once to build them,
        which synchronises.  power: 2.0 or 1.0.  Errors in ``fb`` or ``power`` raise ValueError before any device work.

        Differentiable w.r.t. ``x`` with the mask detached, like ``gated_stft``; for ``power=1`` the derivative at
        ``|X[k]| = 0`` is 0.

        Power-of-two n_fft from 256 to 4096 run on the native kernels: the frame stays in LDS between the transform and
        the features, and the backward transforms it again.  Full-length rows take sg_gate_features (csrc/feat.hip).  A
        call whose ``lengths`` / ``xn_lengths`` are not all full takes sg_gate_features_rows (csrc/rows_feat.hip): row i is
        gated and reduced alone as in ``gated_stft(lengths=)`` -- the padding never read, a row independent of the other
        rows, the gradient that of the row alone up to ``lengths[i]`` and 0 after it, the gradient of the frames at and
        after ``stft_lengths(lengths)[i]`` ignored -- with float64 transforms and sums, so a float64 result is stored
        unrounded and a float32 result rounded once.  Any other n_fft takes the composed, slow route
        (``_filterbank_composed``): the formula above in torch on ``gated_stft(...)``, torch autograd for the backward.
        With ``lengths``, frames at and after ``stft_lengths(lengths)[i]`` hold what the formula gives for a zero
        spectrum: 0, or ``ln(eps)`` with ``log=True``.  All-full lengths are bitwise ``gated_filterbank(x, fb, xn)``."""
        assert x.ndim == 2
        if power not in (1, 2, 1.0, 2.0) or isinstance(power, bool):
            raise ValueError(f"power must be 1.0 or 2.0, got {power!r}")
        eps = float(eps)
        if math.isnan(eps):
            raise ValueError("eps is NaN")
        power = int(power)
        bank = self._bank(fb)
        x, _, xnf, lengths, xn_lengths, full = self._prepare(x, xn, lengths, xn_lengths, xn_rows=True)
        F = self.n_fft // 2 + 1
        if _rows.native(self.n_fft):
            kw = dict(power=power, log=bool(log), eps=eps)
            if full:
                call = (self, _ROUTES["features"], None, None, bank, kw)
            else:
                call = (self, _ROUTES["features_rows"], lengths, xn_lengths, bank, kw)
            feat, mask = _NativeFunction.apply(x, xnf, call)
        else:
            if full:
                lengths, xn_lengths = None, None
            feat, mask = self._filterbank_composed(x, xn, bank, power, log, eps, lengths, xn_lengths)
        out = feat.transpose(1, 2)
        return (out, mask[:, :, :F].transpose(1, 2)) if return_mask else out

    def _filterbank_composed(self, x, xn, bank, power, log, eps, lengths, xn_lengths):
        """The composed route of ``gated_filterbank``: the formula in torch on ``gated_stft(...)``, torch autograd for the
        backward.  Returns the features (B, T, M) and the mask (B, T, F), both in storage order.  Serves every n_fft
        without native kernels (tools/bench_gated_filterbank_rows.py times it against the native route)."""
        Y, Mv = self.gated_stft(x, xn, return_mask=True, lengths=lengths, xn_lengths=xn_lengths)
        mask = Mv.transpose(1, 2)
        dkey = (str(x.device), x.dtype)
        fbd = bank["dev"].get(dkey)
        if fbd is None:
            fbd = bank["dev"][dkey] = torch.from_numpy(bank["host"]).to(device=x.device, dtype=x.dtype)
        Yt = Y.transpose(1, 2)                                  # (B, T, F), the storage order
        p = Yt.real * Yt.real + Yt.imag * Yt.imag if power == 2 else Yt.abs()
        feat = torch.matmul(p, fbd)
        if log:
            feat = torch.log(feat + eps)
        return feat, mask

    def _prepare(self, x, xn, lengths, xn_lengths, xn_rows):
        """The one validation and normalisation of a call of forward, gated_stft or gated_filterbank, before any device
        work.  Returns x in float32 / float64 and the dtype to give back, xn as a detached 2-D tensor like x (None when
        there is none or the gate is non-stationary; its lengths stay, the engine ignores them without xn), the lengths as
        host int64 arrays (or None), and whether every row is in fact full.  The errors and their order are pinned by
        tests/test_torchgate_entry_host.py."""
        B, L = x.shape
        lo = self.win_length * 2
        rows_call = lengths is not None or xn_lengths is not None
        # (a full-length call looks at the length of x before the rank of xn, a call with lengths after it)
        if not rows_call and L < lo:
            raise Exception(f"x must be bigger than {lo}")
        assert xn is None or xn.ndim == 1 or xn.ndim == 2
        if rows_call:
            # xn_rows: a noise batch of neither 1 nor B rows is refused here, whether or not xn_lengths came with it.
            # gated_stft and gated_filterbank ask for that; forward does not and leaves the case to the engine, as it
            # leaves it in a call without lengths (which is why the same input gets past this validation there).
            if xn_rows and xn is not None and xn.ndim == 2 and xn.shape[0] not in (1, B):
                raise ValueError(f"xn rows ({xn.shape[0]}) must be 1 or the batch size")
            if L < lo:
                raise Exception(f"x must be bigger than {lo}")
        if xn is not None and xn.shape[-1] < lo:
            raise Exception(f"xn must be bigger than {lo}")
        if lengths is not None:
            lengths = _rows.as_lengths(lengths, B)
            _rows.plan(lengths, L, self.win_length, self.hop_length)
        if xn_lengths is not None:
            if xn is None:
                raise ValueError("xn_lengths given without xn")
            Bn = 1 if xn.ndim == 1 else xn.shape[0]
            if Bn != 1 and Bn != B:
                raise ValueError(f"xn rows ({Bn}) must be 1 or the batch size")
            xn_lengths = _rows.as_lengths(xn_lengths, Bn, "xn_lengths")
            _rows.plan(xn_lengths, xn.shape[-1], self.win_length, self.hop_length, "xn_lengths")
        if x.device.type != "cuda":
            raise RuntimeError("noisereduce_amd.TorchGate runs on the GPU only (no CPU fallback): "
                               "move the input with x.to('cuda')")
        full = not rows_call or (_rows.all_full(lengths, L) and (xn is None or _rows.all_full(xn_lengths, xn.shape[-1])))
        dtype = x.dtype
        if dtype not in (torch.float32, torch.float64):
            x = x.float()
        if xn is not None:
            xn = xn.detach().to(device=x.device, dtype=x.dtype)
            if xn.ndim == 1:
                # the reference crashes on 1-D xn in stationary mode (torchgate.py:164); a
                # single noise row is the evident intent.
                xn = xn.unsqueeze(0)
            if self.nonstationary:
                xn = None  # unused by the non-stationary mask (torchgate.py:235-236)
        return x, dtype, xn, lengths, xn_lengths, full

    @staticmethod
    def _noise_of_row(xn, xn_lengths, i):
        """Row i's noise for a per-row call: its row of xn (or the shared one) cut at its own length."""
        if xn is None:
            return None
        xi = xn if xn.ndim == 1 else xn[(i if xn.shape[0] > 1 else 0)][None]
        if xn_lengths is not None:
            xi = xi[..., :int(xn_lengths[i if len(xn_lengths) > 1 else 0])]
        return xi

    def __getstate__(self):
        st = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        st = dict(st)
        st["_gates"] = {}  # device handles are not picklable
        st["_banks"] = {}  # weak references neither
        return st
