"""``TorchGate`` -- nn.Module with the constructor, buffer and forward contract of
/root/reference/noisereduce/torchgate/torchgate.py:7-264, evaluated by the HIP engine
(sg_process_batch).  0 parameters, one buffer ``smoothing_filter`` of shape
(1, 1, 2*n_grad_freq+1, 2*n_grad_time+1) (or None), so state_dicts round-trip with the
reference's.  The mask is computed without gradient (torchgate.py:126,167) and the output
is differentiable w.r.t. ``x`` through STFT -> (x mask) -> ISTFT.
"""
import hashlib
import math
import weakref
from typing import Optional, Union

import torch

from noisereduce_amd import _ffi
from noisereduce_amd.torchgate import filterbank as _fbank
from noisereduce_amd.torchgate import rows as _rows
from noisereduce_amd.torchgate.utils import linspace


class _GateFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, xn, module):
        gate = module._gate_for(x.device)
        if ctx.needs_input_grad[0]:
            y, mask = gate.process_batch(x.detach(), xn, save_mask=True)
            ctx.gate = gate
            ctx.L = x.shape[-1]
            ctx.save_for_backward(mask)
        else:
            y = gate.process_batch(x, xn)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        (mask,) = ctx.saved_tensors
        gx = ctx.gate.process_batch_backward(grad_out.contiguous(), mask, ctx.L)
        return gx, None, None


class _RowsFunction(torch.autograd.Function):
    """forward(x, lengths=...): the table-driven kernels of csrc/rows.hip.  ``lengths`` / ``xn_lengths`` are host int64
    arrays (or None); the backward gets the same lengths."""

    @staticmethod
    def forward(ctx, x, xn, module, lengths, xn_lengths):
        gate = module._gate_for(x.device)
        if ctx.needs_input_grad[0]:
            y, mask = gate.process_rows(x.detach(), lengths, xn, xn_lengths, save_mask=True)
            ctx.gate = gate
            ctx.L = x.shape[-1]
            ctx.lengths = lengths
            ctx.save_for_backward(mask)
        else:
            y = gate.process_rows(x, lengths, xn, xn_lengths)
        return y

    @staticmethod
    def backward(ctx, grad_out):
        (mask,) = ctx.saved_tensors
        gx = ctx.gate.process_rows_backward(grad_out.contiguous(), mask, ctx.L, ctx.lengths)
        return gx, None, None, None, None


class _SpectrumFunction(torch.autograd.Function):
    """gated_stft on the native kernels (sg_gate_spectrum): returns the real pairs (B, T, F, 2) -- torch.view_as_complex is
    applied outside, so the complex autograd convention stays torch's -- and the mask, which carries no gradient."""

    @staticmethod
    def forward(ctx, x, xn, module):
        gate = module._gate_for(x.device)
        pairs, mask = gate.gate_spectrum(x.detach(), xn, save_mask=True)
        ctx.gate = gate
        ctx.L = x.shape[-1]
        ctx.save_for_backward(mask)
        ctx.mark_non_differentiable(mask)
        return pairs, mask

    @staticmethod
    def backward(ctx, grad_pairs, _grad_mask):
        (mask,) = ctx.saved_tensors
        gx = ctx.gate.gate_spectrum_backward(grad_pairs.contiguous(), mask, ctx.L)
        return gx, None, None


class _SpectrumRowsFunction(torch.autograd.Function):
    """gated_stft(x, lengths=...) on the table-driven kernels (sg_gate_spectrum_rows): real pairs (B, T, F, 2) and the
    mask, as _SpectrumFunction; ``lengths`` / ``xn_lengths`` are host int64 arrays (or None) and the backward gets the
    same lengths."""

    @staticmethod
    def forward(ctx, x, xn, module, lengths, xn_lengths):
        gate = module._gate_for(x.device)
        pairs, mask = gate.gate_spectrum_rows(x.detach(), lengths, xn, xn_lengths, save_mask=True)
        ctx.gate = gate
        ctx.L = x.shape[-1]
        ctx.lengths = lengths
        ctx.save_for_backward(mask)
        ctx.mark_non_differentiable(mask)
        return pairs, mask

    @staticmethod
    def backward(ctx, grad_pairs, _grad_mask):
        (mask,) = ctx.saved_tensors
        gx = ctx.gate.gate_spectrum_rows_backward(grad_pairs.contiguous(), mask, ctx.L, ctx.lengths)
        return gx, None, None, None, None


def _bind_bank(gate, bank):
    """The handle holds this bank (handles are shared between modules of equal parameters: the caller holds gate.lock)."""
    if gate.fb_key != bank["digest"]:
        gate.set_filterbank(bank["host"], key=bank["digest"])


class _FeaturesFunction(torch.autograd.Function):
    """gated_filterbank on the native kernels (sg_gate_features): the features (B, T, M) and the mask, which carries no
    gradient.  Saves x and the mask: the backward transforms the frames again (sg_gate_features_backward), so nothing of
    size B x T x F is kept but the mask.  ``bank``: the entry of TorchGate._bank (host array and digest)."""

    @staticmethod
    def forward(ctx, x, xn, module, bank, power, log, eps):
        gate = module._gate_for(x.device)
        with gate.lock:
            _bind_bank(gate, bank)
            feat, mask = gate.gate_features(x.detach(), xn, power=power, log=log, eps=eps, save_mask=True)
        ctx.gate, ctx.bank, ctx.args = gate, bank, (power, log, eps)
        ctx.save_for_backward(x, mask)
        ctx.mark_non_differentiable(mask)
        return feat, mask

    @staticmethod
    def backward(ctx, grad_feat, _grad_mask):
        x, mask = ctx.saved_tensors
        power, log, eps = ctx.args
        with ctx.gate.lock:
            _bind_bank(ctx.gate, ctx.bank)
            gx = ctx.gate.gate_features_backward(x.detach(), grad_feat, mask, power=power, log=log, eps=eps)
        return gx, None, None, None, None, None, None


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
        if lengths is not None or xn_lengths is not None:
            return self._forward_rows(x, xn, lengths, xn_lengths)
        if x.shape[-1] < self.win_length * 2:
            raise Exception(f"x must be bigger than {self.win_length * 2}")
        assert xn is None or xn.ndim == 1 or xn.ndim == 2
        if xn is not None and xn.shape[-1] < self.win_length * 2:
            raise Exception(f"xn must be bigger than {self.win_length * 2}")
        if x.device.type != "cuda":
            raise RuntimeError("noisereduce_amd.TorchGate runs on the GPU only (no CPU fallback): "
                               "move the input with x.to('cuda')")
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
        y = _GateFunction.apply(x, xn, self)
        return y.to(dtype=dtype)

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
        if lengths is not None or xn_lengths is not None:
            return self._gated_stft_rows(x, xn, return_mask, lengths, xn_lengths)
        if x.shape[-1] < self.win_length * 2:
            raise Exception(f"x must be bigger than {self.win_length * 2}")
        assert xn is None or xn.ndim == 1 or xn.ndim == 2
        if xn is not None and xn.shape[-1] < self.win_length * 2:
            raise Exception(f"xn must be bigger than {self.win_length * 2}")
        if x.device.type != "cuda":
            raise RuntimeError("noisereduce_amd.TorchGate runs on the GPU only (no CPU fallback): "
                               "move the input with x.to('cuda')")
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        if xn is not None:
            xn = xn.detach().to(device=x.device, dtype=x.dtype)
            if xn.ndim == 1:
                xn = xn.unsqueeze(0)
            if self.nonstationary:
                xn = None  # unused by the non-stationary mask (torchgate.py:235-236)
        F = self.n_fft // 2 + 1
        if _rows.native(self.n_fft):
            pairs, mask = _SpectrumFunction.apply(x, xn, self)
            Yt = torch.view_as_complex(pairs)
        else:
            with torch.no_grad():
                _, mask = self._gate_for(x.device).process_batch(x.detach(), xn, save_mask=True)
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

        Power-of-two n_fft from 256 to 4096 on full-length rows run on the native kernels (sg_gate_features,
        csrc/feat.hip): the frame stays in LDS between the transform and the features, and the backward transforms it
        again.  Any other n_fft, and every call whose ``lengths`` / ``xn_lengths`` are not all full, takes the composed,
        slow route: the formula above in torch on ``gated_stft(...)``, torch autograd for the backward.  With
        ``lengths``, frames at and after ``stft_lengths(lengths)[i]`` hold what the formula gives for a zero spectrum: 0,
        or ``ln(eps)`` with ``log=True``.  All-full lengths are bitwise ``gated_filterbank(x, fb, xn)``."""
        assert x.ndim == 2
        if power not in (1, 2, 1.0, 2.0) or isinstance(power, bool):
            raise ValueError(f"power must be 1.0 or 2.0, got {power!r}")
        eps = float(eps)
        if math.isnan(eps):
            raise ValueError("eps is NaN")
        power = int(power)
        bank = self._bank(fb)
        rows_call = lengths is not None or xn_lengths is not None
        if rows_call:
            lengths, xn_lengths = self._check_rows(x, xn, lengths, xn_lengths, xn_rows=True)
            if _rows.all_full(lengths, x.shape[-1]) and (xn is None or _rows.all_full(xn_lengths, xn.shape[-1])):
                rows_call, lengths, xn_lengths = False, None, None
        if not rows_call:
            if x.shape[-1] < self.win_length * 2:
                raise Exception(f"x must be bigger than {self.win_length * 2}")
            assert xn is None or xn.ndim == 1 or xn.ndim == 2
            if xn is not None and xn.shape[-1] < self.win_length * 2:
                raise Exception(f"xn must be bigger than {self.win_length * 2}")
            if x.device.type != "cuda":
                raise RuntimeError("noisereduce_amd.TorchGate runs on the GPU only (no CPU fallback): "
                                   "move the input with x.to('cuda')")
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        F = self.n_fft // 2 + 1
        if not rows_call and _rows.native(self.n_fft):
            if xn is not None:
                xn = xn.detach().to(device=x.device, dtype=x.dtype)
                if xn.ndim == 1:
                    xn = xn.unsqueeze(0)
                if self.nonstationary:
                    xn = None  # unused by the non-stationary mask (torchgate.py:235-236)
            feat, mask = _FeaturesFunction.apply(x, xn, self, bank, power, bool(log), eps)
        else:
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
        out = feat.transpose(1, 2)
        return (out, mask[:, :, :F].transpose(1, 2)) if return_mask else out

    def _check_rows(self, x, xn, lengths, xn_lengths, xn_rows=False):
        """Validation of a call with per-row lengths (forward and gated_stft alike), before any device work: the
        lengths as host int64 arrays (or None).  xn_rows: refuse a noise batch of neither 1 nor B rows here, whether
        or not xn_lengths came with it (forward leaves that case to the engine)."""
        assert xn is None or xn.ndim == 1 or xn.ndim == 2
        B, L = x.shape
        if xn_rows and xn is not None and xn.ndim == 2 and xn.shape[0] not in (1, B):
            raise ValueError(f"xn rows ({xn.shape[0]}) must be 1 or the batch size")
        if L < self.win_length * 2:
            raise Exception(f"x must be bigger than {self.win_length * 2}")
        if xn is not None and xn.shape[-1] < self.win_length * 2:
            raise Exception(f"xn must be bigger than {self.win_length * 2}")
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
        return lengths, xn_lengths

    @staticmethod
    def _noise_of_row(xn, xn_lengths, i):
        """Row i's noise for a per-row call: its row of xn (or the shared one) cut at its own length."""
        if xn is None:
            return None
        xi = xn if xn.ndim == 1 else xn[(i if xn.shape[0] > 1 else 0)][None]
        if xn_lengths is not None:
            xi = xi[..., :int(xn_lengths[i if len(xn_lengths) > 1 else 0])]
        return xi

    def _gated_stft_rows(self, x, xn, return_mask, lengths, xn_lengths):
        """gated_stft with per-row lengths, routed as _forward_rows: the full-length path (every row full), the
        table-driven kernels, or -- for an n_fft they are not built for -- one gated_stft call per row."""
        lengths, xn_lengths = self._check_rows(x, xn, lengths, xn_lengths, xn_rows=True)
        B, L = x.shape
        if _rows.all_full(lengths, L) and (xn is None or _rows.all_full(xn_lengths, xn.shape[-1])):
            return self.gated_stft(x, xn, return_mask)
        F = self.n_fft // 2 + 1
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        if not _rows.native(self.n_fft):
            T = 1 + L // self.hop_length
            Yt = torch.zeros((B, T, F), dtype=torch.complex64 if x.dtype == torch.float32 else torch.complex128,
                             device=x.device)
            mask = torch.zeros((B, T, F), dtype=torch.float32, device=x.device)
            for i in range(B):
                n = L if lengths is None else int(lengths[i])
                Yi, Mi = self.gated_stft(x[i:i + 1, :n], self._noise_of_row(xn, xn_lengths, i), return_mask=True)
                Yt[i, :Yi.shape[-1]] = Yi[0].transpose(0, 1)
                mask[i, :Mi.shape[-1]] = Mi[0].transpose(0, 1)
        else:
            if xn is not None:
                xn = xn.detach().to(device=x.device, dtype=x.dtype)
                if xn.ndim == 1:
                    xn = xn.unsqueeze(0)
                if self.nonstationary:
                    xn, xn_lengths = None, None  # unused by the non-stationary mask (torchgate.py:235-236)
            pairs, mask = _SpectrumRowsFunction.apply(x, xn, self, lengths, xn_lengths)
            Yt = torch.view_as_complex(pairs)
        Y = Yt.transpose(1, 2)
        return (Y, mask[:, :, :F].transpose(1, 2)) if return_mask else Y

    def _forward_rows(self, x, xn, lengths, xn_lengths):
        """forward with per-row lengths: validation, then the full-length path (every row full), the table-driven
        kernels, or -- for an n_fft they are not built for -- one full-length call per row."""
        lengths, xn_lengths = self._check_rows(x, xn, lengths, xn_lengths)
        B, L = x.shape
        if _rows.all_full(lengths, L) and (xn is None or _rows.all_full(xn_lengths, xn.shape[-1])):
            return self.forward(x, xn)
        if not _rows.native(self.n_fft):
            H = self.hop_length
            y = x.new_zeros((B, H * (L // H)))
            for i in range(B):
                n = L if lengths is None else int(lengths[i])
                y[i, :H * (n // H)] = self.forward(x[i:i + 1, :n], self._noise_of_row(xn, xn_lengths, i))[0]
            return y
        dtype = x.dtype
        if dtype not in (torch.float32, torch.float64):
            x = x.float()
        if xn is not None:
            xn = xn.detach().to(device=x.device, dtype=x.dtype)
            if xn.ndim == 1:
                xn = xn.unsqueeze(0)
            if self.nonstationary:
                xn, xn_lengths = None, None  # unused by the non-stationary mask (torchgate.py:235-236)
        y = _RowsFunction.apply(x, xn, self, lengths, xn_lengths)
        return y.to(dtype=dtype)

    def __getstate__(self):
        st = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        st = dict(st)
        st["_gates"] = {}  # device handles are not picklable
        st["_banks"] = {}  # weak references neither
        return st
