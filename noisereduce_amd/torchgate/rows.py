"""Host-side planning for ``TorchGate.forward(x, lengths=...)`` and ``TorchGate.gated_stft(x, lengths=...)``: padded
batches whose rows end at different samples.

Pure Python / numpy (no GPU, no library): what each row's own STFT geometry is, which lengths are acceptable, and
whether a call is in fact a full-length batch that today's kernels already gate.
"""
import numpy as np

# n_fft the table-driven kernels (csrc/rows.hip) are instantiated for; other n_fft loop over the rows
NATIVE_N_FFT = (256, 512, 1024, 2048, 4096)


def as_lengths(lengths, count, name="lengths"):
    """``lengths`` (sequence, numpy array, CPU or device tensor) as a host int64 array of ``count`` entries.
    A device tensor is copied to the host, which synchronises."""
    if hasattr(lengths, "detach"):
        lengths = lengths.detach().cpu().numpy()
    a = np.asarray(lengths)
    if a.ndim != 1 or a.shape[0] != count:
        raise ValueError(f"{name} must hold {count} integers (one per row), got shape {tuple(a.shape)}")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(a == np.floor(a)):
            raise ValueError(f"{name} must be integers")
    return a.astype(np.int64)


def plan(lengths, L, win_length, hop_length, name="lengths"):
    """Frames ``T_i = 1 + lengths[i] // hop`` and output samples ``Lout_i = hop * (lengths[i] // hop)`` of every row
    (``torch.stft(center=True)`` / ``torch.istft`` on the row alone).  Raises ``ValueError`` naming the first row whose
    length is below ``2 * win_length`` (the reference's minimum) or above the padded length ``L``."""
    a = as_lengths(lengths, len(lengths), name)
    lo = 2 * int(win_length)
    for i, n in enumerate(a.tolist()):
        if n < lo:
            raise ValueError(f"{name}[{i}] = {n}: a row must hold at least 2 * win_length = {lo} samples")
        if n > L:
            raise ValueError(f"{name}[{i}] = {n} exceeds the padded row length {L}")
    q = a // int(hop_length)
    return 1 + q, int(hop_length) * q


def all_full(lengths, L):
    """True when every row reaches the padded length (or no lengths were given): today's full-length path applies."""
    return lengths is None or bool(np.all(np.asarray(lengths) == L))


def native(n_fft):
    """True when csrc/rows.hip gates this n_fft in one table-driven call; otherwise forward / gated_stft loop over the
    rows."""
    return int(n_fft) in NATIVE_N_FFT
