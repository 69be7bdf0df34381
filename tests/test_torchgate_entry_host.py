"""The validation of ``TorchGate.forward``, ``gated_stft`` and ``gated_filterbank`` on CPU tensors: the exact exception
type and message of every path, and the precedence between them.  No GPU is needed: the "runs on the GPU only" error is
itself the last check, so a call that reaches it has passed every other one.

One table, every row run through every entry point it names.  ``x`` is (3, 4096) zeros and the gate the default
``TorchGate(sr=16000)`` (win_length 1024, so a row must hold 2048 samples) unless the row says otherwise."""
import pytest
import torch

FWD, STFT, FBANK = "forward", "gated_stft", "gated_filterbank"
ALL = (FWD, STFT, FBANK)

GPU_ONLY = (RuntimeError, "noisereduce_amd.TorchGate runs on the GPU only (no CPU fallback): move the input with x.to('cuda')")
X_SHORT = (Exception, "x must be bigger than 2048")
XN_SHORT = (Exception, "xn must be bigger than 2048")
XN_ROWS = (ValueError, "xn rows (2) must be 1 or the batch size")
ASSERT = (AssertionError, None)


def _x(n=4096, rows=3):
    return torch.zeros((rows, n))


def _fb(rows=513, **kw):
    return torch.ones((rows, 4), **kw)


# (id, entry points, gate kwargs, call kwargs (x, xn, lengths, xn_lengths; for gated_filterbank also fb, power, eps),
#  (exception type, message))
CASES = [
    ("valid", ALL, {}, dict(x=_x()), GPU_ONLY),
    ("valid-xn-1d", ALL, {}, dict(x=_x(), xn=torch.zeros(3000)), GPU_ONLY),
    ("valid-xn-2d", ALL, {}, dict(x=_x(), xn=_x(3000)), GPU_ONLY),
    ("valid-nonstationary", ALL, dict(nonstationary=True), dict(x=_x(), xn=_x(3000, 1)), GPU_ONLY),
    ("valid-int16", ALL, {}, dict(x=_x().to(torch.int16)), GPU_ONLY),
    ("x-short", ALL, {}, dict(x=_x(2047)), X_SHORT),
    ("x-short-lengths", ALL, {}, dict(x=_x(2047), lengths=[2047] * 3), X_SHORT),
    ("xn-short", ALL, {}, dict(x=_x(), xn=torch.zeros(10)), XN_SHORT),
    ("xn-short-lengths", ALL, {}, dict(x=_x(), xn=torch.zeros(10), lengths=[4096, 3000, 4096]), XN_SHORT),
    ("xn-3d", ALL, {}, dict(x=_x(), xn=torch.zeros((1, 1, 4096))), ASSERT),
    ("xn-3d-lengths", ALL, {}, dict(x=_x(), xn=torch.zeros((1, 1, 4096)), lengths=[4096, 3000, 4096]), ASSERT),
    ("x-1d", ALL, {}, dict(x=torch.zeros(4096)), ASSERT),
    ("x-1d-lengths", ALL, {}, dict(x=torch.zeros(4096), lengths=[4096]), ASSERT),
    ("length-short", ALL, {}, dict(x=_x(), lengths=[4096, 100, 4096]),
     (ValueError, "lengths[1] = 100: a row must hold at least 2 * win_length = 2048 samples")),
    ("length-count", ALL, {}, dict(x=_x(), lengths=[4096, 4096]),
     (ValueError, "lengths must hold 3 integers (one per row), got shape (2,)")),
    ("length-fraction", ALL, {}, dict(x=_x(), lengths=[4096.5, 4096.0, 4096.0]), (ValueError, "lengths must be integers")),
    ("length-long", ALL, {}, dict(x=_x(), lengths=[5000, 4096, 4096]),
     (ValueError, "lengths[0] = 5000 exceeds the padded row length 4096")),
    ("xn-length-short", ALL, {}, dict(x=_x(), xn=_x(3000, 1), xn_lengths=[100]),
     (ValueError, "xn_lengths[0] = 100: a row must hold at least 2 * win_length = 2048 samples")),
    ("xn-lengths-without-xn", ALL, {}, dict(x=_x(), xn_lengths=[4096]), (ValueError, "xn_lengths given without xn")),
    ("xn-rows-xn-lengths", ALL, {}, dict(x=_x(), xn=_x(4096, 2), xn_lengths=[4096, 4096]), XN_ROWS),
    # forward leaves a noise batch of neither 1 nor B rows to the engine unless xn_lengths came with it
    ("xn-rows-lengths", (STFT, FBANK), {}, dict(x=_x(), xn=_x(4096, 2), lengths=[4096, 3000, 4096]), XN_ROWS),
    ("xn-rows-lengths-forward", (FWD,), {}, dict(x=_x(), xn=_x(4096, 2), lengths=[4096, 3000, 4096]), GPU_ONLY),
    ("xn-rows-full", ALL, {}, dict(x=_x(), xn=_x(4096, 2)), GPU_ONLY),
    ("lengths-all-full", ALL, {}, dict(x=_x(), lengths=[4096] * 3), GPU_ONLY),
    ("lengths-all-full-tensor", ALL, {}, dict(x=_x(), lengths=torch.full((3,), 4096)), GPU_ONLY),
    ("lengths-valid", ALL, {}, dict(x=_x(), xn=_x(3000, 1), lengths=[4096, 3000, 2048], xn_lengths=[2500]), GPU_ONLY),
    ("other-n-fft-lengths", (FWD, STFT), dict(n_fft=1000), dict(x=_x(rows=2), lengths=[4096, 3000]), GPU_ONLY),
    # precedence.  A full-length call: x too short, xn's rank, xn too short, the device.  A call with lengths: xn's rank,
    # xn's rows, x too short, xn too short, lengths, xn_lengths, the device.
    ("x-short-before-xn-3d", ALL, {}, dict(x=_x(2047), xn=torch.zeros((1, 1, 10))), X_SHORT),
    ("xn-3d-before-x-short-lengths", ALL, {}, dict(x=_x(2047), xn=torch.zeros((1, 1, 10)), lengths=[2047] * 3), ASSERT),
    ("x-short-before-xn-short", ALL, {}, dict(x=_x(2047), xn=torch.zeros(10)), X_SHORT),
    ("xn-3d-before-xn-short", ALL, {}, dict(x=_x(), xn=torch.zeros((1, 1, 10))), ASSERT),
    ("xn-rows-before-x-short", (STFT, FBANK), {}, dict(x=_x(2047), xn=_x(4096, 2), lengths=[2047] * 3), XN_ROWS),
    ("x-short-before-xn-rows-forward", (FWD,), {}, dict(x=_x(2047), xn=_x(4096, 2), lengths=[2047] * 3), X_SHORT),
    ("xn-short-before-lengths", ALL, {}, dict(x=_x(), xn=torch.zeros(10), lengths=[4096, 100, 4096]), XN_SHORT),
    ("lengths-before-xn-lengths", ALL, {}, dict(x=_x(), lengths=[4096, 100, 4096], xn_lengths=[4096]),
     (ValueError, "lengths[1] = 100: a row must hold at least 2 * win_length = 2048 samples")),
    # gated_filterbank: power, eps and the bank are refused before x is looked at
    ("fb-power-3", (FBANK,), {}, dict(x=_x(2047), power=3), (ValueError, "power must be 1.0 or 2.0, got 3")),
    ("fb-power-bool", (FBANK,), {}, dict(x=_x(2047), power=True), (ValueError, "power must be 1.0 or 2.0, got True")),
    ("fb-eps-nan", (FBANK,), {}, dict(x=_x(2047), eps=float("nan")), (ValueError, "eps is NaN")),
    ("fb-requires-grad", (FBANK,), {}, dict(x=_x(2047), fb=_fb(requires_grad=True)),
     (ValueError, "the filterbank is a constant: fb.requires_grad must be False")),
    ("fb-rows", (FBANK,), {}, dict(x=_x(2047), fb=_fb(512)), (ValueError, "the filterbank must be (513, M), got (512, 4)")),
    ("fb-power-before-eps", (FBANK,), {}, dict(x=_x(2047), power=3, eps=float("nan")),
     (ValueError, "power must be 1.0 or 2.0, got 3")),
    ("fb-eps-before-bank", (FBANK,), {}, dict(x=_x(2047), eps=float("nan"), fb=_fb(512)), (ValueError, "eps is NaN")),
    ("fb-x-1d-before-power", (FBANK,), {}, dict(x=torch.zeros(4096), power=3), ASSERT),
]

ROWS = [pytest.param(entry, gate_kw, kw, want, id=f"{name}-{entry}")
        for name, entries, gate_kw, kw, want in CASES for entry in entries]


def test_the_table_has_no_duplicate_rows():
    ids = [name for name, *_ in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("entry,gate_kw,kw,want", ROWS)
def test_entry_point_raises_exactly(entry, gate_kw, kw, want):
    from noisereduce_amd.torchgate import TorchGate
    tg = TorchGate(sr=16000, **gate_kw)
    kw = dict(kw)
    if entry == FBANK:
        kw.setdefault("fb", _fb())
    exc, message = want
    with pytest.raises(Exception) as info:
        getattr(tg, entry)(**kw)
    assert type(info.value) is exc, (type(info.value), str(info.value))
    if message is not None:
        assert str(info.value) == message
