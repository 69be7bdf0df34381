"""TorchGate: an nn.Module drop-in for /root/reference/noisereduce/torchgate
(torchgate/__init__.py:12)."""
from .filterbank import mel_filterbank  # noqa: F401
from .torchgate import TorchGate  # noqa: F401
