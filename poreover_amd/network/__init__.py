"""The basecalling network (`call`): FAST5 signal -> softmax probabilities, on the GPU (poreover_amd/csrc/po_call.hip)."""
from .network import batch_input, call, call_helper, parse_fast5  # noqa: F401
