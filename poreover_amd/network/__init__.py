"""The basecalling network: `call` (FAST5 signal -> softmax probabilities, poreover_amd/csrc/po_call.hip) and `basecall`
(FAST5 signal -> sequences in one device-resident pass, poreover_amd/csrc/po_basecall.hip; the module .basecall) and
`pair-basecall` (FAST5 pairs -> 1D² consensus in one such pass, poreover_amd/csrc/po_pair_basecall.hip; .pair_basecall)."""
from . import basecall  # noqa: F401
from .basecall import basecall_raw, basecall_signals, frame_window, window_plan  # noqa: F401
from . import pair_basecall  # noqa: F401
from .pair_basecall import pair_basecall_raw, pair_basecall_signals  # noqa: F401
from .network import batch_input, call, call_helper, parse_fast5, prep_signals, read_fast5_raw, round_bf16, split_bf16  # noqa: F401
