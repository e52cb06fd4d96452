"""`python -m poreover_amd train|call|decode|pair-decode|benchmark ...` — the five sub-commands of the reference CLI
(reference __main__.py:19-99) with the same flags and defaults, on the GPU engine — and three the reference lacks:
`find-pairs`, the list of read pairs `pair-decode` starts from, `basecall`, FAST5 to FASTA in one
device-resident pass with overlapping windows, and `pair-basecall`, FAST5 pairs to their 1D² consensus in
one such pass.  `train` runs CTC
training of the basecalling network in HIP and writes .npz checkpoints; `call` runs the network's forward pass and needs
`--weights` (no weights ship with this package: a TF checkpoint prefix or directory, a `train` output directory, or an
.npz from `python -m poreover_amd.network.convert`).  `benchmark` maps decoded reads to a reference genome with the
engine's own mapper (minimap2's map-ont seeds and scores, simplified) and reports their identities."""
import argparse
import logging
import sys

from . import __version__
from .quality import DEFAULT_BAND


RECURRENCE_HELP = ('The product h·U of the GRU recurrence: f32, or bf16x3 (both operands split in two bf16 values, three bf16 products '
                   'with f32 sums; logits stay within the f32 path\'s own bound); independent of --precision')
PRECISION_HELP = ('bf16: GRU input projections with bf16 operands, f32 accumulation; about one base in a thousand differs '
                  'from f32')


def build_parser():
    parser = argparse.ArgumentParser(prog="poreover_amd",
                                     description='PoreOver decoding on MI355X: consensus basecalling for nanopore sequencing')
    subparsers = parser.add_subparsers(dest="command")
    subparsers.required = True

    p = subparsers.add_parser('train', help='Train a neural network base calling model', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--data', help='Location of training data in compressed npz format', required=True)
    p.add_argument('--name', default='run', help='Name of run')
    p.add_argument('--epochs', type=int, default=1, help='Number of epochs to train on')
    p.add_argument('--save_every', type=int, default=1000, help='Frequency with which to save checkpoint files')
    p.add_argument('--holdout', default=0.05, type=float, help='Fraction of training data to hold out for calculating test error')
    p.add_argument('--loss_every', type=int, default=100, help='Frequency with which to output minibatch loss')
    p.add_argument('--ctc_merge_repeated', action='store_true', default=False, help='boolean option for tf.compat.v1.nn.ctc_loss')
    p.add_argument('--model', default='conv1_bigru3', choices=['bigru3', 'conv1_bigru3', 'conv2_bigru3', 'conv1_gru5'], help='Neural network architecture')
    p.add_argument('--restart', default=False, help='Trained model to load (if directory, loads latest from checkpoint file)')
    p.add_argument('--batch_size', default=64, type=int, help='Minibatch size for training')
    p.add_argument('--learning_rate', type=float, default=0.001, help='Learning rate for Adam optimizer')
    p.add_argument('--seed', type=int, default=None, help='Explicitly set random seed')
    p.add_argument('--num_neurons', type=int, default=128, help='Number of neurons in RNN layers')
    p.add_argument('--kernel_size', type=int, default=9, help='Kernel size in Conv1D layer (1 to 64)')
    p.add_argument('--filters', type=int, default=256, help='Number of filters in Conv1D layer (at least 1)')
    p.add_argument('--gemm_precision', choices=['f32', 'bf16'], default='f32',
                   help="Operands of the GRU layers' weight and input GEMMs: f32, or bf16 with f32 sums, f32 master weights and f32 Adam "
                        '(128 GRU units; the recurrences stay f32)')
    p.add_argument('--accumulate', type=int, default=1,
                   help='Batches whose gradients are accumulated into one optimizer step (effective batch: this times --batch_size); '
                        'with it, --save_every and --loss_every count optimizer steps')
    p.add_argument('--clip_norm', type=float, default=0.0, help='Clip the gradient to this global L2 norm (0: no clipping); a step whose '
                                                                 'gradient is not finite is skipped either way')
    p.add_argument('--weight_decay', type=float, default=0.0, help='Decoupled weight decay (AdamW): each step also subtracts '
                                                                    'learning rate x this x the parameter (0: none)')
    p.add_argument('--lr_schedule', choices=['constant', 'linear', 'cosine'], default='constant',
                   help='Learning rate after the warm-up: constant, or falling to --min_lr over the run linearly or by a half cosine')
    p.add_argument('--warmup_steps', type=int, default=0, help='Optimizer steps over which the learning rate rises linearly to --learning_rate')
    p.add_argument('--min_lr', type=float, default=0.0, help='Learning rate at the end of a linear or cosine schedule')
    p.add_argument('--save_optimizer', action='store_true', default=False,
                   help="Write Adam's state (m, v, step) and the schedule position as <checkpoint>.opt.npz beside every checkpoint")
    p.add_argument('--resume_optimizer', action='store_true', default=False,
                   help="With --restart: load the .opt.npz beside the restarted checkpoint (Adam's state and the schedule position); "
                        'the batch plan starts over')
    p.add_argument('--gpus', type=int, default=1,
                   help='Devices to train on, data-parallel (devices 0 .. N-1): an optimizer step takes this times --accumulate batches, '
                        'one batch per device at a time, and the gradients are summed between the devices in a fixed order')
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="train")

    p = subparsers.add_parser('call', help='Run basecalling forward pass on set of FAST5 reads',
                              formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('in', help='Single FAST5 file or directory of FAST5 files')
    p.add_argument('--weights', default=None, help='Trained weights to load into model: a TF checkpoint prefix, a directory (loads latest from its checkpoint file) or an .npz (required: no weights ship with this package)')
    p.add_argument('--model', help='Model config JSON file (default: conv1_bigru3)', default=None)
    p.add_argument('--scaling', default='standard', choices=['standard', 'current', 'median', 'rescale'], help='Type of preprocessing (should be same as training)')
    p.add_argument('--use_id', default=False, action='store_true', help='Save logits by read ID instead of FAST5 filename')
    p.add_argument('--dir', default='.', help='Directory to write logits to')
    p.add_argument('--window', type=int, default=1000, help='Call read using chunks of this size')
    p.add_argument('--format', choices=['csv', 'npy'], default='npy', help='Save softmax probabilities to CSV file or logits to binarized NumPy format')
    p.add_argument('--no_stack', default=False, action='store_true', help='Basecall [1xSIGNAL_LENGTH] tensor instead of splitting it into windows (slower)')
    p.add_argument('--precision', choices=['f32', 'bf16'], default='f32', help=PRECISION_HELP)
    p.add_argument('--recurrence', choices=['f32', 'bf16x3'], default='f32', help=RECURRENCE_HELP)
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="call")

    p = subparsers.add_parser('basecall', help='Basecall FAST5 reads to a FASTA file: the network and the decoder in one pass on the GPU',
                              formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('in', help='Single FAST5 file or directory of FAST5 files')
    p.add_argument('--weights', default=None, help='Trained weights to load into model: a TF checkpoint prefix, a directory (loads latest from its checkpoint file) or an .npz (required: no weights ship with this package)')
    p.add_argument('--model', help='Model config JSON file (default: conv1_bigru3)', default=None)
    p.add_argument('--scaling', default='standard', choices=['standard', 'current', 'median', 'rescale'], help='Type of preprocessing (should be same as training)')
    p.add_argument('--use_id', default=False, action='store_true', help='Name records by read ID instead of FAST5 filename')
    p.add_argument('--window', type=int, default=1000, help='Call read using chunks of this size')
    p.add_argument('--overlap', type=int, default=0, help='Samples that consecutive chunks share (even, smaller than --window); each chunk keeps its middle')
    p.add_argument('--algorithm', default='viterbi', choices=['viterbi', 'beam'], help='Decoder')
    p.add_argument('--beam_width', type=int, default=25, help='Width for beam search')
    p.add_argument('--merge_repeats', default=False, action='store_true', help='Decode as CTC with merged repeats (for weights trained with --ctc_merge_repeated)')
    p.add_argument('--out', default='out', help='Prefix for FASTA sequence output')
    p.add_argument('--fastq', action='store_true', default=False, help='Also write {out}.fastq with a Phred quality per base')
    p.add_argument('--qual_band', type=int, default=DEFAULT_BAND, help='Label positions either side of the basecall\'s frames that the quality lattice admits (<= 0: no band)')
    p.add_argument('--precision', choices=['f32', 'bf16'], default='f32', help=PRECISION_HELP)
    p.add_argument('--recurrence', choices=['f32', 'bf16x3'], default='f32', help=RECURRENCE_HELP)
    p.add_argument('--gpus', type=int, default=None,
                   help='Stream the reads through devices 0 .. N-1 (0: every visible device): files are read by --readers threads in chunks, '
                        'filtered and scaled on the device, and records are appended as chunks complete. Without it: one device, every file parsed first')
    p.add_argument('--readers', type=int, default=4, help='With --gpus: threads reading FAST5 files (1 to 16)')
    p.add_argument('--chunk_files', type=int, default=None, help='With --gpus: files per chunk (default 512)')
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="basecall")

    p = subparsers.add_parser('pair-basecall', help='1D2 consensus of FAST5 read pairs: the network and the pair decoder in one pass on the GPU',
                              formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('in', help='List of read pairs: two read names per line, as find-pairs writes them')
    p.add_argument('--dir', default='.', help='Directory of the FAST5 files the pairs name (a .npy or .fast5 suffix, or none, is replaced by .fast5)')
    p.add_argument('--weights', default=None, help='Trained weights to load into model: a TF checkpoint prefix, a directory (loads latest from its checkpoint file) or an .npz (required: no weights ship with this package)')
    p.add_argument('--model', help='Model config JSON file (default: conv1_bigru3)', default=None)
    p.add_argument('--scaling', default='standard', choices=['standard', 'current', 'median', 'rescale'], help='Type of preprocessing (should be same as training)')
    p.add_argument('--window', type=int, default=1000, help='Call read using chunks of this size')
    p.add_argument('--overlap', type=int, default=0, help='Samples that consecutive chunks share (even, smaller than --window); each chunk keeps its middle')
    p.add_argument('--reverse_complement', default=False, action='store_true', help='Whether to reverse complement the second sequence')
    p.add_argument('--merge_repeats', default=False, action='store_true', help='Decode as CTC with merged repeats (for weights trained with --ctc_merge_repeated)')
    p.add_argument('--beam_width', type=int, default=5, help='Width for beam search')
    p.add_argument('--padding', type=int, default=5, help='Padding for building alignment envelope')
    p.add_argument('--alignment', default='banded', choices=['banded', 'full'], help='Do full Needleman-Wunsch alignment between 1D basecalls to build envelope')
    p.add_argument('--diagonal_envelope', action='store_true', help='Use a simple diagonal band for the signal alignment envelope')
    p.add_argument('--diagonal_width', type=int, default=50, help='Width of diagonal band envelope')
    p.add_argument('--beam_search_method', choices=['row', 'row_col', 'grid'], default="row_col", help=argparse.SUPPRESS)
    p.add_argument('--out', default='out', help='Prefix for FASTA sequence output')
    # what pair-decode offers and this route does not: parsed so that each is refused by name (pair_basecall.check_args)
    p.add_argument('--fastq', action='store_true', default=False, help=argparse.SUPPRESS)
    p.add_argument('--single', default='viterbi', help=argparse.SUPPRESS)
    p.add_argument('--skip_matches', action='store_true', default=False, help=argparse.SUPPRESS)
    p.add_argument('--method', default='envelope', help=argparse.SUPPRESS)
    p.add_argument('--threads', type=int, default=1, help=argparse.SUPPRESS)
    p.add_argument('--precision', choices=['f32', 'bf16'], default='f32', help=PRECISION_HELP)
    p.add_argument('--recurrence', choices=['f32', 'bf16x3'], default='f32', help=RECURRENCE_HELP)
    p.add_argument('--gpus', type=int, default=None,
                   help='Stream the pairs through devices 0 .. N-1 (0: every visible device): the pairs file is cut into chunks of --chunk_pairs lines, '
                        'their FAST5 files are read by --readers threads while the chunk before runs, filter and scaling run on the device')
    p.add_argument('--readers', type=int, default=4, help='With --gpus: threads reading FAST5 files (1 to 16)')
    p.add_argument('--chunk_pairs', type=int, default=256, help='With --gpus: lines of the pairs file per chunk')
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="pair-basecall")

    p = subparsers.add_parser('decode', help='Decode basecaller probabilities to a FASTA file')
    p.add_argument('in', nargs='+', help='Probabilities to decode (.npy from PoreOver/Bonito, .csv, or HDF5/FAST5 from Flappie/Guppy)')
    p.add_argument('--out', default='out', help='Prefix for FASTA sequence output')
    p.add_argument('--basecaller', choices=['poreover', 'flappie', 'guppy', 'bonito'], help='Basecaller used to generate probabilities')
    p.add_argument('--algorithm', default='viterbi', choices=['viterbi', 'beam', 'prefix'], help='')
    p.add_argument('--window', type=int, default=400, help='Use chunks of this size for prefix search')
    p.add_argument('--beam_width', type=int, default=25, help='Width for beam search')
    p.add_argument('--threads', type=int, default=1, help='Upper bound on the GPUs one call is spread over when > 1 (the reference: worker processes); batching replaces processes on each device')
    p.add_argument('--fastq', action='store_true', default=False, help='Also write {out}.fastq with a Phred quality per base (poreover and bonito inputs)')
    p.add_argument('--qual_band', type=int, default=DEFAULT_BAND, help='Label positions either side of the basecall\'s frames that the quality lattice admits (<= 0: no band)')
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="decode")

    p = subparsers.add_parser('pair-decode', help='1D2 consensus decoding of two output probabilities',
                              formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.add_argument('in', nargs='+', help='Softmax probabilities to decode or list of read pairs')
    p.add_argument('--dir', default='.', help='Base directory to look in for basecaller probabilities')
    p.add_argument('--basecaller', choices=['poreover', 'flappie', 'guppy', 'bonito'], help='Basecaller used to generate probabilities')
    p.add_argument('--reverse_complement', default=False, action='store_true', help='Whether to reverse complement the second sequence')
    p.add_argument('--out', default='out', help='Prefix for FASTA sequence output')
    p.add_argument('--threads', type=int, default=1, help='Upper bound on the GPUs one call is spread over when > 1 (the reference: worker processes); batching replaces processes on each device')
    p.add_argument('--method', choices=['align', 'split', 'envelope'], default='envelope', help=argparse.SUPPRESS)
    p.add_argument('--single', choices=['beam', 'viterbi'], default='viterbi', help='Algorithm for 1D basecalling (used to build alignment envelope)')
    p.add_argument('--logging', default="info", choices=['info', 'debug'], help='Level for logging')
    p.add_argument('--debug', default=False, action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--algorithm', default='beam', choices=['prefix', 'beam'], help=argparse.SUPPRESS)
    p.add_argument('--alignment', default='banded', choices=['banded', 'full'], help='Do full Needleman-Wunsch alignment between 1D basecalls to build envelope')
    p.add_argument('--beam_width', type=int, default=5, help='Width for beam search')
    p.add_argument('--debug_envelope', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--diagonal_envelope', action='store_true', help='Use a simple diagonal band for the signal alignment envelope')
    p.add_argument('--diagonal_width', type=int, default=50, help='Width of diagonal band envelope')
    p.add_argument('--padding', type=int, default=5, help='Padding for building alignment envelope')
    p.add_argument('--skip_matches', action='store_true', help='Skip regions of sequence alignment with match columns greater than --skip_threshold')
    p.add_argument('--skip_threshold', type=int, default=10, help='Number of consecutive matches to use for --skip_matches')
    p.add_argument('--beam_search_method', choices=['row', 'row_col', 'grid'], default="row_col", help=argparse.SUPPRESS)
    p.add_argument('--window', type=int, default=200, help=argparse.SUPPRESS)
    p.add_argument('--fastq', action='store_true', default=False, help='Also write FASTQ with a Phred quality per base: {out}.1d.fastq and {out}.2d.fastq for a list of pairs, {out}.fastq for one pair (poreover and bonito inputs)')
    p.add_argument('--qual_band', type=int, default=DEFAULT_BAND, help='Label positions either side of the basecall\'s frames that the quality lattice admits (<= 0: no band)')
    p.set_defaults(func="pair-decode")

    p = subparsers.add_parser('benchmark', help='Assess accuracy of basecalled FASTA/FASTQ files')
    p.add_argument('--fasta', help='FASTA file', default=None)
    p.add_argument('--fasta_pair', help='Prefix with 1D/2D (*.1d.fasta and *.2d.fasta)', default=None)
    p.add_argument('--fastq', help='FASTQ file', default=None)
    p.add_argument('--reference', help='Reference genome', required=True)
    p.add_argument('--full', action="store_true", help="Collect more statistics on types of errors")
    p.set_defaults(func="benchmark")

    p = subparsers.add_parser('find-pairs', help='Find 1D2 read pairs: reads that follow each other in a channel and map to each other on opposite strands',
                              formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('IN', nargs='*', help='Single-read FAST5 files or directories of them: the reads and their metadata')
    p.add_argument('--summary', default=None, help='The reads and their channel / start_time / duration from a tab-separated summary table (then no IN)')
    p.add_argument('--candidates', default=None, help='Two names per line: verify these pairs instead of deriving candidates (then neither IN nor --summary)')
    p.add_argument('--fasta', default=None, help='1D basecalls, one record per read')
    p.add_argument('--dir', default=None, help='Directory of basecaller probabilities as pair-decode finds them; called here by Viterbi')
    p.add_argument('--basecaller', choices=['poreover', 'flappie', 'guppy', 'bonito'], help='Basecaller used to generate probabilities')
    p.add_argument('--max_gap', type=float, default=1.0, help='Seconds between the end of one read and the start of the next in a channel')
    p.add_argument('--min_identity', type=float, default=0.6, help='Smallest mlen / blen of an accepted pair')
    p.add_argument('--min_cover', type=float, default=0.5, help='Smallest share of the shorter read the alignment spans')
    p.add_argument('--out', default='out', help='Prefix for PREFIX.pairs.txt and PREFIX.pairs.csv')
    p.add_argument('-v', '--version', action='version', version=__version__)
    p.set_defaults(func="find-pairs")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(format='%(message)s', level=logging.DEBUG if getattr(args, 'logging', 'info') == 'debug' else logging.INFO)
    if args.func == "train":
        from .network import train as _train
        try:
            _train.train(args)
        except _train.TrainError as e:
            raise SystemExit(str(e))
        return
    if args.func == "call":
        from .network import call as _call
        if args.window < 1:
            raise SystemExit("call: --window must be positive")
        _call(args)
        print(args, file=sys.stderr)
        return
    if args.func == "basecall":
        from .network import basecall as _basecall
        _basecall.basecall(args)
        print(args, file=sys.stderr)
        return
    if args.func == "pair-basecall":
        from .network import pair_basecall as _pair_basecall
        _pair_basecall.pair_basecall(args)
        print(args, file=sys.stderr)
        return
    if args.func == "find-pairs":
        from . import pairs as _pairs
        _pairs.find_pairs_cli(args)
        print(args, file=sys.stderr)
        return
    if args.func == "benchmark":
        from . import benchmark as _benchmark
        _benchmark.benchmark(args)
        print(args, file=sys.stderr)
        return
    from .decoding import decode as _decode, pair_decode as _pair
    if args.func == "decode":
        _decode.decode(args)
    else:
        _pair.pair_decode(args)
    print(args, file=sys.stderr)


if __name__ == "__main__":
    main()
