#!/usr/bin/env python3
"""Write tests/golden/pairs/: what the `find-pairs` tests need of the reference's reads, as data.

  ref_meta.tsv    file name, read id, channel, read number, start time and duration (samples) and sampling rate of the
                  ten reads of data/reads/ and of data/read.fast5, as their FAST5 attributes record them
  ref_1d.fasta    the eleven reads' 1D basecalls: the reference's shipped checkpoint (data/model/checkpoint-124) through
                  the float64 restatement tests/_call_oracle.py, windows of 1000, CTC best path; record id = file stem
  ref_pairs.txt   the reference's data/pairs.txt (five pairs, template first)

Runs where the reference checkout is present (POREOVER_REFERENCE, default /root/reference); about five CPU minutes.

    python3 tests/golden/make_pairs_fixture.py
"""
import glob
import multiprocessing
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from poreover_amd import pairs  # noqa: E402
from poreover_amd.decoding.decode import fasta_format  # noqa: E402

REFERENCE = os.environ.get("POREOVER_REFERENCE", "/root/reference")
COLUMNS = ["filename", "read_id", "channel", "read_number", "start_time", "duration", "sampling_rate"]


def basecall(path):
    import _call_oracle as O
    from poreover_amd.network import checkpoint, parse_fast5
    net = checkpoint.load_network(os.path.join(REFERENCE, "data", "model", "checkpoint-124"))
    _, probs = O.basecall(net, parse_fast5(path)[1], 1000)
    return pairs.read_key(path), O.greedy(probs)


def main():
    out = os.path.join(HERE, "pairs")
    os.makedirs(out, exist_ok=True)
    files = sorted(glob.glob(os.path.join(REFERENCE, "data", "reads", "*.fast5"))) + \
        [os.path.join(REFERENCE, "data", "read.fast5")]
    table = pairs.read_metadata(files)
    with open(os.path.join(out, "ref_meta.tsv"), "w") as f:
        f.write("\t".join(COLUMNS) + "\n")
        for r in table:
            f.write("\t".join([r["name"], r["read_id"], r["channel"], str(r["read_number"]), str(r["start_time"]),
                               str(r["duration"]), "%g" % r["sampling_rate"]]) + "\n")
    shutil.copyfile(os.path.join(REFERENCE, "data", "pairs.txt"), os.path.join(out, "ref_pairs.txt"))
    with multiprocessing.Pool(min(4, len(files))) as pool:
        calls = pool.map(basecall, files)
    with open(os.path.join(out, "ref_1d.fasta"), "w") as f:
        for key, seq in calls:
            f.write(fasta_format(key, seq))
    print("ref_meta.tsv: %d reads; ref_1d.fasta: %d records, %d - %d bases" %
          (len(table), len(calls), min(len(s) for _, s in calls), max(len(s) for _, s in calls)))


if __name__ == "__main__":
    main()
