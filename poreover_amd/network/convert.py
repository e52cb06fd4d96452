"""`python -m poreover_amd.network.convert CKPT out.npz`: a TF checkpoint (prefix, or a directory with a `checkpoint`
file) as an .npz of the same tensor names, every tensor crc32c-checked — what `call --weights` also accepts."""
import argparse

import numpy as np

from . import checkpoint


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m poreover_amd.network.convert", description=__doc__.split(":", 1)[1].strip())
    p.add_argument("checkpoint", help="checkpoint prefix (e.g. model/checkpoint-124) or directory")
    p.add_argument("out", help="output .npz")
    a = p.parse_args(argv)
    w = checkpoint.read_checkpoint(a.checkpoint)
    np.savez(a.out, **w)
    print("%s: %d tensors, %d parameters" % (a.out, len(w), sum(v.size for v in w.values())))


if __name__ == "__main__":
    main()
