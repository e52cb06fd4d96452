#!/usr/bin/env python3
"""Write tests/golden/call_weight_stats.json: the mean / std of every tensor of the reference's shipped checkpoint
(data/model/checkpoint-124, the default conv1_bigru3) and the same pooled per role — what the GPU tests of `call` draw
their seeded synthetic weights from (poreover_amd.network.checkpoint.synthetic_weights).  The 3.6 MB weight shard itself
is not committed.  Runs where the reference checkout is present (POREOVER_REFERENCE, default /root/reference).

    python3 tests/golden/make_call_vectors.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from poreover_amd.network import checkpoint  # noqa: E402


def role(name):
    parts = name.split("/")
    leaf = [p for p in parts if p in ("kernel", "recurrent_kernel", "bias")][0]
    if parts[0] == "layer_with_weights-0":
        return "conv0/" + leaf
    if parts[0] == "layer_with_weights-4":
        return "dense/" + leaf
    return "gru/" + leaf


def main():
    ref = os.environ.get("POREOVER_REFERENCE", "/root/reference")
    w = checkpoint.read_checkpoint(os.path.join(ref, "data", "model", "checkpoint-124"))
    per_tensor = {k: [float(np.mean(v)), float(np.std(v)), list(v.shape)] for k, v in sorted(w.items())}
    pooled = {}
    for k, v in w.items():
        pooled.setdefault(role(k), []).append(v.ravel())
    roles = {r: [float(np.mean(np.concatenate(a))), float(np.std(np.concatenate(a)))] for r, a in sorted(pooled.items())}
    out = {"source": "data/model/checkpoint-124 (conv1_bigru3)", "n_params": int(sum(v.size for v in w.values())),
           "roles": roles, "tensors": per_tensor}
    with open(os.path.join(HERE, "call_weight_stats.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("call_weight_stats.json: %d tensors, %d parameters" % (len(w), out["n_params"]))


if __name__ == "__main__":
    main()
