#!/usr/bin/env python3
"""The reference's own C++ results for the calls of tests/test_oracle_vs_ref.py -> tests/golden/ref_vectors.json.
Needs oracle/_ref/libporef.so (oracle/Makefile `make ref`, from the reference's sources; build container only).
Runs that test module with every reference call live (each comparison with the oracle is made on the way) and
records the answers; the inputs are seeded synthetic pairs (poreover_amd.synth), so only the outputs are stored.

    python3 tests/golden/make_ref_vectors.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_vectors.json")


def main():
    sys.path.insert(0, REPO)
    from oracle import po_oracle as O
    O.build()
    if not O.have_ref():
        raise SystemExit("oracle/_ref/libporef.so is not built: the reference's sources are needed")
    if os.path.exists(OUT):
        os.remove(OUT)
    env = dict(os.environ, PO_RECORD_REF_VECTORS=OUT)
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                           os.path.join(REPO, "tests", "test_oracle_vs_ref.py")], env=env, cwd=REPO)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
