#!/usr/bin/env python3
"""Record tests/golden/ce_parent_bits.json: one SHA-256 per case of tests/ce_bits_cases.py, computed on the GPU by the library that
klab_multimodalmodel_amd loads (KLAB_LIB selects another build).  The fixture states which commit's library it was recorded from;
it is recorded once, from the commit before the three cross-entropy files became csrc/ce.hip, and is not re-recorded from a tree it
is meant to judge.

    KLAB_LIB=<parent build>/libklab_mm.so python tools/record_ce_bits.py --parent <commit hash> [--out tests/golden/ce_parent_bits.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="hash of the commit whose library is loaded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ce_parent_bits.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_ce_bits needs the GPU: nothing is recorded without one")
    from klab_multimodalmodel_amd import ops
    from tests import ce_bits_cases as C
    digests = {}
    for rows, V, dt in C.SHAPES:
        digests.update(C.shape_digests(ops, rows, V, dt))
    assert list(digests) == C.all_ids()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"parent": a.parent, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(digests)} digests from {a.parent} into {a.out}")


if __name__ == "__main__":
    main()
