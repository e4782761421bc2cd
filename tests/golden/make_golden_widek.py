#!/usr/bin/env python3
"""Golden vectors for k > 64: Indexer.query of the UNMODIFIED reference on injected keys at k = 100 (L2) and k = 200 (cosine).

Same generator as the g5 vectors (make_golden.g5_case, which needs the reference next to this checkout and runs it on the CPU);
only the two data files g9_query_widek.{npz,json} are committed.

    python tests/golden/make_golden_widek.py
"""
import json
import os

import numpy as np

import make_golden

HERE = os.path.dirname(os.path.abspath(__file__))


def g9():
    arrays, meta = {}, {}
    make_golden.g5_case("l2_k100", "l2", 128, 6000, 24, 5, 100, 900, arrays, meta)
    make_golden.g5_case("cos_k200", "cosine", 100, 8000, 16, 4, 200, 910, arrays, meta)
    np.savez_compressed(os.path.join(HERE, "g9_query_widek.npz"), **arrays)
    with open(os.path.join(HERE, "g9_query_widek.json"), "w") as f:
        json.dump(meta, f)


if __name__ == "__main__":
    g9()
    print("wrote g9_query_widek.{npz,json}")
