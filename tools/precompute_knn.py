#!/usr/bin/env python3
"""The reference's precompute.py for this project: exact self-kNN of a dataset's training set, stored where the loaders pick it up.

    python tools/precompute_knn.py --dataset /data/sift1m            # TEXMEX directory -> /data/sift1m/<stem>_train_knn.ivecs
    python tools/precompute_knn.py --dataset glove-100-angular.hdf5 --metric cosine   # -> glove-100-angular.hdf5.processed (needs h5py)

The k nearest OTHER rows of every training row come from `nlsh_amd.exact.self_knn` (nlsh_exact_topk: fp32-MFMA distances, fused top-k, no
[chunk, N] distance matrix).  A row is excluded by its id; precompute.py:57-67 drops column 0 of a (k + 1)-list, which among exact
duplicates may drop a duplicate and keep the row itself.  Vectors are used as stored (the reference precomputes on the raw `train` too).
A TEXMEX directory gets `<stem>_train_knn.ivecs` beside `<stem>_base.fvecs` (nlsh_amd.data reads `*train_knn.ivecs`); an HDF5 file gets
`<file>.processed` with the reference's five datasets (train, train_knn, test, neighbors, distances; precompute.py:91-97).
"""
import argparse
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", required=True, help="TEXMEX directory (*base.[fb]vecs ...) or ann-benchmarks HDF5 file")
    ap.add_argument("--k", type=int, default=100, help="neighbours per row (precompute.py: 100)")
    ap.add_argument("--metric", default=None, choices=["l2", "cosine"], help="default: l2 for a directory, cosine for an HDF5 file named *angular*")
    args = ap.parse_args()

    from nlsh_amd import exact, io

    path = os.fspath(args.dataset)
    is_dir = os.path.isdir(path)
    metric = args.metric or ("cosine" if not is_dir and "angular" in os.path.basename(path) else "l2")
    if is_dir:
        hits = sorted(glob.glob(os.path.join(path, "*base.[fb]vecs")))   # the file nlsh_amd.data reads as `training`
        if not hits:
            raise FileNotFoundError(f"{path}: no file matches *base.[fb]vecs")
        base = hits[0]
        train = np.ascontiguousarray(io.read_bvecs(base) if base.endswith(".bvecs") else io.read_fvecs(base), np.float32)
        out = base[: base.rindex("base.")] + "train_knn.ivecs"
    else:
        import h5py   # ImportError when missing: no silent substitute
        with h5py.File(path, "r") as f:
            arrays = {name: np.asarray(f[name]) for name in ("train", "test", "neighbors", "distances")}
        train = np.ascontiguousarray(arrays["train"], np.float32)
        out = path + ".processed"

    t0 = time.time()
    knn = exact.self_knn(torch.from_numpy(train).cuda(), args.k, metric=metric)
    torch.cuda.synchronize()
    knn = knn.cpu().numpy()
    print(f"[precompute] self-kNN of {train.shape[0]} x {train.shape[1]} rows, k = {args.k}, {metric}: {time.time() - t0:.2f}s "
          f"(workspace {exact.workspace_bytes(train.shape[0], train.shape[0], args.k) / 2**20:.1f} MiB)", flush=True)
    if is_dir:
        io.write_vecs(out, knn.astype(np.int32))
    else:
        with h5py.File(out, "w") as f:
            f.create_dataset("train", data=arrays["train"])
            f.create_dataset("train_knn", data=knn)
            f.create_dataset("test", data=arrays["test"])
            f.create_dataset("neighbors", data=arrays["neighbors"])
            f.create_dataset("distances", data=arrays["distances"])
    print(f"[precompute] wrote {out}", flush=True)


if __name__ == "__main__":
    main()
