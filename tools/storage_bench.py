#!/usr/bin/env python3
"""Corpus storage A/B: the same corpus as a float32, a float16 and a uint8 index, timed in ONE process with the storages
interleaved round by round -- the scan kernel alone (HIP events around it, `events=`) and the device-resident batch
(`Indexer.query_tensors`, host clock around `steps` batches ending in a synchronise).  GPU only; reads nothing outside the repository.

Workloads (the generators bench.py uses, the learned hashes of checkpoints/):
  sift1m    synth.sift_manifold, 10^6 x 128, L2, 16-bit hash.  The generator's rows are integers in [0, 218]: they are indexed RAW, so all
            three storages hold identical values; the standardisation the hash was trained behind is folded into its first layer.
  clusters  synth.sift_like (SURVEY 8(d)'s generator), 10^6 x 128, L2, 16-bit hash; raw integers, as above.
  glove     synth.glove_manifold, 1,183,514 x 100, cosine, 24-bit hash.  Real-valued: float16 holds the rounded rows, float32 holds the SAME
            rounded rows (dequantised), uint8 does not apply.
  deep      synth.deep_like, 10^6 x 96, L2-normalised rows, L2, a seeded random 16-bit hash.  Real-valued, as glove.
Every storage of a workload gets the same `corpus_keys=` and the same query key table, so the task tables are identical and the results
are compared bit for bit before anything is timed.  `--sq8` adds an sq8 index of the same rows to every workload (same keys, same task
table, its own distances): recall@10 against the float32 lists and the training pass beside a device copy are reported with the times
(profiles/sq8_storage.txt is made from it).  `--pq 4,8,16` adds a product-quantised index per sub-vector width in the same way (DESIGN.md
4.18; profiles/pq_storage.txt): codebook training time, encoder rows/s, bytes per row, recall@10 against the float32 lists without and
with an exact re-rank of 2 / 4 / 8 x k stage-one candidates.

    python tools/storage_bench.py [--workloads sift1m,clusters,glove,deep] [--sq8] [--pq 4,8,16] [--rounds 7] [--iters 10] [--steps 20] [--out FILE]

Prints one JSON line per workload and a table; `--out` also writes the table to a file (profiles/corpus_storage.txt is made from it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlsh_amd import io, synth  # noqa: E402
from nlsh_amd.data import Glove, SIFT  # noqa: E402
from nlsh_amd.indexer import Indexer  # noqa: E402

HBM_PEAK_GBPS = 8000.0      # bench.py's figure (MI355X: 8.0 TB/s spec)
K, P = 10, 10
WORKLOADS = {
    "sift1m": dict(gen="sift_manifold", N=1_000_000, d=128, ckpt="sift1m_manifold_h16.npz", metric="l2", compat=True, storages=("float32", "float16", "uint8")),
    "clusters": dict(gen="sift_like", N=1_000_000, d=128, ckpt="sift1m_clusters_h16.npz", metric="l2", compat=True, storages=("float32", "float16", "uint8")),
    "glove": dict(gen="glove_manifold", N=1_183_514, d=100, ckpt="glove_manifold_h24.npz", metric="cosine", compat=False, storages=("float32", "float16")),
    # Deep-shaped: synth.deep_like, L2-normalised 96-d rows.  No checkpoint was trained on this generator: a seeded random 16-bit MLP hash
    # (synth.make_weights) gives the buckets -- the storages are compared on one task table, the hash's quality does not enter.
    "deep": dict(gen="deep_like", N=1_000_000, d=96, ckpt=None, metric="l2", compat=False, storages=("float32", "float16")),
}
DTYPE = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8}
# `--sq8`: every workload also gets an sq8 index built from the SAME rows with the same corpus_keys= and timed in the same
# interleaved rounds.  Its rows are deq(enc(x)), not x: it is not held to the float32 bits here (tests/test_gpu_sq8_storage.py holds it to
# its own float32 twin); what is reported instead is recall@10 of its lists against the float32 index's at the same probes, and the
# training pass's time beside a plain device copy of the same bytes.


def train_vs_copy(rows, stride, rounds=7):
    """(median ms of `nlsh_sq8_train` over `rows`, median ms of a device copy of the same bytes), interleaved."""
    from nlsh_amd import _capi
    L, (n, d), dev = _capi.lib(), rows.shape, rows.device
    lo, step = torch.empty((stride,), device=dev), torch.empty((stride,), device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    wb = L.nlsh_sq8_train_workspace(n, d)
    ws = torch.empty((wb,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(rows)
    s = torch.cuda.current_stream().cuda_stream
    t_train, t_copy = [], []
    for r in range(rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _capi.check(L.nlsh_sq8_train(rows.data_ptr(), _capi.STORE_F32, rows.stride(0), d, n, lo.data_ptr(), step.data_ptr(), stride,
                                     bad.data_ptr(), ws.data_ptr(), wb, s))
        ev[1].record()
        dst.copy_(rows)
        ev[2].record()
        torch.cuda.synchronize()
        if r:       # the first round warms up
            t_train.append(ev[0].elapsed_time(ev[1])); t_copy.append(ev[1].elapsed_time(ev[2]))
    return float(np.median(t_train)), float(np.median(t_copy))


def recall_at_k(got_idx, ref_idx):
    """Mean fraction of the reference lists' ids (padding excluded) that the other lists hold."""
    g, r = got_idx.cpu().numpy(), ref_idx.cpu().numpy()
    hits = sum(len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) for a, b in zip(g, r))
    return hits / max(int((r >= 0).sum()), 1)


def pq_index(hashing, stored, dist, w, dsub, keys_of_rows):
    """-> (pq Indexer at this sub-vector width over `stored`, {training seconds, encoder ms (median of 3, HIP events)})."""
    from nlsh_amd.indexer import pq_encode
    from nlsh_amd.training import pq_train
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cb = pq_train(stored, dsub)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    ix = Indexer(hashing, stored, dist, compat=w["compat"], storage="pq", pq_dsub=dsub, quantiser=cb, corpus_keys=keys_of_rows)
    enc = []
    for _ in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        codes = pq_encode(stored, ix.codebook, ix.dim)
        b.record()
        torch.cuda.synchronize()
        enc.append(a.elapsed_time(b))
    del codes
    return ix, {"train_s": train_s, "encode_ms": float(np.median(enc[1:])), "code_bytes_per_row": int(ix._store_dim), "pitch_bytes": int(ix.row_stride)}


def build(tag, n_rows, Q, dev, sq8=False, pq=()):
    """-> ({storage: Indexer}, query batch, key table, (distinct candidate rows, candidates) of the batch, sq8 extras or None, pq extras)."""
    w = WORKLOADS[tag]
    N, d = n_rows or w["N"], w["d"]
    gen = getattr(synth, w["gen"])
    corpus_h, queries_h = gen(N, d, seed=synth.SEED_DATA), gen(Q, d, seed=synth.SEED_QUERY)
    if w["ckpt"]:
        Ws, bs = io.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", w["ckpt"]))
    else:
        Ws, bs = synth.make_weights([d, 256, 16], gain=4.0)
    Ws, bs = [np.asarray(W, np.float32) for W in Ws], [np.asarray(b, np.float32) for b in bs]
    if w["metric"] == "l2" and w["ckpt"]:     # raw integral rows: the hash's standardisation moves into its first layer, W (x - m) / s + b = (W / s) x + (b - (W / s) m)
        _, mean, std = synth.standardise(corpus_h)
        Ws[0] = (Ws[0] / std[None, :]).astype(np.float32)
        bs[0] = (bs[0] - Ws[0] @ mean).astype(np.float32)
        assert np.array_equal(corpus_h, np.rint(corpus_h)) and corpus_h.min() >= 0 and corpus_h.max() <= 255
        stored = torch.from_numpy(corpus_h).to(dev)
    else:                       # real-valued rows: every storage holds the float16-rounded values
        if not w["ckpt"]:       # the seeded hash sees standardised rows, folded into its first layer as above
            _, mean, std = synth.standardise(corpus_h)
            Ws[0] = (Ws[0] / std[None, :]).astype(np.float32)
            bs[0] = (bs[0] - Ws[0] @ mean).astype(np.float32)
        stored = torch.from_numpy(corpus_h).to(dev).half().float()
    hashing = io.hashing_from_weights(Ws, bs, compat=w["compat"])
    dist = SIFT.distance if w["metric"] == "l2" else Glove.distance
    q = torch.from_numpy(queries_h).to(dev)
    ixs, keys_of_rows = {}, None
    for storage in w["storages"] + (("sq8",) if sq8 else ()):
        src = stored if storage in ("float32", "sq8") else stored.to(DTYPE[storage])
        ix = Indexer(hashing, src, dist, compat=w["compat"], storage=storage, algo="tiled" if storage == "float32" else None, corpus_keys=keys_of_rows)
        keys_of_rows = ix.corpus_keys
        ixs[storage] = ix
        del src
    pq_extras = {}
    for dsub in pq:
        ixs[f"pq{dsub}"], pq_extras[f"pq{dsub}"] = pq_index(hashing, stored, dist, w, dsub, keys_of_rows)
    store = None
    if pq:      # the exact second stage over the rows every storage was built from (nlsh_amd/refine.py), driven by hand on stage-one lists
        from nlsh_amd.refine import RefineStore
        store = RefineStore(stored, w["metric"], id_base=0, where="device")
    keys, nkeys = ixs["float32"].hash_device(q, hash_times=P, seed=7)
    ref, extras = None, None
    for storage, ix in ixs.items():                 # sizes the task tables (checked calls) and holds every storage to the float32 bits
        out = ix.scan_tensors(q, keys, nkeys, k=K)
        if ref is None:
            ref = out
        if storage.startswith("pq"):                # other rows, by design: the same candidates, its own distances
            assert torch.equal(out[2], ref[2]), storage
            pq_extras[storage]["recall"] = recall_at_k(out[1], ref[1])
            for f in (2, 4, 8):
                one = ix.scan_tensors(q, keys, nkeys, k=f * K)
                pq_extras[storage][f"recall_refine_{f}"] = recall_at_k(store.rerank(q, one[1], K)[1], ref[1])
        elif storage == "sq8":                      # other rows, by design: the same candidates, its own distances
            assert torch.equal(out[2], ref[2]), storage
            t_train, t_copy = train_vs_copy(stored, ix.row_stride)
            extras = {"recall_at_k_vs_float32": recall_at_k(out[1], ref[1]), "clamped_rows": ix.last_clamped_rows,
                      "train_ms": t_train, "copy_ms": t_copy, "train_bytes": int(stored.numel() * 4)}
        else:
            assert torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2]), storage
        ix.query_tensors(q, k=K, hash_times=P, seed=7)
    ix = ixs["float32"]
    pos = torch.searchsorted(ix.uniq_keys, keys.clamp(min=int(ix.uniq_keys[0]), max=int(ix.uniq_keys[-1]))).clamp(max=ix.n_buckets - 1)
    hit = (ix.uniq_keys[pos] == keys) & (torch.arange(keys.shape[1], device=dev)[None, :] < nkeys[:, None])
    rows = (ix.offsets[1:] - ix.offsets[:-1]).long()
    del store
    return ixs, q, keys, nkeys, (int(rows[torch.unique(pos[hit])].sum().item()), int(ref[2].long().sum().item())), extras, pq_extras


def time_round(ix, q, keys, nkeys, iters, steps):
    """(mean scan-kernel ms over `iters` launches, ms per device-resident batch over `steps` batches)."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:            # (`events=` takes events that have been recorded once: the library re-records their handles)
        a.record(); b.record()
    for ev in evs:
        ix.scan_tensors(q, keys, nkeys, k=K, check=False, events=ev)
    torch.cuda.synchronize()
    scan_ms = float(np.mean([a.elapsed_time(b) for a, b in evs]))
    t0 = time.perf_counter()
    for i in range(steps):
        ix.query_tensors(q, k=K, hash_times=P, seed=100 + i, check=False)
    torch.cuda.synchronize()
    batch_ms = 1e3 * (time.perf_counter() - t0) / steps
    assert int(ix.last_status.cpu()[1]) == 0, "task table overflow inside a timed region"
    return scan_ms, batch_ms


def spread(xs):
    xs = sorted(xs)
    return {"median": float(np.median(xs)), "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="sift1m,clusters,glove")
    ap.add_argument("--rows", type=int, default=0, help="rows of every workload (default: its own size)")
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7, help="interleaved rounds (A B C A B C ...): medians and the min..max spread are over the rounds")
    ap.add_argument("--iters", type=int, default=10, help="scan launches per storage and round")
    ap.add_argument("--steps", type=int, default=20, help="device-resident batches per storage and round")
    ap.add_argument("--sq8", action="store_true", help="also build and time an sq8 index of every workload (recall and training time reported)")
    ap.add_argument("--pq", default="", help="comma-separated sub-vector widths (4, 8, 16): also build and time a pq index per width")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("storage_bench needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    lines = []
    for tag in args.workloads.split(","):
        ixs, q, keys, nkeys, (uniq_rows, sum_c), extras, pq_extras = build(tag, args.rows, args.queries, dev, sq8=args.sq8,
                                                                           pq=tuple(int(v) for v in args.pq.split(",") if v))
        d = ixs["float32"].dim
        for ix in ixs.values():     # warm-up round, untimed
            time_round(ix, q, keys, nkeys, 3, 3)
        rounds = {s: [] for s in ixs}
        for _ in range(args.rounds):
            for s, ix in ixs.items():
                rounds[s].append(time_round(ix, q, keys, nkeys, args.iters, args.steps))
        res = {"workload": tag, "N": int(ixs["float32"].gid.shape[0]), "d": d, "Q": args.queries, "k": K, "hash_times": P, "rounds": args.rounds,
               "distinct_candidate_rows": uniq_rows, "candidates": sum_c, "n_buckets": ixs["float32"].n_buckets, "storages": {}}
        base = None
        for s, ix in ixs.items():
            scan, batch = spread([r[0] for r in rounds[s]]), spread([r[1] for r in rounds[s]])
            elem = ix.corpus_sorted.element_size()
            row_bytes = (ix._store_dim if s.startswith("pq") else d) * elem    # the bytes of a row the scan needs (the pitch may pad)
            base = base or scan["median"]
            res["storages"][s] = {"index_bytes": int(ix.corpus_sorted.numel() * elem), "row_pitch_bytes": int(ix.row_stride * elem), "scan_ms": scan,
                                  "batch_ms": batch, "route": ix.last_query_path, "scan_vs_float32": scan["median"] / base,
                                  "hbm_frac_of_distinct_candidate_rows": uniq_rows * row_bytes / (scan["median"] * 1e-3) / 1e9 / HBM_PEAK_GBPS}
        if extras:
            res["sq8"] = extras
        if pq_extras:
            res["pq"] = pq_extras
        print(json.dumps(res), flush=True)
        lines.append(f"{tag}: N={res['N']} d={d} Q={args.queries} k={K} hash_times={P}, {res['n_buckets']} buckets, {uniq_rows} distinct candidate rows, "
                     f"{sum_c} candidates per batch; {args.rounds} interleaved rounds x ({args.iters} scans, {args.steps} batches)")
        lines.append(f"  {'storage':8} {'index MiB':>10} {'pitch B':>8} {'scan ms median (min..max)':>28} {'x float32':>10} {'HBM frac':>9} "
                     f"{'ms/batch median (min..max)':>28}  route")
        for s, r in res["storages"].items():
            lines.append(f"  {s:8} {r['index_bytes'] / 2 ** 20:10.1f} {r['row_pitch_bytes']:8d} "
                         f"{r['scan_ms']['median']:10.4f} ({r['scan_ms']['min']:.4f}..{r['scan_ms']['max']:.4f}) {r['scan_vs_float32']:10.3f} "
                         f"{r['hbm_frac_of_distinct_candidate_rows']:9.3f} {r['batch_ms']['median']:10.4f} ({r['batch_ms']['min']:.4f}..{r['batch_ms']['max']:.4f})  {r['route']}")
        if extras:
            gbps = lambda ms, passes: extras["train_bytes"] * passes / (ms * 1e-3) / 1e9   # noqa: E731
            lines.append(f"  sq8: recall@{K} against the float32 index at the same probes {extras['recall_at_k_vs_float32']:.4f}; "
                         f"{extras['clamped_rows']} rows saturated; training pass {extras['train_ms']:.3f} ms ({gbps(extras['train_ms'], 1):.0f} GB/s read) "
                         f"beside a device copy of the same {extras['train_bytes'] / 2 ** 20:.0f} MiB {extras['copy_ms']:.3f} ms "
                         f"({gbps(extras['copy_ms'], 2):.0f} GB/s read + written)")
        for s, e in pq_extras.items():
            lines.append(f"  {s}: {e['code_bytes_per_row']} code bytes per row (pitch {e['pitch_bytes']}); pq_train {e['train_s']:.2f} s; nlsh_pq_encode "
                         f"{e['encode_ms']:.2f} ms = {res['N'] / (e['encode_ms'] * 1e-3) / 1e6:.1f} M rows/s; recall@{K} against the float32 lists "
                         f"{e['recall']:.4f}, re-ranked from 2k / 4k / 8k stage-one candidates {e['recall_refine_2']:.4f} / {e['recall_refine_4']:.4f} / "
                         f"{e['recall_refine_8']:.4f}")
        del ixs, q, keys, nkeys
        torch.cuda.empty_cache()
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
