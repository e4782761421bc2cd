#!/usr/bin/env python
"""Categorical hashing on the MI355X, measured (profiles/categorical.txt); needs the GPU.

    python tools/categorical_bench.py [--out profiles/categorical.txt] [--repeats 50] [--skip-recall]

Three parts, every comparison inside this one process, after a warm-up, as medians over `--repeats` launches timed by device events:
  1. bin selection: `nlsh_probe_bins` on 10^4 rows at M = 256 / 4096 and n = 10 / 64, beside `torch.topk(logits, n, sorted=True)` on the same
     tensor (the stock alternative) and `nlsh_probe_ranked` at H = 16 and the same n (the project's own multi-probe kernel);
  2. the logits forward `nlsh_encode_logits` of [128, 256, 256, 256] at 10^4 rows beside `nlsh_encode_hash_stream` of [128, 256, 256, 16];
  3. recall@10 against mean candidates on 10^5 x 128-d `synth.sift_manifold` rows, 10^3 queries: a k-means + `fit_partition` Categorical hash
     at M = 256 probing 1..32 bins, beside the shipped 16-bit Bernoulli hash (checkpoints/sift1m_manifold_h16.npz) with ranked probes, and
     the Bernoulli curve read at each Categorical point's candidate count (linear in log candidates).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neural-locality-sensitive-hashing_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, repeats, warmup=5):
    """Median / p10 / p90 milliseconds of `fn()` between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1, ms = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), []
    for _ in range(repeats):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    a = np.asarray(ms)
    return float(np.median(a)), float(np.percentile(a, 10)), float(np.percentile(a, 90))


def fmt(t):
    return f"{t[0] * 1e3:9.1f} us (p10 {t[1] * 1e3:.1f}, p90 {t[2] * 1e3:.1f})"


def bin_selection(out, repeats, rows=10_000):
    from nlsh_amd import _capi
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    out("## 1. bin selection, %d rows: nlsh_probe_bins | torch.topk(sorted=True) on the same tensor | nlsh_probe_ranked at H = 16" % rows)
    gen = torch.Generator(device="cuda").manual_seed(0)
    z16 = torch.randn((rows, 16), generator=gen, device="cuda")
    code = ((z16 > 0).int() * (2 ** torch.arange(15, -1, -1, device="cuda", dtype=torch.int32))).sum(1).int()       # MSB-first hard codes
    slower = []
    for M in (256, 4096):
        logits = torch.randn((rows, M), generator=gen, device="cuda")
        for n in (10, 64):
            keys = torch.empty((rows, n), dtype=torch.int32, device="cuda")
            nkeys = torch.empty((rows,), dtype=torch.int32, device="cuda")

            def bins():
                _capi.check(L.nlsh_probe_bins(_capi.ptr(logits), M, rows, M, n, rows, _capi.ptr(keys), _capi.ptr(nkeys), None, stream))

            def ranked():
                _capi.check(L.nlsh_probe_ranked(_capi.ptr(z16), 16, _capi.ptr(code), rows, 16, _capi.KEY_FULL, n, rows, _capi.ptr(keys),
                                                _capi.ptr(nkeys), None, stream))
            tb, tt, tr = timed(bins, repeats), timed(lambda: torch.topk(logits, n, dim=1, sorted=True), repeats), timed(ranked, repeats)
            bins()
            same = bool(torch.equal(keys.long(), torch.topk(logits, n, dim=1, sorted=True).indices))       # random rows: no ties
            out(f"M={M:5d} n={n:3d}  probe_bins {fmt(tb)}  torch.topk {fmt(tt)}  probe_ranked(H=16) {fmt(tr)}  "
                f"bins/topk {tb[0] / tt[0]:.2f}x  same bins as topk: {same}")
            if tb[0] > tt[0]:
                slower.append((M, n))
    out("nlsh_probe_bins slower than torch.topk at: " + (", ".join(f"M={M} n={n}" for M, n in slower) or "no shape measured"))


def logits_forward(out, repeats, rows=10_000):
    from nlsh_amd import _capi, synth
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    out("## 2. forward, %d rows: nlsh_encode_logits [128,256,256,256] | nlsh_encode_hash_stream [128,256,256,16] (one probe)" % rows)
    x = torch.randn((rows, 128), device="cuda")
    res = {}
    for name, dims in (("logits", [128, 256, 256, 256]), ("stream", [128, 256, 256, 16])):
        Ws, bs = synth.make_weights(dims)
        Wd, bd = [torch.from_numpy(W).cuda() for W in Ws], [torch.from_numpy(b).cuda() for b in bs]
        arr, nl = _capi.int_array(dims), len(dims) - 1
        count, pack, size = ((L.nlsh_logits_packed_floats, L.nlsh_logits_pack, L.nlsh_logits_workspace) if name == "logits" else
                             (L.nlsh_encoder_stream_packed_floats, L.nlsh_encoder_stream_pack, L.nlsh_encode_stream_workspace))
        packed = torch.empty(count(nl, arr), dtype=torch.float32, device="cuda")
        _capi.check(pack(nl, arr, _capi.ptr_array(Wd), _capi.ptr_array(bd), _capi.ptr(packed), stream))
        ws = torch.empty(size(rows, nl, arr), dtype=torch.uint8, device="cuda")
        if name == "logits":
            o = torch.empty((rows, dims[-1]), dtype=torch.float32, device="cuda")

            def run():
                _capi.check(L.nlsh_encode_logits(_capi.ptr(x), rows, 128, nl, arr, _capi.ptr(packed), _capi.ptr(o), dims[-1], _capi.ptr(ws),
                                                 ws.numel(), stream))
        else:
            keys, nkeys = torch.empty((rows, 1), dtype=torch.int32, device="cuda"), torch.empty((rows,), dtype=torch.int32, device="cuda")

            def run():
                _capi.check(L.nlsh_encode_hash_stream(_capi.ptr(x), rows, 128, nl, arr, _capi.ptr(packed), _capi.ACT_SIGMOID, _capi.KEY_FULL, 1,
                                                      rows, 0, 0, None, None, None, _capi.ptr(keys), _capi.ptr(nkeys), _capi.ptr(ws), ws.numel(),
                                                      stream))
        res[name] = timed(run, repeats)
        out(f"{name:7s} {dims}: {fmt(res[name])}")
    out(f"logits / streamed encode: {res['logits'][0] / res['stream'][0]:.2f}x")


def recall_curve(ix, qd, truth, hash_times, k=10, **kw):
    from nlsh_amd.metrics import calculate_recall
    rows = []
    for P in hash_times:
        ids, counts = ix.query(qd, k=k, hash_times=P, **kw)
        rows.append((P, float(np.mean(counts)), float(calculate_recall(list(truth), ids, np.mean))))
    return rows


def recall(out, n=100_000, q=1_000, M=256, k=10):
    from nlsh_amd import io as nio, synth
    from nlsh_amd.data import SIFT
    from nlsh_amd.encoders import MultiLayerRelu
    from nlsh_amd.exact import exact_topk
    from nlsh_amd.hashings import Categorical
    from nlsh_amd.indexer import Indexer
    from nlsh_amd.training import fit_partition, kmeans_partition, self_knn
    out(f"## 3. recall@{k} against mean candidates: {n} x 128-d synth.sift_manifold rows, {q} queries")
    corpus, mean, std = synth.standardise(synth.sift_manifold(n, 128))
    queries, _, _ = synth.standardise(synth.sift_manifold(q, 128, seed=synth.SEED_QUERY), mean, std)
    cd, qd = torch.from_numpy(corpus).cuda(), torch.from_numpy(queries).cuda()
    truth = exact_topk(qd, cd, k)[1].cpu().numpy()
    t0 = time.perf_counter()
    labels = kmeans_partition(cd, M, iters=15, seed=0)
    knn = self_knn(cd, 10)
    h = Categorical(MultiLayerRelu(128, [256, 256]), M, None)
    losses = fit_partition(h, cd, labels, knn=knn, soft_k=10, n_steps=2000, batch_size=1024, learning_rate=1e-3)
    torch.cuda.synchronize()
    out(f"k-means ({M} bins, 15 steps) + self-kNN + fit_partition (2000 steps, soft targets of 10 neighbours): {time.perf_counter() - t0:.1f} s, "
        f"loss {np.mean(losses[:10]):.3f} -> {np.mean(losses[-10:]):.3f}")
    cat_ix = Indexer(h, cd, SIFT.distance, compat=False)
    cat = recall_curve(cat_ix, qd, truth, (1, 2, 4, 8, 16, 32), k)
    Ws, bs = nio.load_hasher_weights(os.path.join(ROOT, "neural-locality-sensitive-hashing_amd", "checkpoints", "sift1m_manifold_h16.npz"))
    bern_ix = Indexer(nio.hashing_from_weights(Ws, bs, compat=False), cd, SIFT.distance, compat=False)
    bern = recall_curve(bern_ix, qd, truth, (1, 2, 4, 8, 16, 32, 64, 128), k, probes="ranked")
    out(f"buckets: Categorical {cat_ix.n_buckets}, Bernoulli 16-bit {bern_ix.n_buckets}")
    for name, rows in (("Categorical M=256 (k-means + fit_partition)", cat), ("Bernoulli 16-bit, ranked probes (shipped checkpoint)", bern)):
        out(name)
        for P, c, r in rows:
            out(f"  probes {P:4d}  mean candidates {c:10.1f}  recall@{k} {r:.4f}")
    bc, br = np.log([max(c, 1.0) for _, c, _ in bern]), [r for _, _, r in bern]
    out("matched candidate counts (Bernoulli recall interpolated in log candidates; outside its measured range: its end point)")
    wins = 0
    for P, c, r in cat:
        b = float(np.interp(np.log(max(c, 1.0)), bc, br))
        wins += r > b
        out(f"  at {c:10.1f} candidates: Categorical {r:.4f} (probes {P})  Bernoulli {b:.4f}  -> {'Categorical' if r > b else 'Bernoulli'}")
    out(f"Categorical ahead at {wins} of {len(cat)} matched points")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "categorical.txt"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--skip-recall", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("categorical_bench needs the GPU: nothing here can be timed without one")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"# tools/categorical_bench.py --repeats {args.repeats}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    out("# times: median of the repeats between two device events, after a warm-up; every comparison in this one process")
    bin_selection(out, args.repeats)
    logits_forward(out, args.repeats)
    if not args.skip_recall:
        recall(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
