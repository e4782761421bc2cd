"""Minimal trainer to obtain a *learned* hash -- stock PyTorch-ROCm autograd.

Not part of the query-time hot path and not accelerated: it exists because the headline metric is
quoted on a "16-bit learned hash" and no checkpoint exists offline.  It restates the reference's
triplet recipe: Adam(amsgrad) loop with periodic validation through `Indexer` (the live caller of the
hot path, nlsh/trainers/base.py:36-115), triplet loss on the L2 distance between Bernoulli code
vectors (nlsh/trainers/triplet.py:16-26, nlsh/learning/distances.py:245-254), anchors with a random
k-NN positive and a random negative (triplet.py:101-131), brute-force self-kNN of the training set
(precompute.py:57-67).  Validation = the HIP path (`Indexer.query`).
"""
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .indexer import Indexer
from .metrics import calculate_recall


def self_knn(x: torch.Tensor, k: int, chunk: int = 4096, metric: str = "l2") -> torch.Tensor:
    """Row ids [n, k] of each row's k nearest OTHER rows (exact, chunked mm + topk on the device)."""
    n = x.shape[0]
    xn = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if metric == "cosine" else x
    sq = (xn * xn).sum(1)
    out = torch.empty((n, k), dtype=torch.int64, device=x.device)
    for s in range(0, n, chunk):
        q = xn[s:s + chunk]
        dist = sq[None, :] - 2.0 * (q @ xn.T) if metric == "l2" else -(q @ xn.T)
        dist[torch.arange(q.shape[0], device=x.device), torch.arange(s, s + q.shape[0], device=x.device)] = float("inf")
        out[s:s + chunk] = dist.topk(k, dim=1, largest=False).indices
    return out


def code_l2_rowwise(p, q):
    """MVBernoulliL2.rowwise (distances.py:247-254)."""
    return F.pairwise_distance(p, q)


def triplet_loss(anchor, pos, neg, distance_func=code_l2_rowwise, margin=0.1):
    return torch.clamp(distance_func(anchor, pos) - distance_func(anchor, neg) + margin, min=0).mean()


def triplet_batches(n: int, knn: torch.Tensor, positive_k: int, batch_size: int, generator: torch.Generator,
                    negative_band=None):
    """One epoch of (anchor, positive, negative) row-id batches: shuffled anchors, a random one of the
    first `positive_k` neighbours, a uniformly random negative (triplet.py:101-131, method "random").
    negative_band=(lo, hi): negatives are the anchor's neighbours of rank lo..hi-1 instead (a cheap
    stand-in for the reference's unimplemented "hard"/"semi-hard" modes, triplet.py:10-13)."""
    dev = knn.device
    anchors = torch.randperm(n, generator=generator, device=dev)
    cols = torch.randint(0, positive_k, (n,), generator=generator, device=dev)
    if negative_band is None:
        negs = torch.randint(0, n, (n,), generator=generator, device=dev)
    else:
        ncols = torch.randint(negative_band[0], negative_band[1], (n,), generator=generator, device=dev)
    for s in range(0, n - batch_size + 1, batch_size):
        a = anchors[s:s + batch_size]
        neg = negs[s:s + batch_size] if negative_band is None else knn[a, ncols[s:s + batch_size]]
        yield a, knn[a, cols[s:s + batch_size]], neg


def fit_triplet(hashing, train_vectors: torch.Tensor, knn: torch.Tensor, n_steps: int = 3000, batch_size: int = 1024,
                learning_rate: float = 3e-4, margin: float = 0.1, positive_k: int = 10, balance_weight: float = 0.0,
                negative_band=None, seed: int = 0, validate: Optional[Callable[[int], Dict]] = None, test_every_updates: int = 1000,
                log: Callable[[str], None] = print) -> List[Dict]:
    """Adam(amsgrad) triplet training (base.py:58-79).  `balance_weight` > 0 adds a bit-balance
    term (mean probability of every bit -> 0.5), an extension that is OFF by default."""
    gen = torch.Generator(device=train_vectors.device)
    gen.manual_seed(seed)
    opt = torch.optim.Adam(list(hashing.parameters()), lr=learning_rate, amsgrad=True)
    history, step = [], 0
    n = train_vectors.shape[0]
    while step < n_steps:
        for a, p, ng in triplet_batches(n, knn, positive_k, batch_size, gen, negative_band):
            hashing.train_mode(True)
            opt.zero_grad()
            pa, pp, pn = (hashing.predict(train_vectors[i]) for i in (a, p, ng))
            loss = triplet_loss(pa, pp, pn, margin=margin)
            if balance_weight > 0:
                loss = loss + balance_weight * ((pa.mean(0) - 0.5) ** 2).sum()
            loss.backward()
            opt.step()
            step += 1
            if validate is not None and (step % test_every_updates == 0 or step == n_steps):
                hashing.train_mode(False)
                rec = dict(step=step, loss=float(loss.detach()), **validate(step))
                history.append(rec)
                log(f"[train] {rec}")
            if step >= n_steps:
                break
    hashing.train_mode(False)
    return history


def make_validator(hashing, corpus_gpu, queries_gpu, ground_truth, distance_func, k=10, hash_times=10):
    """The reference's validation block (base.py:80-108): build an `Indexer`, time `query`,
    report n_indexes / std_index_rows / recall / query_size / qps -- through the HIP path."""
    def validate(step):
        indexer = Indexer(hashing, corpus_gpu, distance_func)
        torch.cuda.synchronize()
        t1 = time.time()
        recalls, n_candidates = indexer.query(queries_gpu, k=k, hash_times=hash_times)
        t2 = time.time()
        stats = indexer.bucket_stats()
        return {"test/n_indexes": stats["n_indexes"], "test/std_index_rows": stats["std_index_rows"],
                "test/recall": float(calculate_recall(list(ground_truth[:, :k]), recalls, np.mean)),
                "test/query_size": float(np.mean(n_candidates)), "test/qps": queries_gpu.shape[0] / (t2 - t1)}
    return validate


def export_weights(hashing) -> Dict[str, np.ndarray]:
    """Plain arrays (W0, b0, W1, ...) of the folded Linear stack: a portable checkpoint."""
    out = {}
    for i, (w, b) in enumerate(hashing.linear_stack()):
        out[f"W{i}"] = w.detach().cpu().numpy().astype(np.float32)
        if b is not None:
            out[f"b{i}"] = b.detach().cpu().numpy().astype(np.float32)
    return out


def load_weights(hashing, arrays) -> None:
    """Inverse of `export_weights` for encoders without BatchNorm (Linear layers in forward order)."""
    linears = [m for m in hashing._hasher.modules() if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for i, lin in enumerate(linears):
            lin.weight.copy_(torch.as_tensor(arrays[f"W{i}"]))
            if lin.bias is not None and f"b{i}" in arrays:
                lin.bias.copy_(torch.as_tensor(arrays[f"b{i}"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# Partition (Categorical) hashes: the Neural LSH recipe -- partition the training set, then fit a classifier to the partition.

def kmeans_partition(x: torch.Tensor, n_bins: int, iters: int = 10, seed: int = 0) -> torch.Tensor:
    """Lloyd's k-means labels int64 [n] in [0, n_bins) of the device rows `x`: centroids start at `n_bins` distinct random rows (`seed`),
    every assignment is the exact nearest centroid (`exact_topk(..., k=1)`: (distance, centroid id) order, so ties are settled), an
    empty bin keeps its centroid."""
    from .exact import exact_topk
    n = x.shape[0]
    if not 1 <= n_bins <= n:
        raise ValueError(f"n_bins must be in [1, {n}], got {n_bins}")
    gen = torch.Generator(device=x.device)
    gen.manual_seed(seed)
    x = x.float()
    centroids = x[torch.randperm(n, generator=gen, device=x.device)[:n_bins]].contiguous()
    labels = None
    for it in range(max(int(iters), 0) + 1):
        labels = exact_topk(x, centroids, 1)[1][:, 0].long()
        if it == iters:
            break
        sums = torch.zeros_like(centroids).index_add_(0, labels, x)
        counts = torch.bincount(labels, minlength=n_bins)
        live = counts > 0
        centroids = torch.where(live[:, None], sums / counts.clamp_min(1)[:, None].float(), centroids).contiguous()
    return labels


def partition_targets(labels: torch.Tensor, n_bins: int, knn: Optional[torch.Tensor] = None, soft_k: int = 10) -> torch.Tensor:
    """Training targets float32 [n, n_bins] of a partition: one-hot labels, or with `knn` (row ids [n, >= soft_k]) the Neural LSH soft
    target -- the bin histogram of the row's first `soft_k` neighbours, normalised to sum 1."""
    if knn is None:
        return F.one_hot(labels, n_bins).float()
    near = labels[knn[:, :soft_k]]                                  # [n, k'] bins of the neighbours
    hist = torch.zeros((labels.shape[0], n_bins), dtype=torch.float32, device=labels.device)
    hist.scatter_add_(1, near, torch.ones_like(near, dtype=torch.float32))
    return hist / hist.sum(1, keepdim=True)


def fit_partition(hashing, x: torch.Tensor, labels: torch.Tensor, knn: Optional[torch.Tensor] = None, soft_k: int = 10,
                  n_steps: int = 1000, batch_size: int = 1024, learning_rate: float = 1e-3, seed: int = 0,
                  log: Optional[Callable[[str], None]] = None, log_every: int = 0) -> List[float]:
    """Fit a `Categorical` hash (anything with `parameters()`, `train_mode()` and a `predict()` that returns bin probabilities with
    gradients in train mode) to a partition of the rows `x`: Adam on the cross-entropy between `predict(x)` and `partition_targets`.
    Plain torch autograd, outside the hot path.  -> the loss of every step.  Leaves the hashing in eval mode."""
    n, n_bins = x.shape[0], int(hashing.output_dim)
    targets = partition_targets(labels, n_bins, knn, soft_k)
    gen = torch.Generator(device=x.device)
    gen.manual_seed(seed)
    opt = torch.optim.Adam(list(hashing.parameters()), lr=learning_rate)
    losses = []
    hashing.train_mode(True)
    while len(losses) < n_steps:
        order = torch.randperm(n, generator=gen, device=x.device)
        for s in range(0, n, batch_size):
            rows = order[s:s + batch_size]
            opt.zero_grad()
            p = hashing.predict(x[rows])
            loss = -(targets[rows] * torch.log(p.clamp_min(1e-30))).sum(1).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            if log is not None and log_every and len(losses) % log_every == 0:
                log(f"[fit_partition] step {len(losses)} loss {losses[-1]:.4f}")
            if len(losses) >= n_steps:
                break
    hashing.train_mode(False)
    return losses


def pq_train(x: torch.Tensor, dsub: int, iters: int = 10, seed: int = 0, sample: int = 65536) -> torch.Tensor:
    """A product-quantiser codebook for `Indexer(storage="pq")`: float32 [M, 256, dsub] on x's device, M = ceil(d / dsub),
    from `iters` Lloyd iterations per sub-space on a seeded sample of at most `sample` rows of x [n, d] (device).
    The assignment step IS `nlsh_pq_encode` (the index's own encoder); the update is an `index_add_` mean per (sub-space, centroid), taken on
    the host so that its summation order -- and with it the codebook -- is the same on every run of the same seed; an empty centroid keeps
    its previous value.  The centroids start as sample rows; with fewer than 256 of them the rows repeat.  Rows holding a NaN or an infinity
    are left out of the sample (the index refuses them by number when it encodes).  Columns of the last sub-vector at or beyond d are +0.
    Seeded, not bit-defined across devices or library versions: the codebook is an input of the storage's rule, not part of it."""
    from .indexer import PQ_DSUBS, pq_encode
    if isinstance(dsub, bool) or dsub not in PQ_DSUBS:
        raise ValueError(f"dsub must be one of {PQ_DSUBS}, got {dsub!r}")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be a [n, d] tensor")
    if iters < 0 or sample < 1:
        raise ValueError("iters must be >= 0 and sample >= 1")
    n, d = int(x.shape[0]), int(x.shape[1])
    M, dev = (d + dsub - 1) // dsub, x.device
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    rows = x if n <= sample else x[torch.randint(n, (sample,), generator=g).to(dev)]
    rows = rows.float()
    rows = rows[torch.isfinite(rows).all(dim=1)].contiguous()
    S = int(rows.shape[0])
    if S == 0:
        return torch.zeros((M, 256, dsub), dtype=torch.float32, device=dev)
    padded = torch.zeros((S, M * dsub), dtype=torch.float32)
    padded[:, :d] = rows.cpu()
    sub = padded.view(S * M, dsub)      # row s * M + m: sub-vector m of sample row s
    start = torch.arange(256) % S if S < 256 else torch.randperm(S, generator=g)[:256]
    cb = padded[start].view(256, M, dsub).permute(1, 0, 2).contiguous()
    offs = (torch.arange(M) * 256)[None, :]
    for _ in range(iters):
        codes = pq_encode(rows, cb.to(dev), d, "sample").cpu().long()       # [S, M]
        flat = (codes + offs).view(-1)
        sums = torch.zeros((M * 256, dsub), dtype=torch.float32).index_add_(0, flat, sub)
        counts = torch.zeros((M * 256,), dtype=torch.float32).index_add_(0, flat, torch.ones((S * M,), dtype=torch.float32))
        mean = sums / counts.clamp(min=1.0)[:, None]
        cb = torch.where((counts > 0)[:, None], mean, cb.view(M * 256, dsub)).view(M, 256, dsub).contiguous()
    return cb.to(dev)
