"""The CPU oracle over the whole dimension range of the scan (1 <= d <= NLSH_MAX_DIM = 1024).

tests/test_gpu_dim_range.py holds the device to `oracle.query_batch` at dimensions where the oracle itself had never been pinned (the
golden vectors are 128-d and 100-d).  Here the oracle is held to a plain fp64 numpy evaluation of the project's two formulas
(nlsh/data.py:201: sqrt(sum(((q - c) + 1e-6)^2)); nlsh/data.py:109: 1 - q.c / (max(|q|, 1e-8) * max(|c|, 1e-8))) at the same list of
dimensions, and its AVX2 form to its scalar form bit for bit.

Bar: every returned distance within 2e-6 * max(1, |d|) of the fp64 value -- a tenth of the device's 2e-5, so a device result checked
against the oracle keeps nine tenths of its tolerance.  (Measured on an x86-64 host, N = 1500: worst 2.3e-7 over d in {1, 2, 3, 5, 13,
17, 65, 68, 257, 1021, 1024}.)  Id lists: the fp64 (distance, id) order, or another member of a tie.  Two candidates can change places
only when both fp32 values are within the distance bar of their fp64 ones, so the fp64 distances at one rank of the two lists differ by
at most twice the bar: 4e-6 * max(1, |d|)."""
import numpy as np
import pytest

from helpers import assert_lists_differ_only_at_ties, check_topk_against_candidates, fp64_distances
from nlsh_amd import synth
from oracle import oracle

# the dimensions of tests/test_gpu_dim_range.py (what each sits on is said there)
DIMS = [1, 2, 3, 4, 5, 12, 13, 16, 17, 33, 64, 65, 129, 256, 257, 513, 784, 960, 1020, 1021, 1023, 1024]
DIST_RTOL = 2e-6
N, Q, P, K, NB = 1500, 40, 3, 10, 12


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_oracle_scan_against_fp64_over_the_dimension_range(metric, d):
    rng = np.random.default_rng(31 * d + (metric == "l2"))
    gen = synth.sift_like if metric == "l2" else synth.glove_like
    corpus, queries = gen(N, d, seed=3000 + d), gen(Q, d, seed=3001 + d)
    corpus[N // 2:N // 2 + 20] = corpus[:20]                           # exact ties across buckets (integer rows at small d tie en masse anyway)
    corpus_keys = rng.integers(0, NB, N).astype(np.int64) * 5 - 17    # ~125 rows per bucket, signed keys with gaps
    perm, uniq, offs = oracle.build_csr(corpus_keys)
    key_lists = [[int(v) * 5 - 17 for v in rng.choice(NB, P, replace=False)] for _ in range(Q)]
    key_lists[3][1] = 424242                                           # an unknown key
    key_lists[4] = key_lists[4][:1]                                    # fewer probes than columns
    qk, nk = oracle.keys_from_lists(key_lists)

    od, oi, onc = oracle.query_batch(corpus, perm, uniq, offs, queries, qk, nk, K, metric)
    sd, si, snc = oracle.query_batch(corpus, perm, uniq, offs, queries, qk, nk, K, metric, simd=True)
    assert np.array_equal(od.view(np.uint32), sd.view(np.uint32)) and np.array_equal(oi, si) and np.array_equal(onc, snc)

    i2r = {int(u): perm[offs[j]:offs[j + 1]] for j, u in enumerate(uniq)}
    worst = 0.0
    for q in range(Q):
        rows = np.concatenate([i2r.get(kk, np.zeros(0, np.int32)) for kk in key_lists[q]])
        assert int(onc[q]) == len(rows) and len(rows) >= K
        d64 = fp64_distances(queries[q], corpus[rows], metric)
        got = {int(r): float(v) for r, v in zip(rows, d64)}
        worst = max(worst, max(abs(float(od[q][j]) - got[int(oi[q][j])]) / max(1.0, abs(got[int(oi[q][j])])) for j in range(K)))
        check_topk_against_candidates(oi[q], od[q], rows, d64, K, rtol=DIST_RTOL)
        want = rows[np.lexsort((rows, d64))[:K]]                       # the fp64 (distance, id) order
        assert_lists_differ_only_at_ties(oi[q], want, queries[q], corpus, metric, rtol=2 * DIST_RTOL)
    print(f"{metric} d={d}: worst |oracle - fp64| / max(1, |d|) = {worst:.3g}")
