/*
 * nlsh_hip.h -- C ABI of the MI355X (gfx950) implementation of nlsh's query-time hot path.
 *
 * The reference exposes this path as duck-typed Python; the only native
 * boundary it has is the Cython module nlsh/utils.pyx.  The entry points below are what a
 * Python/ctypes (or cgo/JNI) binding of that path would bind; each cites the reference
 * interface it replaces.  INTEGRATION.md shows the reference-side ctypes stub.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer marked [dev] is a DEVICE pointer
 *     (hipMalloc / torch tensor.data_ptr()), [host] is host memory;
 *   - the caller allocates every buffer (workspace sizes come from the *_workspace queries; a workspace starts on a 16-byte
 *     boundary -- any hipMalloc'ed or torch tensor does -- and is refused otherwise);
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream); no call synchronises the device or allocates device memory;
 *   - return 0 on success, a negative NLSH_E_* code on failure; never throws; the message of
 *     the last failure on the calling thread is available from nlsh_last_error();
 *   - integer outputs are bit-exact w.r.t. the oracle; fp32 outputs within the tolerance
 *     stated in DESIGN.md.
 */
#ifndef NLSH_HIP_H
#define NLSH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLSH_ABI_VERSION 4   /* 4 (r06): nlsh_query_batch; the workspace counters are handed back by the PLAN phase; 3 (r05): pipelined batch slots (nlsh_step_*, nlsh_query_step_enqueue); 2 (r04): cells */

typedef void *nlsh_stream_t; /* hipStream_t */

enum {
    NLSH_OK = 0,
    NLSH_E_INVALID = -1,     /* bad argument (null pointer, negative size, k or P out of range) */
    NLSH_E_UNSUPPORTED = -2, /* shape outside what the kernels are built for (see each call) */
    NLSH_E_HIP = -3,         /* a HIP runtime call failed (message has hipGetErrorString) */
    NLSH_E_WORKSPACE = -4    /* workspace too small */
};

enum { NLSH_ACT_SIGMOID = 0, NLSH_ACT_TANH = 1 };      /* nlsh/hashings.py:22-26 (tanh_output) */
enum { NLSH_KEY_REF_INT16 = 0, NLSH_KEY_FULL = 1 };    /* nlsh/utils.pyx:7-15 (int16 wrap) | eval.py:49-53 */
/* nlsh/data.py:191-201 (F.pairwise_distance: sqrt(sum(((q - c) + 1e-6)^2)), the operation order the oracle restates bit for bit) |
 * nlsh/data.py:99-109 | OPT-IN: the same L2 distance evaluated as sqrt(sum(((q + 1e-6) - c)^2)) -- one rounding per element
 * differs from the reference's order (relative 1e-7; |d - d_exact| <= 1e-4 * max(1, d), the tolerance BASELINE.json states), in
 * exchange for 2 instead of 3 vector operations per element in the LDS-tiled schedule; schedules 0 and 1 answer it with the
 * exact form.  Never the default: NLSH_METRIC_L2_EPS is bit-identical to the oracle. */
enum { NLSH_METRIC_L2_EPS = 0, NLSH_METRIC_COSINE = 1, NLSH_METRIC_L2_EPS_FOLDED = 2 };
/* schedules of nlsh_scan_topk: one wave per (query, segment) | one wave per (bucket segment, <= 8 queries) |
 * one workgroup per (bucket segment, <= 16 queries) with the row tile staged through LDS.  0 and 1 give
 * bit-identical results; 2 sums each distance in k order (bit-identical to the oracle), ids agree except fp32 near-ties. */
enum { NLSH_SCAN_QUERY_MAJOR = 0, NLSH_SCAN_BUCKET_MAJOR = 1, NLSH_SCAN_BUCKET_TILED = 2 };
/* Element type of a bucket-sorted corpus copy (the *_typed entry points; every other call takes float32).  No reference counterpart.
 * float16 -> float32 and uint8 -> float32 are exact, so a typed index IS the float32 index over its dequantised rows: every output
 * word of the typed calls equals what the float32 calls give on those rows.  A row's pitch is a multiple of 16 bytes in every storage
 * (4 / 8 / 16 elements), the base 16-byte aligned, columns >= d stored as zero. */
#define NLSH_STORE_F32 0
#define NLSH_STORE_F16 1
#define NLSH_STORE_U8 2

#define NLSH_MAX_LAYERS 8   /* Linear layers incl. the output layer */
#define NLSH_MAX_HASH_BITS 32
#define NLSH_MAX_PROBES 64  /* keys per query one nlsh_scan_topk call takes */
#define NLSH_MAX_ENCODE_PROBES 128  /* hash_times nlsh_encode_hash generates (eval.py:148 sweeps 1..100); scan in slices of 64 */
#define NLSH_MAX_K 64       /* k every scan schedule takes */
#define NLSH_MAX_K_TILED 256  /* k of the tiled schedule (NLSH_SCAN_BUCKET_TILED) and of nlsh_merge_topk: a tiled task scores at most 256 rows
                               * per (task, query) list, so a list is still selected from what one wave holds.  The tiled workspace keeps
                               * 16 lists of k keys per task, max_tasks * 16 * k * 8 bytes: 32 KB per task at k = 256 (17,277 tasks: 566 MB) */
#define NLSH_MAX_DIM 1024   /* vector dimension of corpus / queries for the scan */
#define NLSH_MAX_WIDTH 632  /* widest HIDDEN encoder layer the LDS-resident MLP supports (the input may be NLSH_MAX_DIM wide) */
#define NLSH_MAX_STREAM_WIDTH 4096  /* widest HIDDEN encoder layer of the streamed form (nlsh_encode_hash_stream) */
#define NLSH_MAX_BINS 4096  /* bins of a Categorical hash (nlsh_encode_logits, nlsh_probe_bins): = NLSH_MAX_STREAM_WIDTH, a width the layer GEMM takes */

int nlsh_abi_version(void);
const char *nlsh_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Hash function forward + bit packing + multi-probe key generation.
 * Replaces: encoder forward (encoders.py:18-21, 39-55) -> output Linear + sigmoid/tanh
 * (nlsh/hashings.py:13-27) -> hard bits / Bernoulli samples (hashings.py:66-81) -> D2H ->
 * binarr_to_int + set() (nlsh/utils.pyx:6-32), i.e. everything `MultivariateBernoulli.hash`
 * does, without leaving the device.
 * ------------------------------------------------------------------------------------------- */

/* Number of floats of the packed (MFMA-fragment-ordered) weight blob for a layer stack: every layer in the fragment order of the
 * 32-row-tile forms, then the hidden layers once more in 16x16x4 order (the 16-row form batches of <= 4096 rows take).
 * dims [host] = {d_in, h_1, ..., H}, n_layers = number of Linear layers (len(dims) - 1). */
int64_t nlsh_encoder_packed_floats(int n_layers, const int *dims);

/* Pack nn.Linear-layout weights (W[l] is [dims[l+1], dims[l]] row-major, b[l] is [dims[l+1]] or
 * NULL) into `packed` [dev].  W, b: [host] arrays of n_layers [dev] pointers.
 * BatchNorm1d in eval mode is an affine map: fold it into W/b before packing. */
int nlsh_encoder_pack(int n_layers, const int *dims, const float *const *W, const float *const *b,
                      float *packed, nlsh_stream_t stream);

/* x [dev] fp32 [n, d] with row stride x_stride (floats).  Outputs (all [dev], nullable unless noted):
 *   z_out     [n, H] pre-activation of the output layer
 *   probs_out [n, H] module output: sigmoid(z) or tanh(z)             (hashings.py:39-40 predict)
 *   code_out  [n]    hard code, bit h of the hasher = bit (H-1-h): MSB-first (utils.pyx:12-14)
 *   keys_out  [n, n_probes] (required) distinct keys in first-occurrence order, slot 0 = hard key;
 *             key_mode REF_INT16: sign-extended low 16 bits; FULL: the H-bit code as int32 bits
 *   nkeys_out [n]    (required) number of valid slots in keys_out (>= 1)
 * Probes 1..n_probes-1 are Bernoulli(p) draws from a Philox4x32-10 stream keyed by `seed`,
 * counter (row0 + row, probe, word): reproducible across devices and ranks.  Rows with index
 * >= n_multi_rows are single-probe (Indexer.hash's trailing-batch rule, nlsh/indexer.py:51-53).
 * Limits: H <= 32, n_probes <= NLSH_MAX_ENCODE_PROBES, dims[0] <= NLSH_MAX_DIM, hidden dims[l] <= NLSH_MAX_WIDTH
 * (wider hidden layers: nlsh_encode_hash_stream below). */
int nlsh_encode_hash(const float *x, int64_t n, int64_t x_stride, int n_layers, const int *dims,
                     const float *packed, int act, int key_mode, int n_probes, int64_t n_multi_rows,
                     uint64_t seed, int64_t row0, float *z_out, float *probs_out, uint32_t *code_out,
                     int32_t *keys_out, int32_t *nkeys_out, nlsh_stream_t stream);

/* The kernel forms of nlsh_encode_hash (same arithmetic, different geometry): rows per workgroup 16 | 32 | 32 with three column tiles
 * per wave | 128 | 64 on two LDS images | 32, then 16 for the rows behind the last full round of workgroups. */
enum {
    NLSH_ENC_FORM_H16 = 0, NLSH_ENC_FORM_SINGLE = 1, NLSH_ENC_FORM_SINGLE_WIDE = 2, NLSH_ENC_FORM_BUILD128 = 3, NLSH_ENC_FORM_PINGPONG = 4,
    NLSH_ENC_FORM_HET = 5
};

/* Read-only: the form an nlsh_encode_hash call of n rows, this layer stack and n_probes would take, from the planning code the launch
 * itself runs; nothing is launched and no device is needed.  Outputs ([host], each nullable): the form id, the rows of a workgroup
 * (NLSH_ENC_FORM_HET: 32, its larger workgroups), the dynamic LDS bytes of a workgroup (rows x row stride x 4, twice that for
 * NLSH_ENC_FORM_PINGPONG) and the compute-unit count the NLSH_ENC_FORM_HET rule used (the current device's; 256 when none is visible).
 * Refuses what nlsh_encode_hash refuses for the shape: the limits above (NLSH_E_INVALID / NLSH_E_UNSUPPORTED) and a row image
 * larger than the LDS of a compute unit (NLSH_E_UNSUPPORTED). */
int nlsh_encode_form(int64_t n, int n_layers, const int *dims, int n_probes, int *form_out, int *rows_per_workgroup_out,
                     size_t *lds_bytes_out, int *cus_out);

/* The streamed form: the same function for encoders with hidden layers up to NLSH_MAX_STREAM_WIDTH wide (narrow ones too).
 * The LDS-resident form above keeps a row's whole activation on chip, which bounds a hidden layer at NLSH_MAX_WIDTH; here the
 * activations of a block of rows live in `workspace` between layers: one fp32-MFMA GEMM launch per Linear layer (one k-ascending
 * chain per output element from 0, bias, then ReLU: z is the same bits as nlsh_encode_hash's and the oracle's), then the epilogue
 * of nlsh_encode_hash (sigmoid / tanh, bits, packing, Philox probes, de-duplication) on z.  Pipelined batch slots
 * (nlsh_step_*, nlsh_query_batch) take LDS-resident encoders only.
 * Limits: H <= 32, n_probes <= NLSH_MAX_ENCODE_PROBES, dims[0] <= NLSH_MAX_DIM, hidden dims[l] <= NLSH_MAX_STREAM_WIDTH. */

/* Floats of the streamed form's blob (its own layout; -1 if the shape is outside the limits above). */
int64_t nlsh_encoder_stream_packed_floats(int n_layers, const int *dims);

/* nlsh_encoder_pack for the streamed form: same arguments, `packed` sized by nlsh_encoder_stream_packed_floats. */
int nlsh_encoder_stream_pack(int n_layers, const int *dims, const float *const *W, const float *const *b,
                             float *packed, nlsh_stream_t stream);

/* Workspace bytes of a pass of `rows_per_pass` rows (rounded up to the 128-row tile; 0 for a shape outside the limits). */
size_t nlsh_encode_stream_workspace(int64_t rows_per_pass, int n_layers, const int *dims);

/* nlsh_encode_hash's arguments and outputs, with the streamed blob, plus workspace [dev] (16-byte aligned) of workspace_bytes:
 * the rows are processed in passes of as many 128-row tiles as the workspace holds (at least one: NLSH_E_WORKSPACE otherwise);
 * the outputs do not depend on that size. */
int nlsh_encode_hash_stream(const float *x, int64_t n, int64_t x_stride, int n_layers, const int *dims,
                            const float *packed, int act, int key_mode, int n_probes, int64_t n_multi_rows,
                            uint64_t seed, int64_t row0, float *z_out, float *probs_out, uint32_t *code_out,
                            int32_t *keys_out, int32_t *nkeys_out, void *workspace, size_t workspace_bytes,
                            nlsh_stream_t stream);

/* Standalone bit packing: codes [dev] int32 [B, n, H] (0/1, C-contiguous) -> keys_out [dev] int32
 * [B, n].  Replaces binarr_to_int + the inner loop of hash_codes (nlsh/utils.pyx:6-15, 22-31);
 * the set() of each row is formed by the host binding.  key_mode as above (FULL: eval.py:49-53). */
int nlsh_pack_codes(const int32_t *codes, int64_t B, int n, int H, int key_mode, int32_t *keys_out,
                    nlsh_stream_t stream);

/* Likelihood-ranked multi-probe keys: the n_probes most probable codes of every row in descending probability, instead of
 * nlsh_encode_hash's Bernoulli draws (no seed, n_probes DISTINCT codes, probe sets nested in n_probes).  No reference counterpart
 * (hashings.py:70-81 samples); SURVEY.md 8(f) N3 "flip the least-confident bits", the shift / expand best-first enumeration of
 * multi-probe LSH (Lv et al., VLDB 2007).  For independent bits the log-odds of hasher bit h is z[h] (sigmoid head; 2 z[h] for the
 * tanh head, the same order), so a code that differs from the hard code in the bits of a set costs the sum of their |z[h]|.
 *   z    [dev] fp32 [n, H] with row stride z_stride >= H: the output pre-activations (z_out of nlsh_encode_hash / _stream)
 *   code [dev] [n] the hard codes (code_out); hasher bit h is code bit H-1-h
 *   keys_out [n, n_probes], nkeys_out [n] (required) as for nlsh_encode_hash: slot 0 = hard key, unused slots 0
 *   cost_out [n, n_probes] fp32 (nullable): the cost of each kept slot, +inf past nkeys
 * A row's result is a pure function of its z, its code, H, key_mode, n_probes and whether its index is < n_multi_rows:
 *   1. c[h] = z[h] with the sign bit cleared.  The bit indices are sorted by (bit pattern of c[h] as uint32, h) ascending;
 *      s[i] is the bit index at sorted position i.
 *   2. A subset M of sorted positions is a uint32 mask (bit i = position i).  Its cost is the fp32 chain from t = +0.0f:
 *      for i ascending in M, t = t + c[s[i]] (plain fp32 adds, never contracted).
 *   3. Subsets are ordered by (cost bit pattern, mask as uint32) ascending; the empty set (cost 0: the hard code) is first.  The
 *      first min(n_probes, 2^H) subsets are taken; rows >= n_multi_rows take the empty set only (Indexer.hash's trailing-batch rule).
 *   4. The code of M is code XOR the OR of 1 << (H-1-s[i]) over i in M; its key follows key_mode as in nlsh_encode_hash; keys are
 *      de-duplicated in first-occurrence order (only NLSH_KEY_REF_INT16 with H > 16 can collide); nkeys = number kept.
 * The order is reachable best-first: every non-empty subset has one parent (top position j: remove j if j-1 is in the set -- the
 * child was an EXPAND --, else move j to j-1 -- a SHIFT); a child changes or appends only the LAST term of the chain, rounding is
 * monotone and its mask is larger, so (cost, mask) strictly increases along every edge and popping the frontier's minimum, starting
 * from {0}, yields the global order.  With the chain-without-its-last-term kept beside each entry both children's costs ARE their
 * chains, bit for bit.  After m pops the frontier holds at most m + 1 entries.
 * The kernel makes a fixed n_probes - 1 pops per row and stays inside its buffers whatever the bits of z are: +-inf is legal (handled
 * by the definition), a NaN is a precondition violation with an unspecified order.
 * Checked on the host before anything touches the device: NULL required pointers, n < 0, z_stride < H, a bad key_mode
 * (NLSH_E_INVALID); H outside [1, NLSH_MAX_HASH_BITS], n_probes outside [1, NLSH_MAX_ENCODE_PROBES] (NLSH_E_UNSUPPORTED).
 * n = 0 is NLSH_OK without a launch. */
int nlsh_probe_ranked(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H,
                      int key_mode, int n_probes, int64_t n_multi_rows,
                      int32_t *keys_out, int32_t *nkeys_out, float *cost_out /* nullable */,
                      nlsh_stream_t stream);

/* nlsh_probe_ranked with a per-row CANDIDATE BUDGET: a row walks its ranked keys, looks each one's bucket size up in the index and
 * stops after the first key that brings its candidate count to `budget` (n_probes is the cap).  The query-adaptive form of
 * multi-probe LSH: the work knob is candidates, not probes, whatever the skew of the bucket sizes.
 *   uniq_keys [dev] int32 [n_buckets] ascending as signed int32, offsets [dev] int32 [n_buckets + 1]: the CSR arrays of nlsh_build_csr
 *   budget >= 1;  ncand_out [dev] int32 [n] (nullable): the candidates of the kept keys;  everything else as for nlsh_probe_ranked
 * For one row let K[0..nk) be the keys nlsh_probe_ranked writes for the same z, code, H, key_mode, n_probes, n_multi_rows (already
 * de-duplicated in first-occurrence order).  size(key) = offsets[b+1] - offsets[b] if uniq_keys[b] == key for some b, else 0;
 * cum(m) = sum of size(K[i]) over i < m (distinct keys are disjoint buckets: cum <= N < 2^31).  Then
 *   nkeys_out = min{ m in [1, nk] : cum(m) >= budget }, or nk if there is none  (slot 0, the hard key, is always kept; rows >=
 *   n_multi_rows keep it alone);  keys_out = K[0..nkeys_out) then zeros;  cost_out = the kept costs then +inf;  ncand_out = cum(nkeys_out).
 * The result is a prefix of the unbudgeted row; with budget = INT32_MAX it is nlsh_probe_ranked's output in every word.
 * The pop loop itself ends at the stop (nothing is enumerated and then cut); a popped code whose key was kept before takes no slot and
 * adds no candidates, decided at pop time.  A lookup is a 64-way search across the lanes: ceil(log64(n_buckets)) dependent global round
 * trips, one fewer above 64 buckets (the first round's probes are loaded once per row).
 * Checked on the host before anything touches the device: budget < 1, n_buckets < 0, NULL uniq_keys or offsets with n_buckets > 0
 * (NLSH_E_INVALID), then every refusal of nlsh_probe_ranked.  n_buckets == 0 is legal (every size is 0, no row stops early); n = 0 is
 * NLSH_OK without a launch. */
int nlsh_probe_ranked_budget(const float *z, int64_t z_stride, const uint32_t *code, int64_t n, int H, int key_mode,
                             int n_probes, int64_t n_multi_rows,
                             const int32_t *uniq_keys, const int32_t *offsets, int32_t n_buckets, int32_t budget,
                             int32_t *keys_out, int32_t *nkeys_out, float *cost_out /* nullable */, int32_t *ncand_out /* nullable */,
                             nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Categorical (softmax-bin) hashing.  Replaces the forward and `hash` of the reference's `Categorical` (nlsh/hashings.py:95-139):
 * encoder -> Linear(hash_size = M bins) -> softmax, bucket = argmax bin; multi-probe = the next most probable bins.  Softmax is
 * monotone in the logits, so the device works on logits alone: a forward that leaves [n, M] logits, and a kernel that ranks a row's bins.
 * ------------------------------------------------------------------------------------------- */

/* The logits forward: nlsh_encode_hash_stream's layer stack (its blob layout, one fp32-MFMA GEMM launch per Linear layer, ReLU behind
 * every layer but the last) with an output layer of dims[n_layers] = M bins, 1 <= M <= NLSH_MAX_BINS, and no epilogue.  A logit is one
 * k-ascending chain from 0 over the last hidden activation, then the bias: the oracle's mlp_forward arithmetic, bit for bit.
 * Limits: n_layers in [1, NLSH_MAX_LAYERS] (a single Linear layer is legal), dims[0] <= NLSH_MAX_DIM, hidden dims[l] <=
 * NLSH_MAX_STREAM_WIDTH.  The hashing calls above keep refusing an output layer wider than NLSH_MAX_HASH_BITS. */

/* Floats of the blob (-1 for a shape outside the limits) and the pack call: nlsh_encoder_stream_pack's arguments and layout. */
int64_t nlsh_logits_packed_floats(int n_layers, const int *dims);
int nlsh_logits_pack(int n_layers, const int *dims, const float *const *W, const float *const *b,
                     float *packed, nlsh_stream_t stream);

/* Workspace bytes of a pass of `rows_per_pass` rows (rounded up to the 128-row tile): the hidden activation images, plus a padded
 * logits image when M is no multiple of 32.  At least 16 (a single layer of a 32-multiple width needs none); 0 for a shape outside
 * the limits. */
size_t nlsh_logits_workspace(int64_t rows_per_pass, int n_layers, const int *dims);

/* x [dev] fp32 [n, d], row stride x_stride >= d (any alignment);  logits_out [dev] fp32 [n, M], row stride logits_stride >= M:
 * columns >= M of the caller's rows are never written.  workspace [dev], 16-byte aligned: the rows are processed in passes of as many
 * 128-row tiles as it holds (at least one: NLSH_E_WORKSPACE otherwise); the outputs do not depend on its size.
 * Checked before anything touches the device: the limits (NLSH_E_INVALID / NLSH_E_UNSUPPORTED), n < 0, a stride below its width,
 * NULL pointers with n > 0 (NLSH_E_INVALID).  n = 0 is NLSH_OK without a launch. */
int nlsh_encode_logits(const float *x, int64_t n, int64_t x_stride, int n_layers, const int *dims, const float *packed,
                       float *logits_out, int64_t logits_stride, void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

/* The n_probes best bins of every row, best first: a Categorical hash's keys (slot 0 = the bucket, the reference's probs.argmax(1);
 * the rest = its multi-probe).  No reference counterpart for n_probes > 1 (its hash() is single-probe).
 *   logits [dev] fp32 [n, M] with row stride logits_stride >= M (any alignment; 16-byte-aligned rows are loaded 16 bytes per lane)
 *   keys_out [n, n_probes], nkeys_out [n] (required);  logit_out [n, n_probes] fp32 (nullable)
 * A row's result is a pure function of its M logits, n_probes and whether its index is < n_multi_rows:
 *   1. u(z) is the IEEE total-order map of z's bit pattern to uint32: a negative pattern (sign bit set) is complemented, a
 *      non-negative one gets its sign bit set.  So -0 < +0, -inf is lowest and +inf highest.
 *   2. Bins are ordered by (u(z[b]) descending, b ascending).
 *   3. The first min(n_probes, M) bins are the row's keys, in that order; key = bin index as int32.
 *   4. Rows >= n_multi_rows keep slot 0 alone (Indexer.hash's trailing-batch rule).
 *   5. Unused slots are 0; nkeys = the number kept.
 *   6. logit_out holds the kept bins' logits bit for bit, -inf past nkeys.
 *   7. A NaN is a precondition violation: the order is then unspecified, but the kernel stays inside its buffers (it makes at most
 *      min(n_probes, M) rounds and indexes its LDS image by bin index alone).
 * Checked on the host before anything touches the device: NULL required pointers, n < 0, logits_stride < M (NLSH_E_INVALID); M outside
 * [1, NLSH_MAX_BINS], n_probes outside [1, NLSH_MAX_ENCODE_PROBES] (NLSH_E_UNSUPPORTED).  n = 0 is NLSH_OK without a launch. */
int nlsh_probe_bins(const float *logits, int64_t logits_stride, int64_t n, int M, int n_probes, int64_t n_multi_rows,
                    int32_t *keys_out, int32_t *nkeys_out, float *logit_out /* nullable */, nlsh_stream_t stream);

/* nlsh_probe_bins with nlsh_probe_ranked_budget's per-row CANDIDATE BUDGET, applied to this key order (uniq_keys, offsets, n_buckets,
 * budget, ncand_out as there).  For one row let K[0..nk) be the keys nlsh_probe_bins writes; size(key) = offsets[b+1] - offsets[b] if
 * uniq_keys[b] == key for some b, else 0; cum(m) = sum of size(K[i]) over i < m.  Then
 *   nkeys_out = min{ m in [1, nk] : cum(m) >= budget }, or nk if there is none  (slot 0 is always kept; rows >= n_multi_rows keep it
 *   alone);  keys_out = K[0..nkeys_out) then zeros;  logit_out = the kept logits then -inf;  ncand_out = cum(nkeys_out).
 * The result is a prefix of the unbudgeted row; with budget = INT32_MAX it is nlsh_probe_bins' output in every word.  The selection
 * loop itself ends at the stop (nothing is enumerated and then cut).
 * Checked on the host first: budget < 1, n_buckets < 0, NULL uniq_keys or offsets with n_buckets > 0 (NLSH_E_INVALID), then every
 * refusal of nlsh_probe_bins.  n_buckets == 0 is legal (every size is 0, no row stops early); n = 0 is NLSH_OK without a launch. */
int nlsh_probe_bins_budget(const float *logits, int64_t logits_stride, int64_t n, int M, int n_probes, int64_t n_multi_rows,
                           const int32_t *uniq_keys, const int32_t *offsets, int32_t n_buckets, int32_t budget,
                           int32_t *keys_out, int32_t *nkeys_out, float *logit_out /* nullable */, int32_t *ncand_out /* nullable */,
                           nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Index build.  Replaces build_index (nlsh/indexer.py:6-24): key -> ascending row list, as CSR.
 * ------------------------------------------------------------------------------------------- */
size_t nlsh_build_csr_workspace(int64_t n);

/* keys [dev] int32 [n] (one key per row).  Outputs [dev]: perm [n] row ids grouped by bucket
 * (buckets in ascending signed key order, rows ascending inside a bucket), uniq_keys [n] (first
 * *n_buckets valid), offsets [n + 1] (first *n_buckets + 1 valid), n_buckets [1]. */
int nlsh_build_csr(const int32_t *keys, int64_t n, int32_t *perm, int32_t *uniq_keys, int32_t *offsets,
                   int32_t *n_buckets, void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

/* Schedule order of the buckets for the bucket-major scans: order_out [dev] int32 [n_buckets] = bucket
 * indices by DESCENDING size (ties: ascending index), from offsets [dev] [n_buckets + 1].  Static per index:
 * nlsh_scan_topk numbers its (bucket segment, query group) tasks in this order, so the heavy tasks of the big
 * buckets are dispatched first and the launch does not end on a tail of late-started long tasks.  No reference
 * counterpart (the reference walks `for key in index_keys`, nlsh/indexer.py:66); changes speed, never results. */
size_t nlsh_bucket_order_workspace(int64_t n_buckets);
int nlsh_bucket_order(const int32_t *offsets, int64_t n_buckets, int32_t *order_out, void *workspace,
                      size_t workspace_bytes, nlsh_stream_t stream);

/* Cells: small-bucket packing for the LDS-tiled scan (NLSH_SCAN_BUCKET_TILED).  A task of that schedule is one workgroup on
 * (<= 256 consecutive rows of corpus_sorted) x (<= 16 queries) and costs ~9 us before its first distance; with one task per
 * (bucket, query group) a balanced hash with tiny buckets (GloVe-1.2M-shaped: 104 k buckets, ~1 probing query per touched bucket and
 * batch) pays that latency once per (query, bucket) pair.  The sorted corpus is bucket-contiguous, so consecutive small buckets are
 * consecutive rows: a CELL is either one bucket of more than window_rows rows, or a greedy run (CSR order, restarted every 1024
 * buckets so that the packing is a pure function of (offsets, window_rows)) of consecutive buckets of <= window_rows rows whose rows
 * total <= window_rows.  The scan then counts (query, probe) pairs and lays out tasks per CELL: the queries probing any bucket of a
 * window share its tasks, and each (task, query) carries the row range of ITS bucket inside the window, applied when the top-k is
 * selected -- every distance is still the same k-ascending fmaf chain over the same row, so results are bit-identical with and without
 * cells, for every window_rows.  What changes is the number of tasks (fewer, fuller) against rows scored for queries that do not own
 * them (window_rows 64 adds none: a lone tiny bucket already costs a 64-row tile).
 * Outputs [dev]: cell_of [n_buckets] bucket -> cell; cell_offsets [n_buckets + 1] first sorted row of each cell (entries from
 * *n_cells on hold N); cell_order [n_buckets] cells by descending rows (first *n_cells entries valid) = the bucket_order argument
 * of the scan when cells are passed; n_cells [1].  window_rows in [1, 256].  No reference counterpart (the reference walks
 * `for key in index_keys`, nlsh/indexer.py:66, one gather per key); changes speed, never results. */
size_t nlsh_build_cells_workspace(int64_t n_buckets);
int nlsh_build_cells(const int32_t *offsets, int64_t n_buckets, int window_rows, int32_t *cell_of, int32_t *cell_offsets,
                     int32_t *cell_order, int32_t *n_cells, void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

/* Re-order the corpus bucket-contiguously: sorted[i, :] = corpus[perm[i], :], zero padded to
 * dst_stride floats (dst_stride % 4 == 0, >= d).  Replaces the per-(query,key) index_select
 * gather of nlsh/indexer.py:77-82 by a one-time permutation.  inv_norm (nullable) [n] receives
 * 1 / max(||row||, 1e-8) (cosine).  gid (nullable) [n] receives perm[i] + id_base: the global
 * row id the scan reports (corpus shards pass their row offset as id_base). */
int nlsh_gather_rows(const float *corpus, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                     float *sorted, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                     nlsh_stream_t stream);

/* nlsh_gather_rows between storages: corpus [dev] holds src_storage elements (row stride src_stride elements, any alignment), sorted
 * [dev, 16-byte aligned] receives dst_storage elements, dst_stride (elements) >= d with dst_stride * element size a multiple of 16.
 * float32 -> float16 rounds to nearest even; a value goes to uint8 only if it is integral and in [0, 255].  A source value that does
 * not survive the conversion -- a finite value that float16 turns into an infinity, anything else than an integer in [0, 255] for
 * uint8 -- is reported, not clamped: first_bad [dev] int32 [1] (nullable when src_storage == dst_storage) receives the smallest SOURCE
 * row (perm value) holding one, -1 for none; what `sorted` holds then is unspecified.  inv_norm is computed from the dequantised values
 * in nlsh_gather_rows' operation order: the bits nlsh_gather_rows gives on the dequantised rows.  Everything is checked on the host
 * before anything is launched (NLSH_E_INVALID with the argument's name). */
int nlsh_gather_rows_typed(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                           void *sorted, int dst_storage, int64_t dst_stride, float *inv_norm, int32_t *gid, int32_t id_base,
                           int32_t *first_bad, nlsh_stream_t stream);

/* Index update: add rows to and remove rows from a built index without rebuilding it.  No reference counterpart (the reference's index
 * is a dict built once, nlsh/indexer.py:6-24).  The result is, word for word, the index nlsh_build_csr + nlsh_gather_rows build from
 * the kept rows in their order followed by the new rows in theirs: out of place, into caller-allocated arrays of n_kept + m_new rows.
 *   old index [dev]: corpus_sorted [n_old, row_stride] (16-byte aligned, row_stride % 4 == 0), gid [n_old], inv_norm [n_old] (nullable:
 *     needed when inv_norm_out is given), uniq_keys [n_buckets_old], offsets [n_buckets_old + 1] -- all in sorted order, as built;
 *   keep [dev] uint8 [n_old] (nullable = every row kept), non-zero = the row at that SORTED position stays; n_kept = how many are set
 *     (a wrong count never writes or reads out of bounds, it gives a wrong index);
 *   new rows [dev]: rows_new fp32 [m_new, d] with row stride new_stride >= d (any alignment), keys_new int32 [m_new] their bucket keys,
 *     ids_new int32 [m_new] their global row ids, all in the caller's order;
 *   outputs [dev]: sorted_out [n_kept + m_new, stride_out] (16-byte aligned, stride_out % 4 == 0, >= d; columns >= d written as zero),
 *     gid_out, inv_norm_out (nullable: kept rows' values copied, new rows' computed as nlsh_gather_rows computes them, the same bits),
 *     src_out int32 [n_kept + m_new]: where each row came from -- the old sorted position, or ~j for new row j --, uniq_out
 *     [n_kept + m_new] (first *n_buckets_out valid), offsets_out [n_kept + m_new + 1] (first *n_buckets_out + 1 valid), n_buckets_out [1].
 * Placement (signed key order, as in the build): kept old rows keep their order and stand in front of the new rows of their own key;
 * new rows of one key keep the caller's order.  n_kept + m_new <= 2^31 - 1.
 * Every argument is checked on the host before anything is launched and before any pointer is read: a refusal -- a short workspace
 * included -- is NLSH_E_INVALID with the argument's name in nlsh_last_error().  nlsh_csr_update_workspace is arithmetic on its
 * arguments (0 = invalid: a negative count, a count >= 2^31, n_buckets_old > n_old), no device needed; it bounds what rocPRIM's sort
 * of the m_new keys and its scans ask for, and nlsh_csr_update returns NLSH_E_WORKSPACE before launching anything if a device's
 * rocPRIM ever asked for more. */
size_t nlsh_csr_update_workspace(int64_t n_old, int64_t n_buckets_old, int64_t m_new);
int nlsh_csr_update(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                    const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                    const uint8_t *keep, int64_t n_kept,
                    const float *rows_new, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new, int64_t m_new,
                    float *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                    int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out,
                    void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

/* nlsh_csr_update on an index whose sorted corpus holds `storage` elements (corpus_sorted and sorted_out; row_stride and stride_out in
 * elements, each pitch a multiple of 16 bytes), with new rows of new_storage elements (new_stride elements, any alignment).  Kept
 * rows are moved as bytes; new rows are converted on the way in by nlsh_gather_rows_typed's rule and reported the same way: first_bad
 * [dev] int32 [1] (nullable when new_storage == storage) receives the smallest new row j that does not survive the conversion, -1 for
 * none -- the outputs are then not an index and the caller drops them (the old index is untouched: the update is out of place).  New
 * rows' inv_norm as nlsh_gather_rows_typed computes it.  NLSH_STORE_F32 / NLSH_STORE_F32 is nlsh_csr_update.  The workspace is
 * nlsh_csr_update_workspace's (it holds int32 side arrays only).  Host checks as nlsh_csr_update. */
int nlsh_csr_update_typed(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid, const float *inv_norm,
                          const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                          const uint8_t *keep, int64_t n_kept,
                          const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new,
                          int64_t m_new,
                          void *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                          int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad,
                          void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Candidate scan + top-k.  Replaces the per-query loop of Indexer.query (nlsh/indexer.py:62-95):
 * bucket lookup (:68), gather (:77-82), distance (:84-87, nlsh/data.py:99-109,191-201),
 * cat (:88), topk + id map (:90-91), n_candidates (:71,94).
 * ------------------------------------------------------------------------------------------- */
size_t nlsh_scan_workspace(int64_t Q, int P, int k, int64_t max_tasks, int64_t n_buckets, int d);

/* corpus_sorted [dev] fp32 [N, row_stride] bucket-contiguous (nlsh_gather_rows), gid [dev] [N],
 * uniq_keys [dev] [n_buckets] ascending, offsets [dev] [n_buckets+1], bucket_order (nullable) [dev]
 * [n_buckets] from nlsh_bucket_order (NULL = CSR order), inv_norm [dev] [N] (cosine only), queries [dev] [Q, d] stride q_stride, qkeys [dev] [Q, P] with nkeys [dev] [Q] valid slots
 * (a query's keys are a set, nlsh/utils.pyx:27-31: a key repeated within a row probes its bucket once; unknown keys are
 * empty buckets, never an error: indexer.py:61,68).
 * Outputs [dev]: out_dist [Q, k] ascending, +inf padded; out_idx [Q, k] global row ids, -1 padded;
 * out_keys (nullable) [Q, k] the 64-bit sort keys (monotone(dist) << 32 | id; ~0 padded) used by
 * nlsh_merge_topk; out_ncand [Q] candidates per query; status [2] = {tasks needed, flag}: flag 0 = complete,
 * 1 = task table overflow (repeat with max_tasks >= status[0]), 2 = workspace contract violated (below), 3 = the cells handed
 * to nlsh_scan_topk_cells_phase hold a shared window of more than 256 rows (not from nlsh_build_cells: results incomplete).
 * Order is (distance asc, row id asc): deterministic refinement of torch.topk's tie order.
 * A query's candidate list is cut into segments of `seg_rows` rows (0 = default), one wavefront
 * each; max_tasks bounds the number of segments the workspace holds: if status[1] != 0 the
 * results are incomplete and the call must be repeated with max_tasks >= status[0].
 * Workspace contract of the bucket-major schedules (algo 1, 2): the per-bucket pair counters live in the first
 * 4 * n_buckets bytes of the workspace (an offset that does not depend on Q, P or max_tasks).  Those bytes must be ZERO
 * before the first call that uses the buffer and must not be written by anything else afterwards (do not lend the buffer
 * to algo 0 calls in between); every PLAN phase leaves them zero again (the step that turns the counts into list offsets reads
 * and resets each counter), which is what saves a clearing launch per batch.  The contract is CHECKED on the device: the PLAN
 * phase holds the sum of the counters against the (query, probe) pairs it counted itself, rejects negative counters and rejects
 * any pair that drew a negative slot from its counter -- stale counts that cancel in the sum include a negative one, so every
 * way a stale count can enter a batch is covered --; on a violation the batch gets no task at all, every query's result is
 * empty and status[1] = 2 (the Python facade raises NLSH_E_WORKSPACE).  The counters are zero again after the refused call.
 * ev_scan_begin / ev_scan_end (nullable hipEvent_t): recorded on `stream` immediately before and
 * after the scan kernel, so a caller can time the HBM-bound kernel alone (bench.py roofline).
 * Limits: d <= NLSH_MAX_DIM, P <= NLSH_MAX_PROBES; k <= NLSH_MAX_K for algo NLSH_SCAN_QUERY_MAJOR and NLSH_SCAN_BUCKET_MAJOR,
 * k <= NLSH_MAX_K_TILED for NLSH_SCAN_BUCKET_TILED (NLSH_E_UNSUPPORTED otherwise; the phase, cells, step and batch entry points
 * below validate through the same rule).  The partial lists take max_tasks * 16 * k * 8 bytes of the tiled workspace. */
int nlsh_scan_topk(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid,
                   const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                   const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                   const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                   float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                   int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                   void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream);

/* Diagnostic, for tests of the bucket-major schedules (algo 1, 2): byte offsets, inside a workspace of this shape, of the
 * task table the PLAN phase leaves there -- int32 [status[0]][4] = {first pair of the query group, queries in the group,
 * first corpus row of the segment, rows in the segment} -- and (algo 2 only) of the tasks' per-slot records, ONE interleaved table
 * int32 [max_tasks][16][2] = {query id, row range lo | hi << 16}: *task_queries_offset is the table's offset (the id of (task, slot)
 * sits at + (task * 16 + slot) * 8), *task_ranges_offset = *task_queries_offset + 4 (the same stride of 8 bytes); the range is the
 * rows of the query's own bucket inside the task's rows: the whole segment without cells, the bucket's slice of a shared window
 * with them.  Any out pointer may be NULL.
 * No reference counterpart: the reference has no schedule (it walks `for key in index_keys`, nlsh/indexer.py:66). */
int nlsh_scan_workspace_layout(int64_t Q, int P, int k, int64_t max_tasks, int64_t n_buckets, int d, int algo,
                               size_t *task_table_offset, size_t *task_queries_offset, size_t *task_ranges_offset);

/* The same call cut in three, for callers that pipeline batches over streams: NLSH_PHASE_PLAN runs everything up
 * to the scan kernel (bucket lookup, task table; touches status and the workspace, the query-major schedule also out_ncand),
 * NLSH_PHASE_SCAN the scan kernel (reads what PLAN left in the workspace, leaves per-task partial top-k lists there),
 * NLSH_PHASE_MERGE the per-query merge of those lists (writes out_dist / out_idx / out_keys / out_ncand).  All take the identical
 * argument list and may be combined; each must be ordered after the previous one (an event when they run on
 * different streams), and a workspace belongs to one batch until its MERGE has finished.  All three bits =
 * nlsh_scan_topk.  The plan of batch i+1 and the merge of batch i-1 (latency-bound, small kernels) then overlap the
 * scan of batch i (nlsh_amd/pipeline.py). */
#define NLSH_PHASE_PLAN 1
#define NLSH_PHASE_SCAN 2
#define NLSH_PHASE_MERGE 4
int nlsh_scan_topk_phase(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid,
                         const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                         const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                         const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                         float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                         int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                         void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases);

/* nlsh_scan_topk_phase on an index with cells (nlsh_build_cells): cell_of [dev] [n_buckets], cell_offsets [dev] [n_cells + 1],
 * and `bucket_order` = the cell order [n_cells] (or NULL).  n_cells = 0 (pointers NULL) is nlsh_scan_topk_phase.  Cells only
 * change the task layout of algo NLSH_SCAN_BUCKET_TILED; the other schedules ignore them.  Same outputs, bit for bit. */
int nlsh_scan_topk_cells_phase(const float *corpus_sorted, int64_t row_stride, int d, const int32_t *gid,
                               const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                               const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                               const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                               const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                               float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                               int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                               void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases);

/* nlsh_scan_topk_cells_phase on a corpus copy of `storage` elements (NLSH_STORE_*): corpus_sorted [dev, 16-byte aligned] [N, row_stride]
 * with row_stride in ELEMENTS, >= d, its pitch in bytes a multiple of 16, columns >= d zero (nlsh_gather_rows_typed writes such a copy).
 * NLSH_STORE_F32 is nlsh_scan_topk_cells_phase, argument for argument.  NLSH_STORE_F16 and NLSH_STORE_U8 exist in the tiled schedule
 * only: algo NLSH_SCAN_BUCKET_TILED, every metric, k <= NLSH_MAX_K_TILED; the other two schedules answer NLSH_E_UNSUPPORTED with the
 * reason in nlsh_last_error().  The rows are widened to float32 as they are staged (exact conversions) and scored by the float32
 * code: every output equals, bit for bit, what nlsh_scan_topk_cells_phase gives on the dequantised corpus.  Queries are float32.
 * The step, batch and graph entry points below take float32 indexes only. */
int nlsh_scan_topk_cells_phase_typed(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid,
                                     const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                                     const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                     const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                     const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                     float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                     int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                     void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases);

/* ---------------------------------------------------------------------------------------------
 * Filtered queries: a per-call row allow/deny filter inside the tiled scan.  No reference counterpart.
 *
 * A row filter is a bitset over the SORTED rows: row_filter [dev, 4-byte aligned] uint32 [2 * ceil(N / 64)] words, bit p & 31 of word
 * p >> 5 set iff sorted row p -- the row at position p of corpus_sorted / gid -- may be returned; bits at positions >= N are zero;
 * N = 0 is valid (no words).  Position order, not id order: the scan reads word prow >> 5 with the row position it already has
 * (coalesced, no load that depends on gid), and ids may be any int32, negative and sparse, so a bitset indexed by id is not an option.
 * A filter belongs to one state of one index: nlsh_csr_update moves rows, and every filter built before it is meaningless afterwards.
 *
 * Definition: the filtered result of a call on an index I with filter F is the result of the same call on the index I_F built from the
 * allowed rows alone, with the same ids, the same bucket keys and the same query key table.  out_idx, out_dist (bits) and out_keys
 * equal I_F's in every word, padding (-1, +inf, ~0 behind a list shorter than k) included: a denied row is dropped in front of the
 * top-k selection, it can never push an allowed row out of a list, and no distance bit changes (a distance is one accumulation chain
 * along d whatever task the row is scored in).  Two things are counted BEFORE the filter, because the kernels that count do not know
 * it: out_ncand stays "rows of the probed buckets" -- the work the scan did -- and equals the unfiltered call's value, NOT I_F's; and
 * nlsh_probe_ranked_budget's candidate budget counts bucket rows, allowed or not.  A filter that allows every row gives the
 * unfiltered call's outputs in every word, out_ncand included; one that allows nothing gives all-padding lists.
 *
 * nlsh_row_filter_words: the number of uint32 words of a filter over n_rows rows, 2 * ceil(n_rows / 64) (host arithmetic only;
 * 0 and a message for n_rows < 0).
 *
 * nlsh_row_filter_build: one wavefront per 64 consecutive sorted rows decides, per lane, whether gid[p] is a member of the source --
 * EXACTLY ONE of ids [dev] int32 [n_ids], strictly ascending (binary search; n_ids = 0 with a non-null pointer is the empty list), and
 * dense [dev] uint8 [n_dense], indexed by id - id_base (non-zero = member; ids outside the array are not members) -- and writes the
 * wave's ballot as two words; allowed = member, or NOT member with invert = 1 (a deny list).  n_allowed [dev] int32 [1] receives the
 * number of allowed rows (zeroed by the call, then one atomic add per wave).  Every word of the filter is written; nothing else is
 * read or written.  NLSH_E_INVALID with the argument's name in nlsh_last_error(), before anything is launched, for: n_rows or the
 * source's size negative, both sources or neither, invert not 0 / 1, a null gid / row_filter with n_rows > 0, a null n_allowed,
 * a misaligned row_filter / n_allowed.
 *
 * nlsh_scan_topk_cells_phase_filtered: nlsh_scan_topk_cells_phase_typed with a row filter behind its last argument.  row_filter NULL is
 * the typed call, argument for argument.  A non-null filter is read by the tiled schedule only (algo NLSH_SCAN_BUCKET_TILED; every
 * storage, every metric, k <= NLSH_MAX_K_TILED): the other two schedules answer NLSH_E_UNSUPPORTED and name row_filter; a filter that
 * is not 4-byte aligned is NLSH_E_INVALID.  The call cannot check the filter's size: it must hold nlsh_row_filter_words of the
 * index's row count.  Only the SCAN phase reads the filter.  The step, graph-slot and one-call batch entry points take no filter. */
size_t nlsh_row_filter_words(int64_t n_rows);
int nlsh_row_filter_build(const int32_t *gid, int64_t n_rows, const int32_t *ids, int64_t n_ids, const uint8_t *dense, int64_t n_dense,
                          int32_t id_base, int invert, uint32_t *row_filter, int32_t *n_allowed, nlsh_stream_t stream);
int nlsh_scan_topk_cells_phase_filtered(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid,
                                        const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                                        const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                        const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                        const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                        float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                        int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                        void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases,
                                        const uint32_t *row_filter);

/* ---------------------------------------------------------------------------------------------
 * Radius (range) queries: every candidate within radius[q] of query q, from the tiled scan.  No reference counterpart.
 *
 * Definition: the candidates of query q are the rows of the buckets of its keys (unknown keys: empty buckets), subject to row_filter
 * when one is given (the rule of the filtered call: the index built from the allowed rows alone).  A candidate's distance is the one
 * nlsh_scan_topk_cells_phase computes for that (query, row), bit for bit: one accumulation chain along d, whatever task scores the row.
 * It is in range iff dist <= radius[q] as an IEEE float32 comparison -- a NaN distance never is, not even at radius +inf; a +inf
 * distance only at radius +inf; a negative radius on L2 returns nothing.  The result of a query is every in-range candidate, once,
 * ascending by the 64-bit sort key mono(dist) << 32 | id: the (distance, row id) order of every top-k call.  out_ncand[q] is the top-k
 * call's: the rows of the probed buckets, counted before the radius and before the filter.
 *
 * The length of the output is not known before the scan has run, and the caller allocates everything: two calls, one host read between.
 *
 *   nlsh_range_count   index, query and key-table arguments of nlsh_scan_topk_cells_phase_filtered (no k, no out_* lists), then
 *                      row_filter [dev] (NULL = off), radius [dev] float [Q], out_count [dev] int32 [Q] (zeroed by the call; on return
 *                      the in-range candidates of every query), out_ncand [dev] int32 [Q], status, workspace, max_tasks, the two optional events
 *                      of the top-k calls (recorded around the scan launch alone), stream.
 *                      Runs the PLAN phase, sized as for k = 1 (nlsh_range_workspace), and one scan launch in count mode.  status is the
 *                      top-k call's: status[0] tasks needed; status[1] 1 = task table too small, the counts are incomplete, repeat with
 *                      max_tasks >= status[0]; 2 / 3 as in nlsh_scan_topk_cells_phase.
 *   (caller)           total = sum of the counts, row_offsets [dev] int64 [Q + 1] = their exclusive prefix sum (row_offsets[Q] = total).
 *   nlsh_range_fill    the same arguments, then row_offsets, total, cursor [dev] int32 [Q] (zeroed by the call; on return equal to the
 *                      counts), out_keys [dev] uint64 [total] (NULL = not wanted), out_dist [dev] float [total] (NULL = not wanted),
 *                      out_idx [dev] int32 [total], status, workspace, max_tasks, sort_workspace (nlsh_range_sort_workspace), events, stream.
 *                      Runs one scan launch in fill mode ON THE PLAN THE COUNT CALL LEFT IN `workspace` -- same workspace, same
 *                      max_tasks, same key table, radius and filter; nothing else may use that workspace in between --, sorts every
 *                      query's segment [row_offsets[q], row_offsets[q + 1]) by key (rocPRIM segmented radix sort) and unpacks the
 *                      sorted keys.  Keys within a query are distinct, so the result does not depend on the order of the atomics.
 *                      A key whose slot lies outside its query's segment (offsets that are not the prefix sum of this plan's counts)
 *                      is not stored; cursor[q] then differs from the segment's length.
 *
 * Tiled schedule only (algo NLSH_SCAN_BUCKET_TILED), every storage and metric, P <= NLSH_MAX_PROBES, d <= NLSH_MAX_DIM,
 * total < 2^31.  Q = 0, total = 0 and an empty index are valid.  Checked on the host before anything is launched, NLSH_E_INVALID /
 * NLSH_E_UNSUPPORTED with the argument's name in nlsh_last_error(): a null radius, out_count or row_offsets, a misaligned row_filter,
 * another algo, P or d out of range, negative sizes.  The workspace-size functions return 0 and a message for sizes they refuse. */
size_t nlsh_range_workspace(int64_t Q, int P, int64_t max_tasks, int64_t n_buckets, int d);
size_t nlsh_range_sort_workspace(int64_t Q, int64_t total);
int nlsh_range_count(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid,
                     const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                     const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                     const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                     const int32_t *qkeys, const int32_t *nkeys, int P, int metric, int algo,
                     const uint32_t *row_filter, const float *radius, int32_t *out_count, int32_t *out_ncand,
                     int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                     void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream);
int nlsh_range_fill(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid,
                    const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                    const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                    const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                    const int32_t *qkeys, const int32_t *nkeys, int P, int metric, int algo,
                    const uint32_t *row_filter, const float *radius, const int64_t *row_offsets, int64_t total, int32_t *cursor,
                    uint64_t *out_keys, float *out_dist, int32_t *out_idx,
                    int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                    void *sort_workspace, size_t sort_workspace_bytes, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * sq8 corpus storage: one byte per element with a per-dimension offset and step, for real-valued rows.  No reference counterpart.
 *
 * A quantiser is lo[d], step[d], float32, finite, step > 0.  The rule, in separate IEEE float32 operations (no fused multiply-add):
 *   decode  deq(c, j) = float(c) * step[j] + lo[j]                      -- torch: codes.float() * step + lo
 *   encode  t = (x - lo[j]) / step[j]; code = clamp(rint(t), 0, 255)    -- torch: ((x - lo) / step).round().clamp(0, 255); ties to even.
 *           A finite value outside the range SATURATES and the row is counted; a row holding a NaN or an infinity is refused
 *           (first_bad, as in the typed calls: the smallest such row, -1 for none; the outputs are then to be dropped).
 *   train   lo = min + 0.0f and hi = max + 0.0f over the rows (a zero of either sign becomes +0), step = (hi - lo) / 255.0f, or 1.0f
 *           where hi == lo.  A range that overflows float32 gives step = +inf: the caller refuses such a quantiser.
 * The codes live in the uint8 layout: pitch a multiple of 16 elements from a 16-byte aligned base, columns >= d stored as code 0.  Every
 * lo / step array a call READS has row_stride (the pitch) entries, 16-byte aligned, padded behind d with lo = 0, step = 1 -- a padded
 * column decodes to +0 exactly as the float32 index holds it.  An sq8 index is, by definition, the float32 index over deq(codes): every
 * array and every result bit of the calls below equals what the float32 calls give on those rows.  lo = 0, step = 1 on integers in
 * [0, 255] is NLSH_STORE_U8.  The typed calls keep refusing every storage code past NLSH_STORE_U8: these are entry points of their own.
 *
 * nlsh_sq8_train: rows [dev] of `storage` (NLSH_STORE_F32 | NLSH_STORE_F16) elements, [n, d] with row stride row_stride elements (any
 *   alignment: 16- / 8-byte loads where the rows allow, element loads otherwise); one read of the rows, per-workgroup partial minima and
 *   maxima in the workspace (nlsh_sq8_train_workspace: host arithmetic, 0 = invalid sizes) and a small final pass -- no float atomics,
 *   the result is bit-defined.  lo, step [dev] float [quant_stride], quant_stride >= d: entries >= d are written as the padding; n = 0
 *   gives lo = 0, step = 1.  first_bad [dev] int32 [1].
 * nlsh_gather_rows_sq8: nlsh_gather_rows_typed with the encoding destination.  A NLSH_STORE_F32 / F16 source is encoded, a NLSH_STORE_U8
 *   source is codes and is copied.  inv_norm (nullable) is computed over the DECODED values in nlsh_gather_rows' operation order.
 *   clamped_rows [dev] int32 [1] (nullable) receives the number of rows with at least one saturated element (a refused row is not
 *   counted, here or in nlsh_csr_update_sq8).
 * nlsh_csr_update_sq8: nlsh_csr_update_typed on an sq8 index: kept rows move as bytes, new rows of new_storage are encoded on the way in
 *   (NLSH_STORE_U8: codes, copied), new rows' inv_norm over decoded values; first_bad (nullable for NLSH_STORE_U8 rows) and clamped_rows
 *   (nullable) count among the new rows.  row_stride == stride_out when both sides have rows.  Workspace: nlsh_csr_update_workspace.
 * nlsh_scan_topk_cells_phase_sq8: nlsh_scan_topk_cells_phase_filtered over an sq8 index, lo and step behind corpus_sorted; row_filter
 *   NULL = no filter.  Tiled schedule only (NLSH_E_UNSUPPORTED otherwise), every metric, k <= NLSH_MAX_K_TILED.  lo and step are checked
 *   like every other pointer (null, 16-byte alignment), the pitch and d by the uint8 rules.  The codes are decoded as they are staged.
 *   The radius, step, graph-slot and one-call batch entry points take no sq8 index. */
size_t nlsh_sq8_train_workspace(int64_t n, int d);
int nlsh_sq8_train(const void *rows, int storage, int64_t row_stride, int d, int64_t n, float *lo, float *step, int64_t quant_stride,
                   int32_t *first_bad, void *workspace, size_t workspace_bytes, nlsh_stream_t stream);
int nlsh_gather_rows_sq8(const void *corpus, int src_storage, int64_t src_stride, int d, const int32_t *perm, int64_t n,
                         uint8_t *sorted, int64_t dst_stride, const float *lo, const float *step, float *inv_norm, int32_t *gid,
                         int32_t id_base, int32_t *first_bad, int32_t *clamped_rows, nlsh_stream_t stream);
int nlsh_csr_update_sq8(const uint8_t *corpus_sorted, const float *lo, const float *step, int64_t row_stride, int d, const int32_t *gid,
                        const float *inv_norm, const int32_t *uniq_keys, const int32_t *offsets, int64_t n_old, int64_t n_buckets_old,
                        const uint8_t *keep, int64_t n_kept,
                        const void *rows_new, int new_storage, int64_t new_stride, const int32_t *keys_new, const int32_t *ids_new,
                        int64_t m_new,
                        uint8_t *sorted_out, int64_t stride_out, int32_t *gid_out, float *inv_norm_out, int32_t *src_out,
                        int32_t *uniq_out, int32_t *offsets_out, int32_t *n_buckets_out, int32_t *first_bad, int32_t *clamped_rows,
                        void *workspace, size_t workspace_bytes, nlsh_stream_t stream);
int nlsh_scan_topk_cells_phase_sq8(const uint8_t *corpus_sorted, const float *lo, const float *step, int64_t row_stride, int d,
                                   const int32_t *gid, const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order,
                                   int32_t n_buckets, const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                   const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                   const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                   float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                   int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                   void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases,
                                   const uint32_t *row_filter);

/* ---------------------------------------------------------------------------------------------
 * Per-query tag filters: row tags matched against query masks inside the tiled scan.
 *
 * Every SORTED row carries a 64-bit tag word: row_tags [dev, 8-byte aligned] uint64 [N], entry p = the tag of sorted row p (the caller
 * keeps it in step with gid: tags_sorted = tags[perm]; a signed 64-bit container is reinterpreted, bit 63 is a bit like any other).
 * Every query of the call carries a 64-bit mask: query_masks [dev, 8-byte aligned] uint64 [Q].  The call has ONE match mode, tag_match:
 *   NLSH_TAG_ANY  the row passes iff (tag & mask) != 0
 *   NLSH_TAG_ALL  the row passes iff (tag & mask) == mask
 *   NLSH_TAG_EQ   the row passes iff tag == mask
 * Definition: query q's result is what the same call gives on the index built from the rows that pass q's mask alone, with the same
 * ids, bucket keys and key table -- ids, distance bits and the 64-bit sort keys, with -1 / +inf / ~0 behind a list shorter than k.
 * out_ncand counts the rows of the probed buckets BEFORE the tags, as it does before a row filter.  A denied row is dropped in front of
 * the top-k selection; it changes no distance bit of another row, whatever it holds (NaN, infinities).  NLSH_TAG_ALL with mask 0 passes
 * every row (the untagged call's outputs in every word), NLSH_TAG_ANY with mask 0 passes none (all-padding lists).  With row_filter
 * given as well a row must pass both.  The tags are the rows', not a generation's: nothing is built per call and nothing goes stale.
 *
 * nlsh_scan_topk_cells_phase_tagged: nlsh_scan_topk_cells_phase_filtered plus the trailing row_tags, query_masks, tag_match.
 * nlsh_scan_topk_cells_phase_sq8_tagged: nlsh_scan_topk_cells_phase_sq8 plus the same three arguments.
 * row_tags == NULL (then query_masks must be NULL too; tag_match is not looked at) is the base call, argument for argument.  Tiled
 * schedule only, every storage, every metric, k <= NLSH_MAX_K_TILED.  Refused before anything is enqueued, the argument named in
 * nlsh_last_error(): a schedule other than NLSH_SCAN_BUCKET_TILED (NLSH_E_UNSUPPORTED); one of the two pointers without the other, a
 * pointer that is not 8-byte aligned, tag_match outside the three codes (NLSH_E_INVALID).  The calls cannot check the arrays' sizes.
 * The step, graph-slot, one-call batch and radius entry points take no tags.  Beside what the filtered call reads, the scan reads
 * 8 bytes per (task, row) -- next to the row id -- and 8 bytes per (task, query).
 * ------------------------------------------------------------------------------------------- */
#define NLSH_TAG_ANY 0
#define NLSH_TAG_ALL 1
#define NLSH_TAG_EQ 2
int nlsh_scan_topk_cells_phase_tagged(const void *corpus_sorted, int storage, int64_t row_stride, int d, const int32_t *gid,
                                      const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order, int32_t n_buckets,
                                      const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                      const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                      const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                      float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                      int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                      void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases,
                                      const uint32_t *row_filter, const uint64_t *row_tags, const uint64_t *query_masks, int tag_match);
int nlsh_scan_topk_cells_phase_sq8_tagged(const uint8_t *corpus_sorted, const float *lo, const float *step, int64_t row_stride, int d,
                                          const int32_t *gid, const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order,
                                          int32_t n_buckets, const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                          const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                          const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                          float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                          int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                          void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases,
                                          const uint32_t *row_filter, const uint64_t *row_tags, const uint64_t *query_masks, int tag_match);

/* ---------------------------------------------------------------------------------------------
 * pq corpus storage: product quantisation, M = ceil(d / dsub) bytes per row.  The reference names it (nlsh/hashings.py ends in an empty
 * ProductQuantization class) and has nothing to compare with.
 *
 * THE RULE.
 *   quantiser  a codebook C, float32 [M, 256, dsub], finite, dsub in {4, 8, 16}, M = ceil(d / dsub), 16-byte aligned.  Columns of the last
 *              sub-vector at or beyond d are held as +0 (the Python facade zeroes them on intake; these calls read what they are given).
 *   decode     row element j is C[j / dsub][code[j / dsub]][j % dsub]: a copy, no arithmetic.
 *   encode     per sub-vector m, code[m] is the centroid c with the smallest s(c): acc = 0.0f; for j ascending over the sub-vector's
 *              columns below d: t = x_j - C[m][c][j]; acc = acc + t * t -- a separate IEEE float32 subtract, multiply and add (the
 *              library is built with -ffp-contract=off).  Ties go to the lowest c.  A row holding a NaN or an infinity is refused by its
 *              number (first_bad, as in the sq8 calls: the smallest such row, -1 for none; the codes are then to be dropped).  Nothing
 *              saturates, so nothing is counted as clamped.
 *   cosine     inv_norm of a stored row is the float32 path's rule (nlsh_gather_rows) applied to the decoded row: the same operations
 *              in the same order.
 *   keys       the bucket keys of a pq corpus are the hasher's keys of the DECODED rows, unless the caller gives keys.
 * A pq index is, by definition, the float32 index over the decoded rows: every array and every result bit of the scan call below equals
 * what the float32 calls give on those rows.  The sorted copy is a uint8 row store of width M (pitch a multiple of 16 bytes, bytes behind
 * M stored as 0): nlsh_gather_rows_typed with a NLSH_STORE_U8 source and destination builds it, nlsh_csr_update_typed mutates it (codes
 * encoded first), and nlsh_pq_inv_norm computes the cosine norms of the result afterwards.  The typed calls keep refusing every storage
 * code past NLSH_STORE_U8.
 *
 * nlsh_pq_encode: rows [dev] of `storage` (NLSH_STORE_F32 | NLSH_STORE_F16) elements, [n, d] with row stride row_stride elements (any
 *   alignment of the element size) -> codes [dev] uint8 [n, M] in the rows' order, code_pitch >= M bytes between rows (only the M code
 *   bytes of a row are written).  first_bad [dev] int32 [1].
 * nlsh_pq_decode_rows: codes [n, M] -> out [dev] float32 [n, d], out_stride >= d floats between rows (columns below d are written).
 * nlsh_pq_inv_norm: inv_norm [dev] float [n] of n code rows.
 * nlsh_scan_topk_cells_phase_pq: nlsh_scan_topk_cells_phase_sq8 over a pq index, with the codebook, dsub and the code pitch (bytes,
 *   a multiple of 16) where that call has lo and step; row_stride is the decoded row's width M * dsub; row_filter NULL = no filter.
 *   Tiled schedule only (NLSH_E_UNSUPPORTED otherwise), every metric, k <= NLSH_MAX_K_TILED.  Refused: dsub outside {4, 8, 16}, a null
 *   or misaligned codebook (NLSH_E_INVALID).  The code bytes are decoded as they are staged.  The radius, tagged, step, graph-slot and
 *   one-call batch entry points take no pq index. */
int nlsh_pq_encode(const void *rows, int storage, int64_t row_stride, int d, int64_t n, const float *codebook, int dsub,
                   uint8_t *codes, int64_t code_pitch, int32_t *first_bad, nlsh_stream_t stream);
int nlsh_pq_decode_rows(const uint8_t *codes, int64_t code_pitch, int64_t n, const float *codebook, int dsub, int d, float *out,
                        int64_t out_stride, nlsh_stream_t stream);
int nlsh_pq_inv_norm(const uint8_t *codes, int64_t code_pitch, int64_t n, const float *codebook, int dsub, int d, float *inv_norm,
                     nlsh_stream_t stream);
int nlsh_scan_topk_cells_phase_pq(const uint8_t *corpus_sorted, const float *codebook, int dsub, int64_t code_pitch, int64_t row_stride, int d,
                                  const int32_t *gid, const int32_t *uniq_keys, const int32_t *offsets, const int32_t *bucket_order,
                                  int32_t n_buckets, const int32_t *cell_of, const int32_t *cell_offsets, int32_t n_cells,
                                  const float *inv_norm, const float *queries, int64_t q_stride, int64_t Q,
                                  const int32_t *qkeys, const int32_t *nkeys, int P, int k, int metric, int algo, int seg_rows,
                                  float *out_dist, int32_t *out_idx, uint64_t *out_keys, int32_t *out_ncand,
                                  int32_t *status, void *workspace, size_t workspace_bytes, int64_t max_tasks,
                                  void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream, int phases,
                                  const uint32_t *row_filter);

/* ---------------------------------------------------------------------------------------------
 * One pipelined query batch per call.  Replaces, for a caller that streams batches, the whole body of Indexer.query
 * (nlsh/indexer.py:56-96: hashing.hash on the batch :59 via Indexer.hash :40-54, then the per-query loop :62-95) by ONE
 * enqueue: nlsh_encode_hash + the PLAN, SCAN and MERGE phases of nlsh_scan_topk_cells_phase (five launches since r06: the bucket
 * lookup of the PLAN phase runs in the encode's epilogue) and the events that order them across three or four streams.  A step (slot) is built once from everything that does not change between
 * batches of one shape; nlsh_query_step_enqueue then takes the batch pointer, its row stride and the Philox seed.  The library
 * owns the slot's events; streams and buffers are the caller's.  Results are those of the separate calls, bit for bit.
 *
 *   front:  encode(i+1) plan(i+1)         | ...          (plan on its own stream when `plan` is not NULL: four stages)
 *   mid  :  scan(i)                       | ...
 *   tail :  merge(i-1) [caller's work]    | ...
 *
 * A slot is reused when its previous batch has left the tail stream (event, waited for on the device by the next enqueue).
 * hold_done != 0: the caller queues more work on the tail stream after the merge (a sharded index's all-gather + shard merge)
 * and then calls nlsh_step_release, which marks the slot's batch as finished at that point of the tail stream.
 * A failed enqueue leaves the slot's workspace in an undefined state (workspace contract above): destroy the step.
 * Not thread-safe: one host thread per step.
 * ------------------------------------------------------------------------------------------- */
typedef struct nlsh_step nlsh_step_t;
typedef struct nlsh_step_desc {
    /* hash function: the arguments of nlsh_encode_hash that do not change from batch to batch (dims [host] is copied) */
    int32_t n_layers, act, key_mode, n_probes;
    const int *dims;
    const float *packed;
    int64_t n_multi_rows;
    /* index: the arguments of nlsh_scan_topk_cells_phase in its order */
    const float *corpus_sorted;
    int64_t row_stride;
    const int32_t *gid, *uniq_keys, *offsets, *bucket_order, *cell_of, *cell_offsets;
    const float *inv_norm;
    int32_t d, n_buckets, n_cells, k, metric, algo, seg_rows, hold_done;
    /* batch shape and the slot's own buffers (qkeys [Q, n_probes] and nkeys [Q] are written by the encode, read by the scan) */
    int64_t Q;
    int32_t *qkeys, *nkeys;
    float *out_dist;
    int32_t *out_idx;
    uint64_t *out_keys;
    int32_t *out_ncand, *status;
    void *workspace;
    size_t workspace_bytes;
    int64_t max_tasks;
    /* streams (hipStream_t): front, mid, tail must be three different non-default streams; plan may be NULL, else a fourth different
     * one.  Equal handles are refused by nlsh_step_create, as is every argument the scan call itself would refuse. */
    nlsh_stream_t front, plan, mid, tail;
} nlsh_step_desc_t;

/* desc_bytes = sizeof(nlsh_step_desc_t) of the CALLER's header: a binding built against another layout is refused. */
int nlsh_step_create(const nlsh_step_desc_t *desc, size_t desc_bytes, nlsh_step_t **step_out);
/* A GRAPH slot (r06): the batch's five launches are captured once into a hipGraph and replayed on `lane`, the slot's OWN stream (a real
 * stream, different for every slot; the four stream handles of `desc` are ignored).  nlsh_query_step_enqueue is then one graph launch,
 * two kernel-node updates (the batch pointer / row stride / seed of the encode, the query pointer of the scan) and one event record --
 * a third of the runtime calls of a staged slot.  Batches of different slots overlap because their lanes do; consecutive batches of one
 * slot are ordered by its lane.  hold_done: the caller's extra work goes on `lane`.  A call with scan events is launched eagerly on the
 * lane (same kernels), and so is every batch of a slot whose capture or instantiation the runtime refused (or NLSH_STEP_NO_GRAPH set in the
 * environment when the slot is created: diagnostic).  Bucket-major schedules only (algo 1, 2).  Same results as the staged slots and the
 * separate calls, bit for bit. */
int nlsh_step_create_graph(const nlsh_step_desc_t *desc, size_t desc_bytes, nlsh_stream_t lane, nlsh_step_t **step_out);
int nlsh_step_destroy(nlsh_step_t *step);
/* New packed weights (nlsh_encoder_pack) for the batches enqueued from now on (a training step between two batches). */
int nlsh_step_set_weights(nlsh_step_t *step, const float *packed);
/* queries [dev] fp32 [Q, d] with row stride q_stride.  producer: the stream the batch was produced on (NULL = the default stream, as
 * for every nlsh_stream_t of this header) -- the front stream waits for what is queued there now (one stream query; an event only
 * when the producer has work in flight); pass the step's own front stream when there is never anything to wait for.  ev_scan_begin / ev_scan_end (nullable hipEvent_t): recorded around the scan kernel. */
int nlsh_query_step_enqueue(nlsh_step_t *step, const float *queries, int64_t q_stride, uint64_t seed, nlsh_stream_t producer,
                            void *ev_scan_begin, void *ev_scan_end);
int nlsh_step_release(nlsh_step_t *step);   /* hold_done steps only: the batch ends HERE on the tail stream */
/* The same batch for a caller that does not pipeline: everything on ONE stream, nothing kept between calls (the stream handles and
 * hold_done of `desc` are ignored; desc_bytes as for nlsh_step_create).  Replaces one whole Indexer.query body (nlsh/indexer.py:56-96)
 * by five launches: nlsh_encode_hash with the bucket lookup of :68 in its epilogue (the keys never leave the workgroup that made them
 * before they are looked up), two launches that lay out the (row segment, query group) tasks, the scan kernel, the merge.
 * row0: index of the batch's first row in the Philox counter of the multi-probe draws (as nlsh_encode_hash's row0: a row range of a
 * larger batch draws what it would have drawn inside it; desc->n_multi_rows counts from the range's first row).
 * lookup_done != 0: skip the hashing and repeat the scan part on the keys the previous call of this batch left in desc->qkeys --
 * the retry after status[1] = 1 (task table too small), with a larger max_tasks / workspace. */
int nlsh_query_batch(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, uint64_t seed,
                     int64_t row0, int lookup_done, void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream);
/* nlsh_query_batch for a caller that wants the results on the HOST: the same five launches with the host-writing form of the merge last
 * (k <= NLSH_MAX_K, bucket-major schedules).  host_out [host memory mapped for the device: hipHostMalloc / hipHostRegister] receives,
 * in int32 words,
 *     ids [Q * k] (-1 past a short list, as out_idx) | candidate counts [Q] | status [2] | key rows [Q * (n_probes + 1)]
 * where the key row of query q -- nkeys[q] followed by its n_probes keys of desc->qkeys -- is stored ONLY if the query has fewer than k
 * candidates (the caller's special case, nlsh/indexer.py:89-93); the rows of the other queries are not touched.  The block is complete
 * for the host once the stream has passed the call (an event or a stream synchronisation); no copy command is involved.
 * desc->out_dist / out_idx / out_ncand are NOT written by this form; desc->status is, as by nlsh_query_batch (and copied into the block).
 * host_words: words available at host_out, at least Q * (k + n_probes + 2) + 2.  Refused with NLSH_E_INVALID before anything is
 * enqueued: a NULL or too small host_out, k > NLSH_MAX_K, the query-major schedule, a host_out the runtime does not report as host
 * memory mapped for the device (hipPointerGetAttributes). */
int nlsh_query_batch_host(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, uint64_t seed,
                          int64_t row0, int lookup_done, int32_t *host_out, size_t host_words, nlsh_stream_t stream);
/* The RANKED multi-probe mode (nlsh_probe_ranked; with budget >= 1 nlsh_probe_ranked_budget's per-row stop) as one call of five launches
 * on one stream: nlsh_encode_hash with one probe (z and the hard code go to `scratch`), ONE kernel that ranks every row's keys into
 * desc->qkeys / desc->nkeys -- exactly the words nlsh_probe_ranked[_budget] writes for the same z and code -- and looks them up in the index
 * (the bucket lookup of nlsh/indexer.py:68 rides in the launch that made the keys, as it does in nlsh_query_batch's encode), the two
 * task-layout launches, the scan kernel, the merge.  Same results as nlsh_encode_hash + nlsh_probe_ranked[_budget] + nlsh_scan_topk on the
 * same descriptor, bit for bit.
 *   desc: as for nlsh_query_batch; n_probes in [1, NLSH_MAX_PROBES] is the width of the key table (the budget's cap),
 *         H = desc->dims[desc->n_layers]; n_multi_rows keeps its meaning.  Ranked keys are a function of the row alone: no seed, no row0.
 *   budget: 0 = none, >= 1 = nlsh_probe_ranked_budget's rule on desc->uniq_keys / offsets.
 *   scratch [dev], scratch_bytes >= nlsh_query_batch_ranked_scratch(desc->Q, H): z [Q, H], the hard codes [Q] and the one-probe encode's own
 *         key table; nothing in it is read after the call.  nlsh_query_batch_ranked_scratch is 0 for Q < 0 or H outside [1, 32].
 *   host_out NULL: the results stay on the device (out_dist / out_idx / out_ncand, nlsh_query_batch's form).  Otherwise the host-writing
 *         merge of nlsh_query_batch_host stores its block there, with that call's layout, host_words rule and refusals.
 *   lookup_done != 0: repeat the scan part only, on the keys already in desc->qkeys (their lookup redone by the stand-alone kernel): the
 *         retry after status[1] = 1, exactly as for nlsh_query_batch.
 * Refused before anything is enqueued: what nlsh_query_batch / nlsh_query_batch_host refuse; the query-major schedule (NLSH_E_INVALID);
 * n_buckets <= 0 (NLSH_E_INVALID); H outside [1, 32] (NLSH_E_UNSUPPORTED); budget < 0 (NLSH_E_INVALID); a NULL scratch (NLSH_E_INVALID) or
 * one that is too small (NLSH_E_WORKSPACE).  Q == 0 is NLSH_OK without a launch. */
size_t nlsh_query_batch_ranked_scratch(int64_t Q, int H);
int nlsh_query_batch_ranked(const nlsh_step_desc_t *desc, size_t desc_bytes, const float *queries, int64_t q_stride, int lookup_done,
                            int32_t budget, void *scratch, size_t scratch_bytes, int32_t *host_out, size_t host_words,
                            void *ev_scan_begin, void *ev_scan_end, nlsh_stream_t stream);
/* 1 while the slot's last batch has not left the tail stream, 0 once it has, < 0 on error.  Never blocks. */
int nlsh_step_busy(nlsh_step_t *step);

/* Merge G per-shard top-k lists per query (keys_in [dev] [G, Q, row_stride] u64, the first k of each
 * row as all-gathered from nlsh_scan_topk's out_keys) into the global top-k; same comparator, so the
 * result equals the single-GPU result.  Candidate counts are summed into out_ncand from ncand_in
 * (nullable) [G, Q], or, when ncand_in is NULL and row_stride > k, from element k of every row (so one
 * collective can carry keys and counts together).
 * Limits: k <= NLSH_MAX_K_TILED. */
int nlsh_merge_topk(const uint64_t *keys_in, int64_t row_stride, int G, int64_t Q, int k, const int32_t *ncand_in,
                    float *out_dist, int32_t *out_idx, int32_t *out_ncand, nlsh_stream_t stream);

/* The merge of a MULTI-TABLE index: G lists per query, one per hash table over the same corpus, so the same row may
 * sit in several lists.  nlsh_merge_topk's arguments and output conventions, with out_keys (nullable) in front of out_ncand.
 *   Input: keys_in [dev] [G, Q, row_stride] u64 (8-byte aligned); the first k of each row are one table's list as the scan's out_keys
 *         gives it: ascending, ~0-padded, its real keys distinct WITHIN the list.
 *   De-duplication: equal 64-bit keys in different lists are ONE candidate and appear once in the output.  Padding (~0) is never a
 *         candidate.  Repeats are dropped BEFORE the k best are selected: the output is short only when fewer than k distinct keys exist.
 *   Precondition, NOT checked: an id carries the same distance word in every list (true of the tiled schedule's lists over one
 *         corpus: the distance of a (query, row) pair is a function of the two vectors alone).  Two keys with one id and different
 *         distance words are different keys: both stay, and the id appears twice.
 *   Output: the k smallest distinct keys in ascending (distance bits, id) order -- out_dist [Q, k], out_idx [Q, k], out_keys [Q, k]
 *         (nullable) -- the tail padded as the scan pads it: id -1, dist +inf, key ~0.
 *   Candidate count: out_ncand [Q] (nullable) = the SUM over the lists -- scored (query, row) pairs, a row found by two tables counts
 *         twice -- taken as nlsh_merge_topk takes it: from ncand_in [G, Q], or from element k of every row when ncand_in is NULL and
 *         row_stride > k, or not at all (out_ncand untouched).
 *   On disjoint input (no key repeated across lists) every output word equals nlsh_merge_topk's.
 * Limits: 1 <= k <= NLSH_MAX_K_TILED and 1 <= G <= NLSH_MAX_TABLES (beyond either: NLSH_E_UNSUPPORTED), row_stride >= k, any Q; Q = 0 is
 * NLSH_OK without a launch.  All arguments are checked on the host before anything touches the device.  No workspace, no atomics. */
#define NLSH_MAX_TABLES 16
int nlsh_merge_topk_unique(const uint64_t *keys_in, int64_t row_stride, int G, int64_t Q, int k, const int32_t *ncand_in,
                           float *out_dist, int32_t *out_idx, uint64_t *out_keys /* nullable */, int32_t *out_ncand, nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact re-ranking: the second stage of a two-stage query.  A scan over a compressed (float16 / uint8 / sq8) or a
 * folded-L2 index over-fetches kc > k candidates per query; this call rescores those kc rows on the ORIGINAL float32 rows and keeps
 * the k best.  No reference counterpart (the reference scans the caller's float32 rows and has nothing to refine).
 *   Refine store: the index's rows as float32 in ID ORDER -- store [n_rows, store_stride], row id - id_base is the original row with
 *         that id; store_stride a multiple of 4 floats, >= d, the whole pitch of every row readable (columns >= d are never used);
 *         16-byte aligned.  Cosine: store_inv_norm [dev] [n_rows] holds the bits nlsh_gather_rows gives that row.  The store is device
 *         memory (store_on_host = 0) or pinned host memory mapped for the device (store_on_host = 1: hipHostMalloc / hipHostRegister;
 *         both ends of the store are held against the runtime's record of the mapping, a device pointer is refused); the kernel is
 *         the same, a host store is read over the host link.
 *   Input: queries [dev] [Q, q_stride] (any 4-byte alignment, strided row views allowed); cand [dev] [Q, cand_stride], the first kc
 *         of each row one query's candidate ids (stage one's out_idx as it is).  1 <= k <= kc <= NLSH_MAX_K_TILED.
 *   Ids:  a VALID id is one in [id_base, id_base + n_rows).  -1 is padding and may stand anywhere in a list.  Any other id is DROPPED,
 *         never dereferenced, and reported: first_bad [dev] int32 [1] receives the smallest query number whose list held one, -1 for
 *         none (the call initialises it).  Precondition, NOT checked: the ids within one list are distinct.
 *   Result: per query the k smallest sort keys  mono(dist(q, row(id))) << 32 | id  over its valid ids, ascending -- the (distance bits,
 *         id) order of every other top-k path -- in out_dist [Q, k], out_idx [Q, k], out_keys [Q, k] (nullable), the tail padded as
 *         the scan pads it: id -1, dist +inf, key ~0.  out_count [Q] (nullable) = the number of real entries, min(k, valid ids).
 *   dist has THE BITS THE TILED FLOAT32 SCAN GIVES THE SAME (query, row) PAIR:
 *         one fmaf chain per pair over the dimension, ascending from 0;
 *         NLSH_METRIC_L2_EPS  acc += ((q - c) + 1e-6f)^2, then the correctly rounded square root;
 *         NLSH_METRIC_COSINE  acc += q' * c over q' = q / max(||q||, 1e-8) as the scan's PLAN phase normalises it, then
 *                             1.0f - acc * store_inv_norm[row].
 *         The re-rank is always the EXACT L2 form, whatever form stage one ran with: NLSH_METRIC_L2_EPS_FOLDED is refused.
 *   Limits: 1 <= k <= kc <= NLSH_MAX_K_TILED and 1 <= d <= NLSH_MAX_DIM (NLSH_E_UNSUPPORTED beyond), Q < 2^31; Q = 0 is NLSH_OK
 *         without a launch.  Every argument is checked on the host before anything is enqueued.  One launch; no workspace, no
 *         atomics but the first_bad minimum. */
int nlsh_rerank_topk(const float *queries, int64_t q_stride, int64_t Q, int d,
                     const float *store, int64_t store_stride, int64_t n_rows, int32_t id_base, int store_on_host,
                     const float *store_inv_norm /* cosine, device */,
                     const int32_t *cand, int64_t cand_stride, int kc, int k, int metric /* NLSH_METRIC_L2_EPS | NLSH_METRIC_COSINE */,
                     float *out_dist, int32_t *out_idx, uint64_t *out_keys /* nullable */, int32_t *out_count /* nullable */,
                     int32_t *first_bad, nlsh_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact brute-force k-NN: every row of `corpus` against every query, fp32-MFMA distances with the top-k fused behind them.
 * Replaces the reference's mm + topk precompute (precompute.py:22-67): ground truth of a query set, self-kNN of a training set.
 * Distances take precompute.py's forms, NOT the scan's pairwise_distance form (no square root, no epsilon):
 *   NLSH_EXACT_L2      (||c||^2 - 2 (q.c)) + ||q||^2                    squared L2
 *   NLSH_EXACT_COSINE  1 - ((q.c) * inv||q||) * inv||c||,  inv||x|| = 1 / max(||x||, 1e-12)
 * Every dot product (q.c and the squared norms) is ONE fp32 chain over the dimension, ascending from 0 (an fmaf chain; for q.c the
 * accumulator chain of v_mfma_f32_32x32x2_f32, which is the same bits): the distance of a (query, row) pair depends on the two vectors
 * alone, never on the tile, the column split or the launch shape -- results are bitwise identical for every `splits`.
 * Order: ascending 64-bit key monotone(dist) << 32 | row id, i.e. (distance bits, smaller row id); with fewer than k eligible rows the
 * tail is id -1 / dist +inf (the scan's padding).  Inputs must be finite (precondition, not checked).
 * self_row0 >= 0: query i skips corpus row self_row0 + i -- self-kNN of a row range of the same matrix.  The row is excluded BY ID; the
 * reference drops column 0 of a (k + 1)-list instead, which among exact duplicates may drop a duplicate and keep the row itself.
 * splits: column splits of the corpus per query tile (0 = automatic, a function of (Q, N, k) only); their partial lists are merged by
 * nlsh_merge_topk's kernel.
 * Workspace: 4 N bytes of corpus norms (the only term that depends on N) + O(splits * Q * k): 4 Q bytes of query norms and
 * splits * Q candidate rows of 256 (k <= 64) or 512 keys.  Callers with many queries pass them in chunks to bound it.
 * Limits: 1 <= k <= NLSH_MAX_K_TILED, 1 <= d <= NLSH_MAX_DIM (NLSH_E_UNSUPPORTED), N < 2^31, any Q; Q = 0 and N = 0 are valid
 * (N = 0: padding only).  Arguments are checked on the host before anything touches the device.
 * ------------------------------------------------------------------------------------------- */
#define NLSH_EXACT_L2 0
#define NLSH_EXACT_COSINE 1
size_t nlsh_exact_workspace(int64_t Q, int64_t N, int k, int splits);   /* 0 = invalid arguments; splits 0 = automatic */
int nlsh_exact_topk(const float *corpus, int64_t row_stride, int64_t N, int d,
                    const float *queries, int64_t q_stride, int64_t Q, int k, int metric,
                    int64_t self_row0 /* -1: none */, int splits /* 0: automatic */,
                    float *out_dist, int32_t *out_idx, void *workspace, size_t workspace_bytes, nlsh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NLSH_HIP_H */
