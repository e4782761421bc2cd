// The refused scan calls of tests/test_scan_call_checks_cpu.py as a stand-alone program, for a sanitizer run of the HOST code that checks
// them: `make -C neural-locality-sensitive-hashing_amd/csrc sanitize` compiles scan_topk.hip, scan_bucket.hip, scan_bucket_range.hip and
// step.hip with -Xarch_host -fsanitize=address,undefined, links them and this file into one executable and runs it.  CPU only: every call
// here is refused (or is an empty batch) before anything is enqueued, the pointers are made-up addresses that are never read, and no
// device is needed or touched.  Exit status 0 = every call returned the code in the table and neither sanitizer spoke.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../include/nlsh_hip.h"

namespace {

void *const FAKE = (void *)0x10000;   // 256-byte aligned, never dereferenced
void *off(int bytes) { return (char *)FAKE + bytes; }

struct Args {   // the valid set of the Python test: d = 100 in rows of 112, the tiled schedule, a filter, a workspace of 0 bytes
    void *corpus_sorted = FAKE; int storage = NLSH_STORE_F32; int64_t row_stride = 112; int d = 100;
    void *gid = FAKE, *uniq_keys = FAKE, *offsets = FAKE, *bucket_order = nullptr; int32_t n_buckets = 3;
    void *cell_of = nullptr, *cell_offsets = nullptr; int32_t n_cells = 0;
    void *inv_norm = nullptr, *queries = FAKE; int64_t q_stride = 100, Q = 4; void *qkeys = FAKE, *nkeys = FAKE;
    int P = 2, k = 10, metric = NLSH_METRIC_L2_EPS, algo = NLSH_SCAN_BUCKET_TILED, seg_rows = 0;
    void *out_dist = FAKE, *out_idx = FAKE, *out_keys = nullptr, *out_ncand = FAKE, *status = FAKE, *workspace = FAKE;
    size_t workspace_bytes = 0; int64_t max_tasks = 16; int phases = NLSH_PHASE_PLAN | NLSH_PHASE_SCAN | NLSH_PHASE_MERGE;
    void *row_filter = FAKE, *radius = FAKE, *out_count = FAKE, *row_offsets = FAKE; int64_t total = 5;
    void *cursor = FAKE, *sort_workspace = FAKE; size_t sort_workspace_bytes = 0;
    void *lo = FAKE, *step = FAKE, *row_tags = FAKE, *query_masks = FAKE; int tag_match = NLSH_TAG_ANY;   // the tagged entries' alone
};

enum Entry { SCAN_TOPK, PHASE, CELLS, TYPED, FILTERED, RANGE_COUNT, RANGE_FILL, TAGGED, SQ8_TAGGED, N_ENTRIES };
const char *const ENTRY_NAME[N_ENTRIES] = {"nlsh_scan_topk", "nlsh_scan_topk_phase", "nlsh_scan_topk_cells_phase", "nlsh_scan_topk_cells_phase_typed",
                                           "nlsh_scan_topk_cells_phase_filtered", "nlsh_range_count", "nlsh_range_fill",
                                           "nlsh_scan_topk_cells_phase_tagged", "nlsh_scan_topk_cells_phase_sq8_tagged"};
constexpr unsigned bit(Entry e) { return 1u << e; }
constexpr unsigned TAGS = bit(TAGGED) | bit(SQ8_TAGGED);   // the filtered and the sq8 call plus row_tags, query_masks, tag_match
constexpr unsigned TOPK = bit(SCAN_TOPK) | bit(PHASE) | bit(CELLS) | bit(TYPED) | bit(FILTERED) | TAGS, RANGE = bit(RANGE_COUNT) | bit(RANGE_FILL);
constexpr unsigned HAS_PHASES = TOPK & ~bit(SCAN_TOPK), HAS_CELLS = bit(CELLS) | bit(TYPED) | bit(FILTERED) | RANGE | TAGS;
constexpr unsigned STORED = bit(TYPED) | bit(FILTERED) | RANGE | bit(TAGGED), HAS_FILTER = bit(FILTERED) | RANGE | TAGS, ALL = TOPK | RANGE;

#define F32P(p) ((const float *)(p))
#define I32P(p) ((const int32_t *)(p))
#define TOPK_TAIL(a) F32P(a.inv_norm), F32P(a.queries), a.q_stride, a.Q, I32P(a.qkeys), I32P(a.nkeys), a.P, a.k, a.metric, a.algo, a.seg_rows, (float *)a.out_dist, \
                     (int32_t *)a.out_idx, (uint64_t *)a.out_keys, (int32_t *)a.out_ncand, (int32_t *)a.status, a.workspace, a.workspace_bytes, a.max_tasks,        \
                     nullptr, nullptr, nullptr
#define INDEX(a) a.row_stride, a.d, I32P(a.gid), I32P(a.uniq_keys), I32P(a.offsets), I32P(a.bucket_order), a.n_buckets
#define CELLS_OF(a) I32P(a.cell_of), I32P(a.cell_offsets), a.n_cells
#define RANGE_HEAD(a) a.corpus_sorted, a.storage, INDEX(a), CELLS_OF(a), F32P(a.inv_norm), F32P(a.queries), a.q_stride, a.Q, I32P(a.qkeys), I32P(a.nkeys), a.P, \
                      a.metric, a.algo, (const uint32_t *)a.row_filter, F32P(a.radius)

int call(Entry e, const Args &a) {
    switch (e) {
    case SCAN_TOPK: return nlsh_scan_topk(F32P(a.corpus_sorted), INDEX(a), TOPK_TAIL(a));
    case PHASE: return nlsh_scan_topk_phase(F32P(a.corpus_sorted), INDEX(a), TOPK_TAIL(a), a.phases);
    case CELLS: return nlsh_scan_topk_cells_phase(F32P(a.corpus_sorted), INDEX(a), CELLS_OF(a), TOPK_TAIL(a), a.phases);
    case TYPED: return nlsh_scan_topk_cells_phase_typed(a.corpus_sorted, a.storage, INDEX(a), CELLS_OF(a), TOPK_TAIL(a), a.phases);
    case FILTERED:
        return nlsh_scan_topk_cells_phase_filtered(a.corpus_sorted, a.storage, INDEX(a), CELLS_OF(a), TOPK_TAIL(a), a.phases, (const uint32_t *)a.row_filter);
    case TAGGED:
        return nlsh_scan_topk_cells_phase_tagged(a.corpus_sorted, a.storage, INDEX(a), CELLS_OF(a), TOPK_TAIL(a), a.phases, (const uint32_t *)a.row_filter,
                                                 (const uint64_t *)a.row_tags, (const uint64_t *)a.query_masks, a.tag_match);
    case SQ8_TAGGED:
        return nlsh_scan_topk_cells_phase_sq8_tagged((const uint8_t *)a.corpus_sorted, F32P(a.lo), F32P(a.step), INDEX(a), CELLS_OF(a), TOPK_TAIL(a), a.phases,
                                                     (const uint32_t *)a.row_filter, (const uint64_t *)a.row_tags, (const uint64_t *)a.query_masks, a.tag_match);
    case RANGE_COUNT:
        return nlsh_range_count(RANGE_HEAD(a), (int32_t *)a.out_count, (int32_t *)a.out_ncand, (int32_t *)a.status, a.workspace, a.workspace_bytes, a.max_tasks,
                                nullptr, nullptr, nullptr);
    default:
        return nlsh_range_fill(RANGE_HEAD(a), (const int64_t *)a.row_offsets, a.total, (int32_t *)a.cursor, (uint64_t *)a.out_keys, (float *)a.out_dist,
                               (int32_t *)a.out_idx, (int32_t *)a.status, a.workspace, a.workspace_bytes, a.max_tasks, a.sort_workspace, a.sort_workspace_bytes,
                               nullptr, nullptr, nullptr);
    }
}

struct Fault {
    const char *name;
    std::function<void(Args &)> make;
    const char *fragment;
    unsigned entries;
    int code;
};

int failures = 0;
void expect(Entry e, const char *what, const Args &a, int code, const char *fragment) {
    const int rc = call(e, a);
    const char *msg = nlsh_last_error();
    if (rc != code || (fragment && !strstr(msg, fragment))) {
        ++failures;
        fprintf(stderr, "FAIL %s / %s: returned %d (want %d), message \"%s\" (want \"%s\" in it)\n", ENTRY_NAME[e], what, rc, code, msg, fragment ? fragment : "");
    }
}

}  // namespace

int main() {
    const int INV = NLSH_E_INVALID, UNS = NLSH_E_UNSUPPORTED;
    // (the untagged faults below reach the tagged entries with their tags in place: the tags' own refusals come behind the schedule's)
    auto no_filter = [](Args &a) { a.row_filter = nullptr; a.row_tags = a.query_masks = nullptr; };
    std::vector<Fault> faults = {
        {"Q negative", [](Args &a) { a.Q = -1; }, "Q=-1", ALL, INV},
        {"Q = 2^31", [](Args &a) { a.Q = 1ll << 31; }, "Q=2147483648", ALL, INV},
        {"d = 0", [](Args &a) { a.d = 0; }, "d=0", ALL, UNS},
        {"d > MAX_DIM", [](Args &a) { a.d = NLSH_MAX_DIM + 1; a.row_stride = 1040; a.q_stride = a.d; }, "d=1025", ALL, UNS},
        {"P = 0", [](Args &a) { a.P = 0; }, "P=0", ALL, UNS},
        {"P > MAX_PROBES", [](Args &a) { a.P = NLSH_MAX_PROBES + 1; }, "P=65", ALL, UNS},
        {"k = 0", [](Args &a) { a.k = 0; }, "k=0", TOPK, UNS},
        {"k = 65, query-major", [=](Args &a) { a.k = 65; a.algo = NLSH_SCAN_QUERY_MAJOR; no_filter(a); }, "k=65", TOPK & ~bit(SQ8_TAGGED), UNS},   // (an sq8 call names its storage first)
        {"k = 65, bucket-major", [=](Args &a) { a.k = 65; a.algo = NLSH_SCAN_BUCKET_MAJOR; no_filter(a); }, "k=65", TOPK & ~bit(SQ8_TAGGED), UNS},   // (an sq8 call names its storage first)
        {"k = 257, tiled", [](Args &a) { a.k = 257; }, "k=257", TOPK, UNS},
        {"metric", [](Args &a) { a.metric = 9; }, "metric=9", ALL, INV},
        {"algo", [](Args &a) { a.algo = 9; }, "algo=9", ALL, INV},
        {"n_buckets negative", [](Args &a) { a.n_buckets = -1; }, "n_buckets", ALL, INV},
        {"max_tasks negative", [](Args &a) { a.max_tasks = -1; }, "max_tasks", ALL, INV},
        {"n_cells > n_buckets", [](Args &a) { a.n_cells = 4; a.cell_of = a.cell_offsets = FAKE; }, "n_cells=4", HAS_CELLS, INV},
        {"cells without cell_of", [](Args &a) { a.n_cells = 2; a.cell_offsets = FAKE; }, "cell_of", HAS_CELLS, INV},
        {"cells without cell_offsets", [](Args &a) { a.n_cells = 2; a.cell_of = FAKE; }, "cell_offsets", HAS_CELLS, INV},
        {"null queries", [](Args &a) { a.queries = nullptr; }, "null", ALL, INV},
        {"null qkeys", [](Args &a) { a.qkeys = nullptr; }, "null", ALL, INV},
        {"null nkeys", [](Args &a) { a.nkeys = nullptr; }, "null", ALL, INV},
        {"null status", [](Args &a) { a.status = nullptr; }, "null", ALL, INV},
        {"null workspace", [](Args &a) { a.workspace = nullptr; }, "null", ALL, INV},
        {"null corpus_sorted", [](Args &a) { a.corpus_sorted = nullptr; }, "null", ALL, INV},
        {"null gid", [](Args &a) { a.gid = nullptr; }, "null", ALL, INV},
        {"null uniq_keys", [](Args &a) { a.uniq_keys = nullptr; }, "null", ALL, INV},
        {"null offsets", [](Args &a) { a.offsets = nullptr; }, "null", ALL, INV},
        {"null out_dist", [](Args &a) { a.out_dist = nullptr; }, "null", TOPK, INV},
        {"null out_idx", [](Args &a) { a.out_idx = nullptr; }, "null", TOPK, INV},
        {"null out_ncand", [](Args &a) { a.out_ncand = nullptr; }, "null", TOPK, INV},
        {"cosine without inv_norm", [](Args &a) { a.metric = NLSH_METRIC_COSINE; }, "inv_norm", ALL, INV},
        {"row_stride < d", [](Args &a) { a.row_stride = 96; }, "row_stride=96", ALL, INV},
        {"pitch, float32", [](Args &a) { a.row_stride = 102; }, "multiple of 4", ALL & ~bit(SQ8_TAGGED), INV},
        {"pitch, float16", [](Args &a) { a.storage = NLSH_STORE_F16; a.row_stride = 100; }, "multiple of 8", STORED, INV},
        {"pitch, uint8", [](Args &a) { a.storage = NLSH_STORE_U8; a.row_stride = 104; }, "multiple of 16", STORED, INV},
        {"corpus misaligned", [](Args &a) { a.corpus_sorted = off(4); }, "16-byte aligned", ALL, INV},
        {"corpus misaligned, float16", [](Args &a) { a.corpus_sorted = off(8); a.storage = NLSH_STORE_F16; }, "16-byte aligned", STORED, INV},
        {"workspace misaligned", [](Args &a) { a.workspace = off(4); }, "16-byte aligned", ALL, INV},
        {"out_keys misaligned", [](Args &a) { a.out_keys = off(4); }, "out_keys", TOPK | bit(RANGE_FILL), INV},
        {"row_filter misaligned", [](Args &a) { a.row_filter = off(2); }, "row_filter", HAS_FILTER, INV},
        {"q_stride < d", [](Args &a) { a.q_stride = 99; }, "q_stride", ALL, INV},
        {"phases = 0", [](Args &a) { a.phases = 0; }, "phases=0", HAS_PHASES, INV},
        {"phases: the internal bit", [](Args &a) { a.phases = 8; }, "phases=8", HAS_PHASES, INV},
        {"storage", [](Args &a) { a.storage = 7; }, "storage=7", STORED, INV},
        {"float16, query-major", [=](Args &a) { a.storage = NLSH_STORE_F16; a.algo = NLSH_SCAN_QUERY_MAJOR; no_filter(a); }, "NLSH_SCAN_BUCKET_TILED", bit(TYPED) | bit(FILTERED), UNS},
        {"uint8, bucket-major", [=](Args &a) { a.storage = NLSH_STORE_U8; a.algo = NLSH_SCAN_BUCKET_MAJOR; no_filter(a); }, "NLSH_SCAN_BUCKET_TILED", bit(TYPED) | bit(FILTERED), UNS},
        {"filter, query-major", [](Args &a) { a.algo = NLSH_SCAN_QUERY_MAJOR; }, "row_filter", bit(FILTERED) | TAGS, UNS},
        {"filter, bucket-major", [](Args &a) { a.algo = NLSH_SCAN_BUCKET_MAJOR; }, "row_filter", bit(FILTERED) | TAGS, UNS},
        // per-query tag filters
        {"tags, query-major", [](Args &a) { a.algo = NLSH_SCAN_QUERY_MAJOR; a.row_filter = nullptr; }, "row_tags", TAGS, UNS},
        {"tags, bucket-major", [](Args &a) { a.algo = NLSH_SCAN_BUCKET_MAJOR; a.row_filter = nullptr; }, "row_tags", TAGS, UNS},
        {"query_masks without row_tags", [](Args &a) { a.row_tags = nullptr; }, "query_masks without row_tags", TAGS, INV},
        {"row_tags without query_masks", [](Args &a) { a.query_masks = nullptr; }, "row_tags without query_masks", TAGS, INV},
        {"row_tags misaligned", [](Args &a) { a.row_tags = off(4); }, "row_tags must be 8-byte aligned", TAGS, INV},
        {"query_masks misaligned", [](Args &a) { a.query_masks = off(4); }, "query_masks must be 8-byte aligned", TAGS, INV},
        {"tag_match = 3", [](Args &a) { a.tag_match = 3; }, "tag_match=3", TAGS, INV},
        {"tag_match = -1", [](Args &a) { a.tag_match = -1; }, "tag_match=-1", TAGS, INV},
        {"range, query-major", [=](Args &a) { a.algo = NLSH_SCAN_QUERY_MAJOR; no_filter(a); }, "NLSH_SCAN_BUCKET_TILED", RANGE, UNS},
        {"range, bucket-major", [=](Args &a) { a.algo = NLSH_SCAN_BUCKET_MAJOR; no_filter(a); }, "NLSH_SCAN_BUCKET_TILED", RANGE, UNS},
        // entries that disagree: a compressed top-k call holds its pitch (now < d) before the limits
        {"d > MAX_DIM, float16 (top-k)", [](Args &a) { a.d = NLSH_MAX_DIM + 1; a.storage = NLSH_STORE_F16; }, "row_stride=112", bit(TYPED) | bit(FILTERED) | bit(TAGGED), INV},
        {"d > MAX_DIM, float16 (range)", [](Args &a) { a.d = NLSH_MAX_DIM + 1; a.storage = NLSH_STORE_F16; }, "d=1025", RANGE, UNS},
    };
    int calls = 0;
    for (int e = 0; e < N_ENTRIES; ++e) {
        // the valid set passes every check of the arguments: what stops it is the size of its workspace, on every schedule it may take
        expect((Entry)e, "valid", Args(), NLSH_E_WORKSPACE, "workspace");
        for (int algo : {NLSH_SCAN_QUERY_MAJOR, NLSH_SCAN_BUCKET_MAJOR}) {
            Args a;
            a.algo = algo; a.row_filter = nullptr; a.row_tags = a.query_masks = nullptr;
            if (bit((Entry)e) & TOPK & ~bit(SQ8_TAGGED)) expect((Entry)e, "valid, other schedule", a, NLSH_E_WORKSPACE, "workspace");
        }
        for (const Fault &f : faults) {
            if (!(f.entries & bit((Entry)e))) continue;
            Args a;
            f.make(a);
            expect((Entry)e, f.name, a, f.code, f.fragment);
            ++calls;
        }
        Args empty;   // Q = 0: valid without its pointers (the radius calls keep the three they look at first)
        empty.Q = 0;
        empty.corpus_sorted = empty.gid = empty.uniq_keys = empty.offsets = empty.queries = empty.qkeys = empty.nkeys = empty.out_dist = empty.out_idx =
            empty.out_ncand = empty.status = empty.workspace = empty.row_filter = empty.cursor = empty.sort_workspace = nullptr;
        empty.lo = empty.step = empty.row_tags = empty.query_masks = nullptr;
        expect((Entry)e, "empty batch", empty, NLSH_OK, nullptr);
    }
    printf("%d refused calls over %d entry points, %d failures\n", calls, (int)N_ENTRIES, failures);
    return failures ? 1 : 0;
}
