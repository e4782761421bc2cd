// The refused row calls of tests/test_row_call_checks_cpu.py as a stand-alone program, for a sanitizer run of the HOST code that checks them:
// `make -C neural-locality-sensitive-hashing_amd/csrc sanitize` compiles build_csr.hip with -Xarch_host -fsanitize=address,undefined beside
// the scan units, links it and this file into one executable and runs it.  CPU only: every call here is refused (or is an empty gather)
// before anything is enqueued, the pointers are made-up addresses that are never read, and no device is needed or touched.  Exit status
// 0 = every call returned the code in the table and neither sanitizer spoke.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../include/nlsh_hip.h"

namespace {

void *const FAKE = (void *)0x10000;   // 256-byte aligned, never dereferenced
void *off(int bytes) { return (char *)FAKE + bytes; }

struct Args {   // the valid sets of the Python test: d = 100 in rows of 112; float32 rows arrive, to float16 where there is a storage to name
    int d = 100;
    // a gather (and the training call: rows = corpus, row_stride = src_stride, storage = src_storage, quant_stride = dst_stride)
    void *corpus = FAKE; int src_storage = NLSH_STORE_F32; int64_t src_stride = 100, n = 10; void *perm = FAKE, *sorted = FAKE;
    int dst_storage = NLSH_STORE_F16; int64_t dst_stride = 112; void *g_inv_norm = FAKE, *g_gid = FAKE;
    void *lo = FAKE, *step = FAKE, *first_bad = FAKE, *clamped_rows = FAKE;
    // an update: 10 of 1000 rows removed, 100 added
    void *corpus_sorted = FAKE; int storage = NLSH_STORE_F16; int64_t row_stride = 112; void *gid = FAKE, *inv_norm = FAKE, *uniq_keys = FAKE, *offsets = FAKE;
    int64_t n_old = 1000, n_buckets_old = 10; void *keep = FAKE; int64_t n_kept = 990;
    void *rows_new = FAKE; int new_storage = NLSH_STORE_F32; int64_t new_stride = 100; void *keys_new = FAKE, *ids_new = FAKE; int64_t m_new = 100;
    void *sorted_out = FAKE; int64_t stride_out = 112; void *gid_out = FAKE, *inv_norm_out = FAKE, *src_out = FAKE, *uniq_out = FAKE, *offsets_out = FAKE,
         *n_buckets_out = FAKE;
    void *workspace = FAKE; int64_t workspace_bytes = -1;   // -1: what the entry's workspace query returns, -2: one byte less than that
};

enum Entry { GATHER, GATHER_TYPED, GATHER_SQ8, UPDATE, UPDATE_TYPED, UPDATE_SQ8, TRAIN, N_ENTRIES };
const char *const ENTRY_NAME[N_ENTRIES] = {"nlsh_gather_rows", "nlsh_gather_rows_typed", "nlsh_gather_rows_sq8", "nlsh_csr_update", "nlsh_csr_update_typed",
                                           "nlsh_csr_update_sq8", "nlsh_sq8_train"};
constexpr unsigned bit(Entry e) { return 1u << e; }
constexpr unsigned GATHERS = bit(GATHER) | bit(GATHER_TYPED) | bit(GATHER_SQ8), UPDATES = bit(UPDATE) | bit(UPDATE_TYPED) | bit(UPDATE_SQ8);
constexpr unsigned G_STORED = bit(GATHER_TYPED) | bit(GATHER_SQ8), U_STORED = bit(UPDATE_TYPED) | bit(UPDATE_SQ8), SQ8 = bit(GATHER_SQ8) | bit(UPDATE_SQ8);
constexpr unsigned PLAIN_TYPED = bit(UPDATE) | bit(UPDATE_TYPED);

#define F32P(p) ((const float *)(p))
#define I32P(p) ((const int32_t *)(p))
#define U8P(p) ((const uint8_t *)(p))
#define UPDATE_OLD(a) a.row_stride, a.d, I32P(a.gid), F32P(a.inv_norm), I32P(a.uniq_keys), I32P(a.offsets), a.n_old, a.n_buckets_old, U8P(a.keep), a.n_kept
#define UPDATE_NEW(a) a.new_stride, I32P(a.keys_new), I32P(a.ids_new), a.m_new
#define UPDATE_OUT(a) a.stride_out, (int32_t *)a.gid_out, (float *)a.inv_norm_out, (int32_t *)a.src_out, (int32_t *)a.uniq_out, (int32_t *)a.offsets_out, \
                      (int32_t *)a.n_buckets_out

int call(Entry e, const Args &a) {
    size_t need = e == TRAIN ? nlsh_sq8_train_workspace(a.n, a.d) : e >= UPDATE ? nlsh_csr_update_workspace(a.n_old, a.n_buckets_old, a.m_new) : 0;
    if (need == 0) need = 1 << 20;
    const size_t ws_bytes = a.workspace_bytes == -1 ? need : a.workspace_bytes == -2 ? need - 1 : (size_t)a.workspace_bytes;
    switch (e) {
    case GATHER:
        return nlsh_gather_rows(F32P(a.corpus), a.src_stride, a.d, I32P(a.perm), a.n, (float *)a.sorted, a.dst_stride, (float *)a.g_inv_norm, (int32_t *)a.g_gid, 0,
                                nullptr);
    case GATHER_TYPED:
        return nlsh_gather_rows_typed(a.corpus, a.src_storage, a.src_stride, a.d, I32P(a.perm), a.n, a.sorted, a.dst_storage, a.dst_stride, (float *)a.g_inv_norm,
                                      (int32_t *)a.g_gid, 0, (int32_t *)a.first_bad, nullptr);
    case GATHER_SQ8:
        return nlsh_gather_rows_sq8(a.corpus, a.src_storage, a.src_stride, a.d, I32P(a.perm), a.n, (uint8_t *)a.sorted, a.dst_stride, F32P(a.lo), F32P(a.step),
                                    (float *)a.g_inv_norm, (int32_t *)a.g_gid, 0, (int32_t *)a.first_bad, (int32_t *)a.clamped_rows, nullptr);
    case UPDATE:
        return nlsh_csr_update(F32P(a.corpus_sorted), UPDATE_OLD(a), F32P(a.rows_new), UPDATE_NEW(a), (float *)a.sorted_out, UPDATE_OUT(a), a.workspace, ws_bytes,
                               nullptr);
    case UPDATE_TYPED:
        return nlsh_csr_update_typed(a.corpus_sorted, a.storage, UPDATE_OLD(a), a.rows_new, a.new_storage, UPDATE_NEW(a), a.sorted_out, UPDATE_OUT(a),
                                     (int32_t *)a.first_bad, a.workspace, ws_bytes, nullptr);
    case UPDATE_SQ8:
        return nlsh_csr_update_sq8(U8P(a.corpus_sorted), F32P(a.lo), F32P(a.step), UPDATE_OLD(a), a.rows_new, a.new_storage, UPDATE_NEW(a), (uint8_t *)a.sorted_out,
                                   UPDATE_OUT(a), (int32_t *)a.first_bad, (int32_t *)a.clamped_rows, a.workspace, ws_bytes, nullptr);
    default:
        return nlsh_sq8_train(a.corpus, a.src_storage, a.src_stride, a.d, a.n, (float *)a.lo, (float *)a.step, a.dst_stride, (int32_t *)a.first_bad, a.workspace,
                              ws_bytes, nullptr);
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
    const int INV = NLSH_E_INVALID;
    const unsigned TR = bit(TRAIN);
    std::vector<Fault> faults = {
        {"source storage", [](Args &a) { a.src_storage = 7; }, "storage=7", G_STORED | TR, INV},
        {"destination storage", [](Args &a) { a.dst_storage = 7; }, "dst_storage=7", bit(GATHER_TYPED), INV},
        {"destination storage: sq8 has entries of its own", [](Args &a) { a.dst_storage = 3; }, "dst_storage=3", bit(GATHER_TYPED), INV},
        {"new rows' storage", [](Args &a) { a.new_storage = 7; }, "new_storage=7", U_STORED, INV},
        {"index storage", [](Args &a) { a.storage = 7; }, "storage=7", bit(UPDATE_TYPED), INV},
        {"training on codes", [](Args &a) { a.src_storage = NLSH_STORE_U8; }, "storage=2", TR, INV},
        {"d = 0", [](Args &a) { a.d = 0; }, "d=0", GATHERS | UPDATES | TR, INV},
        {"d > MAX_DIM", [](Args &a) { a.d = NLSH_MAX_DIM + 1; }, "d=1025", GATHERS | UPDATES | TR, INV},
        {"n negative", [](Args &a) { a.n = -1; }, "n=-1", GATHERS | TR, INV},
        {"n_old negative", [](Args &a) { a.n_old = -1; }, "n_old=-1", UPDATES, INV},
        {"n_old = 2^31", [](Args &a) { a.n_old = 1ll << 31; }, "n_old=2147483648", UPDATES, INV},
        {"m_new negative", [](Args &a) { a.m_new = -1; }, "m_new=-1", UPDATES, INV},
        {"n_kept negative", [](Args &a) { a.n_kept = -1; }, "n_kept=-1", UPDATES, INV},
        {"n_kept > n_old", [](Args &a) { a.n_kept = 1001; }, "n_kept=1001", UPDATES, INV},
        {"null keep, n_kept != n_old", [](Args &a) { a.keep = nullptr; }, "keep is null", UPDATES, INV},
        {"n_buckets_old negative", [](Args &a) { a.n_buckets_old = -1; }, "n_buckets_old=-1", UPDATES, INV},
        {"rows without a bucket", [](Args &a) { a.n_buckets_old = 0; }, "n_buckets_old=0", UPDATES, INV},
        {"dst_stride < d", [](Args &a) { a.dst_stride = 96; }, "dst_stride=96", GATHERS, INV},
        {"quant_stride < d", [](Args &a) { a.dst_stride = 96; }, "quant_stride=96", TR, INV},
        {"src_stride < d", [](Args &a) { a.src_stride = 99; }, "src_stride", GATHERS, INV},
        {"training: row_stride < d", [](Args &a) { a.src_stride = 99; }, "row_stride=99", TR, INV},
        {"row_stride < d", [](Args &a) { a.row_stride = 96; }, "row_stride=96", PLAIN_TYPED, INV},
        {"stride_out < d", [](Args &a) { a.stride_out = 96; }, "stride_out=96", PLAIN_TYPED, INV},
        {"stride_out < d, sq8", [](Args &a) { a.stride_out = 96; }, "row_stride=112 != stride_out=96", bit(UPDATE_SQ8), INV},
        {"both pitches < d, sq8", [](Args &a) { a.row_stride = a.stride_out = 96; }, "row_stride=96", bit(UPDATE_SQ8), INV},
        {"new_stride < d", [](Args &a) { a.new_stride = 99; }, "new_stride=99", UPDATES, INV},
        {"pitch, float32 rows", [](Args &a) { a.dst_stride = 102; }, "multiple of 4", bit(GATHER), INV},
        {"pitch, to float32", [](Args &a) { a.dst_storage = NLSH_STORE_F32; a.src_storage = NLSH_STORE_F16; a.dst_stride = 102; }, "multiple of 4", bit(GATHER_TYPED), INV},
        {"pitch, to float16", [](Args &a) { a.dst_stride = 100; }, "multiple of 8", bit(GATHER_TYPED), INV},
        {"pitch, to uint8", [](Args &a) { a.dst_storage = NLSH_STORE_U8; a.dst_stride = 104; }, "multiple of 16", bit(GATHER_TYPED), INV},
        {"pitch, to sq8", [](Args &a) { a.dst_stride = 104; }, "multiple of 16", bit(GATHER_SQ8), INV},
        {"old pitch, float32 index", [](Args &a) { a.row_stride = 102; }, "multiple of 4", bit(UPDATE), INV},
        {"new pitch, float32 index", [](Args &a) { a.stride_out = 102; }, "multiple of 4", bit(UPDATE), INV},
        {"old pitch, float16 index", [](Args &a) { a.row_stride = 100; }, "multiple of 8", bit(UPDATE_TYPED), INV},
        {"new pitch, float16 index", [](Args &a) { a.stride_out = 100; }, "multiple of 8", bit(UPDATE_TYPED), INV},
        {"old pitch, uint8 index", [](Args &a) { a.storage = NLSH_STORE_U8; a.row_stride = 104; }, "multiple of 16", bit(UPDATE_TYPED), INV},
        {"new pitch, uint8 index", [](Args &a) { a.storage = NLSH_STORE_U8; a.stride_out = 104; }, "multiple of 16", bit(UPDATE_TYPED), INV},
        {"old pitch, float32 typed index", [](Args &a) { a.storage = NLSH_STORE_F32; a.new_storage = NLSH_STORE_F16; a.row_stride = 102; }, "multiple of 4",
         bit(UPDATE_TYPED), INV},
        {"pitches, sq8 index", [](Args &a) { a.row_stride = a.stride_out = 104; }, "multiple of 16", bit(UPDATE_SQ8), INV},
        {"unequal sq8 pitches", [](Args &a) { a.stride_out = 128; }, "ONE pitch", bit(UPDATE_SQ8), INV},
        {"null corpus", [](Args &a) { a.corpus = nullptr; }, "null", GATHERS | TR, INV},
        {"null perm", [](Args &a) { a.perm = nullptr; }, "null", GATHERS, INV},
        {"null sorted", [](Args &a) { a.sorted = nullptr; }, "null", GATHERS, INV},
        {"null lo", [](Args &a) { a.lo = nullptr; }, "null", SQ8 | TR, INV},
        {"null step", [](Args &a) { a.step = nullptr; }, "null", SQ8 | TR, INV},
        {"null first_bad on a converting call", [](Args &a) { a.first_bad = nullptr; }, "first_bad", G_STORED | U_STORED | TR, INV},
        {"null corpus_sorted", [](Args &a) { a.corpus_sorted = nullptr; }, "corpus_sorted", UPDATES, INV},
        {"null gid", [](Args &a) { a.gid = nullptr; }, "gid", UPDATES, INV},
        {"null uniq_keys", [](Args &a) { a.uniq_keys = nullptr; }, "uniq_keys", UPDATES, INV},
        {"null offsets", [](Args &a) { a.offsets = nullptr; }, "offsets", UPDATES, INV},
        {"null rows_new", [](Args &a) { a.rows_new = nullptr; }, "rows_new", UPDATES, INV},
        {"null keys_new", [](Args &a) { a.keys_new = nullptr; }, "keys_new", UPDATES, INV},
        {"null ids_new", [](Args &a) { a.ids_new = nullptr; }, "ids_new", UPDATES, INV},
        {"null sorted_out", [](Args &a) { a.sorted_out = nullptr; }, "sorted_out", UPDATES, INV},
        {"null gid_out", [](Args &a) { a.gid_out = nullptr; }, "gid_out", UPDATES, INV},
        {"null src_out", [](Args &a) { a.src_out = nullptr; }, "src_out", UPDATES, INV},
        {"null uniq_out", [](Args &a) { a.uniq_out = nullptr; }, "uniq_out", UPDATES, INV},
        {"null offsets_out", [](Args &a) { a.offsets_out = nullptr; }, "offsets_out", UPDATES, INV},
        {"null n_buckets_out", [](Args &a) { a.n_buckets_out = nullptr; }, "n_buckets_out", UPDATES, INV},
        {"null workspace", [](Args &a) { a.workspace = nullptr; }, "workspace", UPDATES | TR, INV},
        {"null inv_norm of the kept rows", [](Args &a) { a.inv_norm = nullptr; }, "inv_norm", UPDATES, INV},
        {"sorted misaligned", [](Args &a) { a.sorted = off(4); }, "16-byte aligned", GATHERS, INV},
        {"corpus_sorted misaligned", [](Args &a) { a.corpus_sorted = off(4); }, "16-byte aligned", UPDATES, INV},
        {"sorted_out misaligned", [](Args &a) { a.sorted_out = off(4); }, "16-byte aligned", UPDATES, INV},
        {"workspace misaligned", [](Args &a) { a.workspace = off(4); }, "16-byte aligned", UPDATES | TR, INV},
        {"lo misaligned", [](Args &a) { a.lo = off(4); }, "lo and step must be 16-byte aligned", SQ8, INV},
        {"step misaligned", [](Args &a) { a.step = off(4); }, "lo and step must be 16-byte aligned", SQ8, INV},
        {"float32 source off its element", [](Args &a) { a.corpus = off(2); }, "element size", G_STORED | TR, INV},
        {"float16 source off its element", [](Args &a) { a.corpus = off(1); a.src_storage = NLSH_STORE_F16; }, "element size", G_STORED | TR, INV},
        // entries that disagree: a short workspace is NLSH_E_INVALID for an update and NLSH_E_WORKSPACE for the training call
        {"short workspace", [](Args &a) { a.workspace_bytes = -2; }, "workspace_bytes", UPDATES, INV},
        {"no workspace", [](Args &a) { a.workspace_bytes = 0; }, "workspace_bytes", UPDATES, INV},
        {"short workspace, training", [](Args &a) { a.workspace_bytes = 16; }, "workspace 16", TR, NLSH_E_WORKSPACE},
    };
    int calls = 0;
    for (int e = 0; e < N_ENTRIES; ++e) {
        for (const Fault &f : faults) {
            if (!(f.entries & bit((Entry)e))) continue;
            Args a;
            f.make(a);
            expect((Entry)e, f.name, a, f.code, f.fragment);
            ++calls;
        }
        if (bit((Entry)e) & GATHERS) {   // no rows: valid without its pointers (codes to codes: nothing to report, no flag to clear)
            Args empty;
            empty.n = 0; empty.src_storage = empty.dst_storage = NLSH_STORE_U8;
            empty.corpus = empty.perm = empty.sorted = empty.lo = empty.step = empty.g_inv_norm = empty.g_gid = empty.first_bad = empty.clamped_rows = nullptr;
            expect((Entry)e, "no rows", empty, NLSH_OK, nullptr);
        }
    }
    printf("%d refused calls over %d entry points, %d failures\n", calls, (int)N_ENTRIES, failures);
    return failures ? 1 : 0;
}
