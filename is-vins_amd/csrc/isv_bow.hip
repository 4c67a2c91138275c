// isv_bow.hip -- batched loop detection: PoseGraph::detectLoop / addKeyFrameIntoVoc for S sequences in lock step, one DBoW
// database per sequence (include/isvins_bow.h has the contract, the reference lines, the arithmetic, the quirks B1..B4 and the
// deviation; tests/native/isv_bow_oracle.c is the serial restatement the kernels are pinned to, bit for bit).  One packed upload,
// four kernels, one download (isv_stage_launch.h).  FP64, contraction off, no atomics: every sum has one fixed order.
//
// k_bow_transform: one workgroup of four wavefronts per item.  A lane per feature descends the vocabulary, which lies on the
// device breadth-first with a node's children contiguous in file order and the descriptors as two 16-byte planes (128-bit
// loads); the first of equal minima wins (strict <).  The word ids (stop words as a sentinel that sorts last) are sorted in LDS
// by a bitonic network, wavefront 0 finds the run heads and compacts them in word order by a ballot prefix, a head's lane adds
// the word's weight once per occurrence, and the norm is summed in ascending word id (the values pass through the wavefront by
// shuffles, every lane forms the same sum).  Then all lanes divide.
// k_bow_score: a workgroup per (item, block of kEntriesPerBlock entries), a wavefront per eligible entry: lanes stride over the
// entry's words, binary-search the query vector (in LDS where 12 B x max_features fit 64 KiB, else in global memory), and the
// hits' terms are added in word order by walking the ballot mask.  An entry without a common word is marked absent.
// k_bow_select: a wavefront per item: the max_results smallest (raw, id) keys by repeated wave-wide minimum, then detectLoop's
// decision on lane 0.
// k_bow_append: the vector to the database's tail (CSR: entry pointers, uint32 words, double weights), after every query of the
// call has been scored.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "isv_stage_launch.h"
#include "isv_bow_vocab.h"

namespace {

constexpr int kLanes = 64;
constexpr int kThreads = 256, kWaves = kThreads / kLanes;
constexpr int kEntriesPerBlock = 32;
constexpr uint32_t kStop = 0xFFFFFFFFu;        // a stop word's key: sorts behind every word id
constexpr size_t kLdsLimit = 64 * 1024;

struct BwDb {                     // one database: the forward index of its entries, CSR
    uint32_t *eptr = nullptr;     // [cap_e + 1], eptr[0] = 0
    uint32_t *words = nullptr;    // [cap_w]
    double *vals = nullptr;       // [cap_w]
    int32_t n_entries = 0, cap_e = 0;
    uint64_t used = 0, cap_w = 0;
};

struct BwVocabDev {               // device pointers into the vocabulary block
    const int32_t *first_child, *n_children, *word_id;
    const double *weight, *word_weight;
    const ulonglong2 *da, *db;    // words 0 1 / words 2 3 of the nodes' descriptors
};

struct BwHdr {                    // host-packed per-item record
    int32_t status, mode, frame_index, nf;
    int32_t f_off;                // the item's first feature in the call's feature array; also its vector's place
    int32_t n_entries;            // of its database before the call
    int32_t s_off;                // the item's first raw score
    int32_t pad;
    uint32_t *eptr, *ewords;
    double *evals;
};

struct BwParams {
    int32_t max_results, min_gap;
    double neighbour_score, loop_score;
};

}  // namespace

struct isv_bow : StageHandle {
    isv_bow_config_t cfg;
    void *d_vocab = nullptr;
    BwVocabDev vocab{};
    isv_bow_vocab_info_t info{};
    std::vector<BwDb> dbs;
};

__global__ void __launch_bounds__(kThreads) k_bow_transform(const BwHdr *__restrict__ hdrs, const BwVocabDev V, const uint64_t *__restrict__ feats,
                                                            uint32_t *__restrict__ vec_w, double *__restrict__ vec_v,
                                                            isv_bow_result_t *__restrict__ results) {
    extern __shared__ uint32_t keys[];            // [the power of two >= max_features]
    __shared__ double s_norm;
    __shared__ int s_count;
    const BwHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_BOW_OK) return;
    const int t = threadIdx.x, lane = t & (kLanes - 1);
    const int nf = H.nf;
    int P = kLanes;
    while (P < nf) P <<= 1;
    const uint64_t *F = feats + 4 * (size_t)H.f_off;
    for (int i = t; i < P; i += kThreads) {
        uint32_t key = kStop;
        if (i < nf) {
            const uint64_t f0 = F[4 * (size_t)i], f1 = F[4 * (size_t)i + 1], f2 = F[4 * (size_t)i + 2], f3 = F[4 * (size_t)i + 3];
            int node = 0;
            do {   // TemplatedVocabulary.h:1231-1253
                const int fc = V.first_child[node], nc = V.n_children[node];
                int best = fc, best_d = 257;
                for (int c = 0; c < nc; c++) {
                    const ulonglong2 a = V.da[fc + c], b = V.db[fc + c];
                    const int d = __popcll(a.x ^ f0) + __popcll(a.y ^ f1) + __popcll(b.x ^ f2) + __popcll(b.y ^ f3);
                    if (d < best_d) { best_d = d; best = fc + c; }   // strict <: the first of equal minima
                }
                node = best;
            } while (V.n_children[node] != 0);
            key = V.weight[node] > 0 ? (uint32_t)V.word_id[node] : kStop;   // :1092, w > 0
        }
        keys[i] = key;
    }
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = t; i < P; i += kThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
                }
            }
        }
    __syncthreads();
    uint32_t *vw = vec_w + H.f_off;
    double *vv = vec_v + H.f_off;
    if (t < kLanes) {
        const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        int count = 0;
        for (int b = 0; b < nf; b += kLanes) {
            const int i = b + lane;
            uint32_t key = kStop;
            bool head = false;
            if (i < nf) {
                key = keys[i];
                head = key != kStop && (i == 0 || keys[i - 1] != key);
            }
            const unsigned long long bal = __ballot(head);
            if (head) {
                int lo = i + 1, hi = nf;              // the end of the run
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (keys[mid] <= key) lo = mid + 1; else hi = mid;
                }
                const int c = lo - i;
                const double w = V.word_weight[key];
                double v = w;                         // BowVector::addWeight: w once per occurrence
                for (int r = 1; r < c; r++) v += w;
                const int pos = count + __popcll(bal & lt);
                vw[pos] = key; vv[pos] = v;
            }
            count += __popcll(bal);
        }
        __threadfence_block();
        double norm = 0.0;                            // BowVector::normalize, L1: ascending word id
        for (int b = 0; b < count; b += kLanes) {
            const double x = b + lane < count ? vv[b + lane] : 0.0;
            const int m = min(kLanes, count - b);
            for (int j = 0; j < m; j++) norm += fabs(__shfl(x, j));
        }
        if (lane == 0) { s_norm = norm; s_count = count; results[blockIdx.x].n_words = count; }
    }
    __syncthreads();
    const double norm = s_norm;
    const int count = s_count;
    if (norm > 0.0)
        for (int i = t; i < count; i += kThreads) vv[i] = vv[i] / norm;
}

template <bool LDSQ>
__global__ void __launch_bounds__(kThreads) k_bow_score(const BwHdr *__restrict__ hdrs, const uint32_t *__restrict__ vec_w,
                                                        const double *__restrict__ vec_v, const isv_bow_result_t *__restrict__ results,
                                                        double *__restrict__ raw, int min_gap, int qcap) {
    extern __shared__ double lds_q[];             // LDSQ: [qcap] values, then [qcap] word ids
    const BwHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_BOW_OK || H.mode == ISV_BOW_ADD) return;
    const int ne = H.n_entries, e0 = blockIdx.y * kEntriesPerBlock;
    if (e0 >= ne) return;
    const int t = threadIdx.x, lane = t & (kLanes - 1), wv = t / kLanes;
    const int nq = results[blockIdx.x].n_words;
    const uint32_t *qw = vec_w + H.f_off;
    const double *qv = vec_v + H.f_off;
    if (LDSQ) {
        double *lv = lds_q;
        uint32_t *lw = (uint32_t *)(lds_q + qcap);
        for (int i = t; i < nq; i += kThreads) { lv[i] = qv[i]; lw[i] = qw[i]; }
        __syncthreads();
        qw = lw; qv = lv;
    }
    const int max_id = H.frame_index - min_gap;
    const int e1 = min(e0 + kEntriesPerBlock, ne);
    for (int e = e0 + wv; e < e1; e += kWaves) {
        // TemplatedDatabase.h:679.  B1: max_id == -1 reads as "no limit".  B2: the newest entry is always eligible.
        const bool eligible = e < max_id || max_id == -1 || e == ne - 1;
        double s = 0.0;
        bool any = false;
        if (eligible && nq > 0) {
            const uint32_t lo = H.eptr[e], hi = H.eptr[e + 1];
            for (uint32_t b = lo; b < hi; b += kLanes) {
                const uint32_t i = b + lane;
                bool hit = false;
                double term = 0.0;
                if (i < hi) {
                    const uint32_t dw = H.ewords[i];
                    int l = 0, r = nq;
                    while (l < r) {
                        const int mid = (l + r) >> 1;
                        if (qw[mid] < dw) l = mid + 1; else r = mid;
                    }
                    if (l < nq && qw[l] == dw) {
                        const double q = qv[l], d = H.evals[i];
                        term = fabs(q - d) - fabs(q) - fabs(d);    // :681
                        hit = true;
                    }
                }
                unsigned long long bal = __ballot(hit);
                while (bal) {                                       // ascending lane = ascending word id
                    const int j = __ffsll((long long)bal) - 1;
                    bal &= bal - 1;
                    const double x = __shfl(term, j);
                    if (any) s += x; else { s = x; any = true; }
                }
            }
        }
        if (lane == 0) raw[(size_t)H.s_off + e] = any ? s : INFINITY;   // absent, not zero
    }
}

__global__ void __launch_bounds__(kLanes) k_bow_select(const BwHdr *__restrict__ hdrs, const double *__restrict__ raw,
                                                       isv_bow_result_t *__restrict__ results, const BwParams P) {
    __shared__ int s_id[ISV_BOW_MAX_RESULTS];
    __shared__ double s_sc[ISV_BOW_MAX_RESULTS];
    const BwHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_BOW_OK) return;
    const int lane = threadIdx.x;
    const bool has_query = H.mode != ISV_BOW_ADD;
    const int ne = has_query ? H.n_entries : 0;
    const double *rw = raw + (size_t)H.s_off;
    int n_scored = 0;
    for (int b = 0; b < ne; b += kLanes) {
        const int e = b + lane;
        n_scored += __popcll(__ballot(e < ne && rw[e] != INFINITY));
    }
    if (lane < ISV_BOW_MAX_RESULTS) { s_id[lane] = -1; s_sc[lane] = 0.0; }
    __syncthreads();
    int n_res = 0;
    double prev_raw = -INFINITY;
    int prev_id = -1;
    for (int r = 0; r < P.max_results; r++) {
        double br = INFINITY;
        int bi = INT32_MAX;
        for (int e = lane; e < ne; e += kLanes) {
            const double x = rw[e];
            if (x == INFINITY) continue;
            if (!(x > prev_raw || (x == prev_raw && e > prev_id))) continue;   // already taken
            if (x < br || (x == br && e < bi)) { br = x; bi = e; }             // the deviation: of equal scores the lower id first
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double orw = __shfl_xor(br, off);
            const int oi = __shfl_xor(bi, off);
            if (orw < br || (orw == br && oi < bi)) { br = orw; bi = oi; }
        }
        if (bi == INT32_MAX) break;
        if (lane == 0) { s_id[r] = bi; s_sc[r] = -br / 2.0; }                  // :722
        prev_raw = br; prev_id = bi;
        n_res++;
    }
    __syncthreads();
    if (lane != 0) return;
    isv_bow_result_t &R = results[blockIdx.x];
    // pose_graph.cpp:181-216
    bool find_loop = false;
    if (n_res >= 1 && s_sc[0] > P.neighbour_score)
        for (int i = 1; i < n_res; i++)
            if (s_sc[i] > P.loop_score) find_loop = true;
    int loop_index = -1;
    if (find_loop && H.frame_index > P.min_gap) {     // B4: the gate comes after the query and the add
        int min_index = -1;
        for (int i = 0; i < n_res; i++)
            if (min_index == -1 || (s_id[i] < min_index && s_sc[i] > P.loop_score)) min_index = s_id[i];   // B3: ret[0] whatever its score
        loop_index = min_index;
    }
    R.status = ISV_BOW_OK;
    R.entry_id = H.mode != ISV_BOW_QUERY ? H.n_entries : -1;
    R.n_scored = n_scored;
    R.n_results = n_res;
    R.find_loop = find_loop ? 1 : 0;
    R.loop_index = loop_index;
    R._pad = 0;
    for (int i = 0; i < ISV_BOW_MAX_RESULTS; i++) { R.result_id[i] = s_id[i]; R.result_score[i] = s_sc[i]; }
}

__global__ void __launch_bounds__(kThreads) k_bow_append(const BwHdr *__restrict__ hdrs, const uint32_t *__restrict__ vec_w,
                                                         const double *__restrict__ vec_v, const isv_bow_result_t *__restrict__ results) {
    const BwHdr &H = hdrs[blockIdx.x];
    if (H.status != ISV_BOW_OK || H.mode == ISV_BOW_QUERY) return;
    const int nw = results[blockIdx.x].n_words;
    const uint32_t base = H.eptr[H.n_entries];
    for (int i = threadIdx.x; i < nw; i += kThreads) {
        H.ewords[base + i] = vec_w[H.f_off + i];
        H.evals[base + i] = vec_v[H.f_off + i];
    }
    if (threadIdx.x == 0) H.eptr[H.n_entries + 1] = base + (uint32_t)nw;
}

namespace {

void refuse(isv_bow_result_t &r, int status) {
    memset(&r, 0, sizeof(r));
    r.status = status; r.entry_id = -1; r.loop_index = -1;
    for (int i = 0; i < ISV_BOW_MAX_RESULTS; i++) r.result_id[i] = -1;
}

int read_file(const char *path, std::vector<char> &buf) {
    FILE *f = fopen(path, "rb");
    if (!f) return ISV_ERR_INVALID_ARG;
    char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    return bad ? ISV_ERR_INVALID_ARG : ISV_OK;
}

void db_free(BwDb &d) {
    if (d.eptr) (void)hipFree(d.eptr);
    if (d.words) (void)hipFree(d.words);
    if (d.vals) (void)hipFree(d.vals);
    d = BwDb{};
}

// storage for cap_e entries and cap_w words; on failure nothing is kept
hipError_t db_alloc(BwDb &d, int32_t cap_e, uint64_t cap_w) {
    d = BwDb{};
    hipError_t e = hipMalloc(&d.eptr, sizeof(uint32_t) * ((size_t)cap_e + 1));
    if (e == hipSuccess) e = hipMalloc(&d.words, sizeof(uint32_t) * cap_w);
    if (e == hipSuccess) e = hipMalloc(&d.vals, sizeof(double) * cap_w);
    if (e != hipSuccess) { db_free(d); return e; }
    d.cap_e = cap_e; d.cap_w = cap_w;
    return hipSuccess;
}

}  // namespace

extern "C" int isv_bow_vocab_check(const void *bytes, size_t n, isv_bow_vocab_info_t *info) {
    BowVocab v;
    const int rc = bow_vocab_parse(bytes, n, &v);
    if (rc == ISV_OK && info) *info = v.info;
    return rc;
}

extern "C" int isv_bow_vocab_check_file(const char *path, isv_bow_vocab_info_t *info) {
    if (!path) return ISV_ERR_INVALID_ARG;
    std::vector<char> buf;
    if (const int rc = read_file(path, buf); rc != ISV_OK) return rc;
    return isv_bow_vocab_check(buf.data(), buf.size(), info);
}

extern "C" const char *isv_bow_last_error(const isv_bow_t *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" void isv_bow_destroy(isv_bow_t *h) {
    if (!h) return;
    h->close();
    for (BwDb &d : h->dbs) db_free(d);
    if (h->d_vocab) (void)hipFree(h->d_vocab);
    delete h;
}

extern "C" int isv_bow_create(const isv_bow_config_t *c, const void *vocab_bytes, size_t n, isv_bow_t **out) {
    if (!c || !out) return ISV_ERR_INVALID_ARG;
    *out = nullptr;
    if (!vocab_bytes) return ISV_ERR_INVALID_ARG;
    if (c->max_items < 1 || c->n_databases < 1 || c->max_features < 1 || c->max_features > ISV_BOW_MAX_FEATURES || c->max_results < 1 ||
        c->max_results > ISV_BOW_MAX_RESULTS || c->min_gap < 0 || c->initial_entry_capacity < 1 || !std::isfinite(c->neighbour_score) ||
        !std::isfinite(c->loop_score))
        return ISV_ERR_INVALID_ARG;
    BowVocab v;
    if (const int rc = bow_vocab_parse(vocab_bytes, n, &v); rc != ISV_OK) return rc;
    isv_bow *h = new isv_bow();
    h->cfg = *c;
    h->info = v.info;
    hipError_t e = h->open();
    if (e == hipSuccess) {
        // the vocabulary block: [first_child | n_children | word_id | weight | word_weight | descriptor planes a, b]
        const size_t N = (size_t)v.info.n_nodes + 1, W = (size_t)v.info.n_words;
        BlockLayout L;
        const size_t o_fc = L.add(4 * N), o_nc = L.add(4 * N), o_wi = L.add(4 * N), o_wt = L.add(8 * N), o_ww = L.add(8 * W);
        const size_t o_da = L.add(16 * N), o_db = L.add(16 * N);
        std::vector<char> blk(L.end);
        memcpy(blk.data() + o_fc, v.first_child.data(), 4 * N);
        memcpy(blk.data() + o_nc, v.n_children.data(), 4 * N);
        memcpy(blk.data() + o_wi, v.word_id.data(), 4 * N);
        memcpy(blk.data() + o_wt, v.weight.data(), 8 * N);
        double *ww = (double *)(blk.data() + o_ww);
        uint64_t *da = (uint64_t *)(blk.data() + o_da), *db = (uint64_t *)(blk.data() + o_db);
        for (size_t j = 0; j < N; j++) {
            if (v.word_id[j] >= 0) ww[v.word_id[j]] = v.weight[j];
            da[2 * j] = v.desc[4 * j]; da[2 * j + 1] = v.desc[4 * j + 1];
            db[2 * j] = v.desc[4 * j + 2]; db[2 * j + 1] = v.desc[4 * j + 3];
        }
        e = hipMalloc(&h->d_vocab, L.end);
        if (e == hipSuccess) e = hipMemcpy(h->d_vocab, blk.data(), L.end, hipMemcpyHostToDevice);
        char *d = (char *)h->d_vocab;
        h->vocab = BwVocabDev{(const int32_t *)(d + o_fc), (const int32_t *)(d + o_nc), (const int32_t *)(d + o_wi), (const double *)(d + o_wt),
                              (const double *)(d + o_ww), (const ulonglong2 *)(d + o_da), (const ulonglong2 *)(d + o_db)};
    }
    if (e == hipSuccess) {
        h->dbs.resize(c->n_databases);
        const uint64_t cap_w = (uint64_t)c->initial_entry_capacity * (uint64_t)(c->max_features < 64 ? c->max_features : 64);
        for (BwDb &d : h->dbs) {
            if (e == hipSuccess) e = db_alloc(d, c->initial_entry_capacity, cap_w);
            if (e == hipSuccess) e = hipMemset(d.eptr, 0, sizeof(uint32_t));
        }
    }
    if (stage_open_failed("isv_bow_create", e)) {
        isv_bow_destroy(h);
        return ISV_ERR_DEVICE;
    }
    *out = h;
    return ISV_OK;
}

extern "C" int isv_bow_last_ms(isv_bow_t *h, double out_ms[5]) {
    if (!h || !out_ms) return ISV_ERR_INVALID_ARG;
    out_ms[0] = h->slot.call_ms;
    for (int i = 0; i < 4; i++) out_ms[1 + i] = h->slot.part_ms[i];
    return ISV_OK;
}

extern "C" int isv_bow_reset(isv_bow_t *h, int32_t db) {
    if (!h || db < 0 || db >= h->cfg.n_databases) return ISV_ERR_INVALID_ARG;
    h->dbs[db].n_entries = 0; h->dbs[db].used = 0;    // eptr[0] stays 0
    return ISV_OK;
}

extern "C" int isv_bow_entries(const isv_bow_t *h, int32_t db) {
    if (!h || db < 0 || db >= h->cfg.n_databases) return ISV_ERR_INVALID_ARG;
    return h->dbs[db].n_entries;
}

extern "C" int isv_bow_detect_batch(isv_bow_t *h, int32_t n, const isv_bow_item_t *const *items, isv_bow_result_t *results,
                                    uint32_t *const *word_ids, double *const *word_weights) {
    StageCall call{h ? h->ctx() : StageCtx{}, "isv_bow_detect_batch"};
    if (const int rc = call.enter(n, items, results); rc != ISV_OK || n == 0) return rc;
    if (n > h->cfg.max_items) return call.fail(ISV_ERR_CAPACITY, "more items than max_items");
    const isv_bow_config_t cfg = h->cfg;
    // how often a database appears, and whether by anything but a QUERY
    std::vector<int32_t> seen(cfg.n_databases, 0);
    std::vector<char> writes(cfg.n_databases, 0);
    for (int i = 0; i < n; i++) {
        const isv_bow_item_t *it = items[i];
        if (it->database < 0 || it->database >= cfg.n_databases) continue;
        seen[it->database]++;
        if (it->mode != ISV_BOW_QUERY) writes[it->database] = 1;
    }
    std::vector<BwHdr> hd(n);
    size_t n_ft = 0, n_sc = 0;
    int max_entries = 0;
    for (int i = 0; i < n; i++) {
        const isv_bow_item_t *it = items[i];
        BwHdr &H = hd[i];
        memset(&H, 0, sizeof(H));
        if (it->database < 0 || it->database >= cfg.n_databases) H.status = ISV_BOW_INPUT;
        else if (seen[it->database] > 1 && writes[it->database]) H.status = ISV_BOW_DUPLICATE;
        else if (it->mode < ISV_BOW_DETECT || it->mode > ISV_BOW_QUERY || it->n_features < 0 || (it->n_features > 0 && !it->brief)) H.status = ISV_BOW_INPUT;
        else if (it->n_features > cfg.max_features) H.status = ISV_BOW_CAPACITY;
        if (H.status != ISV_BOW_OK) continue;
        const BwDb &D = h->dbs[it->database];
        H.mode = it->mode; H.frame_index = it->frame_index; H.nf = it->n_features;
        H.f_off = (int32_t)n_ft; H.n_entries = D.n_entries; H.s_off = (int32_t)n_sc;
        n_ft += it->n_features;
        if (it->mode != ISV_BOW_ADD) { n_sc += D.n_entries; if (D.n_entries > max_entries) max_entries = D.n_entries; }
        if (n_ft > INT32_MAX || n_sc > INT32_MAX) return call.fail(ISV_ERR_CAPACITY, "batch too large");
    }
    // grow what this call appends to: every new block first, so that a failed allocation leaves every database as it was
    struct Grown { int db; BwDb fresh; };
    std::vector<Grown> grown;
    for (int i = 0; i < n; i++) {
        if (hd[i].status != ISV_BOW_OK || hd[i].mode == ISV_BOW_QUERY) continue;
        const BwDb &D = h->dbs[items[i]->database];
        int32_t cap_e = D.cap_e;
        uint64_t cap_w = D.cap_w;
        if (D.n_entries + 1 > cap_e) cap_e = cap_e > INT32_MAX / 2 ? INT32_MAX - 1 : 2 * cap_e;
        while (D.used + (uint64_t)hd[i].nf > cap_w) cap_w *= 2;
        if (cap_w > UINT32_MAX || D.n_entries + 1 > cap_e) {
            for (Grown &g : grown) db_free(g.fresh);
            return call.fail(ISV_ERR_CAPACITY, "database full");
        }
        if (cap_e == D.cap_e && cap_w == D.cap_w) continue;
        Grown g{items[i]->database, BwDb{}};
        if (const hipError_t e = db_alloc(g.fresh, cap_e, cap_w); e != hipSuccess) {
            for (Grown &o : grown) db_free(o.fresh);
            (void)hipGetLastError();
            return call.hip_fail("hipMalloc (growing a database)", e);
        }
        grown.push_back(g);
    }
    std::vector<BwDb> retired;
    for (Grown &g : grown) {
        BwDb &D = h->dbs[g.db];
        hipError_t e = hipMemcpyAsync(g.fresh.eptr, D.eptr, sizeof(uint32_t) * ((size_t)D.n_entries + 1), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && D.used) e = hipMemcpyAsync(g.fresh.words, D.words, sizeof(uint32_t) * D.used, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess && D.used) e = hipMemcpyAsync(g.fresh.vals, D.vals, sizeof(double) * D.used, hipMemcpyDeviceToDevice, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            for (Grown &o : grown)
                if (&o >= &g) db_free(o.fresh);       // (the ones before g already serve their databases, with the same content)
            for (BwDb &r : retired) db_free(r);
            return call.hip_fail("hipMemcpyAsync (growing a database)", e);
        }
        g.fresh.n_entries = D.n_entries; g.fresh.used = D.used;
        retired.push_back(D);
        D = g.fresh;
    }
    for (int i = 0; i < n; i++) {
        if (hd[i].status != ISV_BOW_OK) continue;
        const BwDb &D = h->dbs[items[i]->database];
        hd[i].eptr = D.eptr; hd[i].ewords = D.words; hd[i].evals = D.vals;
    }
    // one upload block: [headers | descriptors]; then, device only: results (zeroed before the launch), the vectors, the raw scores
    BlockLayout L;
    const size_t o_hd = L.add(sizeof(BwHdr) * n), o_ft = L.add(32 * (n_ft + 1));
    std::vector<char> up(L.end);
    const size_t o_res = L.add(sizeof(isv_bow_result_t) * n);
    const size_t clear_end = L.end;
    const size_t o_vw = L.add(4 * (n_ft + 1)), o_vv = L.add(8 * (n_ft + 1)), o_raw = L.add(8 * (n_sc + 1));
    memcpy(up.data() + o_hd, hd.data(), sizeof(BwHdr) * n);
    for (int i = 0; i < n; i++)
        if (hd[i].status == ISV_BOW_OK && hd[i].nf)
            memcpy(up.data() + o_ft + 32 * (size_t)hd[i].f_off, items[i]->brief, 32 * (size_t)hd[i].nf);
    std::vector<uint32_t> vw(word_ids ? n_ft + 1 : 0);
    std::vector<double> vv(word_weights ? n_ft + 1 : 0);
    int P = kLanes;
    while (P < cfg.max_features) P <<= 1;
    const size_t lds_q = 12 * (size_t)cfg.max_features;
    const BwParams prm{cfg.max_results, cfg.min_gap, cfg.neighbour_score, cfg.loop_score};
    const BwVocabDev V = h->vocab;
    hipStream_t stream = h->stream;
    const int rc = call.run(
        up, {{up.size(), clear_end}}, L.end,
        [&](char *d, auto &&mark) {
            const BwHdr *dh = (const BwHdr *)(d + o_hd);
            isv_bow_result_t *dr = (isv_bow_result_t *)(d + o_res);
            uint32_t *dvw = (uint32_t *)(d + o_vw);
            double *dvv = (double *)(d + o_vv), *draw = (double *)(d + o_raw);
            hipLaunchKernelGGL(k_bow_transform, dim3(n), dim3(kThreads), sizeof(uint32_t) * P, stream, dh, V, (const uint64_t *)(d + o_ft), dvw, dvv, dr);
            mark();
            if (max_entries > 0) {
                const dim3 grid(n, (max_entries + kEntriesPerBlock - 1) / kEntriesPerBlock);
                if (lds_q <= kLdsLimit)
                    hipLaunchKernelGGL(k_bow_score<true>, grid, dim3(kThreads), lds_q, stream, dh, dvw, dvv, dr, draw, (int)cfg.min_gap, (int)cfg.max_features);
                else
                    hipLaunchKernelGGL(k_bow_score<false>, grid, dim3(kThreads), 0, stream, dh, dvw, dvv, dr, draw, (int)cfg.min_gap, (int)cfg.max_features);
            }
            mark();
            hipLaunchKernelGGL(k_bow_select, dim3(n), dim3(kLanes), 0, stream, dh, draw, dr, prm);
            mark();
            hipLaunchKernelGGL(k_bow_append, dim3(n), dim3(kThreads), 0, stream, dh, dvw, dvv, dr);
        },
        {{results, o_res, sizeof(isv_bow_result_t) * n}, {word_ids ? vw.data() : nullptr, o_vw, 4 * n_ft},
         {word_weights ? vv.data() : nullptr, o_vv, 8 * n_ft}},
        [&] {
            for (int i = 0; i < n; i++) {
                const BwHdr &H = hd[i];
                if (H.status != ISV_BOW_OK) { refuse(results[i], H.status); continue; }
                const int nw = results[i].n_words;
                if (H.mode != ISV_BOW_QUERY) {
                    BwDb &D = h->dbs[items[i]->database];
                    D.n_entries++; D.used += (uint64_t)nw;
                }
                if (nw > 0 && word_ids && word_ids[i]) memcpy(word_ids[i], vw.data() + H.f_off, 4 * (size_t)nw);
                if (nw > 0 && word_weights && word_weights[i]) memcpy(word_weights[i], vv.data() + H.f_off, 8 * (size_t)nw);
            }
            return hipSuccess;
        });
    for (BwDb &r : retired) db_free(r);
    return rc;
}
