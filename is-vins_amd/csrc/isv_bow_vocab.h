// isv_bow_vocab.h -- host only (plain C++17, no HIP): parser and validator of the vocabulary file of include/isvins_bow.h
// (VINSLoop::Vocabulary::deserialize, thirdparty/VocabularyBinary.cpp; the tree of TemplatedVocabulary::loadBin,
// thirdparty/DBoW/TemplatedVocabulary.h:1509-1561), and the breadth-first layout the kernels descend: node 0 is the root, every
// node's children are contiguous and in the order of their records in the file.  Every read is bounds-checked against the image's
// length before it happens; nothing is allocated from a count the length has not confirmed.
// tests/native/bow_vocab_sanitize.cpp runs it under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/isvins_bow.h"

struct BowVocab {
    isv_bow_vocab_info_t info{};
    // breadth-first arrays, [n_nodes + 1]
    std::vector<int32_t> first_child, n_children, word_id;   // word_id: -1 for an inner node
    std::vector<double> weight;
    std::vector<uint64_t> desc;                              // [n_nodes + 1][4] (the root's is zero and never read)
};

namespace bow_vocab_detail {
constexpr size_t kHeader = 24, kNode = 48, kWord = 8;
inline int32_t rd_i32(const unsigned char *p) { int32_t v; memcpy(&v, p, 4); return v; }
inline double rd_f64(const unsigned char *p) { double v; memcpy(&v, p, 8); return v; }
inline uint64_t rd_u64(const unsigned char *p) { uint64_t v; memcpy(&v, p, 8); return v; }
}  // namespace bow_vocab_detail

// ISV_OK, ISV_ERR_INPUT, ISV_ERR_UNSUPPORTED or ISV_ERR_INVALID_ARG; `out` (may be null) is filled on ISV_OK only
inline int bow_vocab_parse(const void *bytes, size_t n, BowVocab *out) {
    using namespace bow_vocab_detail;
    if (!bytes) return ISV_ERR_INVALID_ARG;
    const unsigned char *p = (const unsigned char *)bytes;
    if (n < kHeader) return ISV_ERR_INPUT;
    const int32_t k = rd_i32(p), L = rd_i32(p + 4), scoring = rd_i32(p + 8), weighting = rd_i32(p + 12);
    const int32_t nn = rd_i32(p + 16), nw = rd_i32(p + 20);
    if (nn <= 0 || nw <= 0) return ISV_ERR_INPUT;
    if (n != kHeader + kNode * (uint64_t)nn + kWord * (uint64_t)nw) return ISV_ERR_INPUT;   // short or over-long
    if (weighting != 0 || scoring != 0) return ISV_ERR_UNSUPPORTED;                          // TF_IDF with L1_NORM only
    const unsigned char *nodes = p + kHeader, *words = nodes + kNode * (size_t)nn;
    const size_t N = (size_t)nn + 1;
    // file ids: record of every node, its parent, the number of its children
    std::vector<int32_t> rec(N, -1), parent(N, 0), nch(N, 0);
    for (int32_t i = 0; i < nn; i++) {
        const unsigned char *r = nodes + kNode * (size_t)i;
        const int32_t id = rd_i32(r), pid = rd_i32(r + 4);
        const double w = rd_f64(r + 8);
        if (id < 1 || id > nn || pid < 0 || pid > nn || rec[id] >= 0) return ISV_ERR_INPUT;
        if (!std::isfinite(w) || w < 0) return ISV_ERR_INPUT;
        rec[id] = i; parent[id] = pid; nch[pid]++;
    }
    // children lists in record order (a counting sort by parent)
    std::vector<int32_t> start(N + 1, 0), fill(N, 0), child(nn);
    for (size_t v = 0; v < N; v++) start[v + 1] = start[v] + nch[v];
    for (int32_t i = 0; i < nn; i++) {
        const int32_t id = rd_i32(nodes + kNode * (size_t)i), pid = parent[id];
        child[start[pid] + fill[pid]++] = id;
    }
    // breadth-first from the root: bfs[j] is the file id of breadth-first node j.  A node on a cycle or below one is never reached.
    std::vector<int32_t> bfs, depth(N, 0), pos(N, -1);
    bfs.reserve(N);
    bfs.push_back(0); pos[0] = 0;
    int32_t max_depth = 0, n_leaves = 0;
    for (size_t j = 0; j < bfs.size(); j++) {
        const int32_t v = bfs[j];
        if (nch[v] == 0) { n_leaves++; if (depth[v] > max_depth) max_depth = depth[v]; }
        for (int32_t c = start[v]; c < start[v + 1]; c++) {
            const int32_t u = child[c];
            if (pos[u] >= 0) return ISV_ERR_INPUT;             // (cannot happen with one parent per node; kept as a guard)
            pos[u] = (int32_t)bfs.size(); depth[u] = depth[v] + 1;
            bfs.push_back(u);
        }
    }
    if (bfs.size() != N) return ISV_ERR_INPUT;
    // words: a leaf each, every leaf exactly once, word ids a permutation of [0, nWords)
    std::vector<int32_t> word_of(N, -1);
    std::vector<char> seen(nw, 0);
    for (int32_t i = 0; i < nw; i++) {
        const unsigned char *r = words + kWord * (size_t)i;
        const int32_t id = rd_i32(r), wid = rd_i32(r + 4);
        if (id < 1 || id > nn || wid < 0 || wid >= nw) return ISV_ERR_INPUT;
        if (nch[id] != 0 || word_of[id] >= 0 || seen[wid]) return ISV_ERR_INPUT;
        word_of[id] = wid; seen[wid] = 1;
    }
    if (n_leaves != nw) return ISV_ERR_INPUT;                  // a leaf without a word
    int32_t n_stop = 0;
    for (size_t v = 1; v < N; v++)
        if (nch[v] == 0 && rd_f64(nodes + kNode * (size_t)rec[v] + 8) == 0.0) n_stop++;
    if (!out) return ISV_OK;
    out->info = isv_bow_vocab_info_t{k, L, nn, nw, n_leaves, max_depth, n_stop, 0};
    out->first_child.assign(N, 0); out->n_children.assign(N, 0); out->word_id.assign(N, -1);
    out->weight.assign(N, 0.0); out->desc.assign(4 * N, 0);
    for (size_t j = 0; j < N; j++) {
        const int32_t v = bfs[j];
        out->n_children[j] = nch[v];
        out->first_child[j] = nch[v] ? pos[child[start[v]]] : 0;   // children were appended to bfs together, in record order
        if (v == 0) continue;
        const unsigned char *r = nodes + kNode * (size_t)rec[v];
        out->word_id[j] = word_of[v];
        out->weight[j] = rd_f64(r + 8);
        for (int w = 0; w < 4; w++) out->desc[4 * j + w] = rd_u64(r + 16 + 8 * w);
    }
    return ISV_OK;
}
