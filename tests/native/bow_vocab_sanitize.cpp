// bow_vocab_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the host-only vocabulary parser
// (is-vins_amd/csrc/isv_bow_vocab.h): a valid k=2 L=2 file, every truncation length of it, every over-long length up to 64
// bytes, every malformed case of include/isvins_bow.h, every single-byte corruption of the header and of the id fields, and a
// larger shuffled k=3 L=4 file.  Built and run as a child process by tests/test_bow_sanitize.py; prints "ok: ..." and exits 0.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>
#include "../../is-vins_amd/csrc/isv_bow_vocab.h"

namespace {

struct Node { int32_t id, parent; double weight; uint64_t desc[4]; };
struct Word { int32_t node, word; };
static_assert(sizeof(Node) == 48 && sizeof(Word) == 8, "the file's record sizes");

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

std::vector<unsigned char> pack(int32_t k, int32_t L, int32_t scoring, int32_t weighting, int32_t nn, int32_t nw, const std::vector<Node> &nodes,
                                const std::vector<Word> &words) {
    const int32_t head[6] = {k, L, scoring, weighting, nn, nw};
    std::vector<unsigned char> out(24 + 48 * nodes.size() + 8 * words.size());
    memcpy(out.data(), head, 24);
    if (!nodes.empty()) memcpy(out.data() + 24, nodes.data(), 48 * nodes.size());
    if (!words.empty()) memcpy(out.data() + 24 + 48 * nodes.size(), words.data(), 8 * words.size());
    return out;
}

// a full k-ary tree of depth L, ids level by level, random descriptors, weights on the leaves
void make_tree(int k, int L, std::vector<Node> &nodes, std::vector<Word> &words) {
    nodes.clear(); words.clear();
    std::vector<int32_t> level{0};
    int32_t next = 1;
    for (int d = 1; d <= L; d++) {
        std::vector<int32_t> below;
        for (int32_t p : level)
            for (int c = 0; c < k; c++) {
                Node n{next++, p, d == L ? 0.5 + (double)(rnd() % 1000) / 400.0 : 0.0, {rnd(), rnd(), rnd(), rnd()}};
                nodes.push_back(n); below.push_back(n.id);
            }
        level = below;
    }
    int32_t w = 0;
    for (int32_t id : level) words.push_back(Word{id, w++});
}

int g_checks = 0;
void expect(const char *what, const std::vector<unsigned char> &bytes, size_t n, int want) {
    // the parser must not read past n: hand it an exact-size heap copy, so that AddressSanitizer sees one byte too many
    unsigned char *copy = (unsigned char *)malloc(n ? n : 1);
    if (n) memcpy(copy, bytes.data(), n);
    BowVocab v;
    const int got = bow_vocab_parse(copy, n, &v);
    const int got_null = bow_vocab_parse(copy, n, nullptr);
    free(copy);
    g_checks++;
    if (got != want || got_null != want) {
        printf("FAILED: %s (length %zu): status %d / %d, expected %d\n", what, n, got, got_null, want);
        exit(1);
    }
}

}  // namespace

int main() {
    std::vector<Node> nodes;
    std::vector<Word> words;
    make_tree(2, 2, nodes, words);
    const int32_t nn = (int32_t)nodes.size(), nw = (int32_t)words.size();
    const std::vector<unsigned char> good = pack(2, 2, 0, 0, nn, nw, nodes, words);
    expect("valid", good, good.size(), ISV_OK);
    {
        BowVocab v;
        if (bow_vocab_parse(good.data(), good.size(), &v) != ISV_OK || v.info.n_nodes != 6 || v.info.n_words != 4 || v.info.n_leaves != 4 ||
            v.info.max_depth != 2 || v.first_child[0] != 1 || v.n_children[0] != 2 || v.first_child[1] != 3 || v.first_child[2] != 5) {
            printf("FAILED: the valid file's layout\n");
            return 1;
        }
    }
    for (size_t n = 0; n < good.size(); n++) expect("truncated", good, n, ISV_ERR_INPUT);
    for (size_t extra = 1; extra <= 64; extra++) {
        std::vector<unsigned char> longer = good;
        longer.resize(good.size() + extra, 0xAB);
        expect("over-long", longer, longer.size(), ISV_ERR_INPUT);
    }
    if (bow_vocab_parse(nullptr, 0, nullptr) != ISV_ERR_INVALID_ARG) return 1;
    // counts
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    for (int32_t bad : {0, -1, imin, imax, nn + 1, nn - 1}) {
        const auto f = pack(2, 2, 0, 0, bad, nw, nodes, words);
        expect("nNodes", f, f.size(), ISV_ERR_INPUT);
        const auto g = pack(2, 2, 0, 0, nn, bad == nn + 1 ? nw + 1 : bad == nn - 1 ? nw - 1 : bad, nodes, words);
        expect("nWords", g, g.size(), ISV_ERR_INPUT);
    }
    { const auto f = pack(2, 2, 0, 0, imax, imax, nodes, words); expect("huge counts", f, f.size(), ISV_ERR_INPUT); }
    // weighting / scoring
    for (int32_t t : {1, 2, 3, -1, imax}) {
        const auto f = pack(2, 2, 0, t, nn, nw, nodes, words), g = pack(2, 2, t, 0, nn, nw, nodes, words);
        expect("weighting", f, f.size(), ISV_ERR_UNSUPPORTED);
        expect("scoring", g, g.size(), ISV_ERR_UNSUPPORTED);
    }
    // ids, parents, weights
    for (int i = 0; i < nn; i++) {
        for (int32_t bad : {0, -1, nn + 1, imax, imin, nodes[(i + 1) % nn].id}) {
            auto m = nodes; m[i].id = bad;
            const auto f = pack(2, 2, 0, 0, nn, nw, m, words);
            expect("node id", f, f.size(), ISV_ERR_INPUT);
        }
        for (int32_t bad : {-1, nn + 1, imax, imin, nodes[i].id}) {
            auto m = nodes; m[i].parent = bad;
            const auto f = pack(2, 2, 0, 0, nn, nw, m, words);
            expect("parent id", f, f.size(), ISV_ERR_INPUT);
        }
        for (double bad : {-1.0, -1e-300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                           -std::numeric_limits<double>::infinity()}) {
            auto m = nodes; m[i].weight = bad;
            const auto f = pack(2, 2, 0, 0, nn, nw, m, words);
            expect("weight", f, f.size(), ISV_ERR_INPUT);
        }
    }
    { auto m = nodes; m[0].parent = 3; const auto f = pack(2, 2, 0, 0, nn, nw, m, words); expect("cycle 1 -> 3 -> 1", f, f.size(), ISV_ERR_INPUT); }
    { auto m = nodes; m[2].parent = 4; m[3].parent = 3; const auto f = pack(2, 2, 0, 0, nn, nw, m, words); expect("cycle 3 <-> 4, unreachable", f, f.size(), ISV_ERR_INPUT); }
    // words
    for (int i = 0; i < nw; i++) {
        for (int32_t bad : {0, 1, 2, -1, nn + 1, imax, imin, words[(i + 1) % nw].node}) {
            auto m = words; m[i].node = bad;
            const auto f = pack(2, 2, 0, 0, nn, nw, nodes, m);
            expect("word's node", f, f.size(), ISV_ERR_INPUT);
        }
        for (int32_t bad : {-1, nw, imax, imin, words[(i + 1) % nw].word}) {
            auto m = words; m[i].word = bad;
            const auto f = pack(2, 2, 0, 0, nn, nw, nodes, m);
            expect("word id", f, f.size(), ISV_ERR_INPUT);
        }
    }
    // every single-byte corruption of the header and of the id / parent / node / word fields: any status, no bad access
    for (size_t at = 0; at < good.size(); at++) {
        const bool in_header = at < 24, in_node = at >= 24 && at < 24 + 48 * (size_t)nn && (at - 24) % 48 < 8, in_word = at >= 24 + 48 * (size_t)nn;
        if (!in_header && !in_node && !in_word) continue;
        for (unsigned char x : {0x00, 0x01, 0x7F, 0x80, 0xFF}) {
            std::vector<unsigned char> f = good;
            f[at] = x;
            unsigned char *copy = (unsigned char *)malloc(f.size());
            memcpy(copy, f.data(), f.size());
            BowVocab v;
            (void)bow_vocab_parse(copy, f.size(), &v);
            free(copy);
            g_checks++;
        }
    }
    // a larger file with its records in a scrambled order; the layout keeps every node's children together and in record order
    make_tree(3, 4, nodes, words);
    std::vector<Node> scr(nodes.size());
    for (size_t i = 0; i < nodes.size(); i++) scr[(i * 7) % nodes.size()] = nodes[i];      // 7 is coprime with 120
    const auto big = pack(3, 4, 0, 0, (int32_t)scr.size(), (int32_t)words.size(), scr, words);
    expect("scrambled", big, big.size(), ISV_OK);
    BowVocab v;
    if (bow_vocab_parse(big.data(), big.size(), &v) != ISV_OK || v.info.n_nodes != 120 || v.info.n_words != 81 || v.info.max_depth != 4) { printf("FAILED: scrambled info\n"); return 1; }
    for (size_t j = 0; j < v.n_children.size(); j++) {
        if (v.n_children[j] != (v.word_id[j] >= 0 ? 0 : 3)) { printf("FAILED: scrambled layout\n"); return 1; }
        if (v.n_children[j] && (v.first_child[j] <= (int32_t)j || v.first_child[j] + 3 > (int32_t)v.n_children.size())) { printf("FAILED: scrambled children\n"); return 1; }
    }
    printf("ok: %d parses\n", g_checks);
    return 0;
}
