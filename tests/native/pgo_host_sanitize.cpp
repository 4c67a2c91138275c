// pgo_host_sanitize.cpp -- stand-alone AddressSanitizer / UBSan run of the host half of the pose-graph call
// (is-vins_amd/csrc/isv_pgo_host.h): the steps of isv_pgo_optimize_batch with a stand-in device, whose enqueue does nothing and
// whose drain presents the staged poses as the solved ones (zero covariances, status OK).  Small graphs at the shapes where the
// logic can go wrong and a batch of 70 mixed ones; checked: the structure against brute force from the edge list, cold / cached /
// fresh staging byte for byte, the write-back, every refusal, a failing enqueue.  Built and run as a child process by
// tests/test_pgo_host_sanitize.py (ISV_HOST_THREADS = 1 and 4); prints "ok: ..." and exits 0.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "../../is-vins_amd/csrc/isv_pgo_host.h"

namespace {

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
double unif() { return (double)(rnd() % 2000001) / 1e6 - 1.0; }       // [-1, 1]
void random_R(double *R) { h_q2R(h_qn(HQ{unif() + 1.5, unif(), unif(), unif()}), R); }

// ---- keyframe lists ---------------------------------------------------------------------------------------------------
struct Graph { std::vector<isv_pg_keyframe_t> kf; int32_t first = 0, cur = 0; int first_pos = 0, cur_pos = 0; };
constexpr double SENTINEL = 1e9;       // T_w_i before a call: the write-back has to replace it

void fill_numbers(isv_pg_keyframe_t &f) {      // (leaves what the structure depends on alone)
    for (int c = 0; c < 3; c++) { f.vio_T_w_i[c] = 5 * unif(); f.T_w_i[c] = SENTINEL; f.relative_pose.delta_t[c] = unif(); f.loop_info[c] = unif(); }
    random_R(f.vio_R_w_i); random_R(f.R_w_i); random_R(f.relative_pose.delta_R); random_R(f.rollpitch.R);
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) f.relative_pose.sqrt_info[a * 6 + b] = a == b ? 200 + 50 * unif() : 5 * unif();
    for (int a = 0; a < 2; a++) for (int b = a; b < 2; b++) f.rollpitch.sqrt_info[a * 2 + b] = a == b ? 300 + 50 * unif() : 5 * unif();
    const HQ q = h_qn(HQ{unif() + 1.5, unif(), unif(), unif()});
    f.loop_info[3] = q.w; f.loop_info[4] = q.x; f.loop_info[5] = q.y; f.loop_info[6] = q.z; f.loop_info[7] = unif();
    f.loop_weight = 40 + 20 * (unif() + 1);
}
// n keyframes, indices 10, 13, 16, ...; the first n_seq0 belong to sequence 0; loops: (keyframe, matched keyframe) list positions
Graph make_graph(int n, int first_pos, int cur_pos, int n_seq0, const std::vector<std::pair<int, int>> &loops, int rp_every = 1) {
    Graph G; G.kf.resize((size_t)n); G.first_pos = first_pos; G.cur_pos = cur_pos;
    memset(G.kf.data(), 0, sizeof(isv_pg_keyframe_t) * (size_t)n);
    for (int k = 0; k < n; k++) {
        isv_pg_keyframe_t &f = G.kf[k];
        f.time_stamp = 0.25 * k; f.index = 10 + 3 * k; f.sequence = k < n_seq0 ? 0 : 1; f.loop_index = -1; f.has_rollpitch = k % rp_every == 0;
        fill_numbers(f);
    }
    for (auto &l : loops) { G.kf[l.first].has_loop = 1; G.kf[l.first].loop_index = G.kf[l.second].index; }
    G.first = G.kf[first_pos].index; G.cur = G.kf[cur_pos].index;
    return G;
}
Graph random_graph() {                                        // 8 - 25 keyframes, mixed
    const int n = 8 + (int)(rnd() % 18), first_pos = (int)(rnd() % 3), cur_pos = n - 1 - (int)(rnd() % 3), n_seq0 = rnd() % 4 == 0 ? first_pos + 1 + (int)(rnd() % 3) : 0;
    std::vector<std::pair<int, int>> loops;
    for (int l = (int)(rnd() % 4); l > 0; l--) { const int k = first_pos + 2 + (int)(rnd() % (n - first_pos - 2)); loops.push_back({k, first_pos + (int)(rnd() % (k - first_pos - 1))}); }
    return make_graph(n, first_pos, cur_pos, n_seq0, loops, 1 + (int)(rnd() % 2));
}

// ---- the stand-in handle and the call -----------------------------------------------------------------------------------
struct FakeDev { double *pose = nullptr, *cov = nullptr; PgEdge *edges = nullptr; isv_pgo_result_t *res = nullptr;
                 int32_t *free_of = nullptr, *adj_ptr = nullptr, *adj = nullptr, *start = nullptr, *rowptr = nullptr, *colptr = nullptr, *colrows = nullptr; };
struct Host {
    isv_pgo_config_t cfg; PgCaps cap; FakeDev d; std::string err; int64_t hits = 0;
    std::vector<PgStructure> cache; std::vector<char> staging;
    // what the last call left for the checks
    std::vector<unsigned char> staged;                       // the nine uploaded arrays' bytes + the PgGraph records
    std::vector<double> staged_pose; std::vector<PgGraph> graphs; std::vector<isv_pgo_result_t> results;
    std::vector<int> wb_count; int wb_before_drain = 0, drains = 0;
    Host(int max_keyframes, int max_graphs, int max_loop_blocks) {
        cfg = isv_pgo_config_t{max_keyframes, max_graphs, max_loop_blocks, 10, 0.1};
        const size_t G = (size_t)max_graphs, K = (size_t)max_keyframes;
        cap.pose = G * K; cap.edge = G * 3 * K; cap.blk = G * (2 * K + (size_t)max_loop_blocks); cap.adj = 2 * cap.edge; cap.col = cap.blk;
        cache.resize(G);
    }
};

// the steps of isv_pgo_optimize_batch (isv_posegraph.hip) over the stand-in device; fail_chunk: the chunk whose enqueue fails
int run(Host &H, std::vector<Graph> &gs, int chunks, int fail_chunk = -1, bool no_cache = false) {
    const int ng = (int)gs.size();
    std::vector<int32_t> ns, firsts, curs; std::vector<isv_pg_keyframe_t *> kfs;
    for (Graph &g : gs) { ns.push_back((int32_t)g.kf.size()); kfs.push_back(g.kf.data()); firsts.push_back(g.first); curs.push_back(g.cur); }
    H.results.assign((size_t)ng, isv_pgo_result_t());
    H.wb_count.assign((size_t)ng, 0); H.wb_before_drain = 0; H.drains = 0;
    PgCall call;
    call.ng = ng; call.ns = ns.data(); call.kfs = kfs.data(); call.firsts = firsts.data(); call.curs = curs.data(); call.results = H.results.data(); call.slots = H.cache.data();
    call.T = pg_host_threads(ng); call.C = std::min(chunks, ng);
    int64_t hits = 0;
    int rc = pg_prepare_batch(call, H.cfg, no_cache, H.err, &hits);
    if (rc != ISV_OK) return rc;
    H.hits += hits;
    if ((rc = pg_layout(call, H.d, H.cfg, H.cap, false, H.err)) != ISV_OK) return rc;
    H.staging.resize(call.sec_off[PGA_COUNT] + 64);
    pg_carve(call, H.staging.data() + (64 - (uintptr_t)H.staging.data() % 64) % 64);
    std::vector<std::atomic<int>> wb((size_t)ng), drained((size_t)call.C);
    for (auto &x : wb) x.store(0);
    for (auto &x : drained) x.store(0);
    std::atomic<int> early{0};
    PgPipeTimes tm;
    rc = pg_run_pipeline(call, tm, H.err, [&](int g) { pg_assemble(call, H.d, g); },
        [&](int c, std::string &msg) { if (c != fail_chunk) return (int)ISV_OK; msg = "stand-in enqueue failed"; return (int)ISV_ERR_DEVICE; },
        [&](int c, std::string &) {
            const auto &lo = call.off[call.chunk_lo(c)], &hi = call.off[call.chunk_lo(c + 1)];
            if (hi[PGA_COV] > lo[PGA_COV]) memset((double *)call.sec[PGA_COV] + lo[PGA_COV], 0, sizeof(double) * (hi[PGA_COV] - lo[PGA_COV]));
            memset((isv_pgo_result_t *)call.sec[PGA_RES] + lo[PGA_RES], 0, sizeof(isv_pgo_result_t) * (hi[PGA_RES] - lo[PGA_RES]));
            drained[c].fetch_add(1);
            pg_publish_results(call, c);
            return (int)ISV_OK;
        },
        [&](int g) { if (drained[call.chunk_of(g)].load() != 1) early.fetch_add(1); wb[g].fetch_add(1); pg_write_back(call, g); });
    for (int g = 0; g < ng; g++) H.wb_count[g] = wb[g].load();
    for (int c = 0; c < call.C; c++) H.drains += drained[c].load();
    H.wb_before_drain = early.load();
    H.staged.clear();
    pg_for_each_array(call, H.d, PG_NO_GRAPH, [&](int a, unsigned dir, auto *sp, auto *, size_t, const auto *) {
        if (dir & PG_UP) H.staged.insert(H.staged.end(), (unsigned char *)sp, (unsigned char *)(sp + call.off[ng][a]));
    });
    H.staged.insert(H.staged.end(), (unsigned char *)call.graphs.data(), (unsigned char *)(call.graphs.data() + ng));
    H.staged_pose.assign((double *)call.sec[PGA_POSE], (double *)call.sec[PGA_POSE] + call.off[ng][PGA_POSE]);
    H.graphs = call.graphs;
    return rc;
}

// ---- checks ---------------------------------------------------------------------------------------------------------------
// the slot's structure against the keyframe list (the edge list, from scratch) and against brute force from the edge list alone
void check_structure(const PgStructure &S, const Graph &G) {
    const int n = (int)G.kf.size();
    CHECK(S.valid && (int)S.loc.size() == n && S.cur_pos == G.cur_pos && S.P1 == G.cur_pos - G.first_pos + 1);
    const std::vector<int32_t> &fo = S.ix(PGA_FREE_OF);
    CHECK((int)fo.size() == S.P1);
    int nf = 0, e = 0, n_loops = 0;
    for (int k = 0; k < n; k++) {
        const int li = k - G.first_pos;
        CHECK(S.loc[k] == (k >= G.first_pos && k <= G.cur_pos ? li : -1));
        if (S.loc[k] >= 0) CHECK(fo[li] == ((k == G.first_pos || G.kf[k].sequence == 0) ? -1 : nf++));
    }
    CHECK(nf == S.nf);
    auto is = [&](const PgEdgeTpl &T, int kind, int a, int b, int dim, int robust, int src) {
        return T.kind == kind && T.a == a && T.b == b && T.fa == fo[a] && T.fb == (kind == 0 ? -1 : fo[b]) && T.dim == dim && T.robust == robust && T.src == src;
    };
    for (int k = G.first_pos; k < G.cur_pos; k++) {
        const int li = k - G.first_pos;
        if (G.kf[k].has_rollpitch) { CHECK(e < (int)S.edges.size() && is(S.edges[e], 0, li, li, 2, 0, k)); e++; }
        CHECK(e < (int)S.edges.size() && is(S.edges[e], 1, li, li + 1, 6, 0, k)); e++;
        if (G.kf[k].has_loop) { CHECK(e < (int)S.edges.size() && is(S.edges[e], 2, (G.kf[k].loop_index - 10) / 3 - G.first_pos, li, 6, 1, k)); e++; n_loops++; }
    }
    CHECK(e == (int)S.edges.size() && n_loops == S.n_loops);
    // brute force: start[f] = the smallest free index a two-sided edge joins to f, or f
    std::vector<int> st(nf);
    for (int f = 0; f < nf; f++) st[f] = f;
    std::multiset<int32_t> sides;
    for (int id = 0; id < (int)S.edges.size(); id++) {
        const PgEdgeTpl &T = S.edges[id];
        if (T.fa >= 0) sides.insert((id << 1) | 0);
        if (T.kind != 0 && T.fb >= 0) sides.insert((id << 1) | 1);
        if (T.kind != 0 && T.fa >= 0 && T.fb >= 0) { const int hi = std::max(T.fa, T.fb); st[hi] = std::min(st[hi], (int)std::min(T.fa, T.fb)); }
    }
    const std::vector<int32_t> &start = S.ix(PGA_START), &rowptr = S.ix(PGA_ROWPTR), &colptr = S.ix(PGA_COLPTR), &colrows = S.ix(PGA_COLROWS), &adj_ptr = S.ix(PGA_ADJ_PTR), &adj = S.ix(PGA_ADJ);
    CHECK((int)start.size() == nf && (int)rowptr.size() == nf + 1 && (int)colptr.size() == nf + 1 && (int)adj_ptr.size() == nf + 1);
    int nb = 0;
    for (int f = 0; f < nf; f++) { CHECK(start[f] == st[f] && rowptr[f] == nb); nb += f - st[f] + 1; }
    CHECK(rowptr[nf] == nb && S.nblk == nb);
    size_t q = 0;
    for (int j = 0; j < nf; j++) {
        CHECK(colptr[j] == (int32_t)q);
        for (int i = j + 1; i < nf; i++) if (st[i] <= j) { CHECK(q < colrows.size() && colrows[q] == i); q++; }
    }
    CHECK(colptr[nf] == (int32_t)q && q == colrows.size());
    // adjacency: every free side of every edge exactly once, in the list of the free pose it touches
    CHECK(adj_ptr[0] == 0 && adj_ptr[nf] == (int32_t)adj.size());
    std::multiset<int32_t> seen;
    for (int f = 0; f < nf; f++)
        for (int p = adj_ptr[f]; p < adj_ptr[f + 1]; p++) {
            const PgEdgeTpl &T = S.edges[(size_t)(adj[p] >> 1)];
            CHECK(((adj[p] & 1) ? T.fb : T.fa) == f);
            seen.insert(adj[p]);
        }
    CHECK(seen == sides && seen.size() == std::set<int32_t>(seen.begin(), seen.end()).size());
}

// the write-back under the identity stand-in; before: the lists as they went in
void check_write_back(const Host &H, const std::vector<Graph> &gs, const std::vector<Graph> &before) {
    CHECK(H.wb_before_drain == 0);
    for (size_t g = 0; g < gs.size(); g++) {
        const Graph &G = gs[g]; const PgGraph &P = H.graphs[g]; const isv_pgo_result_t &R = H.results[g];
        CHECK(H.wb_count[g] == 1 && R.status == ISV_OK);
        int n_loops = 0;
        for (int k = G.first_pos; k < G.cur_pos; k++) n_loops += G.kf[k].has_loop != 0;
        CHECK(R.n_loop_edges == n_loops);
        for (int k = 0; k < (int)G.kf.size(); k++) {
            const isv_pg_keyframe_t &f = G.kf[k];
            if (k < G.first_pos) { CHECK(memcmp(&f, &before[g].kf[k], sizeof(f)) == 0); continue; }       // outside the problem: untouched
            if (k <= G.cur_pos) {
                CHECK(memcmp(f.T_w_i, H.staged_pose.data() + (size_t)(P.pose0 + k - G.first_pos) * 7, 24) == 0 && memcmp(f.T_w_i, f.vio_T_w_i, 24) == 0);
                CHECK(f.cov_computed == (k < G.cur_pos));
                for (int c = 0; c < 36; c++) CHECK(f.cov[c] == 0.0);
                continue;
            }
            double Pn[3], Rn[9];                                             // after cur: moved by the drift
            h_mv(R.r_drift, f.vio_T_w_i, Pn); h_mm(R.r_drift, f.vio_R_w_i, Rn);
            for (int c = 0; c < 3; c++) Pn[c] += R.t_drift[c];
            CHECK(memcmp(f.T_w_i, Pn, 24) == 0 && memcmp(f.R_w_i, Rn, 72) == 0);
        }
    }
}

std::vector<Graph> special_graphs() {
    std::vector<Graph> gs;
    gs.push_back(make_graph(2, 0, 1, 0, {}));                              // 2 keyframes, the minimum
    gs.push_back(make_graph(3, 0, 2, 0, {{1, 0}}));                        // 3 keyframes, one loop closure
    gs.push_back(make_graph(9, 0, 8, 4, {{6, 2}}));                        // the head is sequence 0: constant poses
    gs.push_back(make_graph(12, 3, 11, 0, {{9, 4}}));                      // first_looped_index > 0
    gs.push_back(make_graph(14, 2, 9, 0, {{7, 3}, {12, 5}}));              // keyframes after cur (one with a loop closure of its own)
    gs.push_back(make_graph(10, 0, 9, 0, {{8, 1}}));                       // a loop closure spanning the whole free range
    gs.push_back(make_graph(11, 1, 10, 0, {{9, 1}, {6, 3}}, 2));           // ... onto the constant first pose; roll/pitch on every other keyframe
    return gs;
}

// cold, cached, changed numbers against a fresh slot, never-trusted slots: same staged bytes; structure; write-back
void check_batch(const std::vector<Graph> &proto, int chunks) {
    const int ng = (int)proto.size();
    Host H(32, ng, 8 * 32), fresh(32, ng, 8 * 32), untrusted(32, ng, 8 * 32);
    std::vector<Graph> a = proto, b = proto, c = proto;
    CHECK(run(H, a, chunks) == ISV_OK && H.hits == 0 && H.drains == std::min(chunks, ng));
    for (int g = 0; g < ng; g++) check_structure(H.cache[g], proto[g]);
    check_write_back(H, a, proto);
    const std::vector<unsigned char> cold = H.staged;
    CHECK(run(H, b, chunks) == ISV_OK && H.hits == ng && H.staged == cold);
    check_write_back(H, b, proto);
    for (int g = 0; g < ng; g++) { CHECK(memcmp(a[g].kf.data(), b[g].kf.data(), sizeof(isv_pg_keyframe_t) * a[g].kf.size()) == 0); check_structure(H.cache[g], proto[g]); }
    for (Graph &g : c) for (isv_pg_keyframe_t &f : g.kf) fill_numbers(f);       // other numbers, same structure
    const std::vector<Graph> c0 = c;
    std::vector<Graph> c2 = c, c3 = c, c4 = c;
    CHECK(run(H, c, chunks) == ISV_OK && H.hits == 2 * ng && run(fresh, c2, chunks) == ISV_OK && fresh.hits == 0);
    CHECK(H.staged == fresh.staged && H.staged != cold);
    check_write_back(H, c, c0);
    CHECK(run(untrusted, c3, chunks, -1, true) == ISV_OK && run(untrusted, c4, chunks, -1, true) == ISV_OK && untrusted.hits == 0 && untrusted.staged == fresh.staged);
}

void expect_refusal(Host &H, Graph bad, const Graph &good, int rc, const char *msg) {
    std::vector<Graph> one{std::move(bad)};
    const std::vector<Graph> before = one;
    H.err.clear();
    CHECK(run(H, one, 1) == rc && H.err == msg && !H.cache[0].valid);
    CHECK(memcmp(one[0].kf.data(), before[0].kf.data(), sizeof(isv_pg_keyframe_t) * one[0].kf.size()) == 0);      // nothing written
    const int64_t hits = H.hits;
    std::vector<Graph> ok{good};
    CHECK(run(H, ok, 1) == ISV_OK && H.hits == hits);            // the next valid call on the slot is a miss
    check_structure(H.cache[0], good);
}

void check_refusals() {
    const char *NO_CUR = "cur_index is not in the keyframe list (or lies before first_looped_index)", *NONFINITE = "non-finite keyframe pose";
    const char *LOOP = "loop_index outside the optimised range (the reference asserts loop_index >= first_looped_index)";
    Host H(16, 4, 20);
    const Graph good = make_graph(12, 3, 11, 0, {{9, 4}});
    Graph bad = good; bad.cur = 9999;
    expect_refusal(H, bad, good, ISV_ERR_INVALID_ARG, NO_CUR);
    bad = good; bad.cur = good.kf[1].index;                                    // ... or lies before first_looped_index
    expect_refusal(H, bad, good, ISV_ERR_INVALID_ARG, NO_CUR);
    bad = good; bad.kf[9].loop_index = good.kf[1].index;                       // loop partner before first_looped_index
    expect_refusal(H, bad, good, ISV_ERR_INVALID_ARG, LOOP);
    bad = good; bad.kf[5].vio_R_w_i[7] = std::nan("");                         // the slot is warm (the same structure, valid): a hit that is refused
    CHECK(H.cache[0].valid);
    expect_refusal(H, bad, good, ISV_ERR_NONFINITE, NONFINITE);
    { Host cold(16, 4, 20); expect_refusal(cold, bad, good, ISV_ERR_NONFINITE, NONFINITE); }
    bad.kf[9].loop_index = good.kf[1].index;                                   // the order of the checks: non-finite before the loop partner
    expect_refusal(H, bad, good, ISV_ERR_NONFINITE, NONFINITE);
    bad = good; bad.kf[2].vio_R_w_i[0] = std::nan("");                         // a keyframe outside the problem is not looked at
    { std::vector<Graph> one{bad}; CHECK(run(H, one, 1) == ISV_OK); }
    expect_refusal(H, make_graph(20, 2, 19, 0, {}), good, ISV_ERR_CAPACITY, "more keyframes than max_keyframes");
    expect_refusal(H, make_graph(16, 0, 15, 0, {{14, 1}, {13, 2}}), good, ISV_ERR_CAPACITY, "loop closures span more blocks than max_loop_blocks");
    // a batch: the first refused graph in index order reports, the hit counter does not move, the good graphs' slots stay valid
    std::vector<Graph> batch{good, good, good, good};
    CHECK(run(H, batch, 1) == ISV_OK);
    const int64_t hits = H.hits;
    batch = {good, good, good, good}; batch[1].kf[5].vio_R_w_i[0] = std::nan(""); batch[2].cur = 9999;
    CHECK(run(H, batch, 1) == ISV_ERR_NONFINITE && H.err == NONFINITE && H.hits == hits);
    CHECK(H.cache[0].valid && !H.cache[1].valid && !H.cache[2].valid && H.cache[3].valid);
    batch = {good, good, good, good};
    CHECK(run(H, batch, 1) == ISV_OK && H.hits == hits + 2);
    // more than the handle's pools hold
    Host tiny(16, 2, 0); tiny.cap.edge = 10;
    std::vector<Graph> two{make_graph(8, 0, 7, 0, {}), make_graph(8, 0, 7, 0, {})};
    CHECK(run(tiny, two, 1) == ISV_ERR_CAPACITY && tiny.err == "pose graphs exceed the handle's capacity");
}

// a chunk whose enqueue fails: the call returns that error; once it is recorded nothing more is drained or written back, so no
// graph of that chunk or of a later one is written back (their tasks wait for the failed enqueue; every chunk here has more
// graphs than there are threads)
void check_failing_enqueue(const std::vector<Graph> &proto) {
    const int ng = (int)proto.size();
    for (int fail : {0, 2}) {
        Host H(32, ng, 8 * 32);
        std::vector<Graph> a = proto;
        CHECK(run(H, a, 4, fail) == ISV_ERR_DEVICE && H.err == "stand-in enqueue failed" && H.wb_before_drain == 0 && H.drains <= fail);
        const int lo = (int)((int64_t)ng * fail / 4);
        for (int g = 0; g < ng; g++) {
            CHECK(H.wb_count[g] <= 1);
            if (g >= lo) { CHECK(H.wb_count[g] == 0); for (const isv_pg_keyframe_t &f : a[g].kf) CHECK(f.T_w_i[0] == SENTINEL); }
        }
    }
}

}  // namespace

int main() {
    const std::vector<Graph> special = special_graphs();
    for (const Graph &g : special) check_batch({g}, 1);                  // every shape as a call of its own
    std::vector<Graph> mixed = special;
    while (mixed.size() < 70) mixed.push_back(random_graph());
    for (int chunks : {1, 3, 4}) check_batch(mixed, chunks);
    CHECK(getenv("ISV_PGO_CHUNKS") || (pg_chunk_count(70) == 4 && pg_chunk_count(64) == 4 && pg_chunk_count(63) == 1));
    check_refusals();
    check_failing_enqueue(mixed);
    printf("ok: %d special shapes, 70 mixed graphs in 1 / 3 / 4 chunks on %d host thread(s); structure, staging, write-back, refusals, failing enqueue\n",
           (int)special.size(), pg_host_threads(70));
    return 0;
}
