/* isv_bow_oracle.c -- the serial restatement of include/isvins_bow.h in plain C: one vocabulary, ONE database.
 * The kernels of is-vins_amd/csrc/isv_bow.hip are pinned to it bit for bit; tests/test_bow_oracle.py pins it independently
 * (a brute-force numpy descent, a dense numpy L1 score).  Built with gcc -O2 -ffp-contract=off by tests/bow_oracle.py.
 * The vocabulary is assumed valid (isv_bow_vocab_check has passed).
 *
 * Restated from the reference (own text):
 *   TemplatedVocabulary::loadBin    thirdparty/DBoW/TemplatedVocabulary.h:1509-1561    voc_load
 *   TemplatedVocabulary::transform  :1065-1121, :1217-1258                             descend, bow_transform
 *   BowVector::addWeight/normalize  thirdparty/DBoW/BowVector.cpp:29-84                bow_transform
 *   TemplatedDatabase::queryL1      thirdparty/DBoW/TemplatedDatabase.h:656-723        bow_query
 *   TemplatedDatabase::add          :514-545                                           bow_add
 *   PoseGraph::detectLoop           src/pose_graph/pose_graph.cpp:138-218              isvo_bow_detect
 * queryL1 walks the inverted file word by word and accumulates per entry in a map; every entry's sum therefore receives its terms
 * in ascending word id.  Here each entry's own (ascending) word list is merged with the query's: the same terms in the same order.
 *
 * isvo_bow_set_quirks_off(bits) switches the kept reference quirks off one at a time, for the tests that show each one matters:
 *   1  B1  max_id == -1 no longer reads as "no limit"
 *   2  B2  the newest entry is no longer always eligible
 *   4  B3  ret[0] is taken for the neighbour and left out of the minimum (the scan starts at i = 1, as the find_loop scan does)
 *   8  B4  the frame_index > min_gap gate comes first: a frame that fails it is not queried (it is still added)
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "isvins_bow.h"

enum { QB1 = 1, QB2 = 2, QB3 = 4, QB4 = 8 };
static int g_quirks_off = 0;
void isvo_bow_set_quirks_off(int bits) { g_quirks_off = bits; }

typedef struct {
    int32_t n_nodes, n_words;
    int32_t *child_start, *child;      /* children of file id v: child[child_start[v] .. child_start[v + 1]), in record order */
    int32_t *word_of;                  /* -1: inner node */
    double *weight;
    uint64_t *desc;                    /* [n_nodes + 1][4] */
} voc_t;

typedef struct isvo_bow {
    isv_bow_config_t cfg;
    voc_t v;
    /* the database: entry e holds words[ptr[e] .. ptr[e + 1]) ascending, with vals */
    int32_t n_entries, cap_e;
    size_t cap_w;
    size_t *ptr;
    uint32_t *words;
    double *vals;
    /* transform scratch */
    double *acc;
    char *present;
} isvo_bow_t;

static int32_t le_i32(const unsigned char *p) { int32_t x; memcpy(&x, p, 4); return x; }

static void voc_load(voc_t *v, const unsigned char *p) {
    const int32_t nn = le_i32(p + 16), nw = le_i32(p + 20);
    const unsigned char *nodes = p + 24, *words = nodes + 48 * (size_t)nn;
    const size_t N = (size_t)nn + 1;
    v->n_nodes = nn; v->n_words = nw;
    v->child_start = calloc(N + 1, sizeof(int32_t)); v->child = calloc(N, sizeof(int32_t));
    v->word_of = malloc(N * sizeof(int32_t)); v->weight = calloc(N, sizeof(double)); v->desc = calloc(4 * N, sizeof(uint64_t));
    int32_t *fill = calloc(N, sizeof(int32_t));
    for (int32_t i = 0; i < nn; i++) v->child_start[le_i32(nodes + 48 * (size_t)i + 4) + 1]++;
    for (size_t k = 0; k < N; k++) v->child_start[k + 1] += v->child_start[k];
    for (size_t k = 0; k < N; k++) v->word_of[k] = -1;
    for (int32_t i = 0; i < nn; i++) {                  /* m_nodes[pid].children.push_back(nid), :1538 */
        const unsigned char *r = nodes + 48 * (size_t)i;
        const int32_t id = le_i32(r), pid = le_i32(r + 4);
        v->child[v->child_start[pid] + fill[pid]++] = id;
        memcpy(&v->weight[id], r + 8, 8);
        memcpy(&v->desc[4 * (size_t)id], r + 16, 32);
    }
    for (int32_t i = 0; i < nw; i++) v->word_of[le_i32(words + 8 * (size_t)i)] = le_i32(words + 8 * (size_t)i + 4);
    free(fill);
}

static int hamming(const uint64_t *a, const uint64_t *b) {
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) +
           __builtin_popcountll(a[3] ^ b[3]);
}

/* :1217-1258: the leaf a feature falls into */
static int32_t descend(const voc_t *v, const uint64_t *f) {
    int32_t at = 0;
    do {
        const int32_t *c = v->child + v->child_start[at], nc = v->child_start[at + 1] - v->child_start[at];
        int32_t best = c[0];
        int best_d = hamming(f, v->desc + 4 * (size_t)best);
        for (int32_t k = 1; k < nc; k++) {
            const int d = hamming(f, v->desc + 4 * (size_t)c[k]);
            if (d < best_d) { best_d = d; best = c[k]; }      /* strict <: the first of equal minima */
        }
        at = best;
    } while (v->child_start[at + 1] != v->child_start[at]);
    return at;
}

static int cmp_u32(const void *a, const void *b) {
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

/* :1065-1121 with TF_IDF and L1: words / vals [nf] receive the vector, ascending word id; returns its size */
static int bow_transform(isvo_bow_t *h, int32_t nf, const uint64_t *brief, uint32_t *words, double *vals) {
    int n = 0;
    for (int32_t i = 0; i < nf; i++) {
        const int32_t leaf = descend(&h->v, brief + 4 * (size_t)i);
        const int32_t id = h->v.word_of[leaf];
        const double w = h->v.weight[leaf];
        if (!(w > 0)) continue;                                /* a stop word */
        if (h->present[id]) h->acc[id] += w;                   /* addWeight: once per occurrence, in feature order */
        else { h->present[id] = 1; h->acc[id] = w; words[n++] = (uint32_t)id; }
    }
    qsort(words, (size_t)n, sizeof(uint32_t), cmp_u32);
    double norm = 0.0;
    for (int i = 0; i < n; i++) norm += fabs(h->acc[words[i]]);      /* BowVector.cpp:66-69 */
    for (int i = 0; i < n; i++) {
        vals[i] = h->acc[words[i]];
        if (norm > 0.0) vals[i] = vals[i] / norm;                    /* :71-75 */
        h->present[words[i]] = 0;
    }
    return n;
}

typedef struct { double raw; int32_t id; } scored_t;
static int cmp_scored(const void *a, const void *b) {
    const scored_t *x = a, *y = b;
    if (x->raw != y->raw) return x->raw < y->raw ? -1 : 1;
    return x->id < y->id ? -1 : x->id > y->id;                      /* the deviation: of equal scores the lower id first */
}

/* :656-723; fills R's n_scored, n_results, result_id, result_score */
static void bow_query(const isvo_bow_t *h, int n, const uint32_t *qw, const double *qv, int max_id, isv_bow_result_t *R) {
    scored_t *s = malloc(sizeof(scored_t) * (size_t)(h->n_entries + 1));
    int ns = 0;
    for (int32_t e = 0; e < h->n_entries; e++) {
        const int eligible = e < max_id || (max_id == -1 && !(g_quirks_off & QB1)) || (e == h->n_entries - 1 && !(g_quirks_off & QB2));
        if (!eligible) continue;
        size_t a = h->ptr[e];
        const size_t a1 = h->ptr[e + 1];
        int b = 0, any = 0;
        double sum = 0.0;
        while (a < a1 && b < n) {
            if (h->words[a] < qw[b]) a++;
            else if (h->words[a] > qw[b]) b++;
            else {
                const double q = qv[b], d = h->vals[a];
                const double value = fabs(q - d) - fabs(q) - fabs(d);
                if (any) sum += value; else { sum = value; any = 1; }
                a++; b++;
            }
        }
        if (any) { s[ns].raw = sum; s[ns].id = e; ns++; }
    }
    qsort(s, (size_t)ns, sizeof(scored_t), cmp_scored);
    R->n_scored = ns;
    R->n_results = ns < h->cfg.max_results ? ns : h->cfg.max_results;
    for (int i = 0; i < R->n_results; i++) { R->result_id[i] = s[i].id; R->result_score[i] = -s[i].raw / 2.0; }
    free(s);
}

static void bow_add(isvo_bow_t *h, int n, const uint32_t *w, const double *v) {
    if (h->n_entries + 1 > h->cap_e) {
        h->cap_e = 2 * h->cap_e + 1;
        h->ptr = realloc(h->ptr, sizeof(size_t) * ((size_t)h->cap_e + 1));
    }
    const size_t used = h->ptr[h->n_entries];
    if (used + (size_t)n > h->cap_w) {
        h->cap_w = 2 * (used + (size_t)n);
        h->words = realloc(h->words, sizeof(uint32_t) * h->cap_w);
        h->vals = realloc(h->vals, sizeof(double) * h->cap_w);
    }
    if (n) { memcpy(h->words + used, w, sizeof(uint32_t) * (size_t)n); memcpy(h->vals + used, v, sizeof(double) * (size_t)n); }
    h->ptr[++h->n_entries] = used + (size_t)n;
}

isvo_bow_t *isvo_bow_new(const isv_bow_config_t *cfg, const void *vocab, size_t n) {
    (void)n;
    isvo_bow_t *h = calloc(1, sizeof(*h));
    h->cfg = *cfg;
    voc_load(&h->v, vocab);
    h->ptr = calloc(1, sizeof(size_t));
    h->acc = calloc((size_t)h->v.n_words, sizeof(double));
    h->present = calloc((size_t)h->v.n_words, 1);
    return h;
}

void isvo_bow_free(isvo_bow_t *h) {
    if (!h) return;
    free(h->v.child_start); free(h->v.child); free(h->v.word_of); free(h->v.weight); free(h->v.desc);
    free(h->ptr); free(h->words); free(h->vals); free(h->acc); free(h->present);
    free(h);
}

int isvo_bow_entries(const isvo_bow_t *h) { return h->n_entries; }
void isvo_bow_reset(isvo_bow_t *h) { h->n_entries = 0; }

int isvo_bow_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(isv_bow_config_t);
    case 1: return (int)sizeof(isv_bow_item_t);
    case 2: return (int)sizeof(isv_bow_result_t);
    case 3: return (int)sizeof(isv_bow_vocab_info_t);
    }
    return -1;
}

/* the transform alone: words / vals [n_features]; returns n_words */
int isvo_bow_transform(isvo_bow_t *h, int32_t nf, const uint64_t *brief, uint32_t *words, double *vals) {
    return bow_transform(h, nf, brief, words, vals);
}

/* one item on this database (item->database is not read).  words / vals: NULL or [n_features]. */
void isvo_bow_detect(isvo_bow_t *h, const isv_bow_item_t *it, isv_bow_result_t *R, uint32_t *words, double *vals) {
    memset(R, 0, sizeof(*R));
    R->entry_id = -1; R->loop_index = -1;
    for (int i = 0; i < ISV_BOW_MAX_RESULTS; i++) R->result_id[i] = -1;
    if (it->mode < ISV_BOW_DETECT || it->mode > ISV_BOW_QUERY || it->n_features < 0 || (it->n_features > 0 && !it->brief)) { R->status = ISV_BOW_INPUT; return; }
    if (it->n_features > h->cfg.max_features) { R->status = ISV_BOW_CAPACITY; return; }
    const int32_t nf = it->n_features;
    uint32_t *w = malloc(sizeof(uint32_t) * (size_t)(nf + 1));
    double *v = malloc(sizeof(double) * (size_t)(nf + 1));
    const int n = bow_transform(h, nf, it->brief, w, v);
    R->n_words = n;
    const int min_gap = h->cfg.min_gap;
    if (it->mode != ISV_BOW_ADD) {
        /* pose_graph.cpp:153: db.query(..., 4, frame_index - 50) */
        if (!((g_quirks_off & QB4) && !(it->frame_index > min_gap))) bow_query(h, n, w, v, it->frame_index - min_gap, R);
    }
    if (it->mode != ISV_BOW_QUERY) {                               /* :158, :232 */
        R->entry_id = h->n_entries;
        bow_add(h, n, w, v);
    }
    if (it->mode != ISV_BOW_ADD) {                                 /* :181-216 */
        int find_loop = 0;
        if (R->n_results >= 1 && R->result_score[0] > h->cfg.neighbour_score)
            for (int i = 1; i < R->n_results; i++)
                if (R->result_score[i] > h->cfg.loop_score) find_loop = 1;
        R->find_loop = find_loop;
        if (find_loop && it->frame_index > min_gap) {              /* B4: only now */
            int min_index = -1;
            for (int i = (g_quirks_off & QB3) ? 1 : 0; i < R->n_results; i++)
                if (min_index == -1 || (R->result_id[i] < min_index && R->result_score[i] > h->cfg.loop_score))
                    min_index = R->result_id[i];                   /* B3: i = 0 is in */
            R->loop_index = min_index;
        }
    }
    if (words && n) memcpy(words, w, sizeof(uint32_t) * (size_t)n);
    if (vals && n) memcpy(vals, v, sizeof(double) * (size_t)n);
    free(w); free(v);
}
