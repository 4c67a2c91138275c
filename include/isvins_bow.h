/*
 * isvins_bow.h -- C ABI of the batched loop DETECTION: the bag-of-words query that proposes an old keyframe, and the add,
 *   PoseGraph::detectLoop                 src/pose_graph/pose_graph.cpp:138-218                    (MI355X)
 *   PoseGraph::addKeyFrameIntoVoc         :220-233
 *     TemplatedVocabulary::transform      thirdparty/DBoW/TemplatedVocabulary.h:1065-1121, :1217-1258   kernel k_bow_transform
 *     BowVector::addWeight / normalize    thirdparty/DBoW/BowVector.cpp:29-84
 *     TemplatedDatabase::queryL1          thirdparty/DBoW/TemplatedDatabase.h:656-723              kernels k_bow_score, k_bow_select
 *     TemplatedDatabase::add              :514-545                                                 kernel k_bow_append
 * for S sequences in lock step: one database per sequence, at most one keyframe added per database per call.  Its result,
 * loop_index, is the old_index of isv_loop_pair_t (isvins_loop.h), whose result isvins_posegraph.h consumes.
 *
 * The vocabulary is an input: the file format of VINSLoop::Vocabulary::deserialize (thirdparty/VocabularyBinary.cpp), little endian:
 *   24 bytes             int32 k, L, scoringType, weightingType, nNodes, nWords
 *   nNodes x 48 bytes    int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]
 *   nWords x 8 bytes     int32 nodeId, int32 wordId
 * with the tree of TemplatedVocabulary::loadBin (:1509-1561): the root is node 0 and is not in the file, a node's children are in
 * the order of their records, a leaf is a node without children.  Bit 64 w + b of a descriptor is bit b of word w (as in
 * isvins_loop.h).  Only weightingType TF_IDF (0) with scoringType L1_NORM (0) is implemented (BowVector.h:36-53), what the
 * reference's vocabulary uses.  No vocabulary ships with this project: the loader is tested on synthetic files of this format.
 *
 * The arithmetic, restated:
 *   transform   per feature a descent from the root: at each node the child of least Hamming distance, the FIRST of equal minima
 *               (strict <), until a leaf -- which may sit above level L.  A word of weight 0 is a stop word and is dropped (w > 0).
 *               A word hit c times has the value w added c times (w + w + ..., not c * w).  L1 normalisation: the norm is summed
 *               in ascending word id, every value is divided by it; no division when the norm is 0.
 *   queryL1     max_id = frame_index - min_gap.  Entry e is eligible iff e < max_id || max_id == -1 || e == n_entries - 1.  Per
 *               eligible entry sharing at least one word, raw = sum over the common words in ascending word id of
 *               (|q - d| - |q| - |d|); entries sharing no word are absent.  The max_results smallest raw, Score = -raw / 2.0.
 *   detectLoop  :181-216 as written, with neighbour_score for 0.05 and loop_score for 0.015.
 * Reference quirks that are KEPT (marked B1.. in the kernels and in the restatement tests/native/isv_bow_oracle.c):
 *   B1  frame_index - min_gap == -1 (frame 49) reads as "no limit": every entry is eligible.
 *   B2  the newest entry is always eligible, hence ret[0] "is the neighbour".
 *   B3  min_index starts as ret[0].Id whatever its score.
 *   B4  the frame_index > min_gap gate is applied after the query and the add.
 * Deviation (documented, not a quirk): std::sort leaves the order of equal scores unspecified; here the lower entry id comes first.
 * Every floating-point operation is an IEEE double + - / or fabs in a fixed order, so the GPU and the restatement agree bit for bit.
 */
#ifndef ISVINS_BOW_H
#define ISVINS_BOW_H

#include <stddef.h>
#include <stdint.h>
#include "isvins_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISV_BOW_MAX_RESULTS 8
#define ISV_BOW_MAX_FEATURES 8192

typedef enum isv_bow_status {
    ISV_BOW_OK = 0,
    ISV_BOW_CAPACITY = 1,         /* n_features > max_features                                                    */
    ISV_BOW_INPUT = 2,            /* negative count, null array with a non-zero count, database out of range, unknown mode */
    ISV_BOW_DUPLICATE = 3         /* the database appears more than once in the call and not all of its items are QUERY */
} isv_bow_status_t;

typedef enum isv_bow_mode {
    ISV_BOW_DETECT = 0,           /* query, then add: detectLoop                                                  */
    ISV_BOW_ADD = 1,              /* addKeyFrameIntoVoc                                                           */
    ISV_BOW_QUERY = 2             /* query only; the database is untouched                                        */
} isv_bow_mode_t;

typedef struct isv_bow_vocab_info {
    int32_t k, L;                 /* as the file states them                                                      */
    int32_t n_nodes, n_words;     /* without the root                                                             */
    int32_t n_leaves;
    int32_t max_depth;            /* deepest leaf (the root's children are at depth 1)                            */
    int32_t n_stop_words;         /* words of weight 0                                                            */
    int32_t _pad;
} isv_bow_vocab_info_t;

typedef struct isv_bow_config {
    int32_t max_items;            /* items per call                                                               */
    int32_t n_databases;
    int32_t max_features;         /* per keyframe, at most ISV_BOW_MAX_FEATURES                                   */
    int32_t max_results;          /* 4 (pose_graph.cpp:153), at most ISV_BOW_MAX_RESULTS                          */
    int32_t min_gap;              /* 50 (:153, :205)                                                              */
    int32_t initial_entry_capacity;   /* per database; the storage only grows                                     */
    double  neighbour_score;      /* 0.05 (:182)                                                                  */
    double  loop_score;           /* 0.015 (:186, :210)                                                           */
} isv_bow_config_t;

typedef struct isv_bow_item {
    int32_t database;
    int32_t frame_index;
    int32_t mode;                 /* isv_bow_mode_t                                                               */
    int32_t n_features;
    const uint64_t *brief;        /* [n_features][4]   brief_descriptors                                          */
} isv_bow_item_t;

typedef struct isv_bow_result {
    int32_t status;               /* isv_bow_status_t                                                             */
    int32_t n_words;              /* the vector's size after stop words                                           */
    int32_t entry_id;             /* what add returned; -1 for QUERY                                              */
    int32_t n_scored;             /* pairs.size() in queryL1 (0 for ADD)                                          */
    int32_t n_results;
    int32_t find_loop;
    int32_t loop_index;           /* detectLoop's return value; -1 where the mode has no query                    */
    int32_t _pad;
    int32_t result_id[ISV_BOW_MAX_RESULTS];      /* -1 past n_results                                             */
    double  result_score[ISV_BOW_MAX_RESULTS];   /* 0 past n_results                                              */
} isv_bow_result_t;

typedef struct isv_bow isv_bow_t;

/* Host only, usable without a GPU: validate a vocabulary file image and describe it.  Status codes as in isvins_backend.h, and one
 * more, ISV_ERR_INPUT, for a malformed file: short or over-long; nNodes <= 0 or nWords <= 0; ids outside [1, nNodes], duplicate
 * ids, parentId outside [0, nNodes]; a cycle or a node not reachable from the root; a word whose node is not a leaf, a leaf
 * without a word, a duplicate or out-of-range wordId; a non-finite or negative weight.  ISV_ERR_UNSUPPORTED for a header with
 * another weighting or scoring type.  ISV_ERR_INVALID_ARG for null arguments or a file that cannot be read.  info (may be NULL) is
 * written on ISV_OK only. */
#define ISV_ERR_INPUT (-6)
int  isv_bow_vocab_check(const void *bytes, size_t n, isv_bow_vocab_info_t *info);
int  isv_bow_vocab_check_file(const char *path, isv_bow_vocab_info_t *info);

/* Fails with ISV_ERR_DEVICE without a GPU: there is no CPU path.  The vocabulary is checked as by isv_bow_vocab_check and copied
 * to the device, breadth-first with every node's children contiguous in file order. */
int  isv_bow_create(const isv_bow_config_t *cfg, const void *vocab_bytes, size_t n, isv_bow_t **out);
void isv_bow_destroy(isv_bow_t *h);
const char *isv_bow_last_error(const isv_bow_t *h);

/* items[0..n): one packed upload, k_bow_transform, k_bow_score, k_bow_select, k_bow_append, one download, synchronous on the
 * handle's own stream.  results [n].  word_ids / word_weights: NULL, or [n] pointers each NULL or to [n_features] values; they
 * receive the item's bag-of-words vector, ascending word id, [n_words].  Every query of the call sees the databases as they were
 * before the call.  A database may appear more than once only if all of its items are QUERY; otherwise each of its items gets
 * ISV_BOW_DUPLICATE and the database is unchanged.  A refused item changes nothing and leaves its arrays untouched; the call returns
 * ISV_OK whenever it ran.  A failed device allocation while growing a database leaves every database as it was before the call
 * (ISV_ERR_DEVICE).  An item's result record and vector do not depend, bit for bit, on the batch it is in. */
int  isv_bow_detect_batch(isv_bow_t *h, int32_t n, const isv_bow_item_t *const *items, isv_bow_result_t *results,
                          uint32_t *const *word_ids, double *const *word_weights);
/* milliseconds of the last successful call: the whole call, k_bow_transform, k_bow_score, k_bow_select, k_bow_append (HIP events) */
int  isv_bow_last_ms(isv_bow_t *h, double out_ms[5]);
/* empty database db (its storage is kept) */
int  isv_bow_reset(isv_bow_t *h, int32_t db);
/* number of entries of database db, or a negative isv_status_t */
int  isv_bow_entries(const isv_bow_t *h, int32_t db);

#ifdef __cplusplus
}
#endif
#endif /* ISVINS_BOW_H */
