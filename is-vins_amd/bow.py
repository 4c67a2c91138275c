"""Host-side mirror of include/isvins_bow.h: the batched loop detection, PoseGraph::detectLoop / addKeyFrameIntoVoc (reference
src/pose_graph/pose_graph.cpp:138-233: the DBoW2 transform of a keyframe's BRIEF descriptors, the L1 query of the sequence's
database, the add, and detectLoop's decision) for many sequences in one call.  `LoopDetector(...)` raises when the HIP extension is
missing or there is no GPU: no CPU path.  `vocab_check` is host only.

`make_vocabulary` writes a deterministic synthetic vocabulary in the reference's binary format (no vocabulary ships with this
package) and `make_place_stream` keyframes that revisit earlier ones, for the tests and scripts/bow_bench.py."""
import ctypes as C
import functools

import numpy as np

from . import _stage, backend

ISV_BOW_OK, ISV_BOW_CAPACITY, ISV_BOW_INPUT, ISV_BOW_DUPLICATE = range(4)
ISV_BOW_DETECT, ISV_BOW_ADD, ISV_BOW_QUERY = range(3)
ISV_BOW_MAX_RESULTS, ISV_BOW_MAX_FEATURES = 8, 8192
ISV_ERR_INPUT, ISV_ERR_UNSUPPORTED = -6, -5

_u64p, _u32p, _f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)


class isv_bow_vocab_info_t(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("n_nodes", C.c_int32), ("n_words", C.c_int32), ("n_leaves", C.c_int32),
                ("max_depth", C.c_int32), ("n_stop_words", C.c_int32), ("_pad", C.c_int32)]


class isv_bow_config_t(C.Structure):
    _fields_ = [("max_items", C.c_int32), ("n_databases", C.c_int32), ("max_features", C.c_int32), ("max_results", C.c_int32),
                ("min_gap", C.c_int32), ("initial_entry_capacity", C.c_int32), ("neighbour_score", C.c_double), ("loop_score", C.c_double)]


class isv_bow_item_t(C.Structure):
    _fields_ = [("database", C.c_int32), ("frame_index", C.c_int32), ("mode", C.c_int32), ("n_features", C.c_int32), ("brief", _u64p)]


class isv_bow_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_words", C.c_int32), ("entry_id", C.c_int32), ("n_scored", C.c_int32), ("n_results", C.c_int32),
                ("find_loop", C.c_int32), ("loop_index", C.c_int32), ("_pad", C.c_int32), ("result_id", C.c_int32 * ISV_BOW_MAX_RESULTS),
                ("result_score", C.c_double * ISV_BOW_MAX_RESULTS)]


EXPORTS = ["isv_bow_vocab_check", "isv_bow_vocab_check_file", "isv_bow_create", "isv_bow_destroy", "isv_bow_last_error",
           "isv_bow_detect_batch", "isv_bow_last_ms", "isv_bow_reset", "isv_bow_entries"]


def make_config(max_items=1, n_databases=1, max_features=2048, max_results=4, min_gap=50, neighbour_score=0.05, loop_score=0.015,
                initial_entry_capacity=64):
    """the reference's constants as defaults (pose_graph.cpp:153, :182, :186, :205)"""
    c = isv_bow_config_t()
    c.max_items, c.n_databases, c.max_features, c.max_results = max_items, n_databases, max_features, max_results
    c.min_gap, c.initial_entry_capacity, c.neighbour_score, c.loop_score = min_gap, initial_entry_capacity, neighbour_score, loop_score
    return c


class BowItem:
    """one keyframe for one database: its descriptors (kept alive here) behind an isv_bow_item_t (`.c`)"""

    def __init__(self, database, frame_index, brief, mode=ISV_BOW_DETECT):
        self.brief = np.ascontiguousarray(brief, dtype=np.uint64).reshape(-1, 4)
        c = self.c = isv_bow_item_t()
        c.database, c.frame_index, c.mode, c.n_features = database, frame_index, mode, len(self.brief)
        c.brief = self.brief.ctypes.data_as(_u64p)


@_stage.bind_once("bow")
def _bind(lib):
    vp = C.c_void_p
    infop = C.POINTER(isv_bow_vocab_info_t)
    lib.isv_bow_vocab_check.argtypes = [C.c_char_p, C.c_size_t, infop]
    lib.isv_bow_vocab_check_file.argtypes = [C.c_char_p, infop]
    lib.isv_bow_create.argtypes = [C.POINTER(isv_bow_config_t), C.c_char_p, C.c_size_t, C.POINTER(vp)]
    lib.isv_bow_destroy.argtypes = [vp]; lib.isv_bow_destroy.restype = None
    lib.isv_bow_last_error.argtypes = [vp]; lib.isv_bow_last_error.restype = C.c_char_p
    lib.isv_bow_detect_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_bow_item_t)), C.POINTER(isv_bow_result_t),
                                         C.POINTER(_u32p), C.POINTER(_f64p)]
    lib.isv_bow_last_ms.argtypes = [vp, _f64p]
    lib.isv_bow_reset.argtypes = [vp, C.c_int32]
    lib.isv_bow_entries.argtypes = [vp, C.c_int32]


def vocab_check(data, lib=None):
    """isv_bow_vocab_check (host only) on the file's bytes, or isv_bow_vocab_check_file on a path (str) -> (status, info)"""
    lib = lib or backend.load_library()
    _bind(lib)
    info = isv_bow_vocab_info_t()
    if isinstance(data, str):
        return lib.isv_bow_vocab_check_file(data.encode(), C.byref(info)), info
    data = bytes(data)
    return lib.isv_bow_vocab_check(data, len(data), C.byref(info)), info


class LoopDetector(_stage.StageHandle):
    """PoseGraph::detectLoop on the MI355X for n_databases sequences in lock step: one keyframe per database per call"""
    PREFIX, N_MS = "isv_bow", 5

    def __init__(self, vocab, max_items=1, n_databases=1, max_features=2048, **kw):
        self.cfg = make_config(max_items, n_databases, max_features, **kw)
        vocab = bytes(vocab)
        self._create(_bind, C.byref(self.cfg), vocab, len(vocab),
                     why=" (a valid vocabulary, a MI355X and the HIP extension are required; there is no CPU path)")

    def detect_batch(self, items, vectors=False):
        """items: BowItem list -> isv_bow_result_t list; with vectors also (word_ids, word_weights), each a list of arrays [n_words]
        (a refused item's arrays come back empty and were left untouched)"""
        n = len(items)
        res = (isv_bow_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_bow_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        args = [None, None]
        if vectors:
            ws = [np.full(max(it.c.n_features, 1), 0xFFFFFFFE, dtype=np.uint32) for it in items]
            vs = [np.full(max(it.c.n_features, 1), -2.0) for it in items]
            args = [(_u32p * max(n, 1))(*[a.ctypes.data_as(_u32p) for a in ws]), (_f64p * max(n, 1))(*[a.ctypes.data_as(_f64p) for a in vs])]
        rc = self.lib.isv_bow_detect_batch(self.h, n, ptrs, res, *args)
        self._check(rc, "isv_bow_detect_batch", with_last_error=True)
        out = list(res)[:n]
        if not vectors:
            return out
        for r, w, v in zip(out, ws, vs):
            if r.status != ISV_BOW_OK:
                assert (w == 0xFFFFFFFE).all() and (v == -2.0).all(), "a refused item's arrays were written"
        return out, [w[:r.n_words] for r, w in zip(out, ws)], [v[:r.n_words] for r, v in zip(out, vs)]

    def last_ms(self):
        """(whole call, k_bow_transform, k_bow_score, k_bow_select, k_bow_append) milliseconds of the last successful call"""
        return super().last_ms()

    def reset(self, db):
        if self.lib.isv_bow_reset(self.h, db) != 0:
            raise backend.BackendError("isv_bow_reset: bad database")

    def entries(self, db):
        n = self.lib.isv_bow_entries(self.h, db)
        if n < 0:
            raise backend.BackendError("isv_bow_entries: bad database")
        return n


# ---------------------------------------------------------------------------------------------------------------------
NODE_DTYPE = np.dtype([("id", "<i4"), ("parent", "<i4"), ("weight", "<f8"), ("desc", "<u8", (4,))])
WORD_DTYPE = np.dtype([("node", "<i4"), ("word", "<i4")])


def pack_vocabulary(k, L, nodes, words, scoring=0, weighting=0, n_nodes=None, n_words=None):
    """the file's bytes from a NODE_DTYPE and a WORD_DTYPE array (the counts in the header can be overridden, for malformed files)"""
    head = np.array([k, L, scoring, weighting, len(nodes) if n_nodes is None else n_nodes, len(words) if n_words is None else n_words], dtype="<i4")
    return head.tobytes() + np.ascontiguousarray(nodes, dtype=NODE_DTYPE).tobytes() + np.ascontiguousarray(words, dtype=WORD_DTYPE).tobytes()


def unpack_vocabulary(data):
    """(k, L, scoring, weighting, nodes, words) of a well-formed file"""
    head = np.frombuffer(data, dtype="<i4", count=6)
    nn, nw = int(head[4]), int(head[5])
    nodes = np.frombuffer(data, dtype=NODE_DTYPE, count=nn, offset=24)
    words = np.frombuffer(data, dtype=WORD_DTYPE, count=nw, offset=24 + 48 * nn)
    return int(head[0]), int(head[1]), int(head[2]), int(head[3]), nodes, words


def make_vocabulary(seed, k=10, L=3, leaf_above=False, single_child=False, duplicate_children=False, equidistant_children=False,
                    zero_weight=0.0, weight=None, shuffle=False, as_arrays=False):
    """A deterministic synthetic vocabulary as the file's bytes: a k-ary tree of depth L with random 256-bit node descriptors and
    word weights in [0.5, 3) (`weight`: that value for every word).
      leaf_above            the root's first child has no children: a leaf (a word) at level 1 beside the deeper branches
      single_child          the root's last child has a single child
      duplicate_children    in every inner node the second child repeats the first child's descriptor
      equidistant_children  in every inner node the last child is the first child's descriptor with bits 0 and 1 flipped: the
                            first child's descriptor with bit 0 flipped is at distance 1 from both
      zero_weight           this fraction of the words (1.0: all) has weight 0: stop words
      shuffle               node and word records in a random order; node ids and word ids are random permutations as well
    """
    rng = np.random.Generator(np.random.PCG64(0xB0E_0000 + int(seed)))
    parents, descs = [], []                   # of nodes 1.., level by level; the children of a node are consecutive
    level, n_made = np.array([0]), 0          # the ids of the level being expanded
    for d in range(1, L + 1):
        nc = np.full(len(level), k)
        if d == 2 and leaf_above:
            nc[0] = 0
        if d == 2 and single_child:
            nc[-1] = 1
        first = np.concatenate([[0], np.cumsum(nc)[:-1]])
        ds = rng.integers(0, 2 ** 64, size=(int(nc.sum()), 4), dtype=np.uint64)
        if duplicate_children:
            two = nc >= 2
            ds[first[two] + 1] = ds[first[two]]
        if equidistant_children:
            two = nc >= 2
            ds[first[two] + nc[two] - 1] = ds[first[two]]
            ds[first[two] + nc[two] - 1, 0] ^= np.uint64(3)
        parents.append(np.repeat(level, nc)); descs.append(ds)
        level = n_made + 1 + np.arange(int(nc.sum()))
        n_made += int(nc.sum())
    parent = np.concatenate(parents); desc = np.concatenate(descs)
    nn = len(parent)
    has_child = np.zeros(nn + 1, bool); has_child[parent] = True
    leaves = 1 + np.nonzero(~has_child[1:])[0]
    nw = len(leaves)
    wts = np.zeros(nn + 1)
    wts[leaves] = rng.uniform(0.5, 3.0, nw) if weight is None else weight
    n_zero = int(round(zero_weight * nw))
    if n_zero:
        wts[rng.permutation(leaves)[:n_zero]] = 0.0
    new_id = np.arange(nn + 1)
    word_ids = np.arange(nw)
    if shuffle:
        new_id[1:] = 1 + rng.permutation(nn)
        word_ids = rng.permutation(nw)
    nodes = np.zeros(nn, dtype=NODE_DTYPE)
    nodes["id"] = new_id[1:]; nodes["parent"] = new_id[parent]; nodes["weight"] = wts[1:]; nodes["desc"] = desc
    words = np.zeros(nw, dtype=WORD_DTYPE)
    words["node"] = new_id[leaves]; words["word"] = word_ids
    if shuffle:
        # (the order of a node's children IS the order of their records: the shuffled file describes another, equally valid tree)
        nodes = nodes[rng.permutation(nn)]
        words = words[rng.permutation(nw)]
    if as_arrays:
        return k, L, nodes, words
    return pack_vocabulary(k, L, nodes, words)


@functools.lru_cache(maxsize=4)
def _tree_tables(vocab):
    """(children [n_nodes + 1][kmax] file ids padded with -1, descriptors, weights, word ids) by file id"""
    _, _, _, _, nodes, words = unpack_vocabulary(vocab)
    nn = len(nodes)
    order = np.argsort(nodes["parent"], kind="stable")                 # records grouped by parent, record order kept
    par = nodes["parent"][order]
    start = np.searchsorted(par, np.arange(nn + 2))                    # children of v: order[start[v]:start[v + 1]]
    kmax = int((start[1:] - start[:-1]).max())
    children = np.full((nn + 1, kmax), -1, np.int64)
    children[par, np.arange(nn) - start[par]] = nodes["id"][order]
    desc = np.zeros((nn + 1, 4), np.uint64); desc[nodes["id"]] = nodes["desc"]
    wt = np.zeros(nn + 1); wt[nodes["id"]] = nodes["weight"]
    word_of = np.full(nn + 1, -1); word_of[words["node"]] = words["word"]
    return children, desc, wt, word_of


def words_of(vocab, brief):
    """the word id and weight of every descriptor by a vectorised descent of the file's tree (children in record order, the first of
    equal minima) -- a helper for make_place_stream; the kernels are not tested against it but against the tests' own brute force"""
    children, desc, wt, word_of = _tree_tables(bytes(vocab))
    brief = np.ascontiguousarray(brief, dtype=np.uint64).reshape(-1, 4)
    at = np.zeros(len(brief), np.int64)
    active = np.nonzero(children[at, 0] >= 0)[0]
    while len(active):
        ch = children[at[active]]                                      # [n][kmax]
        d = np.bitwise_count(brief[active][:, None, :] ^ desc[np.maximum(ch, 0)]).sum(axis=-1).astype(np.int64)
        d[ch < 0] = 1 << 20
        at[active] = ch[np.arange(len(active)), np.argmin(d, axis=1)]  # argmin: the first of equal minima
        active = active[children[at[active], 0] >= 0]
    return word_of[at], wt[at]


def make_place_stream(vocab, seed, n_keyframes=80, n_shared=20, n_private=40, revisits=None, flipped_bits=4, private=None):
    """Keyframes of a sequence as BRIEF descriptor arrays.  Keyframe i holds three groups: noisy copies (`flipped_bits` random bits
    flipped) of keyframe i - 1's `shared` group, a new `shared` group of n_shared descriptors that keyframe i + 1 will see again (so
    neighbours score high), and a `private` group of n_private descriptors nobody else sees -- except a keyframe that revisits
    it: revisits = {i: j} gives keyframe i noisy copies of keyframe j's private group instead of one of its own.  `private` =
    {j: array} supplies keyframe j's private group.  Every generated descriptor falls into a word of its own, so that keyframes
    that share no group share (flipped bits apart) no word.  Deterministic.  Returns the list of [n][4] uint64 arrays."""
    from .loop import flip_bits
    rng = np.random.Generator(np.random.PCG64(0xB0E_8000 + int(seed)))
    revisits, private = dict(revisits or {}), dict(private or {})
    used = set()
    for arr in private.values():
        used.update(words_of(vocab, arr)[0].tolist())

    def fresh(n):
        out = np.zeros((0, 4), np.uint64)
        while len(out) < n:
            cand = rng.integers(0, 2 ** 64, size=(4 * (n - len(out)) + 8, 4), dtype=np.uint64)
            ws, wt = words_of(vocab, cand)
            keep = []
            for c, w, t in zip(cand, ws.tolist(), wt.tolist()):
                if t > 0 and w not in used and len(out) + len(keep) < n:
                    used.add(w); keep.append(c)
            if not keep and len(used) >= int((unpack_vocabulary(vocab)[4]["weight"] > 0).sum()):
                raise ValueError("the vocabulary has too few words for this stream")
            if keep:
                out = np.vstack([out, np.array(keep, dtype=np.uint64)])
        return out

    def noisy(arr):
        return np.array([flip_bits(d, rng.permutation(256)[:flipped_bits]) for d in arr], dtype=np.uint64).reshape(-1, 4)

    shared, priv, frames = [], [], []
    for i in range(n_keyframes):
        shared.append(fresh(n_shared))
        if i in revisits:
            priv.append(None)
            mine = noisy(priv[revisits[i]])
        else:
            priv.append(np.ascontiguousarray(private[i], dtype=np.uint64).reshape(-1, 4) if i in private else fresh(n_private))
            mine = priv[i]
        groups = [noisy(shared[i - 1])] if i > 0 else []
        frames.append(np.vstack(groups + [shared[i], mine]))
    return frames
