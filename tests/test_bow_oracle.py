"""Pins the serial restatement tests/native/isv_bow_oracle.c (to which the GPU is compared bit for bit) independently of it:
  * the transform against a brute-force descent written here (word ids identical; the values against the repeated addition and
    the ordered norm done in Python floats, which are IEEE doubles: identical);
  * Score against 1 - 0.5 ||v - w||_1 formed densely in numpy: |difference| <= 1e-12, pure rounding of sums of at most 8192 terms
    of magnitude <= 1 (2 x 8192 x 2^-53 = 1.8e-12 is the crude bound; the vectors here have at most 300 words).  Measured worst
    over the scenario list: 4.4e-16;
  * each kept quirk B1..B4 flips a result when switched off, and a tie gives the lower id;
  * -O0 and -O2 builds answer the whole GPU scenario list with identical bits."""
import numpy as np
import pytest

import bow_cases
import bow_oracle
from isvins_amd import bow


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bow_oracle.build(tmp_path_factory.mktemp("bow_oracle"))


@pytest.fixture(scope="module")
def vocabs():
    return bow_cases.vocabularies()


def cfg():
    return bow.make_config(1, 1, bow_cases.MAX_FEATURES)


def brute_words(vocab, brief, last=False):
    """(word id or -1 for a stop word, weight) per descriptor: a plain descent of the file's tree"""
    _, _, _, _, nodes, words = bow.unpack_vocabulary(vocab)
    children, rec = {}, {}
    for r in nodes:
        children.setdefault(int(r["parent"]), []).append(int(r["id"]))
        rec[int(r["id"])] = r
    word_of = {int(w["node"]): int(w["word"]) for w in words}
    out = []
    for f in brief:
        at = 0
        while at in children:
            best, best_d = None, None
            for c in children[at]:
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(f, rec[c]["desc"]))
                if best is None or d < best_d or (last and d == best_d):
                    best, best_d = c, d
            at = best
        out.append((word_of[at], float(rec[at]["weight"])))
    return out


def brute_vector(vocab, brief):
    acc = {}
    for w, wt in brute_words(vocab, brief):
        if wt > 0:
            acc[w] = acc[w] + wt if w in acc else wt
    ids = sorted(acc)
    norm = 0.0
    for w in ids:
        norm += abs(acc[w])
    return np.array(ids, dtype=np.uint32), np.array([acc[w] / norm if norm > 0 else acc[w] for w in ids])


def test_transform_against_brute_force(lib, vocabs):
    for name, vb in vocabs.items():
        o = bow_oracle.Oracle(lib, vb, cfg())
        sets = [bow_cases.features(7, n) for n in (0, 1, 65, 257)] + [bow_cases.tie_features(vb)]
        if name == "w0.1":
            sets.append(bow_cases.repeated_features(vb))
        for f in sets:
            w, v = o.transform(f)
            bw, bv = brute_vector(vb, f)
            assert np.array_equal(w, bw), name
            assert v.tobytes() == bv.tobytes(), name
            if name == "all_stop":
                assert len(w) == 0
        o.close()


def test_repeated_addition_is_not_a_product(lib, vocabs):
    """0.1 added 7 times is not 7 * 0.1: the restatement (and the reference) adds"""
    vb = vocabs["w0.1"]
    o = bow_oracle.Oracle(lib, vb, cfg())
    f = bow_cases.repeated_features(vb)
    ws = [w for w, _ in brute_words(vb, f)]
    counts = sorted(ws.count(w) for w in set(ws))
    assert counts == [1, 2, 7, 100]
    w, v = o.transform(f)
    acc = {c: sum([0.1] * c) for c in counts}
    assert acc[7] != 7 * 0.1
    norm = 0.0
    for wid in w.tolist():
        norm += acc[ws.count(wid)]
    assert [x for x in v.tolist()] == [acc[ws.count(wid)] / norm for wid in w.tolist()]
    prod = [ws.count(wid) * 0.1 for wid in w.tolist()]
    assert v.tolist() != [p / sum(prod) for p in prod]
    o.close()


def test_tie_takes_the_first_child(lib, vocabs):
    """on descriptors at equal distance from two children the restatement answers as the strict < descent does, and a descent that
    took the last of equal minima would answer differently"""
    for name in ("duplicates", "equidistant"):
        vb = vocabs[name]
        f = bow_cases.tie_features(vb)
        first = [w for w, _ in brute_words(vb, f)]
        last = [w for w, _ in brute_words(vb, f, last=True)]
        assert first != last, name
        o = bow_oracle.Oracle(lib, vb, cfg())
        w, _ = o.transform(f)
        assert w.tolist() == sorted(set(first)) and w.tolist() != sorted(set(last)), name
        o.close()


def dense_score(n_words, qw, qv, dw, dv):
    a, b = np.zeros(n_words), np.zeros(n_words)
    a[qw] = qv; b[dw] = dv
    return 1.0 - 0.5 * np.abs(a - b).sum()


def test_score_against_dense_l1(lib, vocabs):
    worst = 0.0
    for sc in bow_cases.scenarios():
        vb = vocabs[sc["vocab"]]
        nw = len(bow.unpack_vocabulary(vb)[5])
        o = bow_oracle.Oracle(lib, vb, cfg())
        entries = []
        for it in sc["items"]:
            r, w, v = o.detect(it)
            if r.status != bow.ISV_BOW_OK:
                continue
            for i in range(r.n_results):
                dw, dv = entries[r.result_id[i]]
                if len(w) and len(dw):       # (an empty vector has norm 0, not 1: the identity needs two normalised vectors)
                    worst = max(worst, abs(r.result_score[i] - dense_score(nw, w, v, dw, dv)))
            if it.c.mode != bow.ISV_BOW_QUERY:
                assert r.entry_id == len(entries)
                entries.append((w.copy(), v.copy()))
        o.close()
    print(f"worst |Score - (1 - 0.5 |v - w|_1)| = {worst:.3e}")
    assert worst <= 1e-12


def _db70(lib, vocabs, vn="k10L3"):
    o = bow_oracle.Oracle(lib, vocabs[vn], cfg())
    h = bow_cases.history(vocabs[vn], 70, 70)
    for i, f in enumerate(h):
        o.detect(bow.BowItem(0, i, f, bow.ISV_BOW_ADD))
    return o, h


def test_each_quirk_flips_a_result(lib, vocabs):
    o, h = _db70(lib, vocabs)
    q = bow.ISV_BOW_QUERY
    # B1: frame 49 has max_id == -1: every entry is eligible; frame 48 (max_id -2) sees the newest entry only
    r49, r48 = o.detect(bow.BowItem(0, 49, h[12], q))[0], o.detect(bow.BowItem(0, 48, h[12], q))[0]
    off = o.detect(bow.BowItem(0, 49, h[12], q), bow_oracle.B1)[0]
    assert r49.n_scored > 4 and r48.n_scored <= 1 and off.n_scored == r48.n_scored
    # B2: the newest entry (69) is eligible although 69 >= max_id
    r, off = o.detect(bow.BowItem(0, 69, h[69], q))[0], o.detect(bow.BowItem(0, 69, h[69], q), bow_oracle.B2)[0]
    assert r.result_id[0] == 69 and r.result_score[0] > 0.99 and 69 not in list(off.result_id) and off.n_scored == r.n_scored - 1
    # B4: at frame 49 the query runs (B1: over everything), the loop is found, and only then the gate says -1
    assert r49.find_loop == 1 and r49.loop_index == -1
    off = o.detect(bow.BowItem(0, 49, h[12], q), bow_oracle.B4)[0]
    assert off.find_loop == 0 and off.n_scored == 0 and off.n_results == 0
    r50, r51 = o.detect(bow.BowItem(0, 50, h[12], q))[0], o.detect(bow.BowItem(0, 51, h[12], q))[0]
    assert r50.n_scored == 1 and r50.result_id[0] == 69 and r50.loop_index == -1      # max_id 0: the newest entry alone
    assert r51.n_scored == 2 and sorted(r51.result_id[:2]) == [0, 69]
    assert r51.find_loop == 1 and r51.loop_index == 0
    o.close()
    # B3: ret[0] belongs to the minimum
    o = bow_oracle.Oracle(lib, vocabs["k10L3"], cfg())
    items = bow_cases.b3_case(vocabs["k10L3"])
    for it in items[:-1]:
        o.detect(it)
    r, off = o.detect(items[-1])[0], o.detect(items[-1], bow_oracle.B3)[0]
    assert list(r.result_id[:3]) == [3, 7, 11] and r.loop_index == 3 and off.loop_index == 7
    o.close()


def test_newest_entry_as_ret0_and_not(lib, vocabs):
    o, h = _db70(lib, vocabs)
    r = o.detect(bow.BowItem(0, 120, h[69], bow.ISV_BOW_QUERY))[0]
    assert r.result_id[0] == 69
    r = o.detect(bow.BowItem(0, 120, h[12], bow.ISV_BOW_QUERY))[0]
    assert r.result_id[0] != 69 and r.n_results == 4
    o.close()


def test_ties_give_the_lower_id(lib, vocabs):
    """history() repeats every fifth keyframe: entries 2 and 3 are identical, so are their scores"""
    o, h = _db70(lib, vocabs)
    assert h[2].tobytes() == h[3].tobytes()
    r = o.detect(bow.BowItem(0, 120, h[3], bow.ISV_BOW_QUERY))[0]
    assert list(r.result_id[:2]) == [2, 3] and r.result_score[0] == r.result_score[1]
    o.close()


def test_absent_entries_and_counts(lib, vocabs):
    o, h = _db70(lib, vocabs)
    r = o.detect(bow.BowItem(0, 1000, bow_cases.features(99999, 3), bow.ISV_BOW_QUERY))[0]
    assert r.n_scored < 70                        # entries sharing no word are absent, and the empty entries always are
    r = o.detect(bow.BowItem(0, 1000, np.zeros((0, 4), np.uint64), bow.ISV_BOW_QUERY))[0]
    assert (r.n_words, r.n_scored, r.n_results, r.loop_index) == (0, 0, 0, -1)
    o.close()


def test_o0_and_o2_agree_bitwise(lib, vocabs, tmp_path):
    lib0 = bow_oracle.build(tmp_path, "-O0")
    for sc in bow_cases.scenarios():
        a, b = bow_oracle.Oracle(lib, vocabs[sc["vocab"]], cfg()), bow_oracle.Oracle(lib0, vocabs[sc["vocab"]], cfg())
        for it in sc["items"]:
            (ra, wa, va), (rb, wb, vb) = a.detect(it), b.detect(it)
            assert bytes(ra) == bytes(rb) and wa.tobytes() == wb.tobytes() and va.tobytes() == vb.tobytes(), sc["name"]
        a.close(); b.close()
