"""GPU parity of the batched keyframe extraction (k_kf_blur / k_kf_fast / k_kf_select / k_kf_brief, include/isvins_keyframe.h)
against the serial CPU restatement tests/native/isv_kf_oracle.c over the scenario list of tests/kf_cases.py, batch invariance, the
refusals, both camera models, the grow-only block, and the way onward into the loop detection and the loop verification.

Compared with the restatement, with no tolerance anywhere: the result records byte for byte, keypoints_uv, score, brief and
window_brief byte for byte, keypoints_norm bitwise as float32, and -- through the debug read-back -- the blurred image and the
score map, so that a wrong blur is reported as a wrong blur.  Only integers and correctly rounded double + - * / in one fixed order
occur on both sides."""
import numpy as np
import pytest

import kf_cases
import kf_oracle
from isvins_amd import bow, keyframe as kf, loop

pytestmark = pytest.mark.gpu

FIELDS = ("keypoints_uv", "score", "brief", "window_brief", "keypoints_norm")


def _extractor(cfg):
    pat = {k: np.array(getattr(cfg, k), dtype=np.int8) for k in ("x1", "y1", "x2", "y2")}
    return kf.KeyframeExtractor(cfg.max_items, cfg.max_width, cfg.max_height, max_keypoints=cfg.max_keypoints, max_points=cfg.max_points,
                                fast_threshold=cfg.fast_threshold, pattern=pat, fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, k1=cfg.k1, k2=cfg.k2,
                                p1=cfg.p1, p2=cfg.p2)


def _same(got, want, where):
    (rg, ag), (ro, ao) = got, want
    assert bytes(rg) == bytes(ro), (where, kf_oracle.describe(rg), kf_oracle.describe(ro))
    for f in FIELDS:
        g, o = getattr(ag, f), getattr(ao, f)
        assert g.shape == o.shape and g.tobytes() == o.tobytes(), (where, f)


@pytest.mark.parametrize("distorted", [True, False])
def test_scenarios_in_one_call_against_restatement(distorted):
    cfg, scen, ref = kf_oracle.reference(distorted)
    ext = _extractor(cfg)
    rs, arrs = ext.extract_batch([s["item"] for s in scen])
    seen = set()
    for i, (s, (ro, ao, blur, smap)) in enumerate(zip(scen, ref)):
        if blur is not None:              # the intermediate images first: a wrong blur is a wrong blur
            gb, gs = ext.read_back(i, s["item"].c.width, s["item"].c.height)
            assert np.array_equal(gb, blur), (s["name"], "blurred image")
            assert np.array_equal(gs, smap), (s["name"], "score map")
        _same((rs[i], arrs[i]), (ro, ao), s["name"])
        assert rs[i].status == s["want"], s["name"]
        seen.add(rs[i].status)
    assert seen == {kf.ISV_KF_OK, kf.ISV_KF_CAPACITY, kf.ISV_KF_INPUT}
    over = [i for i, s in enumerate(scen) if s["name"] == "over_keypoints"][0]
    assert rs[over].n_keypoints == ref[over][0].n_keypoints > cfg.max_keypoints
    ms = ext.last_ms()
    assert len(ms) == 7 and all(m >= 0 for m in ms) and ms[0] > 0
    ext.close()


def test_batch_invariance():
    cfg, scen, ref = kf_oracle.reference(True)
    ext = _extractor(cfg)
    items = [s["item"] for s in scen]
    rs, arrs = ext.extract_batch(items[::-1])
    for s, want, r, a in zip(scen[::-1], ref[::-1], rs, arrs):
        _same((r, a), want[:2], ("reversed", s["name"]))
    for s, want in zip(scen, ref):
        r, a = ext.extract_batch([s["item"]])
        _same((r[0], a[0]), want[:2], ("alone", s["name"]))
    assert ext.extract_batch([]) == ([], [])
    ext.close()


def test_refused_items_between_good_ones():
    cfg, scen, ref = kf_oracle.reference(True)
    by = {s["name"]: (s["item"], want) for s, want in zip(scen, ref)}
    names = ["over_keypoints", "small", "nan_point", "too_wide", "mid", "bad_stride", "over_points", "tiny7", "null_image", "strided", "inf_point"]
    ext = _extractor(cfg)
    # extract_batch pre-fills every array with a pattern and asserts that a refused item's are untouched
    rs, arrs = ext.extract_batch([by[n][0] for n in names])
    for n, r, a in zip(names, rs, arrs):
        _same((r, a), by[n][1][:2], n)
    assert [r.status for r in rs] == [1, 0, 2, 1, 0, 2, 1, 0, 2, 0, 2]
    assert rs[0].n_keypoints == by["over_keypoints"][1][0].n_keypoints and all(len(getattr(arrs[0], f)) == 0 for f in FIELDS)
    ext.close()


def test_grow_only_block():
    cfg, scen, ref = kf_oracle.reference(True)
    by = {s["name"]: (s["item"], want) for s, want in zip(scen, ref)}
    ext = _extractor(cfg)
    for names in (["small", "tiny7"], ["big"], ["tiny7", "small"], ["mid", "big", "strided"], ["small"]):
        rs, arrs = ext.extract_batch([by[n][0] for n in names])
        for n, r, a in zip(names, rs, arrs):
            _same((r, a), by[n][1][:2], (names, n))
    ext.close()


def test_onward_without_conversion():
    a_img, b_img, (dx, dy) = kf_cases.texture_crops()
    H, W = a_img.shape
    ext = kf.KeyframeExtractor(2, W, H, max_keypoints=2048, max_points=2048)
    (rb,), (b,) = ext.extract_batch([kf.KfItem(b_img)])
    # the current keyframe: crop a, its window points the old keyframe's (crop b's) corners shifted by the offset
    pts = b.keypoints_uv + np.array([dx, dy], np.float32)
    (ra, rb2), (a, b2) = ext.extract_batch([kf.KfItem(a_img, pts), kf.KfItem(b_img)])
    assert ra.status == rb.status == rb2.status == kf.ISV_KF_OK and rb.n_keypoints > 50
    assert b2.brief.tobytes() == b.brief.tobytes()
    ext.close()
    # into the loop detection as they are
    vocab = bow.make_vocabulary(3, k=10, L=3)
    det = bow.LoopDetector(vocab, 2, 2, 2048)
    items = [bow.BowItem(0, 0, a.brief), bow.BowItem(1, 0, b.brief)]
    assert items[0].brief.ctypes.data == a.brief.ctypes.data or np.shares_memory(items[0].brief, a.brief)
    res = det.detect_batch(items)
    assert [r.status for r in res] == [bow.ISV_BOW_OK] * 2 and all(r.n_words > 0 for r in res)
    det.close()
    # into the loop verification as they are: every interior corner of crop b is found again in crop a at distance 0
    n = len(pts)
    p3d = np.column_stack([b.keypoints_norm * 4.0, np.full(n, 4.0)]).astype(np.float32)
    pair = loop.LoopPair(a.window_brief, p3d, b.keypoints_norm, b.brief, b.keypoints_norm, np.zeros(3), np.eye(3))
    assert np.shares_memory(pair.window_brief, a.window_brief) and np.shares_memory(pair.brief, b.brief) and np.shares_memory(pair.keypoints_norm, b.keypoints_norm)
    ver = loop.LoopVerifier(1, 2048, 2048)
    _, mi, md, _ = ver.verify_batch([pair], per_point=True)
    ver.close()
    m = 28 + 4
    xb, yb = b.keypoints_uv[:, 0], b.keypoints_uv[:, 1]
    interior = (xb >= m) & (xb < W - m) & (yb >= m) & (yb < H - m) & (pts[:, 0] >= m) & (pts[:, 0] < W - m) & (pts[:, 1] >= m) & (pts[:, 1] < H - m)
    assert interior.sum() >= 10
    assert (md[0][interior] == 0).all()
    assert (mi[0][interior] >= 0).all()
