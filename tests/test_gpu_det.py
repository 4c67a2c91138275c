"""GPU parity of the batched feature detection (k_det_mask / k_det_eig / k_det_cand / k_det_select, include/isvins_detect.h) against
the serial CPU restatement tests/native/isv_det_oracle.c over the scenario list of tests/det_cases.py, for min_dist 1, 3 and 30 on
separate handles and for both camera models; batch invariance, the slots left unchanged, the refusals that need a slot's state,
the grow-only block, and a three-frame chain of detection and tracking on one slot.

Compared with the restatement, with no tolerance anywhere: first the mask plane, the response plane and the candidate count through
the debug read-back, so that a wrong plane is reported as a wrong plane; then the result records, kept_index, new_pts and
new_un_pts byte for byte.  Only integers and correctly rounded float32 / double + - * / sqrt in one fixed order occur on both sides.

The selection keeps no bands on chip, so there is no band size to shrink and no parity test for one."""
import numpy as np
import pytest

import det_cases
import det_oracle as do
import trk_oracle as to
from isvins_amd import backend, detect as det, tracker as trk

pytestmark = pytest.mark.gpu

FIELDS = ("kept_index", "new_pts", "new_un_pts")


def _tracker(cfg):
    return trk.Tracker(cfg.max_slots, cfg.max_items, cfg.max_width, cfg.max_height, max_points=cfg.max_points,
                       fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, k1=cfg.k1, k2=cfg.k2, p1=cfg.p1, p2=cfg.p2)


def _detector(tr, cfg):
    return det.Detector(tr, cfg.max_items, max_points=cfg.max_points, max_corners=cfg.max_corners, min_dist=cfg.min_dist, quality_level=cfg.quality_level)


def _seed(tr, scen):
    """every scenario's image into its slot: a tracking item without points, prev == cur (an empty-slot scenario seeds nothing)"""
    items = [trk.TrkItem(s["item"].c.slot, s["image"], s["image"], None, s["width"]) for s in scen if s["image"] is not None]
    rs, _ = tr.track_batch(items)
    assert all(r.status == trk.ISV_TRK_OK for r in rs)


def _same(got, want, where):
    (rg, ag), (ro, ao) = got, (want.r, want.arrays)
    assert bytes(rg) == bytes(ro), (where, do.describe(rg), do.describe(ro))
    for f in FIELDS:
        g, o = getattr(ag, f), getattr(ao, f)
        assert g.shape == o.shape and g.tobytes() == o.tobytes(), (where, f, np.flatnonzero((g != o).reshape(len(g), -1).any(axis=1))[:8])


def _same_planes(dt, i, want, where):
    mask, nc = dt.read_plane(i, 1)
    assert np.array_equal(mask, want.mask), (where, "mask plane", np.argwhere(mask != want.mask)[:4])
    if want.eig is not None:
        eig, nc = dt.read_plane(i, 0)
        assert eig.tobytes() == want.eig.tobytes(), (where, "response plane", np.argwhere(eig != want.eig)[:4])
    else:
        with pytest.raises(backend.BackendError):
            dt.read_plane(i, 0)
    assert nc == want.r.n_candidates, (where, "candidate count")


@pytest.fixture(scope="module")
def seeded():
    """one tracker per camera model with the scenario images resident, shared by the tests: detection never modifies a slot"""
    out = {}
    for distorted in (True, False):
        tr = _tracker(det_cases.trk_config(distorted))
        _seed(tr, det_cases.scenarios())
        out[distorted] = tr
    yield out
    for tr in out.values():
        tr.close()


@pytest.mark.parametrize("min_dist,distorted", [(30, True), (30, False), (3, True), (1, True)])
def test_scenarios_in_one_call_against_restatement(seeded, min_dist, distorted):
    cfg, cam, scen, items, ref = do.reference(min_dist, distorted)
    tr = seeded[distorted]
    before = {(s["item"].c.slot, l): tr.read_level(s["item"].c.slot, l)
              for s in scen if s["image"] is not None for l in range(len(trk.levels(s["width"], s["image"].shape[0])))}
    dt = _detector(tr, cfg)
    rs, arrs = dt.detect_batch(items)
    seen = set()
    for i, (s, want) in enumerate(zip(scen, ref)):
        if want.r.status == det.ISV_DET_OK:          # the planes first: a wrong plane is a wrong plane
            _same_planes(dt, i, want, s["name"])
        else:
            with pytest.raises(backend.BackendError):
                dt.read_plane(i, 1)
        _same((rs[i], arrs[i]), want, s["name"])
        assert rs[i].status == s["want"], s["name"]
        seen.add(rs[i].status)
    assert seen == {det.ISV_DET_OK, det.ISV_DET_CAPACITY, det.ISV_DET_INPUT}
    for (slot, l), level in before.items():          # detection never modifies a slot
        assert np.array_equal(tr.read_level(slot, l), level), (slot, l)
    ms = dt.last_ms()
    assert len(ms) == 5 and all(0 <= m < 10000 for m in ms) and ms[0] > 0 and ms[1] > 0 and ms[0] >= ms[1] + ms[2] + ms[3]
    dt.close()


def test_batch_invariance(seeded):
    cfg, cam, scen, items, ref = do.reference(30, True)
    dt = _detector(seeded[True], cfg)
    rs, arrs = dt.detect_batch(items[::-1])
    for s, want, r, a in zip(scen[::-1], ref[::-1], rs, arrs):
        _same((r, a), want, ("reversed", s["name"]))
    for s, it, want in zip(scen, items, ref):
        r, a = dt.detect_batch([it])
        _same((r[0], a[0]), want, ("alone", s["name"]))
    assert dt.detect_batch([]) == ([], [])
    dt.close()


def test_small_large_small_calls_on_one_handle(seeded):
    cfg, cam, scen, items, ref = do.reference(3, True)
    by = {s["name"]: (it, want) for s, it, want in zip(scen, items, ref)}
    dt = _detector(seeded[True], cfg)
    for names in (["s64", "s24"], ["big"], ["s24", "s64"], ["s200", "big", "s97", "checker"], ["s64_one"], ["const"], ["nan_point"], ["s3x3", "rects"]):
        rs, arrs = dt.detect_batch([by[n][0] for n in names])
        for k, (n, r, a) in enumerate(zip(names, rs, arrs)):
            _same((r, a), by[n][1], (names, n))
            if by[n][1].r.status == det.ISV_DET_OK:
                _same_planes(dt, k, by[n][1], (names, n))
    dt.close()


def test_slot_refusals():
    lib = do.load()
    cfg, cam, scen, items, ref = do.reference(30, True)
    by = {s["name"]: (s, it, want) for s, it, want in zip(scen, items, ref)}
    tcfg = trk.make_config(4, 4, 200, 170, max_points=40)
    tr = _tracker(tcfg)
    dt = det.Detector(tr, 8, max_points=40, max_corners=400, min_dist=30)
    s, it, want = by["s64_one"]
    first = by["s64_first"]
    # an empty slot; a slot outside the tracker's; the good item between them is not disturbed
    (r,), _ = tr.track_batch([trk.TrkItem(1, s["image"], s["image"])])
    assert r.status == trk.ISV_TRK_OK
    rs, arrs = dt.detect_batch([it.on_slot(0), it.on_slot(1), it.on_slot(4), it.on_slot(-1)])
    assert [r.status for r in rs] == [det.ISV_DET_INPUT, det.ISV_DET_OK, det.ISV_DET_INPUT, det.ISV_DET_INPUT]
    _same((rs[1], arrs[1]), want, "between empty slots")
    # a slot named twice: both items are refused, whatever their order; a malformed item naming the slot does not count
    rs, arrs = dt.detect_batch([it.on_slot(1), first[1].on_slot(1)])
    assert [r.status for r in rs] == [det.ISV_DET_INPUT, det.ISV_DET_INPUT] and rs[0].n_points == 1 and rs[0].n_new == 0
    bad = det.DetItem(1, [[np.inf, 3.0]], [1], 5)
    rs, arrs = dt.detect_batch([bad, it.on_slot(1)])
    assert [r.status for r in rs] == [det.ISV_DET_INPUT, det.ISV_DET_OK]
    _same((rs[1], arrs[1]), want, "beside a malformed item on the same slot")
    # a point inside a larger image's bounds but outside this slot's; a reset slot is empty again
    rs, _ = dt.detect_batch([det.DetItem(1, [[63.0, 48.0]], [1], 5), det.DetItem(1, [[-0.75, 3.0]], [1], 5)])
    assert [r.status for r in rs] == [det.ISV_DET_INPUT, det.ISV_DET_INPUT]
    tr.slot_reset(1)
    (r,), _ = dt.detect_batch([it.on_slot(1)])
    assert r.status == det.ISV_DET_INPUT
    with pytest.raises(backend.BackendError):
        dt.detect_batch([it.on_slot(1)] * 9)         # more items than max_items
    dt.close()
    tr.close()


def test_three_frame_chain_of_detection_and_tracking_on_one_slot():
    dlib, tlib = do.load(), to.load()
    w, h, MAX_CNT = 200, 120, 40
    tcfg = trk.make_config(2, 2, w, h, max_points=64)
    dcfg = det.make_config(2, 64, MAX_CNT, 12, det.QUALITY)
    frames = [trk.analytic_image(w, h, s, 50) for s in ((0, 0), (2.25, -1.5), (5.0, -2.75))]
    tr = _tracker(tcfg)
    dt = _detector(tr, dcfg)

    def both_detect(frame, pts, cnt, max_new):
        item = det.DetItem(1, pts, cnt, max_new)
        want = do.detect(dlib, dcfg, tcfg, frame, item)
        (r,), (a,) = dt.detect_batch([item])
        _same_planes(dt, 0, want, "chain")
        _same((r, a), want, "chain")
        return a

    def both_track(cur, prev, pts):
        want = to.track(tlib, tcfg, trk.TrkItem(1, cur, prev, pts))
        (r,), (a,) = tr.track_batch([trk.TrkItem(1, cur, None, pts)])
        assert bytes(r) == bytes(want.r) and a.cur_pts.tobytes() == want.arrays.cur_pts.tobytes() and a.flags.tobytes() == want.arrays.flags.tobytes()
        return a

    # frame 0: the slot takes the image, the first corners are born
    (r,), _ = tr.track_batch([trk.TrkItem(1, frames[0], frames[0])])
    assert r.status == trk.ISV_TRK_OK
    a0 = both_detect(frames[0], None, None, MAX_CNT)
    pts, cnt = a0.new_pts.copy(), np.ones(len(a0.new_pts), np.int32)
    assert 10 <= len(pts) <= MAX_CNT
    for f in (1, 2):
        # track into frame f, compact (reduceVector), track_cnt++, setMask and the new corners
        t = both_track(frames[f], frames[f - 1], pts)
        pts, _, cnt = t.kept(cnt)
        cnt = cnt + 1
        assert len(pts) >= 8
        a = both_detect(frames[f], pts, cnt, MAX_CNT - len(pts))
        pts = np.vstack([pts[a.kept_index], a.new_pts]) if len(a.new_pts) else pts[a.kept_index]
        cnt = np.concatenate([cnt[a.kept_index], np.ones(len(a.new_pts), np.int32)])
        d2 = ((np.rint(pts)[:, None, :] - np.rint(pts)[None, :, :]) ** 2).sum(axis=2) + np.eye(len(pts)) * 1e9
        assert d2.min() >= 1 and len(pts) <= MAX_CNT
    dt.close()
    tr.close()
