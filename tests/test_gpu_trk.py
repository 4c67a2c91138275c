"""GPU parity of the batched feature tracking (k_trk_level0 / k_trk_pyrdown / k_trk_track, include/isvins_tracker.h) against the
serial CPU restatement tests/native/isv_trk_oracle.c over the scenario list of tests/trk_cases.py, batch invariance, prev uploaded
against prev resident, a chain of frames on one slot, the slot refusals, isv_trk_slot_reset, both camera models and the grow-only
block.

Compared with the restatement, with no tolerance anywhere: first every level of both pyramids through the debug read-back, so that
a wrong pyramid is reported as a wrong pyramid; then the result records, cur_pts, flags, err and cur_un_pts byte for byte.  Only
integers and correctly rounded float32 / double + - * / sqrt in one fixed order occur on both sides."""
import numpy as np
import pytest

import trk_oracle as to
from isvins_amd import backend, tracker as trk

pytestmark = pytest.mark.gpu

FIELDS = ("cur_pts", "flags", "err", "cur_un_pts")


def _tracker(cfg):
    return trk.Tracker(cfg.max_slots, cfg.max_items, cfg.max_width, cfg.max_height, max_points=cfg.max_points,
                       fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, k1=cfg.k1, k2=cfg.k2, p1=cfg.p1, p2=cfg.p2)


def _same(got, want, where):
    (rg, ag), (ro, ao) = got, (want.r, want.arrays)
    assert bytes(rg) == bytes(ro), (where, to.describe(rg), to.describe(ro))
    for f in FIELDS:
        g, o = getattr(ag, f), getattr(ao, f)
        assert g.shape == o.shape and g.tobytes() == o.tobytes(), (where, f, np.flatnonzero((g != o).reshape(len(g), -1).any(axis=1))[:8])


def _same_pyramids(tr, slot, want, where):
    for which, pyr in ((0, want.pyr_cur), (1, want.pyr_prev)):
        for l, level in enumerate(pyr):
            assert np.array_equal(tr.read_level(slot, l, which), level), (where, "cur" if which == 0 else "prev", "pyramid level", l)
        with pytest.raises(backend.BackendError):
            tr.read_level(slot, len(pyr), which)


def _good(ref):
    cfg, scen, res = ref
    return [(s, t) for s, t in zip(scen, res) if t.r.status == trk.ISV_TRK_OK]


@pytest.mark.parametrize("distorted", [True, False])
def test_scenarios_in_one_call_against_restatement(distorted):
    cfg, scen, ref = to.reference(distorted)
    tr = _tracker(cfg)
    rs, arrs = tr.track_batch([s["item"] for s in scen])
    seen = set()
    for i, (s, want) in enumerate(zip(scen, ref)):
        if want.pyr_cur is not None:      # the pyramids first: a wrong pyramid is a wrong pyramid
            _same_pyramids(tr, s["item"].c.slot, want, s["name"])
        _same((rs[i], arrs[i]), want, s["name"])
        assert rs[i].status == s["want"], s["name"]
        seen.add(rs[i].status)
    assert seen == {trk.ISV_TRK_OK, trk.ISV_TRK_CAPACITY, trk.ISV_TRK_INPUT}
    assert {r.n_levels for r in rs if r.status == trk.ISV_TRK_OK} == {1, 2, 3, 4}
    ms = tr.last_ms()
    assert len(ms) == 5 and all(0 <= m < 10000 for m in ms) and ms[0] > 0 and ms[2] > 0 and ms[0] >= ms[1] + ms[2]
    tr.close()


def test_batch_invariance():
    cfg, scen, ref = to.reference(True)
    tr = _tracker(cfg)
    items = [s["item"] for s in scen]
    rs, arrs = tr.track_batch(items[::-1])
    for s, want, r, a in zip(scen[::-1], ref[::-1], rs, arrs):
        _same((r, a), want, ("reversed", s["name"]))
    for s, want in zip(scen, ref):
        r, a = tr.track_batch([s["item"]])
        _same((r[0], a[0]), want, ("alone", s["name"]))
    assert tr.track_batch([]) == ([], [])
    tr.close()


def test_prev_uploaded_against_prev_resident():
    ref = to.reference(True)
    cfg = ref[0]
    good = _good(ref)
    tr = _tracker(cfg)
    # the slots take the prev images (as cur, without points), then the same frames without prev: the same bytes
    seeds = [trk.TrkItem(s["item"].c.slot, s["item"].prev, s["item"].prev, None, s["item"].c.width) for s, _ in good]
    rs, _ = tr.track_batch(seeds)
    assert all(r.status == trk.ISV_TRK_OK and r.n_points == 0 and r.n_kept == 0 for r in rs)
    rs, arrs = tr.track_batch([s["item"].with_prev(None) for s, _ in good])
    for (s, want), r, a in zip(good, rs, arrs):
        _same_pyramids(tr, s["item"].c.slot, want, ("resident", s["name"]))
        _same((r, a), want, ("resident", s["name"]))
    tr.close()


def test_three_frame_chain_on_one_slot():
    lib = to.load()
    cfg = trk.make_config(2, 2, 200, 120, max_points=64)
    w, h = 200, 120
    frames = [trk.analytic_image(w, h, s, 50) for s in ((0, 0), (2.25, -1.5), (5.0, -2.75))]
    pts0 = np.array([(x, y) for y in np.arange(20.0, h, 27.5) for x in np.arange(15.0, w, 31.25)], np.float32)
    tr = _tracker(cfg)
    w1 = to.track(lib, cfg, trk.TrkItem(1, frames[1], frames[0], pts0))
    (r1,), (a1,) = tr.track_batch([trk.TrkItem(1, frames[1], frames[0], pts0)])
    _same((r1, a1), w1, "frame 1")
    pts1, _, kept0 = a1.kept(pts0)
    assert len(pts1) >= 10
    w2 = to.track(lib, cfg, trk.TrkItem(1, frames[2], frames[1], pts1))
    (r2,), (a2,) = tr.track_batch([trk.TrkItem(1, frames[2], None, pts1)])
    _same_pyramids(tr, 1, w2, "frame 2")
    _same((r2, a2), w2, "frame 2")
    assert r2.n_kept >= 10 and np.abs(a2.kept()[0] - a2.kept(kept0)[2] - [5.0, -2.75]).max() < 0.5
    tr.close()


def test_slot_refusals_leave_the_slot_untouched():
    ref = to.reference(True)
    cfg, scen, res = ref
    by = {s["name"]: (s["item"], t) for s, t in zip(scen, res)}
    s64, w64 = by["s64"]
    s97, _ = by["s97"]
    s24, w24 = by["s24"]
    tr = _tracker(cfg)
    A, B = 3, 5
    # an empty slot cannot supply prev; the good item in the same call is not disturbed
    rs, arrs = tr.track_batch([s64.with_prev(None, slot=A), s24.with_prev(s24.prev, slot=B)])
    assert [r.status for r in rs] == [trk.ISV_TRK_INPUT, trk.ISV_TRK_OK] and rs[0].n_points == s64.c.n_points and rs[0].n_levels == 0
    _same((rs[1], arrs[1]), w24, "beside an empty slot")
    with pytest.raises(backend.BackendError):
        tr.read_level(A, 0)
    # slot A takes s64's prev image
    (r,), _ = tr.track_batch([trk.TrkItem(A, s64.prev, s64.prev, None, 64)])
    assert r.status == trk.ISV_TRK_OK
    before = [tr.read_level(A, l) for l in range(2)]
    # a changed size, the same slot twice (both items are refused), and all of it between good items
    other = trk.TrkItem(A, s97.cur, None, s97.points, 97)
    twice = [s64.with_prev(None, slot=A), s64.with_prev(s64.prev, slot=A)]
    rs, arrs = tr.track_batch([other, s24.with_prev(None, slot=B)])
    assert [r.status for r in rs] == [trk.ISV_TRK_INPUT, trk.ISV_TRK_OK]
    rs, arrs = tr.track_batch([twice[0], s24.with_prev(s24.prev, slot=B), twice[1]])
    assert [r.status for r in rs] == [trk.ISV_TRK_INPUT, trk.ISV_TRK_OK, trk.ISV_TRK_INPUT]
    _same((rs[1], arrs[1]), w24, "between a slot named twice")
    # a malformed item naming the slot does not count as naming it
    nan = s64.with_prev(None, slot=A); nan.points = s64.points.copy(); nan.points[0, 0] = np.nan
    nan.c.prev_pts = nan.points.ctypes.data_as(trk._f32p)
    rs, arrs = tr.track_batch([nan])
    assert rs[0].status == trk.ISV_TRK_INPUT
    for l in range(2):
        assert np.array_equal(tr.read_level(A, l), before[l])
    # provably untouched: the next good item on the slot, prev resident, gives the restatement's bytes
    (r,), (a,) = tr.track_batch([s64.with_prev(None, slot=A)])
    _same((r, a), w64, "after the refusals")
    _same_pyramids(tr, A, w64, "after the refusals")
    # isv_trk_slot_reset empties the slot
    tr.slot_reset(A)
    with pytest.raises(backend.BackendError):
        tr.read_level(A, 0)
    (r,), _ = tr.track_batch([s64.with_prev(None, slot=A)])
    assert r.status == trk.ISV_TRK_INPUT
    (r,), (a,) = tr.track_batch([s64.with_prev(s64.prev, slot=A)])
    _same((r, a), w64, "after the reset")
    with pytest.raises(backend.BackendError):
        tr.slot_reset(cfg.max_slots)
    tr.close()


def test_small_large_small_calls_on_one_handle():
    ref = to.reference(True)
    by = {s["name"]: (s["item"], t) for s, t in zip(ref[1], ref[2])}
    tr = _tracker(ref[0])
    for names in (["s64", "s24"], ["big"], ["s24", "s64"], ["s200", "big", "s97", "checker"], ["s64"], ["no_points"]):
        rs, arrs = tr.track_batch([by[n][0] for n in names])
        for n, r, a in zip(names, rs, arrs):
            _same((r, a), by[n][1], (names, n))
    ms = tr.last_ms()
    assert all(0 <= m < 10000 for m in ms)
    tr.close()
