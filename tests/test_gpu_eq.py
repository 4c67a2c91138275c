"""GPU parity of the batched CLAHE (k_eq_lut / k_eq_interp, include/isvins_equalize.h) against the serial CPU restatement
tests/native/isv_eq_oracle.c, with no tolerance anywhere: isv_eq_apply_batch over nine sizes, five contents and four parameter sets
in one call each, refused items between the good ones, first the tiles' LUTs through the debug read-back, so that a wrong LUT is
reported as a wrong LUT, then the images byte for byte; isv_eq_track_batch against the tracker's restatement run on the restated images (level 0 of both slot buffers first), prev uploaded and resident,
batch invariance and the grow-only block; the slots' tags; and a three-frame chain of detection and equalised tracking on one slot.

Only integers and correctly rounded float32 / double + - * / in one fixed order occur on both sides."""
import functools

import numpy as np
import pytest

import det_oracle as do
import eq_oracle as eo
import trk_oracle as to
from isvins_amd import backend, detect as det, equalize as eq, tracker as trk
from test_gpu_det import _detector, _same, _same_planes, _tracker

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, None), (3, 3, None), (8, 8, None), (9, 9, None), (15, 17, None), (64, 48, None), (97, 61, 104), (200, 120, None), (752, 480, None)]
MAX_W, MAX_H = 752, 480


def _cfg(p, max_items=1):
    return eq.make_config(p[0], p[1], p[2], max_items)


def _equalizer(tr, p, max_items):
    return eq.Equalizer(tr, max_items, clip_limit=p[0], tiles_x=p[1], tiles_y=p[2])


@functools.lru_cache(maxsize=None)
def apply_reference(p):
    """the items of the apply test for one parameter set, computed once: [(name, EqImage, want status, Equalized or None)]"""
    lib = eo.load()
    tcfg = trk.make_config(1, 1, MAX_W, MAX_H)
    out = []

    def add(name, item):
        st = eo.check(lib, tcfg, item)
        out.append((name, item, st, eo.apply(lib, _cfg(p), item.image, item.c.width) if st == trk.ISV_TRK_OK else None))

    z = np.zeros((20, 32), np.uint8)
    bad = [("width 0", eq.EqImage(z, 0)), ("stride below width", eq.EqImage(z, 33)), ("too wide", eq.EqImage(np.zeros((4, MAX_W + 1), np.uint8))),
           ("too high", eq.EqImage(np.zeros((MAX_H + 1, 4), np.uint8))), ("no data", eq.EqImage(z))]
    bad[4][1].c.data = None
    for k, (w, h, stride) in enumerate(SIZES):
        for name, img in eo.images(w, h, stride).items():
            add(f"{w}x{h} {name}", eq.EqImage(img, w))
        if k < len(bad):
            add(*bad[k])                           # a refused item between the good ones
    assert [o[2] for o in out if o[3] is None] == [trk.ISV_TRK_INPUT, trk.ISV_TRK_INPUT, trk.ISV_TRK_CAPACITY, trk.ISV_TRK_CAPACITY, trk.ISV_TRK_INPUT]
    return out


@pytest.fixture(scope="module")
def tracker():
    tr = trk.Tracker(4, 8, MAX_W, MAX_H, max_points=64)
    yield tr
    tr.close()


@pytest.mark.parametrize("p", eo.PARAMS, ids=str)
def test_apply_batch_in_one_call_against_restatement(tracker, p):
    ref = apply_reference(p)
    e = _equalizer(tracker, p, len(ref))
    st, imgs = e.apply_batch([r[1] for r in ref])
    assert st == [r[2] for r in ref]
    for i, (name, item, want_st, want) in enumerate(ref):           # the LUTs first: a wrong LUT is a wrong LUT
        if want is None:
            with pytest.raises(backend.BackendError):
                e.read_luts(i)
            continue
        luts = e.read_luts(i)
        assert np.array_equal(luts, want.luts), (name, "luts", np.argwhere(luts != want.luts)[:4])
    for i, (name, item, want_st, want) in enumerate(ref):
        if want is None:
            assert imgs[i] is None, name
        else:
            assert imgs[i].shape == want.out.shape and imgs[i].tobytes() == want.out.tobytes(), (name, "image", np.argwhere(imgs[i] != want.out)[:4])
    ms = e.last_ms()
    assert len(ms) == 6 and all(0 <= m < 10000 for m in ms) and ms[0] > 0 and ms[1] > 0 and ms[2] == 0 and ms[3] == 0 and ms[0] >= ms[1]
    # alone and reversed: an item's image does not depend on its batch; then the call's own refusals
    order = list(range(len(ref)))[::-1]
    st, imgs = e.apply_batch([ref[i][1] for i in order])
    for k, i in enumerate(order):
        assert st[k] == ref[i][2] and (imgs[k] is None if ref[i][3] is None else imgs[k].tobytes() == ref[i][3].out.tobytes()), ("reversed", ref[i][0])
    for i in (0, 7, len(ref) - 1):
        st, imgs = e.apply_batch([ref[i][1]])
        assert st == [ref[i][2]] and imgs[0].tobytes() == ref[i][3].out.tobytes(), ("alone", ref[i][0])
    assert e.apply_batch([]) == ([], [])
    with pytest.raises(backend.BackendError):
        e.apply_batch([ref[0][1]] * (len(ref) + 1))   # more items than max_items
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
TRACK_SIZES = [(64, 48, None), (97, 61, 104), (200, 120, None), (752, 480, None)]
P0 = (eq.CLIP, eq.TILES, eq.TILES)


def _dim(img):
    """a dark, low-contrast version of a texture: what CLAHE is for"""
    return (img.astype(np.int32) // 3 + 12).astype(np.uint8)


@functools.lru_cache(maxsize=1)
def track_reference():
    """three frames per size; per size: (frames [3] with stride, width, points, restated frames [3], Tracked of frame 0 -> 1 and 1 -> 2
    on the restated frames)"""
    elib, tlib = eo.load(), to.load()
    tcfg = trk.make_config(4, 8, MAX_W, MAX_H, max_points=64)
    out = []
    for k, (w, h, stride) in enumerate(TRACK_SIZES):
        frames = []
        for s in ((0.0, 0.0), (1.75, -1.25), (3.5, -2.0)):
            f = np.full((h, stride or w), 0xEE, np.uint8)
            f[:, :w] = _dim(trk.analytic_image(w, h, s, 70 + k))
            frames.append(f)
        rng = np.random.Generator(np.random.PCG64(90 + k))
        pts = np.column_stack([rng.uniform(-4, w + 4, 24), rng.uniform(-4, h + 4, 24)]).astype(np.float32)
        restated = [eo.apply(elib, _cfg(P0), f, w).out for f in frames]
        want = [to.track(tlib, tcfg, trk.TrkItem(k, restated[i + 1], restated[i], pts)) for i in (0, 1)]
        assert all(t.r.status == trk.ISV_TRK_OK for t in want) and any(t.r.n_kept > 0 for t in want)
        out.append((frames, w, pts, restated, want))
    return tcfg, out


def _same_track(got, want, where):
    (rg, ag), (ro, ao) = got, (want.r, want.arrays)
    assert bytes(rg) == bytes(ro), (where, to.describe(rg), to.describe(ro))
    for f in ("cur_pts", "flags", "err", "cur_un_pts"):
        g, o = getattr(ag, f), getattr(ao, f)
        assert g.shape == o.shape and g.tobytes() == o.tobytes(), (where, f)


def test_track_batch_against_restatements(tracker):
    tcfg, ref = track_reference()
    e = _equalizer(tracker, P0, 8)
    for s in range(4):
        tracker.slot_reset(s)
    # prev uploaded: frame 0 -> 1 of every size in one call; level 0 of both buffers first
    first = [trk.TrkItem(k, fr[1], fr[0], pts, w) for k, (fr, w, pts, re, want) in enumerate(ref)]
    rs, arrs = e.track_batch(first)
    for k, (fr, w, pts, re, want) in enumerate(ref):
        for which, img in ((0, re[1]), (1, re[0])):
            luts = e.read_luts(k, which)
            assert np.array_equal(luts, eo.apply(eo.load(), _cfg(P0), fr[1 - which], w).luts), (k, which, "luts")
            lvl = tracker.read_level(k, 0, which)
            assert np.array_equal(lvl, img), (k, which, "level 0", np.argwhere(lvl != img)[:4])
        pyr = want[0].pyr_cur
        for l in range(1, len(pyr)):
            assert np.array_equal(tracker.read_level(k, l), pyr[l]), (k, "level", l)
        _same_track((rs[k], arrs[k]), want[0], ("uploaded", k))
    ms = e.last_ms()
    assert len(ms) == 6 and all(0 < m < 10000 for m in ms) and ms[0] >= ms[1] + ms[2] + ms[3]
    # prev resident: frame 1 -> 2
    rs, arrs = e.track_batch([trk.TrkItem(k, fr[2], None, pts, w) for k, (fr, w, pts, re, want) in enumerate(ref)])
    for k, (fr, w, pts, re, want) in enumerate(ref):
        assert np.array_equal(tracker.read_level(k, 0), re[2]) and np.array_equal(tracker.read_level(k, 0, 1), re[1]), k
        with pytest.raises(backend.BackendError):
            e.read_luts(k, 1)                      # no prev was uploaded
        _same_track((rs[k], arrs[k]), want[1], ("resident", k))
    # the batch reversed, each item alone, and small, large and small calls on the one handle (prev given: the slots' state is no input)
    rs, arrs = e.track_batch(first[::-1])
    for k in range(len(ref)):
        _same_track((rs[len(ref) - 1 - k], arrs[len(ref) - 1 - k]), ref[k][4][0], ("reversed", k))
    for ks in ([0], [3], [1], [3, 0, 2], [2]):
        rs, arrs = e.track_batch([first[k] for k in ks])
        for r, a, k in zip(rs, arrs, ks):
            _same_track((r, a), ref[k][4][0], ("alone", ks, k))
    assert e.track_batch([]) == ([], [])
    e.close()


def test_slot_tags(tracker):
    tcfg, ref = track_reference()
    fr, w, pts, re, want = ref[0]
    e, other = _equalizer(tracker, P0, 8), _equalizer(tracker, P0, 8)
    for s in range(4):
        tracker.slot_reset(s)
    raw_seed, resident = trk.TrkItem(0, fr[0], fr[0], None, w), trk.TrkItem(0, fr[1], None, pts, w)
    # a raw-seeded slot refuses the equaliser's resident prev, and nothing changes: the tracker's own item still runs
    (r,), _ = tracker.track_batch([raw_seed])
    assert r.status == trk.ISV_TRK_OK
    (r,), (a,) = e.track_batch([resident])
    assert r.status == trk.ISV_TRK_INPUT and r.n_points == len(pts) and len(a.cur_pts) == 0
    assert np.array_equal(tracker.read_level(0, 0), fr[0][:, :w])
    (r,), _ = tracker.track_batch([resident])
    assert r.status == trk.ISV_TRK_OK and np.array_equal(tracker.read_level(0, 0), fr[1][:, :w])
    # the reverse: a slot the equaliser seeded refuses the tracker's resident prev, and another equaliser's
    (r,), _ = e.track_batch([raw_seed.with_prev(fr[0], 1)])
    assert r.status == trk.ISV_TRK_OK
    (r,), _ = tracker.track_batch([resident.with_prev(None, 1)])
    assert r.status == trk.ISV_TRK_INPUT
    (r,), _ = other.track_batch([resident.with_prev(None, 1)])
    assert r.status == trk.ISV_TRK_INPUT
    assert np.array_equal(tracker.read_level(1, 0), re[0])
    (r,), (a,) = e.track_batch([resident.with_prev(None, 1)])
    _same_track((r, a), want[0], "its own resident prev")
    # with prev given both work on either slot, with and without a reset: the tag is only about a resident prev
    tracker.slot_reset(0)
    for slot in (0, 1):
        (r,), (a,) = e.track_batch([resident.with_prev(fr[0], slot)])
        _same_track((r, a), want[0], ("prev given", slot))
        (r,), _ = tracker.track_batch([resident.with_prev(fr[0], slot)])
        assert r.status == trk.ISV_TRK_OK and np.array_equal(tracker.read_level(slot, 0), fr[1][:, :w])
    e.close(); other.close()


def test_three_frame_chain_of_detection_and_equalised_tracking_on_one_slot():
    dlib, tlib, elib = do.load(), to.load(), eo.load()
    w, h, MAX_CNT = 200, 120, 40
    tcfg = trk.make_config(2, 2, w, h, max_points=64)
    dcfg = det.make_config(2, 64, MAX_CNT, 12, det.QUALITY)
    frames = [_dim(trk.analytic_image(w, h, s, 50)) for s in ((0, 0), (2.25, -1.5), (5.0, -2.75))]
    restated = [eo.apply(elib, _cfg(P0), f).out for f in frames]
    tr = _tracker(tcfg)
    dt = _detector(tr, dcfg)
    e = _equalizer(tr, P0, 2)

    def both_detect(f, pts, cnt, max_new):
        item = det.DetItem(1, pts, cnt, max_new)
        want = do.detect(dlib, dcfg, tcfg, restated[f], item)      # detection reads the equalised image
        (r,), (a,) = dt.detect_batch([item])
        _same_planes(dt, 0, want, "chain")
        _same((r, a), want, "chain")
        return a

    def both_track(f, pts):
        want = to.track(tlib, tcfg, trk.TrkItem(1, restated[f], restated[f - 1], pts))
        (r,), (a,) = e.track_batch([trk.TrkItem(1, frames[f], None, pts)])
        _same_track((r, a), want, ("chain", f))
        return a

    # frame 0: the slot takes the equalised image, the first corners are born
    (r,), _ = e.track_batch([trk.TrkItem(1, frames[0], frames[0])])
    assert r.status == trk.ISV_TRK_OK and np.array_equal(tr.read_level(1, 0), restated[0])
    a0 = both_detect(0, None, None, MAX_CNT)
    raw0 = do.detect(dlib, dcfg, tcfg, frames[0], det.DetItem(1, None, None, MAX_CNT))
    assert a0.new_pts.tobytes() != raw0.arrays.new_pts.tobytes()    # the raw image gives other corners: the equalisation is seen
    pts, cnt = a0.new_pts.copy(), np.ones(len(a0.new_pts), np.int32)
    assert 10 <= len(pts) <= MAX_CNT
    for f in (1, 2):
        # track into frame f, compact (reduceVector), track_cnt++, setMask and the new corners
        t = both_track(f, pts)
        pts, _, cnt = t.kept(cnt)
        cnt = cnt + 1
        assert len(pts) >= 8
        a = both_detect(f, pts, cnt, MAX_CNT - len(pts))
        pts = np.vstack([pts[a.kept_index], a.new_pts]) if len(a.new_pts) else pts[a.kept_index]
        cnt = np.concatenate([cnt[a.kept_index], np.ones(len(a.new_pts), np.int32)])
        assert len(pts) <= MAX_CNT
    e.close(); dt.close(); tr.close()
