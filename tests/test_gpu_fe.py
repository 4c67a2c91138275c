"""GPU parity of the whole-frame feature tracker (include/isvins_frontend.h, csrc/isv_frontend.hip) against its restatement
tests/fe_oracle.py, and against the hand-driven chain of the four public GPU calls with the restatement's host bookkeeping, at
160 x 120 with MAX_CNT 40 and max_points 160.  Every comparison is bitwise on the result record, on every output array and on the
slot's state (slot_get), except that a NaN velocity equals a NaN velocity (dt = 0).

The sequences' references are computed once per module and shared unchanged."""
import numpy as np
import pytest

import fe_oracle as fo
from isvins_amd import backend, detect as det, equalize as eqm, frontend as fe, reject as rej, tracker as trk

pytestmark = pytest.mark.gpu

W, H, MAX_CNT, MIN_DIST, MAX_POINTS, SLOTS = 160, 120, 40, 10, 160, 132
SEQS = ((60, (2.25, -1.5)), (61, (-1.75, 2.5)))      # (texture seed, shift per frame)
UNPUBLISHED = (3, 5)
N_FRAMES = 6


def image(seq, frame):
    seed, (sx, sy) = SEQS[seq]
    return trk.analytic_image(W, H, (sx * frame, sy * frame), seed)


def stamp(frame):
    return 10.0 + 0.05 * frame


class Rig:
    def __init__(self, equalize):
        self.cfg = fo.Config(W, H, MAX_CNT, MIN_DIST, MAX_POINTS, equalize=equalize)
        self.tr = trk.Tracker(SLOTS, SLOTS, W, H, max_points=MAX_POINTS)
        self.rj = rej.Rejector(self.tr)
        self.dt = det.Detector(self.tr, max_points=MAX_POINTS, max_corners=MAX_CNT, min_dist=MIN_DIST)
        self.eq = eqm.Equalizer(self.tr) if equalize else None
        self.fe = fe.FrontEnd(self.tr, self.rj, self.dt, self.eq)
        assert (self.fe.cfg.max_items, self.fe.cfg.max_cnt, self.fe.cfg.max_points) == (SLOTS, MAX_CNT, MAX_POINTS)

    def close(self):
        for h in (self.fe, self.eq, self.dt, self.rj, self.tr):
            if h is not None:
                h.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig(False)
    yield r
    r.close()


@pytest.fixture(scope="module")
def want():
    """the restatement over the six frames of both sequences, plain and equalised: {equalize: [[Frame per frame] per sequence]} with
    the Sequence after every frame beside it"""
    out = {}
    for equalize in (False, True):
        cfg = fo.Config(W, H, MAX_CNT, MIN_DIST, MAX_POINTS, equalize=equalize)
        st = fo.OracleStages(cfg)
        per_seq = []
        for q in range(len(SEQS)):
            s, frames = fo.Sequence(), []
            for f in range(N_FRAMES):
                fr = fo.read_image(st, cfg, s, image(q, f), stamp(f), f not in UNPUBLISHED)
                frames.append((fr, state_key(s)))
            per_seq.append(frames)
        out[equalize] = per_seq
    return out


def state_key(s):
    """a restatement Sequence as the bytes slot_get gives"""
    return fe.State(s.prev_pts, s.ids, s.track_cnt, s.prev_un_pts, s.in_map(), s.n_id, s.prev_time).key()


def assert_frame(r, got, ref, what):
    assert tuple(getattr(r, f) for f in fe.RESULT_FIELDS) == ref.result(), (what, [getattr(r, f) for f in fe.RESULT_FIELDS], ref.result())
    for name in fe.Frame.ARRAYS:
        assert fo.same(getattr(got, name), getattr(ref, name)), (what, name, getattr(got, name)[:4], getattr(ref, name)[:4])


class GpuStages:
    """the four public GPU calls on one slot, for fe_oracle's bookkeeping: the chain a caller drives by hand.  The lifted points are
    the stage calls' own (cur_un_pts of the tracking call, new_un_pts of the detection), found again by the point's bytes."""

    def __init__(self, rig, slot):
        self.r, self.slot, self.un, self.seeded = rig, slot, {}, False
        self.trk_call = (rig.eq or rig.tr).track_batch

    def image(self, img):
        return img                                   # (with an equaliser the tracking call equalises on the device)

    def track(self, prev_img, cur_img, prev_pts):
        (r,), (a,) = self.trk_call([trk.TrkItem(self.slot, cur_img, None, prev_pts)])
        assert r.status == trk.ISV_TRK_OK
        self.un = {p.tobytes(): u for p, u in zip(a.cur_pts, a.cur_un_pts)}
        return a.cur_pts, a.flags

    def reject(self, prev_pts, cur_pts):
        (r,), (st,) = self.r.rj.reject_batch([rej.RejItem(W, H, prev_pts, cur_pts)])
        assert r.status == trk.ISV_TRK_OK
        return st, r.method, r.iters

    def detect(self, cur_img, cur_pts, track_cnt, max_new):
        if not self.seeded:                          # the first frame: the slot takes the image
            (r,), _ = self.trk_call([trk.TrkItem(self.slot, cur_img, cur_img)])
            assert r.status == trk.ISV_TRK_OK
        self.seeded = True
        (r,), (a,) = self.r.dt.detect_batch([det.DetItem(self.slot, cur_pts, track_cnt, max_new)])
        assert r.status == det.ISV_DET_OK
        self.un.update({p.tobytes(): u for p, u in zip(a.new_pts, a.new_un_pts)})
        return a.kept_index, a.new_pts

    def lift(self, pts):
        return np.array([self.un[p.tobytes()] for p in np.asarray(pts, np.float32).reshape(-1, 2)], np.float32).reshape(-1, 2)


def run_six_frames(r, want, equalize):
    chains = [(GpuStages(r, 100 + q), fo.Sequence()) for q in range(len(SEQS))]
    for f in range(N_FRAMES):
        pub = f not in UNPUBLISHED
        res, frames = r.fe.read_image_batch([fe.FeItem(q, image(q, f), stamp(f), pub) for q in range(len(SEQS))])
        for q in range(len(SEQS)):
            ref, key = want[equalize][q][f]
            print("frame", f, "seq", q, [getattr(res[q], n) for n in fe.RESULT_FIELDS], ref.result())
            assert_frame(res[q], frames[q], ref, ("restatement", f, q))
            assert r.fe.slot_get(q).key() == key, ("state", f, q)
            st, s = chains[q]
            assert_frame(res[q], frames[q], fo.read_image(st, r.cfg, s, image(q, f), stamp(f), pub), ("chain", f, q))
    # the frames mean something: both branches of rejectWithF's method, drops, births, real velocities
    last = want[equalize][0][N_FRAMES - 1][0]
    assert last.n_points >= 20 and (last.pts_velocity != 0).any() and max(fr.n_new for fr, _ in want[equalize][0][1:]) >= 1
    for q in range(len(SEQS)):
        r.fe.slot_reset(q)


def test_six_frames_against_restatement_and_chain(rig, want):
    run_six_frames(rig, want, False)


def test_six_frames_with_an_equaliser(want):
    r = Rig(True)
    try:
        run_six_frames(r, want, True)
        assert any(not fo.same(a[0].cur_pts, b[0].cur_pts) for a, b in zip(want[True][0], want[False][0]))      # CLAHE changes the corners
    finally:
        r.close()


def test_batch_independence(rig, want):
    """every sequence alone on a slot of its own, then 130 items in a shuffled order, copies of the two sequences on 130 slots"""
    for q in range(len(SEQS)):
        for f in range(4):
            (r,), (fr,) = rig.fe.read_image_batch([fe.FeItem(130 + q, image(q, f), stamp(f), f not in UNPUBLISHED)])
            assert_frame(r, fr, want[False][q][f][0], ("alone", f, q))
    order = np.random.Generator(np.random.PCG64(11)).permutation(130)
    for f in range(4):
        res, frames = rig.fe.read_image_batch([fe.FeItem(int(s), image(int(s) % 2, f), stamp(f), f not in UNPUBLISHED) for s in order])
        for s, r, fr in zip(order, res, frames):
            assert_frame(r, fr, want[False][int(s) % 2][f][0], ("padded", f, int(s)))
    assert rig.fe.slot_get(int(order[0])).key() == want[False][int(order[0]) % 2][3][1]
    for s in range(132):
        rig.fe.slot_reset(s)
    assert rig.fe.read_image_batch([]) == ([], [])


# ---- planted states ----
COUNTS = (0, 1, 7, 8, 14, 15, 63, 64, 65, 129)


def planted_points(n, bad=lambda i: i % 4 == 1):
    """n points in image 0 of sequence 1, whose frame 1 is shifted by (-1.75, 2.5): the points `bad` picks sit at x = 1.5 and leave
    the border (or the flow loses them); the others lie on an 8-pixel grid in the interior"""
    grid = [(12.0 + 8 * (k % 18), 12.0 + 8 * (k // 18)) for k in range(18 * 13)]
    return np.array([(1.5, 8.0 + 0.75 * i) if bad(i) else grid[i] for i in range(n)], np.float32).reshape(-1, 2)


def planted_case(name):
    """(State to plant, prev_time, frames [(image, time, pub)])"""
    img1, img2 = image(1, 1), image(1, 2)
    mk = lambda pts, cnt=None, **kw: dict(pts=pts, cnt=(1 + np.arange(len(pts)) % 5) if cnt is None else cnt, prev_time=10.0, frames=[(img1, 10.05, True)], **kw)
    if isinstance(name, int):
        return mk(planted_points(name))
    if name == "lose_all_then_empty_map":
        return dict(mk(planted_points(5, bad=lambda i: True)), frames=[(img1, 10.05, False), (img2, 10.1, True), (image(1, 3), 10.15, True)])
    if name == "equal_counts":
        return mk(planted_points(15), cnt=np.full(15, 3))
    if name == "dt_zero":
        return dict(mk(planted_points(15)), frames=[(img1, 10.0, True)])
    raise KeyError(name)


PLANTED = COUNTS + ("lose_all_then_empty_map", "equal_counts", "dt_zero")


def planted_ids(n):
    """a permutation of 0 .. n - 1 (11 divides none of the counts): the id names the planted index"""
    return np.array([(11 * i + 3) % n for i in range(n)], np.int32)


def test_planted_states(rig):
    """slot_set plants counts the detector would not produce: all cases in one batch per frame, each against the restatement"""
    st = fo.OracleStages(rig.cfg)
    img0 = image(1, 0)
    cases = {n: planted_case(n) for n in PLANTED}
    slots = {n: k for k, n in enumerate(PLANTED)}
    res, _ = rig.fe.read_image_batch([fe.FeItem(k, img0, 9.95, True) for k in slots.values()])        # the slots take image 0
    assert all(r.status == 0 for r in res)
    seqs = {}
    for name, c in cases.items():
        pts, n = c["pts"], len(c["pts"])
        ids, in_map = planted_ids(n), (np.arange(n) % 3 != 0).astype(np.uint8)
        un = (st.lift(pts) + np.float32(0.001)).astype(np.float32)
        state = fe.State(pts, ids, c["cnt"], un, in_map, n_id=n + 7, prev_time=c["prev_time"])
        rig.fe.slot_set(slots[name], state)
        assert rig.fe.slot_get(slots[name]).key() == state.key(), name
        seqs[name] = fo.Sequence.planted(img0, pts, ids, c["cnt"], un, in_map, n + 7, c["prev_time"])
        if isinstance(name, int) and name >= 2:       # from the restatement's own flow: some are dropped, not all
            _, flags = st.track(img0, c["frames"][0][0], pts)
            alive = np.flatnonzero(flags == (trk.FLAG_STATUS | trk.FLAG_BORDER))
            assert 1 <= len(alive) <= name - 1, (name, len(alive))
            if name in (65, 129):
                assert (alive < 64).any() and (alive >= 64).any(), (name, alive)     # survivors on both sides of lane 64
    for step in range(3):
        live = [n for n in PLANTED if step < len(cases[n]["frames"])]
        res, frames = rig.fe.read_image_batch([fe.FeItem(slots[n], *cases[n]["frames"][step]) for n in live])
        for name, r, fr in zip(live, res, frames):
            img, t, pub = cases[name]["frames"][step]
            ref = fo.read_image(st, rig.cfg, seqs[name], img, t, pub)
            print(name, step, ref.result())
            assert_frame(r, fr, ref, (name, step))
            assert rig.fe.slot_get(slots[name]).key() == state_key(seqs[name]), (name, step)
            if step == 0 and name == 129:             # n >= MAX_CNT: setMask runs and drops, nothing is born
                assert ref.n_after_reject >= MAX_CNT and ref.n_new == 0 and 1 <= ref.n_kept < ref.n_after_reject, ref.result()
            if step == 0 and name == "dt_zero":       # infinities or NaNs, compared as such
                assert ref.n_msg >= 1 and not np.isfinite(ref.velocity).all()
            if step == 0 and name == "lose_all_then_empty_map":
                assert ref.n_points == 0
            if step == 1 and name == "lose_all_then_empty_map":
                assert ref.n_tracked == 0 and ref.n_new >= 20 and (ref.pts_velocity == 0).all()
    for k in slots.values():
        rig.fe.slot_reset(k)


def test_refusals_leave_slots_untouched_and_round_trip(rig, want):
    f = rig.fe
    rig.tr.slot_reset(4)                                                              # (an earlier test's image: slot 4 has none from here on)
    for fr in range(2):                                                            # slots 0..3 run sequence 0; slot 4 stays empty
        res, _ = f.read_image_batch([fe.FeItem(s, image(0, fr), stamp(fr), True) for s in range(4)])
        assert all(r.status == 0 for r in res)
    # slot 1's resident image is replaced by a plain tracking call: the front end must not track against it
    (r,), _ = rig.tr.track_batch([trk.TrkItem(1, image(1, 0), image(1, 0))])
    assert r.status == 0
    before = [f.slot_get(s).key() for s in range(5)]
    img = image(0, 2)
    small = fe.FeItem(0, img[:100], stamp(2), True)                                   # another size than the slot's sequence
    wide = fe.FeItem(4, np.zeros((H, W + 8), np.uint8), stamp(2), True)               # beyond the tracker's max_width
    nan = fe.FeItem(4, img, float("nan"), True)
    items = [fe.FeItem(2, img, stamp(2), True), small, fe.FeItem(1, img, stamp(2), True), wide, nan, fe.FeItem(3, img, stamp(2), True),
             fe.FeItem(3, img, stamp(2), True), fe.FeItem(99, img, stamp(2), True).on_slot(SLOTS)]
    res, frames = f.read_image_batch(items)                                           # (read_image_batch asserts a refused item's arrays untouched)
    assert [r.status for r in res] == [0, trk.ISV_TRK_INPUT, trk.ISV_TRK_INPUT, trk.ISV_TRK_CAPACITY, trk.ISV_TRK_INPUT, trk.ISV_TRK_INPUT,
                                       trk.ISV_TRK_INPUT, trk.ISV_TRK_INPUT]
    assert_frame(res[0], frames[0], want[False][0][2][0], "good item between refused ones")
    after = [f.slot_get(s).key() for s in range(5)]
    assert after[0] == before[0] and after[1] == before[1] and after[3] == before[3] and after[4] == before[4] and after[2] != before[2]
    assert all(r.n_points == 0 and r.n_msg == 0 for r in res[1:]) and all(len(fr.cur_pts) == 0 for fr in frames[1:])
    # slot 3 was only named twice: it goes on; its twin, slot 0, goes through get -> reset -> set first
    saved = f.slot_get(0)
    f.slot_reset(0)
    assert f.slot_get(0).has_sequence == 0
    f.slot_set(0, saved)
    assert f.slot_get(0).key() == saved.key()
    for fr in (2, 3, 4):
        res, frames = f.read_image_batch([fe.FeItem(s, image(0, fr), stamp(fr), fr not in UNPUBLISHED) for s in (0, 3)])
        for r, got in zip(res, frames):
            assert_frame(r, got, want[False][0][fr][0], ("round trip", fr))
    # slot_set's refusals change nothing
    bad = fe.State(saved.prev_pts, saved.ids, saved.track_cnt, saved.prev_un_pts, saved.in_map, saved.n_id, saved.prev_time)
    bad.ids = bad.ids.copy(); bad.ids[1] = bad.ids[0]
    keep = f.slot_get(0).key()
    with pytest.raises(backend.BackendError, match="ISV_ERR_INVALID_ARG"):
        f.slot_set(0, bad)
    with pytest.raises(backend.BackendError, match="ISV_ERR_INVALID_ARG"):
        f.slot_set(4, saved)                                                          # slot 4 has no resident image
    assert f.slot_get(0).key() == keep
    ms = f.last_ms()
    with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
        f.read_image_batch([fe.FeItem(0, img, 0.0)] * (SLOTS + 1))                    # more items than max_items: nothing is enqueued
    assert f.last_ms() == ms and f.slot_get(0).key() == keep
    for s in range(5):
        f.slot_reset(s)


def test_timing_contract(rig):
    for fr in range(2):
        rig.fe.read_image_batch([fe.FeItem(s, image(s % 2, fr), stamp(fr), True) for s in range(16)])
    ms = rig.fe.last_ms()
    assert len(ms) == 6 and all(np.isfinite(m) and 0 <= m < 10000 for m in ms), ms
    assert all(m > 0 for m in ms[:5]) and ms[0] >= sum(ms[1:]), ms
    for s in range(16):
        rig.fe.slot_reset(s)
