"""CPU checks of tests/fe_oracle.py, the restatement of include/isvins_frontend.h.  The bookkeeping of readImage is pinned on hand-made
states with scripted stages (every flag, status, kept list and corner is written down here, so each expectation below can be read off
the reference's lines): the compactions and track_cnt++, setMask's reorder, F1 with its control, F2, max_new <= 0, the first frame,
the message filter, the velocity formula against exact rationals; then two real frames through the four restatements; then
PubImageData's gate, restatement and library alike, on a 20 Hz stamp list."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import fe_oracle as fo
from isvins_amd import backend, frontend as fe, reject as rej, tracker as trk

F32, I32 = np.float32, np.int32
IMG = np.zeros((4, 4), np.uint8)


class Scripted:
    """stages that do what the test says: the flow moves every point by (1, 0.5) and flags them by `flags`; rejectWithF answers
    `status`; setMask orders by track_cnt (stable, descending) and drops the list positions in `drop`; goodFeaturesToTrack returns
    the first min(max_new, len(corners)) of `corners`; the lift is the exact float32 halving"""

    def __init__(self, flags=None, status=None, drop=(), corners=()):
        self.flags, self.status, self.drop, self.corners, self.calls = flags, status, set(drop), np.array(corners, F32).reshape(-1, 2), []

    def image(self, img):
        return img

    def track(self, prev_img, cur_img, prev_pts):
        self.calls.append(("track", len(prev_pts)))
        return (prev_pts + F32([1.0, 0.5])).astype(F32), np.array(self.flags, np.uint8)

    def reject(self, prev_pts, cur_pts):
        self.calls.append(("reject", len(prev_pts)))
        return np.array(self.status, np.uint8), rej.RANSAC, 7

    def detect(self, cur_img, cur_pts, track_cnt, max_new):
        self.calls.append(("detect", len(cur_pts), max_new))
        order = sorted(range(len(cur_pts)), key=lambda i: -int(track_cnt[i]))
        kept = np.array([i for r, i in enumerate(order) if r not in self.drop], I32)
        return kept, self.corners[:max_new]

    def lift(self, pts):
        return (np.asarray(pts, F32).reshape(-1, 2) * F32(0.5)).astype(F32)


CFG = fo.Config(160, 120, max_cnt=6, min_dist=10, max_points=32)


def planted(n, ids=None, cnt=None, in_map=None, n_id=100, prev_time=1.0):
    pts = np.array([[10.0 + 7 * i, 20.0 + 3 * i] for i in range(n)], F32)
    return fo.Sequence.planted(IMG, pts, np.arange(n) if ids is None else ids, np.full(n, 2) if cnt is None else cnt, pts * F32(0.5),
                               np.ones(n) if in_map is None else in_map, n_id, prev_time)


def test_compactions_track_cnt_and_the_unpublished_frame():
    s = planted(5, cnt=[5, 1, 3, 3, 9])
    st = Scripted(flags=[3, 1, 3, 2, 3])
    f = fo.read_image(st, CFG, s, IMG, 1.5, pub=False)
    assert st.calls == [("track", 5)]                              # neither rejectWithF nor setMask nor a detection
    assert f.ids.tolist() == [0, 2, 4] and f.track_cnt.tolist() == [6, 4, 10]
    assert f.cur_pts.tolist() == [[11.0, 20.5], [25.0, 26.5], [39.0, 32.5]]
    assert f.result() == (0, 3, 3, 3, 0, 3, 0, rej.NONE, 0) and len(f.feature_id) == 0
    assert s.prev_pts.tolist() == f.cur_pts.tolist() and s.prev_time == 1.5 and s.n_id == 100


def test_fewer_than_eight_points_skip_reject_and_set_mask_reorders_ids():
    s = planted(5, cnt=[5, 1, 3, 3, 9])
    st = Scripted(flags=[3] * 5, corners=[[50, 60], [70, 80], [90, 100]])
    f = fo.read_image(st, CFG, s, IMG, 1.5, pub=True)
    assert st.calls == [("track", 5), ("detect", 5, 1)]            # 5 < 8: no findFundamentalMat; MAX_CNT - 5 = 1
    assert f.ids.tolist() == [4, 0, 2, 3, 1, 100] and f.track_cnt.tolist() == [10, 6, 4, 4, 2, 1]          # stable among the two 4s
    assert f.result() == (0, 5, 5, 5, 1, 6, 5, rej.NONE, 0) and s.n_id == 101
    assert f.feature_id.tolist() == [4, 0, 2, 3, 1] and f.uv.tolist() == f.cur_pts[:5].tolist()          # the newborn has track_cnt 1
    assert f.point.dtype == np.float64 and f.point[:, 2].tolist() == [1.0] * 5 and f.point[:, :2].tolist() == f.cur_un_pts[:5].astype(np.float64).tolist()


def test_reject_status_compacts_and_max_new_counts_before_set_mask():
    s = planted(9, cnt=[2, 3, 4, 5, 6, 7, 8, 9, 10])
    st = Scripted(flags=[3] * 9, status=[1, 1, 0, 1, 1, 1, 0, 1, 1], drop=[1], corners=[[50, 60], [70, 80]])
    f = fo.read_image(st, CFG, s, IMG, 1.5, pub=True)
    # 9 tracked, 7 after rejectWithF, 7 >= MAX_CNT = 6: max_new = 0 and no corner is born, but setMask ran and dropped its second point
    assert st.calls == [("track", 9), ("reject", 9), ("detect", 7, 0)]
    assert f.ids.tolist() == [8, 5, 4, 3, 1, 0] and f.result() == (0, 9, 7, 6, 0, 6, 6, rej.RANSAC, 7)


def test_first_frame_detects_whatever_pub_says():
    for pub in (False, True):
        s = fo.Sequence()
        st = Scripted(corners=[[5, 6], [7, 8], [9, 10]])
        f = fo.read_image(st, CFG, s, IMG, 0.25, pub=pub)
        assert st.calls == [("detect", 0, 6)]
        assert f.ids.tolist() == [0, 1, 2] and f.track_cnt.tolist() == [1, 1, 1] and f.n_msg == 0 and s.n_id == 3
        assert f.pts_velocity.tolist() == [[0, 0]] * 3 and s.prev_img is IMG and list(s.prev_un_pts_map) == [-1]      # F1: only the first newborn


def test_f1_first_published_observation_has_zero_velocity():
    """a newborn is in the map under -1, so its next frame finds no entry: velocity 0 at track_cnt 2, real from 3 on.  The control
    keys the map by the final ids and gives the newborn a velocity at once."""
    for control in (False, True):
        s = fo.Sequence()
        fo.read_image(Scripted(corners=[[5, 6], [7, 8]]), CFG, s, IMG, 0.0, True, key_map_by_final_ids=control)
        f2 = fo.read_image(Scripted(flags=[3, 3]), CFG, s, IMG, 0.5, True, key_map_by_final_ids=control)
        f3 = fo.read_image(Scripted(flags=[3, 3]), CFG, s, IMG, 1.0, True, key_map_by_final_ids=control)
        assert f2.track_cnt.tolist() == [2, 2] and f2.n_msg == 2 and f3.track_cnt.tolist() == [3, 3]
        moved = [[1.0, 0.5]] * 2                                    # half a (1, 0.5) step per 0.5 s
        assert f2.velocity.tolist() == (moved if control else [[0.0, 0.0]] * 2)
        assert f3.velocity.tolist() == moved


def test_f2_stale_velocities_are_all_zero():
    s = planted(3)
    f = fo.read_image(Scripted(flags=[1, 0, 2]), CFG, s, IMG, 1.5, pub=False)         # every point is lost
    assert f.n_points == 0 and s.prev_un_pts_map == {} and s.pts_velocity == []
    f = fo.read_image(Scripted(flags=[], corners=[[5, 6], [7, 8]]), CFG, s, IMG, 2.0, pub=True)        # the else branch: appends, does not clear
    assert f.n_tracked == 0 and f.n_new == 2 and f.pts_velocity.tolist() == [[0, 0], [0, 0]]
    s.prev_un_pts_map = {}                                                             # force the branch again: the vector grows, the read entries stay zero
    f = fo.read_image(Scripted(flags=[3, 3]), CFG, s, IMG, 2.5, pub=True)
    assert len(s.pts_velocity) == 4 and f.pts_velocity.tolist() == [[0, 0], [0, 0]] and f.velocity.tolist() == [[0, 0], [0, 0]]


def test_message_filter_and_map_flags():
    s = planted(4, ids=[7, -1, 9, 3], cnt=[1, 1, 4, 1], in_map=[1, 0, 1, 0], n_id=10)
    assert s.in_map().tolist() == [1, 1, 1, 0] and s.prev_un_pts_map[-1] == (F32(8.5), F32(11.5))        # (-1 is a key: the second point's)
    f = fo.read_image(Scripted(flags=[3] * 4), CFG, s, IMG, 3.0, pub=True)
    assert f.ids.tolist() == [9, 7, 10, 3] and f.track_cnt.tolist() == [5, 2, 2, 2] and s.n_id == 11
    assert f.pts_velocity.tolist() == [[0.25, 0.125], [0.25, 0.125], [0, 0], [0, 0]]                     # id -1 is never looked up; id 3 was not in the map
    assert f.n_msg == 4 and s.in_map().tolist() == [1, 1, 0, 1]


def test_velocity_formula_against_exact_rationals():
    rng = np.random.Generator(np.random.PCG64(21))
    for _ in range(200):
        a, b = F32(rng.uniform(-1, 1)), F32(rng.uniform(-1, 1))
        t0, t1 = rng.uniform(0, 100), 0.0
        t1 = t0 + rng.uniform(1e-3, 0.2)
        d32 = F32(a) - F32(b)
        exact_d = Fraction(float(a)) - Fraction(float(b))
        assert abs(Fraction(float(d32)) - exact_d) <= abs(exact_d) * Fraction(1, 2 ** 24)               # the float32 difference, rounded once
        dt = t1 - t0
        q = Fraction(float(d32)) / Fraction(dt)
        v = fo.velocity(a, b, dt)
        assert abs(Fraction(float(v)) - q) <= abs(q) * (Fraction(1, 2 ** 24) + Fraction(1, 2 ** 52))    # one double and one float32 rounding of the quotient
    with np.errstate(all="ignore"):
        assert np.isinf(fo.velocity(F32(1), F32(0), 0.0)) and np.isnan(fo.velocity(F32(1), F32(1), 0.0))
    assert fo.same(np.array([np.nan, 1], F32), np.array([-np.nan, 1], F32)) and not fo.same(np.array([0.0], F32), np.array([-0.0], F32))


def test_two_real_frames_through_the_four_restatements():
    cfg = fo.Config(160, 120, max_cnt=40, min_dist=10, max_points=160)
    st = fo.OracleStages(cfg)
    s = fo.Sequence()
    f0 = fo.read_image(st, cfg, s, trk.analytic_image(160, 120, (0, 0), 60), 0.0, pub=False)
    assert 20 <= f0.n_new <= 40 and f0.ids.tolist() == list(range(f0.n_new))
    f1 = fo.read_image(st, cfg, s, trk.analytic_image(160, 120, (2.25, -1.5), 60), 0.05, pub=True)
    assert 15 <= f1.n_tracked <= f0.n_new and f1.method == rej.RANSAC and f1.n_kept <= f1.n_after_reject <= f1.n_tracked
    assert f1.n_points == f1.n_kept + f1.n_new <= 40 and f1.n_msg == f1.n_kept and (f1.velocity == 0).all()      # F1
    assert (np.diff(f1.track_cnt) <= 0).all() and s.n_id == f0.n_new + f1.n_new


# ---- the gate ----
@pytest.fixture(scope="module")
def lib():
    backend.build()
    return backend.load_library()


def run_gates(lib, stamps, freq=10):
    g, c = fo.Gate(freq), fe.Gate(freq)
    out = []
    for t in stamps:
        want = fo.gate_step(g, t)
        assert c.step(t) == want, t
        assert (c.g.pub_count, c.g.first_image_time, c.g.last_image_time, bool(c.g.first_image_flag)) == (g.pub_count, g.first_image_time, g.last_image_time, g.first_image_flag), t
        out.append(want)
    return out, g


def test_gate_on_a_20_hz_stream(lib):
    stamps = [100.0 + 0.05 * i for i in range(14)]
    out, g = run_gates(lib, stamps)
    SKIP, NO, PUB, FIRST = (True, False, False), (False, False, False), (False, True, True), (False, True, False)
    # init_feature and first_image_flag skip a frame each; then pub_count = 1 over 0.05 s is 20 Hz > FREQ: not published; over 0.1 s it
    # is 10 Hz: published, within 1 % of FREQ, so the window restarts (pub_count 0, then 1 again) -- and init_pub drops that message.
    # With pub_count 0 -> 1 after a restart, the next frame (0.05 s later) sees 20 Hz again: every other frame publishes.
    assert out[:2] == [SKIP, SKIP] and out[2] == NO and out[3] == FIRST
    assert out[4:] == [NO, PUB] * 5
    assert g.first_image_time == stamps[13] and g.pub_count == 1


def test_gate_discontinuity_resets_no_tracker_and_counts_again(lib):
    stamps = [10.0, 10.05, 10.1, 10.15, 11.5, 11.55, 11.6, 11.65, 11.0, 11.05]
    out, g = run_gates(lib, stamps)
    assert out[3] == (False, True, False)
    assert out[4] == (True, False, False)                         # more than 1 s later: first_image_flag again, pub_count 1
    assert out[5] == (True, False, False) and out[6][0] is False  # the next frame only restarts the clock; init_pub stays set
    assert out[7] == (False, True, True)
    assert out[8] == (True, False, False) and out[9] == (True, False, False)          # a stamp going back
    # a stamp equal to first_image_time: the rate is an infinity, nothing is published, nothing traps
    out, _ = run_gates(lib, [1.0, 2.0, 2.0])
    assert out[2] == (False, False, False)
    assert lib.isv_fe_gate_init(None, 10) == -1 and lib.isv_fe_gate_init(C.byref(fe.isv_fe_gate_t()), 0) == -1
    assert lib.isv_fe_gate_step(None, 0.0, C.byref(fe.isv_fe_gate_out_t())) == -1
