"""The restatement of include/isvins_frontend.h: FeatureTracker::readImage (reference src/feature_tracker/feature_tracker_simple.cpp
:81-151, :182-244) and the message of System::PubImageData (src/System.cpp:102-129) for one sequence, and PubImageData's scalar gate
(:56-95, :131-135).  The arithmetic stages are the four existing restatements (eq_oracle, trk_oracle, rej_oracle, det_oracle) behind
`OracleStages`; the bookkeeping is numpy and plain Python written from the reference's lines, with the reference's own data
structures: a std::map keyed by id (a dict, first insert wins), a pts_velocity that the else branch does not clear.  Nothing here
knows how the device carries its state.

`read_image(stages, cfg, seq, img, t, pub)` advances `seq` (a Sequence) by one frame and returns a Frame.  The stages are pluggable so
that the GPU tests drive the same bookkeeping over the four public GPU calls."""
import math

import numpy as np

import det_oracle as do
import eq_oracle as eo
import rej_oracle as ro
import trk_oracle as to
from isvins_amd import detect as det, reject as rej, tracker as trk

F32, I32 = np.float32, np.int32
RESULT_FIELDS = ("status", "n_tracked", "n_after_reject", "n_kept", "n_new", "n_points", "n_msg", "method", "iters")


class Config:
    """the constants of one front end: image size, MAX_CNT, MIN_DIST, max_points, the camera (a tracker config), optional CLAHE"""

    def __init__(self, width, height, max_cnt=40, min_dist=10, max_points=160, equalize=False, **cam):
        self.width, self.height, self.max_cnt, self.min_dist, self.max_points = width, height, max_cnt, min_dist, max_points
        self.tcfg = trk.make_config(1, 1, width, height, max_points=max_points, **cam)
        self.dcfg = det.make_config(1, max_points, max_cnt, min_dist, det.QUALITY)
        self.rcfg = rej.make_config(1, max_points)
        self.ecfg = None
        if equalize:
            from isvins_amd import equalize as eq
            self.ecfg = eq.make_config()


class OracleStages:
    """the four stages through their serial CPU restatements"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.tlib, self.rlib, self.dlib = to.load(), ro.load(), do.load()
        self.elib = eo.load() if cfg.ecfg is not None else None

    def image(self, img):
        """readImage :86-92"""
        return eo.apply(self.elib, self.cfg.ecfg, img).out if self.elib is not None else np.ascontiguousarray(img, np.uint8)

    def track(self, prev_img, cur_img, prev_pts):
        """calcOpticalFlowPyrLK and inBorder -> (cur_pts, flags)"""
        t = to.track(self.tlib, self.cfg.tcfg, trk.TrkItem(0, cur_img, prev_img, prev_pts))
        assert t.r.status == trk.ISV_TRK_OK
        return t.arrays.cur_pts, t.arrays.flags

    def reject(self, prev_pts, cur_pts):
        """findFundamentalMat's status on at least 8 points -> (status, method, iters)"""
        r = ro.reject(self.rlib, self.cfg.tcfg, self.cfg.rcfg, rej.RejItem(self.cfg.width, self.cfg.height, prev_pts, cur_pts))
        assert r.res.status == trk.ISV_TRK_OK
        return r.status, r.res.method, r.res.iters

    def detect(self, cur_img, cur_pts, track_cnt, max_new):
        """setMask and goodFeaturesToTrack -> (kept_index, new_pts)"""
        d = do.detect(self.dlib, self.cfg.dcfg, self.cfg.tcfg, cur_img, det.DetItem(0, cur_pts, track_cnt, max_new))
        assert d.r.status == det.ISV_DET_OK
        return d.arrays.kept_index, d.arrays.new_pts

    def lift(self, pts):
        return to.lift(self.tlib, self.cfg.tcfg, pts)


class Sequence:
    """FeatureTracker's members"""

    def __init__(self):
        self.prev_img = None
        self.prev_pts = np.zeros((0, 2), F32)
        self.ids = np.zeros(0, I32)
        self.track_cnt = np.zeros(0, I32)
        self.prev_un_pts = np.zeros((0, 2), F32)
        self.prev_un_pts_map = {}          # id -> (x, y) float32
        self.pts_velocity = []             # [(vx, vy)], never cleared by the else branch (F2)
        self.n_id = 0
        self.prev_time = 0.0

    @classmethod
    def planted(cls, prev_img, prev_pts, ids, track_cnt, prev_un_pts, in_map, n_id, prev_time):
        """the members that a slot's planted state stands for: the map holds the flagged points under their ids, and the key -1 as
        soon as a point is not flagged (F1: a newborn's entry); pts_velocity is all zero (F2)"""
        s = cls()
        s.prev_img = prev_img
        s.prev_pts, s.ids, s.track_cnt = np.array(prev_pts, F32).reshape(-1, 2), np.array(ids, I32).reshape(-1), np.array(track_cnt, I32).reshape(-1)
        s.prev_un_pts = np.array(prev_un_pts, F32).reshape(-1, 2)
        for i, f in enumerate(np.asarray(in_map).reshape(-1)):
            key = int(s.ids[i]) if f else -1
            s.prev_un_pts_map.setdefault(key, (s.prev_un_pts[i, 0], s.prev_un_pts[i, 1]))
        s.pts_velocity = [(F32(0), F32(0))] * len(s.prev_pts)
        s.n_id, s.prev_time = int(n_id), float(prev_time)
        return s

    def in_map(self):
        """per point: the map holds it under its own id"""
        return np.array([int(i) in self.prev_un_pts_map for i in self.ids], np.uint8)


class Frame:
    """one readImage: the result record's fields, the message and the end-of-frame lists"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def result(self):
        return tuple(getattr(self, f) for f in RESULT_FIELDS)


def velocity(cur, prev, dt):
    """:225-227: the float32 difference, divided in double, stored as float32"""
    with np.errstate(all="ignore"):
        return F32(np.float64(F32(cur) - F32(prev)) / np.float64(dt))


def read_image(stages, cfg, s, img, cur_time, pub, key_map_by_final_ids=False):
    """FeatureTracker::readImage on `s`, then PubImageData's message.  key_map_by_final_ids is the control of F1: updateID before
    UndistortPixelMotion."""
    n_tracked = n_after = n_kept = n_new = 0
    method, iters = rej.NONE, 0
    cur_img = stages.image(img)                                                  # :86-92
    if s.prev_img is None:                                                       # :94-107
        cur_pts, ids, track_cnt = np.zeros((0, 2), F32), np.zeros(0, I32), np.zeros(0, I32)
        kept, n_pts = stages.detect(cur_img, cur_pts, track_cnt, cfg.max_cnt)    # setMask on nothing; goodFeaturesToTrack(MAX_CNT)
        assert len(kept) == 0
        n_new = len(n_pts)
        cur_pts, ids, track_cnt = n_pts.copy(), np.full(n_new, -1, I32), np.ones(n_new, I32)     # addPoints
    else:
        cur_pts, flags = stages.track(s.prev_img, cur_img, s.prev_pts)           # :114-118
        status = flags == (trk.FLAG_STATUS | trk.FLAG_BORDER)
        prev_pts, cur_pts, ids, track_cnt = s.prev_pts[status], cur_pts[status], s.ids[status], s.track_cnt[status]     # :119-122
        track_cnt = track_cnt + 1                                                # :124-125
        n_tracked = n_after = n_kept = len(cur_pts)
        if pub:                                                                  # :126-143
            if len(prev_pts) >= 8:                                               # rejectWithF (:155)
                st, method, iters = stages.reject(prev_pts, cur_pts)
                st = st.astype(bool)
                prev_pts, cur_pts, ids, track_cnt = prev_pts[st], cur_pts[st], ids[st], track_cnt[st]
            n_after = len(cur_pts)
            # setMask (:37-69): the stable descending order by track_cnt and the kept list, with the detection it masks for.
            # n_max_cnt is formed from the count before setMask (F3)
            kept, n_pts = stages.detect(cur_img, cur_pts, track_cnt, max(cfg.max_cnt - n_after, 0))
            cur_pts, ids, track_cnt = cur_pts[kept], ids[kept], track_cnt[kept]
            n_kept, n_new = len(kept), len(n_pts)
            cur_pts = np.concatenate([cur_pts, n_pts.reshape(-1, 2)]).astype(F32)            # addPoints (:71-79)
            ids = np.concatenate([ids, np.full(n_new, -1, I32)]).astype(I32)
            track_cnt = np.concatenate([track_cnt, np.ones(n_new, I32)]).astype(I32)
    ids = ids.copy()
    if key_map_by_final_ids:
        s.n_id = update_id(ids, s.n_id)
    # UndistortPixelMotion (:197-244)
    cur_un_pts = stages.lift(cur_pts).reshape(-1, 2)
    cur_un_pts_map = {}
    for i in range(len(cur_pts)):
        cur_un_pts_map.setdefault(int(ids[i]), (cur_un_pts[i, 0], cur_un_pts[i, 1]))         # std::map::insert: the first one stays
    if s.prev_un_pts_map:
        dt = cur_time - s.prev_time
        s.pts_velocity = []
        for i in range(len(cur_un_pts)):
            it = s.prev_un_pts_map.get(int(ids[i])) if ids[i] != -1 else None
            s.pts_velocity.append((velocity(cur_un_pts[i, 0], it[0], dt), velocity(cur_un_pts[i, 1], it[1], dt)) if it is not None else (F32(0), F32(0)))
    else:
        s.pts_velocity = s.pts_velocity + [(F32(0), F32(0))] * len(cur_pts)                   # no clear() (F2)
    s.prev_un_pts_map = cur_un_pts_map
    if not key_map_by_final_ids:
        s.n_id = update_id(ids, s.n_id)                                                       # :147
    s.prev_img, s.prev_pts, s.prev_time = cur_img, cur_pts, float(cur_time)                   # :148-150
    s.ids, s.track_cnt, s.prev_un_pts = ids, track_cnt, cur_un_pts
    n = len(ids)
    vel = np.array(s.pts_velocity[:n], F32).reshape(-1, 2)                                    # the entries an index below ids.size() reads
    rows = [j for j in range(n) if track_cnt[j] > 1] if pub else []                           # System.cpp:102, :114-116
    return Frame(status=0, n_tracked=n_tracked, n_after_reject=n_after, n_kept=n_kept, n_new=n_new, n_points=n, n_msg=len(rows), method=method, iters=iters,
                 feature_id=ids[rows].astype(I32), point=np.array([[float(cur_un_pts[j, 0]), float(cur_un_pts[j, 1]), 1.0] for j in rows], np.float64).reshape(-1, 3),
                 uv=cur_pts[rows].astype(F32).reshape(-1, 2), velocity=vel[rows].reshape(-1, 2),
                 cur_pts=cur_pts, cur_un_pts=cur_un_pts, ids=ids, track_cnt=track_cnt, pts_velocity=vel)


def update_id(ids, n_id):
    """:182-188"""
    for i in range(len(ids)):
        if ids[i] == -1:
            ids[i] = n_id
            n_id += 1
    return n_id


def same(a, b):
    """bitwise equality of two arrays, but NaN equals NaN whatever its bits"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


# ---- System::PubImageData's scalar logic ----
class Gate:
    """System.h:46-50, :67"""

    def __init__(self, freq=10):
        self.init_feature, self.first_image_flag, self.init_pub, self.pub_count = False, True, False, 1
        self.first_image_time, self.last_image_time, self.freq = 0.0, 0.0, freq


def c_round(x):
    """C's round: half away from zero"""
    if math.isnan(x) or math.isinf(x):
        return x
    return math.copysign(math.floor(abs(x) + 0.5), x)


def gate_step(g, t):
    """System.cpp:56-95, :102-104, :131-135 -> (skip, pub_this_frame, deliver)"""
    if not g.init_feature:
        g.init_feature = True
        return True, False, False
    if g.first_image_flag:
        g.first_image_flag = False
        g.first_image_time = g.last_image_time = t
        return True, False, False
    if t - g.last_image_time > 1.0 or t < g.last_image_time:
        g.first_image_flag, g.last_image_time, g.pub_count = True, 0, 1           # no tracker is reset
        return True, False, False
    g.last_image_time = t
    den = t - g.first_image_time
    rate = 1.0 * g.pub_count / den if den != 0 else (math.nan if g.pub_count == 0 else math.copysign(math.inf, g.pub_count) * math.copysign(1.0, den))
    pub = False
    if c_round(rate) <= g.freq:
        pub = True
        if abs(rate - g.freq) < 0.01 * g.freq:
            g.first_image_time, g.pub_count = t, 0
    deliver = False
    if pub:
        g.pub_count += 1
        if not g.init_pub:
            g.init_pub = True
        else:
            deliver = True
    return False, pub, deliver
