"""The timing contract of the batched stages' shared launcher (is-vins_amd/csrc/isv_stage_launch.h), stage by stage on each
stage's smallest fixture: a successful call leaves a tuple of the documented length, finite and non-negative, with the whole call
and every section in which a kernel ran above zero and the sections within the whole; a call refused on the host leaves exactly
the previous call's tuple; the next successful call leaves fresh times.

The refusal is each handle stage's capacity refusal (more items than max_items / max_pairs: ISV_ERR_CAPACITY before anything is
enqueued).  The three initialisation stages have no capacity a small call can exceed; theirs is the argument refusal
(ISV_ERR_INVALID_ARG for null arrays), which returns at the same place.

The inequality between the sections and the whole is the one the stage's own GPU test states.  tests/test_gpu_kf.py states none:
here all six of its sections (four kernels, the upload, the host's packing) are taken, since they are disjoint parts of the call."""
import math

import numpy as np
import pytest

import bow_cases
from isvins_amd import backend, bow, detect as det, initial, keyframe as kf, loop, tracker as trk

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _image(seed=0, shift=(0.0, 0.0)):
    return trk.analytic_image(W, H, shift, seed)


def _points():
    return np.array([[20.0, 15.0], [40.5, 30.25], [31.0, 24.0], [12.25, 36.5], [50.0, 10.0]], np.float32)


def _digest(results, *arrays):
    return b"".join(bytes(r) for r in results) + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


class Stage:
    """n_ms: the tuple's length; ran: the sections a kernel ran in, per call (first, third); within: the sections whose sum is at
    most the whole call; good() is a successful call (returns a digest of its outputs, or None where the handle's state moves on),
    refused() a call the host refuses"""
    ran_later = None

    def close(self):
        for h in self.handles:
            h.close()


class Loop(Stage):
    n_ms, ran, within = 3, (1, 2), (1, 2)

    def __init__(self):
        self.pair, _ = loop.make_loop_scene(3, n_points=20, n_keypoints=40)
        self.lv = loop.LoopVerifier(1, 32, 64)
        self.handles, self.last_ms = [self.lv], self.lv.last_ms

    def good(self):
        return _digest(self.lv.verify_batch([self.pair]))

    def refused(self):
        with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
            self.lv.verify_batch([self.pair, self.pair])


class Track(Stage):
    n_ms, ran, within = 5, (1, 2), (1, 2)

    def __init__(self):
        self.item = trk.TrkItem(0, _image(0, (1.5, -0.75)), _image(0), _points())
        self.tr = trk.Tracker(1, 1, W, H, max_points=8)
        self.handles, self.last_ms = [self.tr], self.tr.last_ms

    def good(self):
        rs, arrs = self.tr.track_batch([self.item])
        assert rs[0].status == trk.ISV_TRK_OK and rs[0].n_levels == 2
        return _digest(rs, arrs[0].cur_pts, arrs[0].flags, arrs[0].err, arrs[0].cur_un_pts)

    def refused(self):
        with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
            self.tr.track_batch([self.item, self.item])


class Detect(Stage):
    n_ms, ran, within = 5, (1, 2, 3), (1, 2, 3)

    def __init__(self):
        self.tr = trk.Tracker(1, 1, W, H, max_points=8)
        rs, _ = self.tr.track_batch([trk.TrkItem(0, _image(0), _image(0))])
        assert rs[0].status == trk.ISV_TRK_OK
        self.dt = det.Detector(self.tr, 1, max_points=8, max_corners=16, min_dist=3)
        self.item = det.DetItem(0, _points(), None, max_new=10)
        self.handles, self.last_ms = [self.dt, self.tr], self.dt.last_ms

    def good(self):
        rs, arrs = self.dt.detect_batch([self.item])
        assert rs[0].status == det.ISV_DET_OK and rs[0].n_new > 0
        return _digest(rs, arrs[0].kept_index, arrs[0].new_pts, arrs[0].new_un_pts)

    def refused(self):
        with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
            self.dt.detect_batch([self.item, self.item])


class Keyframe(Stage):
    n_ms, ran, within = 7, (1, 2, 3, 4), (1, 2, 3, 4, 5, 6)

    def __init__(self):
        self.item = kf.KfItem(_image(1), _points())
        self.ext = kf.KeyframeExtractor(1, W, H, max_keypoints=64, max_points=8)
        self.handles, self.last_ms = [self.ext], self.ext.last_ms

    def good(self):
        rs, arrs = self.ext.extract_batch([self.item])
        assert rs[0].status == kf.ISV_KF_OK
        a = arrs[0]
        return _digest(rs, a.brief, a.keypoints_uv, a.keypoints_norm, a.score, a.window_brief)

    def refused(self):
        with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
            self.ext.extract_batch([self.item, self.item])


class Bow(Stage):
    # the first call scores against an empty database: k_bow_score is not launched, its section is still marked
    n_ms, ran, ran_later, within = 5, (1, 3, 4), (1, 2, 3, 4), (1, 2, 3, 4)

    def __init__(self):
        self.ld = bow.LoopDetector(bow_cases.vocabularies()["k3L2"], 1, 1, bow_cases.MAX_FEATURES)
        self.frame = 0
        self.handles, self.last_ms = [self.ld], self.ld.last_ms

    def _item(self):
        self.frame += 1
        return bow.BowItem(0, self.frame, bow_cases.features(self.frame, 40))

    def good(self):
        rs = self.ld.detect_batch([self._item()])
        assert rs[0].status == bow.ISV_BOW_OK and self.ld.entries(0) == rs[0].entry_id + 1
        return None

    def refused(self):
        n = self.ld.entries(0)
        with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
            self.ld.detect_batch([self._item(), self._item()])
        assert self.ld.entries(0) == n


class Init(Stage):
    n_ms, ran, within = 2, (1,), (1,)

    def __init__(self, entry, run, last_ms, problem, extra=()):
        self.be = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
        self.entry, self.run, self.problem, self.extra = entry, run, problem, extra
        self.handles, self.last_ms = [self.be], lambda: last_ms(self.be)

    def good(self):
        return _digest(self.run(self.be, [self.problem]))

    def refused(self):
        assert getattr(self.be.lib, self.entry)(self.be.h, 1, None, None, *self.extra) == -1      # ISV_ERR_INVALID_ARG


STAGES = {
    "align": lambda: Init("isv_internal_visual_imu_align_batch", initial.align_batch, initial.last_ms, initial.make_problem()),
    "sfm": lambda: Init("isv_internal_sfm_batch", initial.sfm_batch, initial.sfm_last_ms, initial.make_scene(seed=12, l=0, n_window=5)[0]),
    "relpose": lambda: Init("isv_internal_relpose_batch", initial.relpose_batch, initial.relpose_last_ms,
                            initial.make_relpose_scene(seed=0, n_window=5, per_frame=30)[0], extra=(None,)),
    "loop": Loop, "bow": Bow, "keyframe": Keyframe, "tracker": Track, "detect": Detect,
}


def _check(ms, stage, ran):
    print(type(stage).__name__, ms)
    assert len(ms) == stage.n_ms and all(math.isfinite(m) and m >= 0 for m in ms), ms
    assert ms[0] > 0 and all(ms[i] > 0 for i in ran), ms
    assert sum(ms[i] for i in stage.within) <= ms[0], ms


@pytest.mark.parametrize("name", list(STAGES))
def test_times_of_success_refusal_success(name):
    stage = STAGES[name]()
    try:
        first = stage.good()
        t1 = stage.last_ms()
        _check(t1, stage, stage.ran)
        stage.refused()
        assert stage.last_ms() == t1                       # a failure leaves the previous call's times
        third = stage.good()
        t3 = stage.last_ms()
        _check(t3, stage, stage.ran_later or stage.ran)
        assert t3 != t1 and third == first                 # fresh times; the handle still computes the same
    finally:
        stage.close()
