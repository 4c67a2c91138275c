"""Host-side mirror of include/isvins_loop.h: the batched loop-closure verification, KeyFrame::findConnection
(reference src/pose_graph/keyframe.cpp:231-295: brute-force BRIEF matching, PnP-RANSAC, the relative pose, the yaw /
distance gate and loop_weight) for many keyframe pairs in one call.  `LoopVerifier(...)` raises when the HIP extension is
missing or there is no GPU: no CPU path.

`make_loop_scene` builds deterministic synthetic pairs for the tests and scripts/loop_bench.py; descriptors and the loop
candidate are inputs (the DBoW query is bow.py, the extraction of descriptors and corners from an image keyframe.py)."""
import ctypes as C

import numpy as np

from . import _stage, backend, posegraph, synth

(ISV_LOOP_OK, ISV_LOOP_FEW_MATCHES, ISV_LOOP_UNDEFINED_POSE, ISV_LOOP_PNP_FAILED, ISV_LOOP_GATE, ISV_LOOP_PLANAR, ISV_LOOP_CAPACITY,
 ISV_LOOP_INPUT) = range(8)

_u64p, _f32p, _i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_int32)


class isv_loop_config_t(C.Structure):
    _fields_ = [("max_pairs", C.c_int32), ("max_points", C.c_int32), ("max_keypoints", C.c_int32), ("min_loop_num", C.c_int32),
                ("ransac_iterations", C.c_int32), ("match_max_dist", C.c_int32), ("match_accept_dist", C.c_int32), ("_pad", C.c_int32),
                ("ric", C.c_double * 9), ("tic", C.c_double * 3), ("focal_length", C.c_double), ("ransac_threshold", C.c_double),
                ("ransac_confidence", C.c_double), ("max_yaw_deg", C.c_double), ("max_distance", C.c_double)]


class isv_loop_pair_t(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_keypoints", C.c_int32), ("old_index", C.c_int32), ("_pad", C.c_int32),
                ("window_brief", _u64p), ("point_3d", _f32p), ("point_2d_norm", _f32p), ("brief", _u64p), ("keypoints_norm", _f32p),
                ("origin_vio_T", C.c_double * 3), ("origin_vio_R", C.c_double * 9)]


class isv_loop_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matched", C.c_int32), ("ransac_iters", C.c_int32), ("ransac_inliers", C.c_int32),
                ("pnp_iterations", C.c_int32), ("n_final", C.c_int32), ("has_loop", C.c_int32), ("loop_index", C.c_int32),
                ("loop_info", C.c_double * 8), ("loop_weight", C.c_double), ("PnP_T_old", C.c_double * 3), ("PnP_R_old", C.c_double * 9),
                ("res", C.c_double)]

    def arr(self, name):
        return np.array(getattr(self, name))


EXPORTS = ["isv_loop_create", "isv_loop_destroy", "isv_loop_last_error", "isv_loop_verify_batch", "isv_loop_last_ms", "isv_loop_apply"]


def make_config(max_pairs=1, max_points=256, max_keypoints=2048, ric=None, tic=None, min_loop_num=15, focal_length=460.0,
                ransac_threshold=10.0 / 460.0, ransac_confidence=0.99, ransac_iterations=100, max_yaw_deg=30.0, max_distance=20.0,
                match_max_dist=128, match_accept_dist=80):
    """the reference's constants as defaults (keyframe.cpp:84, :97, :187, :262, :282; MIN_LOOP_NUM, FOCAL_LENGTH, RIC[0] / TIC[0])"""
    c = isv_loop_config_t()
    c.max_pairs, c.max_points, c.max_keypoints = max_pairs, max_points, max_keypoints
    c.min_loop_num, c.ransac_iterations, c.match_max_dist, c.match_accept_dist = min_loop_num, ransac_iterations, match_max_dist, match_accept_dist
    c.ric[:] = np.asarray(synth.RIC if ric is None else ric, float).ravel()
    c.tic[:] = np.asarray(synth.TIC if tic is None else tic, float).ravel()
    c.focal_length, c.ransac_threshold, c.ransac_confidence = focal_length, ransac_threshold, ransac_confidence
    c.max_yaw_deg, c.max_distance = max_yaw_deg, max_distance
    return c


class LoopPair:
    """one candidate pair: numpy arrays (kept alive here) behind an isv_loop_pair_t (`.c`)"""

    def __init__(self, window_brief, point_3d, point_2d_norm, brief, keypoints_norm, origin_vio_T, origin_vio_R, old_index=0):
        self.window_brief = np.ascontiguousarray(window_brief, dtype=np.uint64).reshape(-1, 4)
        self.point_3d = np.ascontiguousarray(point_3d, dtype=np.float32).reshape(-1, 3)
        self.point_2d_norm = np.ascontiguousarray(point_2d_norm, dtype=np.float32).reshape(-1, 2)
        self.brief = np.ascontiguousarray(brief, dtype=np.uint64).reshape(-1, 4)
        self.keypoints_norm = np.ascontiguousarray(keypoints_norm, dtype=np.float32).reshape(-1, 2)
        self.origin_vio_T = np.asarray(origin_vio_T, float).copy()
        self.origin_vio_R = np.asarray(origin_vio_R, float).reshape(3, 3).copy()
        assert len(self.point_3d) == len(self.window_brief) == len(self.point_2d_norm) and len(self.brief) == len(self.keypoints_norm)
        c = self.c = isv_loop_pair_t()
        c.n_points, c.n_keypoints, c.old_index = len(self.window_brief), len(self.brief), old_index
        c.window_brief = self.window_brief.ctypes.data_as(_u64p); c.point_3d = self.point_3d.ctypes.data_as(_f32p)
        c.point_2d_norm = self.point_2d_norm.ctypes.data_as(_f32p)
        c.brief = self.brief.ctypes.data_as(_u64p); c.keypoints_norm = self.keypoints_norm.ctypes.data_as(_f32p)
        c.origin_vio_T[:] = self.origin_vio_T; c.origin_vio_R[:] = self.origin_vio_R.ravel()

    @property
    def n_points(self):
        return self.c.n_points


@_stage.bind_once("loop")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_loop_create.argtypes = [C.POINTER(isv_loop_config_t), C.POINTER(vp)]
    lib.isv_loop_destroy.argtypes = [vp]; lib.isv_loop_destroy.restype = None
    lib.isv_loop_last_error.argtypes = [vp]; lib.isv_loop_last_error.restype = C.c_char_p
    lib.isv_loop_verify_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_loop_pair_t)), C.POINTER(isv_loop_result_t),
                                          C.POINTER(_i32p), C.POINTER(_i32p), C.POINTER(_i32p)]
    lib.isv_loop_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_loop_apply.argtypes = [C.POINTER(isv_loop_result_t), C.POINTER(posegraph.isv_pg_keyframe_t)]


def apply(result, keyframe, lib=None):
    """isv_loop_apply (host only): what keyframe.cpp:285-289 and :224 write into the current keyframe"""
    lib = lib or backend.load_library()
    _bind(lib)
    rc = lib.isv_loop_apply(C.byref(result), C.byref(keyframe))
    if rc != 0:
        raise backend.BackendError(f"isv_loop_apply: {backend.STATUS.get(rc, rc)}")


class LoopVerifier(_stage.StageHandle):
    """KeyFrame::findConnection on the MI355X: one workgroup per keyframe pair in each of two kernels"""
    PREFIX, N_MS = "isv_loop", 3

    def __init__(self, max_pairs=1, max_points=256, max_keypoints=2048, **kw):
        self.cfg = make_config(max_pairs, max_points, max_keypoints, **kw)
        self._create(_bind, C.byref(self.cfg), why=" (a MI355X and the HIP extension are required; there is no CPU path)")

    def verify_batch(self, pairs, per_point=False):
        """pairs: LoopPair list -> isv_loop_result_t list; with per_point also (match_index, match_dist, inlier), each a list of
        int32 arrays [n_points] (pre-filled with -2: a refused pair's stay untouched)"""
        n = len(pairs)
        res = (isv_loop_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_loop_pair_t) * max(n, 1))(*[C.pointer(p.c) for p in pairs])
        outs = None
        args = [None, None, None]
        if per_point:
            outs = [[np.full(max(p.c.n_points, 1), -2, dtype=np.int32) for p in pairs] for _ in range(3)]
            args = [(_i32p * max(n, 1))(*[a.ctypes.data_as(_i32p) for a in o]) for o in outs]
        rc = self.lib.isv_loop_verify_batch(self.h, n, ptrs, res, *args)
        self._check(rc, "isv_loop_verify_batch", with_last_error=True)
        out = list(res)[:n]
        if not per_point:
            return out
        return (out,) + tuple([a[:max(p.c.n_points, 0)] for a, p in zip(o, pairs)] for o in outs)

    def last_ms(self):
        """(whole call, k_loop_match, k_loop_pnp) milliseconds of the last successful call"""
        return super().last_ms()

    def apply(self, result, keyframe):
        apply(result, keyframe, self.lib)


# ---------------------------------------------------------------------------------------------------------------------
def flip_bits(desc, positions):
    """a copy of the 256-bit descriptor desc [4] uint64 with the given bit positions (bit 64 w + b = bit b of word w) flipped"""
    d = np.array(desc, dtype=np.uint64).copy()
    for pos in positions:
        d[int(pos) // 64] ^= np.uint64(1) << np.uint64(int(pos) % 64)
    return d


def make_loop_scene(seed, n_points=150, n_keypoints=600, outliers=0.0, pixel_noise=0.0, flipped_bits=20, yaw=0.2, offset=(0.4, -0.3, 0.1),
                    n_matchable=None, planar=False, old_index=0, old_pose=None, cur_pose=None):
    """A loop candidate: the old keyframe at a fixed pose, the current keyframe (origin_vio pose) turned by `yaw` radians about z and
    moved by `offset` (in the old keyframe's frame) from it; old_pose / cur_pose = (R, T) give the two poses instead.  Window points get random 256-bit descriptors and float32 world
    points in front of the old camera (on a plane when `planar`).  The first n_matchable (default: all) points have a counterpart
    among the old corners: a true match is the descriptor with `flipped_bits` random bits flipped, sitting at the point's projection
    into the old camera plus pixel_noise (normalised units); an outlier (the fraction `outliers` of the counterparts) is such a near
    copy sitting at a wrong location.  The other old corners are random distractors; the corners are shuffled.  Deterministic.
    Returns (LoopPair, truth): truth has R_old / T_old (the old keyframe's pose, what PnP_R_old / PnP_T_old estimate), relative_t,
    relative_R, yaw_deg, is_outlier [n_points] and counterpart [n_points] (old corner index or -1)."""
    rng = np.random.Generator(np.random.PCG64(0x100F_0000 + int(seed)))
    ric, tic = synth.RIC, synth.TIC
    R_old = synth._rot_zyx(0.3 + 0.1 * seed, 0.05, -0.04)
    T_old = np.array([1.0, -2.0, 0.5]) + 0.1 * seed
    if old_pose is not None:
        R_old, T_old = np.asarray(old_pose[0], float), np.asarray(old_pose[1], float)
    R_cur = R_old @ synth._rot_zyx(yaw, 0.02, -0.01)
    T_cur = T_old + R_old @ np.asarray(offset, float)
    if cur_pose is not None:
        R_cur, T_cur = np.asarray(cur_pose[0], float), np.asarray(cur_pose[1], float)
    R_wc, T_wc = R_old @ ric, T_old + R_old @ tic               # the old camera in the world
    nm = n_points if n_matchable is None else int(n_matchable)
    assert 0 <= nm <= n_points and nm <= n_keypoints
    z = rng.uniform(2.0, 8.0, n_points)
    if planar:
        z = 4.0 + 0.0 * z
    pc = np.stack([rng.uniform(-0.6, 0.6, n_points) * z, rng.uniform(-0.45, 0.45, n_points) * z, z], 1)
    p3d = (pc @ R_wc.T + T_wc).astype(np.float32)               # L5: the reference holds them as cv::Point3f
    pcf = (p3d.astype(np.float64) - T_wc) @ R_wc                # the float32 points seen from the old camera
    proj = pcf[:, :2] / pcf[:, 2:3]
    wb = rng.integers(0, 2 ** 64, size=(n_points, 4), dtype=np.uint64)
    kb = rng.integers(0, 2 ** 64, size=(n_keypoints, 4), dtype=np.uint64)
    kpn = np.stack([rng.uniform(-0.7, 0.7, n_keypoints), rng.uniform(-0.5, 0.5, n_keypoints)], 1)
    perm = rng.permutation(n_keypoints)
    is_out = np.zeros(n_points, bool)
    is_out[:nm] = rng.uniform(0, 1, nm) < outliers
    counterpart = np.full(n_points, -1, np.int64)
    for i in range(nm):
        k = int(perm[i])
        counterpart[i] = k
        kb[k] = flip_bits(wb[i], rng.permutation(256)[:flipped_bits])
        if is_out[i]:
            wrong = proj[i] + rng.choice([-1.0, 1.0], 2) * rng.uniform(0.1, 0.3, 2)     # 46 .. 138 px away
            kpn[k] = wrong
        else:
            kpn[k] = proj[i] + pixel_noise * rng.standard_normal(2)
    p2d = rng.uniform(-0.5, 0.5, (n_points, 2))
    pair = LoopPair(wb, p3d, p2d, kb, kpn.astype(np.float32), T_cur, R_cur, old_index)
    rel_R = R_old.T @ R_cur
    yaw_deg = np.degrees(np.arctan2(R_cur[1, 0], R_cur[0, 0]) - np.arctan2(R_old[1, 0], R_old[0, 0]))
    truth = dict(R_old=R_old, T_old=T_old, relative_t=R_old.T @ (T_cur - T_old), relative_R=rel_R, yaw_deg=yaw_deg, is_outlier=is_out,
                 counterpart=counterpart)
    return pair, truth
