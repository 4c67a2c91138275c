"""Host-side mirror of the INTERNAL entry point is-vins_amd/csrc/isv_initial.h: the visual-inertial alignment of the
estimator's initialisation (reference src/initial/initial_aligment.cpp `VisualIMUAlignment`, src/estimator.cpp:357-429
`visualInitialAlign`), batched over sequences on the MI355X.  It is the building block of the window manager's
self-initialisation, which is not built yet; this module serves the tests and scripts/init_bench.py and is not a public API.
`align_batch` raises when the HIP extension is missing or there is no GPU: no CPU path.

`make_problem` builds one deterministic synthetic all_image_frame as GlobalSFM + the all-frame PnP would leave it (exact
SfM poses at an arbitrary scale, in the reference camera's frame) from a `synth.Trajectory`, with the IMU samples between
frames and their pre-integration, plus the ground truth the alignment should recover."""
import ctypes as C

import numpy as np

from . import backend, synth

ISV_ALIGN_MAX_FRAMES = 40
ISV_ALIGN_MAX_WINDOW = 20
STAGES = {0: "ok", 1: "gravity", 2: "scale", 3: "refined_scale", 4: "capacity", 5: "input", 6: "antiparallel"}


class isv_align_frame_t(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("delta_q", C.c_double * 4), ("jac_rr", C.c_double * 9),
                ("linearized_acc", C.c_double * 3), ("linearized_gyr", C.c_double * 3),
                ("imu_begin", C.c_int32), ("imu_count", C.c_int32), ("is_key_frame", C.c_int32), ("_pad", C.c_int32)]


class isv_align_problem_t(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_window", C.c_int32), ("n_imu", C.c_int32), ("_pad", C.c_int32),
                ("frames", C.POINTER(isv_align_frame_t)), ("imu", C.POINTER(C.c_double)),
                ("window_frame", C.c_int32 * ISV_ALIGN_MAX_WINDOW), ("G", C.c_double * 3), ("tic", C.c_double * 3),
                ("Bgs", (C.c_double * 3) * ISV_ALIGN_MAX_WINDOW)]


class isv_align_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_state", C.c_int32), ("delta_bg", C.c_double * 3),
                ("Bgs", (C.c_double * 3) * ISV_ALIGN_MAX_WINDOW), ("g_linear", C.c_double * 3), ("s_linear", C.c_double),
                ("g_c0", C.c_double * 3), ("g", C.c_double * 3), ("s", C.c_double),
                ("Ps", (C.c_double * 3) * ISV_ALIGN_MAX_WINDOW), ("Rs", (C.c_double * 9) * ISV_ALIGN_MAX_WINDOW),
                ("Vs", (C.c_double * 3) * ISV_ALIGN_MAX_WINDOW), ("R0", C.c_double * 9),
                ("x", C.c_double * (3 * ISV_ALIGN_MAX_FRAMES + 3)),
                ("rp_delta_p", (C.c_double * 3) * ISV_ALIGN_MAX_FRAMES), ("rp_delta_q", (C.c_double * 4) * ISV_ALIGN_MAX_FRAMES),
                ("rp_delta_v", (C.c_double * 3) * ISV_ALIGN_MAX_FRAMES), ("rp_sum_dt", C.c_double * ISV_ALIGN_MAX_FRAMES)]

    def arr(self, name):
        return np.ctypeslib.as_array(getattr(self, name)).copy()


class Problem:
    """one isv_align_problem_t and the numpy arrays it points into (kept alive with it)"""

    def __init__(self, frames, imu, window_frame, G, tic, Bgs):
        self.frames = (isv_align_frame_t * len(frames))(*frames)
        self.imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        self.c = isv_align_problem_t()
        self.c.n_frames, self.c.n_window, self.c.n_imu = len(frames), len(window_frame), self.imu.shape[0]
        self.c.frames = C.cast(self.frames, C.POINTER(isv_align_frame_t))
        self.c.imu = self.imu.ctypes.data_as(C.POINTER(C.c_double))
        for i, w in enumerate(window_frame):
            self.c.window_frame[i] = int(w)
        for k in range(3):
            self.c.G[k], self.c.tic[k] = G[k], tic[k]
        for i in range(len(window_frame)):
            for k in range(3):
                self.c.Bgs[i][k] = Bgs[i][k]
        self.truth = {}


def _bind(lib):
    if getattr(lib, "_align_bound", False):
        return
    lib.isv_internal_visual_imu_align_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(isv_align_problem_t)), C.POINTER(isv_align_result_t)]
    lib.isv_internal_visual_imu_align_batch.restype = C.c_int
    lib.isv_internal_align_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.isv_internal_align_last_ms.restype = C.c_int
    lib._align_bound = True


def align_batch(be, problems):
    """isv_internal_visual_imu_align_batch on the backend handle `be` (backend.Backend); returns the list of results"""
    lib = be.lib
    _bind(lib)
    n = len(problems)
    ptrs = (C.POINTER(isv_align_problem_t) * max(n, 1))(*[C.pointer(p.c) for p in problems])
    res = (isv_align_result_t * max(n, 1))()
    rc = lib.isv_internal_visual_imu_align_batch(be.h, n, ptrs, res)
    if rc != 0:
        raise backend.BackendError(f"isv_internal_visual_imu_align_batch: {backend.STATUS.get(rc, rc)}: {lib.isv_backend_last_error(be.h)}")
    return [res[i] for i in range(n)]


def last_ms(be):
    """(whole call, kernel) milliseconds of the last align_batch on this handle"""
    _bind(be.lib)
    out = (C.c_double * 2)()
    be.lib.isv_internal_align_last_ms(be.h, out)
    return out[0], out[1]


def make_problem(seed=0, n_frames=11, window_frame=None, cam_dt=0.1, imu_per_frame=10, radius=1.0, speed=1.0, sfm_scale=0.37,
                 bg=(0.0, 0.0, 0.0), acc_noise=0.0, gyr_noise=0.0, Bgs0=None, t0=0.0, hover=False,
                 discrete=False, R_w_c0=None):
    """all_image_frame of n_frames images cam_dt apart on a circle of `radius` at `speed` (synth.Trajectory's attitude
    wobble), IMU at imu_per_frame samples per image (white noise acc_noise / gyr_noise, constant gyro bias bg), SfM
    poses exact but scaled by sfm_scale in the first camera's frame.  hover: the body stands still (no excitation).
    discrete: the poses after the first follow the pre-integration exactly (R_j = R_i dq, p_j = p_i + v_i dt - g dt^2 / 2 +
    R_i dp, v_j = v_i - g dt + R_i dv), so the alignment's equations hold to rounding.  R_w_c0: the SfM frame's orientation
    (default: the first camera's)."""
    rng = synth.SplitMix64(0x1A11A1000000 + seed)
    traj = synth.Trajectory(phase=2 * np.pi * rng.uniform(1)[0])
    traj.r, traj.v = radius, (0.0 if hover else speed)
    traj.w = traj.v / traj.r
    if hover:
        traj.amp = traj.pamp = 0.0
    G = np.array([0.0, 0.0, synth.G_NORM])
    ric, tic = synth.RIC, synth.TIC
    dt = cam_dt / imu_per_frame
    times = t0 + cam_dt * np.arange(n_frames)
    bg = np.asarray(bg, dtype=np.float64)

    def acc_at(t):
        return traj.R(t).T @ (traj.acc(t) + G)

    def gyr_at(t):
        return traj.gyro(t) + bg

    n_acc = acc_noise * rng.normal(3 * (n_frames * (imu_per_frame + 1))).reshape(n_frames, imu_per_frame + 1, 3)
    n_gyr = gyr_noise * rng.normal(3 * (n_frames * (imu_per_frame + 1))).reshape(n_frames, imu_per_frame + 1, 3)
    # R_c0_w: the first camera's frame unless given
    R_w_c0 = traj.R(times[0]) @ ric if R_w_c0 is None else np.asarray(R_w_c0, dtype=np.float64)
    p_w_c0 = traj.p(times[0]) + traj.R(times[0]) @ tic
    frames, imu, states = [], [], []
    Rwb, pwb, vwb = traj.R(times[0]), traj.p(times[0]), traj.vel(times[0])
    for f, t in enumerate(times):
        fr = isv_align_frame_t()
        fr.is_key_frame = 0
        if f > 0:
            ts = times[f - 1] + dt * np.arange(imu_per_frame + 1)
            acc = np.array([acc_at(s) for s in ts]) + n_acc[f]
            gyr = np.array([gyr_at(s) for s in ts]) + n_gyr[f]
            pre = synth.preintegrate(dt, acc[None], gyr[None], np.zeros((1, 3)), np.zeros((1, 3)))
            q = pre["delta_q"][0]                            # w x y z
            fr.delta_q[:] = [q[1], q[2], q[3], q[0]]
            fr.jac_rr[:] = pre["jacobian"][0][3:6, 3:6].ravel().tolist()
            fr.linearized_acc[:] = acc[0].tolist(); fr.linearized_gyr[:] = gyr[0].tolist()
            fr.imu_begin, fr.imu_count = len(imu), imu_per_frame
            for k in range(1, imu_per_frame + 1):
                imu.append([dt, *acc[k], *gyr[k]])
            if discrete:
                T_ = pre["sum_dt"]
                pwb, vwb = (pwb + vwb * T_ - 0.5 * G * T_ * T_ + Rwb @ pre["delta_p"][0], vwb - G * T_ + Rwb @ pre["delta_v"][0])
                Rwb = Rwb @ synth._q2R(pre["delta_q"][0])
        else:
            fr.delta_q[:] = [0, 0, 0, 1]
        if not discrete or f == 0:
            Rwb, pwb, vwb = traj.R(t), traj.p(t), traj.vel(t)
        R = R_w_c0.T @ Rwb                                  # ImageFrame::R = R_c0_ck * RIC^T
        T = R_w_c0.T @ (pwb + Rwb @ tic - p_w_c0) * sfm_scale
        fr.R[:] = R.ravel().tolist(); fr.T[:] = T.tolist()
        states.append((Rwb, pwb, vwb))
        frames.append(fr)
    if window_frame is None:
        window_frame = list(range(n_frames))
    nw = len(window_frame)
    Bgs0 = np.zeros((nw, 3)) if Bgs0 is None else np.asarray(Bgs0)
    for w in window_frame:
        frames[w].is_key_frame = 1
    p = Problem(frames, np.array(imu) if imu else np.zeros((0, 7)), window_frame, G, tic, Bgs0)
    sw = [states[w] for w in window_frame]
    p.truth = dict(scale=1.0 / sfm_scale, P=np.array([x[1] for x in sw]), R=np.array([x[0] for x in sw]),
                   V=np.array([x[2] for x in sw]), bg=bg, G=G)
    return p


def ate_4dof(res, truth, n):
    """errors of a successful alignment against truth after the 4-DoF (yaw + translation) alignment that anchors window
    frame 0: (max position error, max rotation error [rad], max velocity error, |g - (0, 0, |G|)|, relative scale error)"""
    Rs = np.array([np.array(res.Rs[i]).reshape(3, 3) for i in range(n)])
    Ps = np.array([list(res.Ps[i]) for i in range(n)])
    Vs = np.array([list(res.Vs[i]) for i in range(n)])
    Ryaw = Rs[0] @ truth["R"][0].T                         # a rotation about z when gravity is right
    P_gt = (truth["P"] - truth["P"][0]) @ Ryaw.T
    ep = np.abs(Ps - P_gt).max()
    er = max(np.linalg.norm(Rs[i] - Ryaw @ truth["R"][i]) for i in range(n))
    ev = np.abs(Vs - truth["V"] @ Ryaw.T).max()
    eg = np.linalg.norm(np.array(res.g) - truth["G"])
    es = abs(res.s - truth["scale"]) / truth["scale"]
    return ep, er, ev, eg, es
