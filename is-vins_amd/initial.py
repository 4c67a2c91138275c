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
    """argument types of the batched initialisation stages' internal entry points and their *_last_ms readers (the SfM and
    relative-pose structs are defined further down)"""
    if getattr(lib, "_init_bound", False):
        return
    pp = lambda t: C.POINTER(C.POINTER(t))
    for name, args in (("isv_internal_visual_imu_align_batch", [pp(isv_align_problem_t), C.POINTER(isv_align_result_t)]),
                       ("isv_internal_sfm_batch", [pp(isv_sfm_problem_t), C.POINTER(isv_sfm_result_t)]),
                       ("isv_internal_relpose_batch", [pp(isv_sfm_problem_t), C.POINTER(isv_relpose_result_t), pp(C.c_int32)])):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int32] + args
        getattr(lib, name).restype = C.c_int
    for stage in ("align", "sfm", "relpose"):
        getattr(lib, f"isv_internal_{stage}_last_ms").argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        getattr(lib, f"isv_internal_{stage}_last_ms").restype = C.c_int
    lib._init_bound = True


_bind_sfm = _bind_relpose = _bind   # the names the SfM and relative-pose tests bind through


def _run(be, entry, problem_t, result_t, problems, *extra):
    """one call of a batched stage's entry point on the backend handle `be`; returns the list of results"""
    _bind(be.lib)
    n = len(problems)
    ptrs = (C.POINTER(problem_t) * max(n, 1))(*[C.pointer(p.c) for p in problems])
    res = (result_t * max(n, 1))()
    rc = getattr(be.lib, entry)(be.h, n, ptrs, res, *extra)
    if rc != 0:
        raise backend.BackendError(f"{entry}: {backend.STATUS.get(rc, rc)}: {be.lib.isv_backend_last_error(be.h)}")
    return [res[i] for i in range(n)]


def _last_ms(be, stage):
    """(whole call, kernel) milliseconds of the stage's last call on this handle"""
    _bind(be.lib)
    out = (C.c_double * 2)()
    getattr(be.lib, f"isv_internal_{stage}_last_ms")(be.h, out)
    return out[0], out[1]


def align_batch(be, problems):
    """isv_internal_visual_imu_align_batch on the backend handle `be` (backend.Backend); returns the list of results"""
    return _run(be, "isv_internal_visual_imu_align_batch", isv_align_problem_t, isv_align_result_t, problems)


def last_ms(be):
    """(whole call, kernel) milliseconds of the last align_batch on this handle"""
    return _last_ms(be, "align")


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


# ---------------------------------------------------------------------------------------------------------------------
# The SfM stage (is-vins_amd/csrc/isv_sfm.h): IMU excitation, GlobalSFM::construct with its BA, the all-frame PnP.

ISV_SFM_MAX_TRACKS = 1024
ISV_SFM_MAX_OBS = 4096
SFM_STATUS = {0: "ok", 1: "excitation", 2: "sfm_pnp_points", 3: "ba_not_converged", 4: "all_pnp_points", 5: "capacity", 6: "input"}
_W, _F = ISV_ALIGN_MAX_WINDOW, ISV_ALIGN_MAX_FRAMES


class isv_sfm_track_t(C.Structure):
    _fields_ = [("id", C.c_int32), ("start_frame", C.c_int32), ("n_obs", C.c_int32), ("obs_off", C.c_int32)]


class isv_sfm_problem_t(C.Structure):
    _fields_ = [("n_window", C.c_int32), ("n_frames", C.c_int32), ("l", C.c_int32), ("n_tracks", C.c_int32), ("n_obs", C.c_int32),
                ("n_pts", C.c_int32), ("relative_R", C.c_double * 9), ("relative_T", C.c_double * 3), ("RIC", C.c_double * 9),
                ("tracks", C.POINTER(isv_sfm_track_t)), ("obs", C.POINTER(C.c_double)), ("pt_off", C.POINTER(C.c_int32)),
                ("pt_id", C.POINTER(C.c_int32)), ("pt_uv", C.POINTER(C.c_double)), ("delta_v", C.POINTER(C.c_double)),
                ("sum_dt", C.POINTER(C.c_double)), ("window_frame", C.c_int32 * _W),
                ("position", C.POINTER(C.c_double)), ("state", C.POINTER(C.c_int32))]


class isv_sfm_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("fail_frame", C.c_int32), ("ba_iterations", C.c_int32), ("ba_termination", C.c_int32),
                ("ba_residuals", C.c_int32), ("ba_successful", C.c_int32), ("n_triangulated", C.c_int32), ("n_ba_cols", C.c_int32),
                ("excitation_var", C.c_double), ("ba_initial_cost", C.c_double), ("ba_final_cost", C.c_double),
                ("Q", (C.c_double * 4) * _W), ("T", (C.c_double * 3) * _W),
                ("sfm_pnp_iterations", C.c_int32 * _W), ("sfm_pnp_points", C.c_int32 * _W),
                ("R", (C.c_double * 9) * _F), ("Tf", (C.c_double * 3) * _F), ("is_key_frame", C.c_int32 * _F),
                ("pnp_iterations", C.c_int32 * _F), ("pnp_points", C.c_int32 * _F)]

    def arr(self, name):
        return np.ctypeslib.as_array(getattr(self, name)).copy()


class SfmProblem:
    """one isv_sfm_problem_t, the arrays it points into and its per-track outputs (kept alive with it)"""

    def __init__(self, n_window, l, relative_R, relative_T, RIC, tracks, obs, frame_pts, delta_v, sum_dt, window_frame):
        """tracks: [(id, start_frame, n_obs)] in IDsfeatures order, obs: [sum n_obs][2] in track order; frame_pts: per
        all_image_frame entry a list of (feature_id, u, v) ascending by id; delta_v [n_frames][3], sum_dt [n_frames]"""
        n_frames = len(frame_pts)
        self.tracks = (isv_sfm_track_t * max(len(tracks), 1))()
        off = 0
        for j, (tid, s, n) in enumerate(tracks):
            self.tracks[j].id, self.tracks[j].start_frame, self.tracks[j].n_obs, self.tracks[j].obs_off = int(tid), int(s), int(n), off
            off += int(n)
        self.obs = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 2))
        self.pt_off = np.zeros(n_frames + 1, dtype=np.int32)
        ids, uvs = [], []
        for f, pts in enumerate(frame_pts):
            for (i, u, v) in pts:
                ids.append(int(i)); uvs.append((u, v))
            self.pt_off[f + 1] = len(ids)
        self.pt_id = np.array(ids if ids else [0], dtype=np.int32)
        self.pt_uv = np.ascontiguousarray(np.array(uvs if uvs else [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2))
        self.delta_v = np.ascontiguousarray(np.asarray(delta_v, dtype=np.float64).reshape(-1, 3))
        self.sum_dt = np.ascontiguousarray(np.asarray(sum_dt, dtype=np.float64))
        self.position = np.zeros((max(len(tracks), 1), 3))
        self.state = np.zeros(max(len(tracks), 1), dtype=np.int32)
        c = self.c = isv_sfm_problem_t()
        c.n_window, c.n_frames, c.l, c.n_tracks, c.n_obs, c.n_pts = n_window, n_frames, l, len(tracks), off, len(ids)
        c.relative_R[:] = np.asarray(relative_R, dtype=np.float64).ravel().tolist()
        c.relative_T[:] = np.asarray(relative_T, dtype=np.float64).ravel().tolist()
        c.RIC[:] = np.asarray(RIC, dtype=np.float64).ravel().tolist()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        c.tracks = C.cast(self.tracks, C.POINTER(isv_sfm_track_t))
        c.obs = self.obs.ctypes.data_as(dp)
        c.pt_off, c.pt_id, c.pt_uv = self.pt_off.ctypes.data_as(ip), self.pt_id.ctypes.data_as(ip), self.pt_uv.ctypes.data_as(dp)
        c.delta_v, c.sum_dt = self.delta_v.ctypes.data_as(dp), self.sum_dt.ctypes.data_as(dp)
        for i, w in enumerate(window_frame):
            c.window_frame[i] = int(w)
        c.position, c.state = self.position.ctypes.data_as(dp), self.state.ctypes.data_as(ip)
        self.truth = {}


def sfm_batch(be, problems):
    """isv_internal_sfm_batch on the backend handle `be`; returns the results (each problem's position / state arrays are
    filled in place)"""
    return _run(be, "isv_internal_sfm_batch", isv_sfm_problem_t, isv_sfm_result_t, problems)


def sfm_last_ms(be):
    """(whole call, kernel) milliseconds of the last sfm_batch on this handle"""
    return _last_ms(be, "sfm")


def copy_sfm_to_align(res, align_problem):
    """ImageFrame::R / T / is_key_frame of every all_image_frame entry, as the SfM result has them, into an alignment problem"""
    for f in range(align_problem.c.n_frames):
        fr = align_problem.frames[f]
        fr.R[:] = list(res.R[f]); fr.T[:] = list(res.Tf[f]); fr.is_key_frame = res.is_key_frame[f]


def initial_structure_batch(be, sfm_problems, align_problems):
    """initialStructure after relativePose: the SfM stage on every problem, then the alignment on the problems whose SfM
    succeeded (their R / T / is_key_frame copied in).  Returns (sfm results, alignment results with None where the SfM
    refused)"""
    sr = sfm_batch(be, sfm_problems)
    ok = [i for i, r in enumerate(sr) if r.status == 0]
    for i in ok:
        copy_sfm_to_align(sr[i], align_problems[i])
    ar = align_batch(be, [align_problems[i] for i in ok]) if ok else []
    out = [None] * len(sfm_problems)
    for i, r in zip(ok, ar):
        out[i] = r
    return sr, out


def _rotvec(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def make_scene(seed=0, n_window=11, extra=0, l=None, per_frame=150, pixel_noise=0.0, rel_rot_err=0.0, rel_dir_err=0.0,
               cam_dt=0.1, imu_per_frame=10, acc_noise=0.0, gyr_noise=0.0, depth=(6.0, 16.0), max_obs=ISV_SFM_MAX_OBS, behind=0, **kw):
    """a seeded synthetic initialisation scene: (SfmProblem, alignment Problem).  The trajectory and IMU are make_problem's
    (same seed), with `extra` non-keyframes spread between the window frames of all_image_frame (S4).  Landmarks lie
    `depth` metres in front of the camera of their first frame and are tracked through RIC / TIC by a pinhole camera for
    2..n_window consecutive window frames while in view (about `per_frame` observations per frame, at most max_obs in all).
    relative_R / T between l (default n_window // 2) and the last window frame come from ground truth with |T| = 1, turned by
    rel_rot_err [rad] and rel_dir_err [rad] when given.  pixel_noise: white noise on the normalised image points.  behind:
    that many extra tracks of a point BEHIND the cameras of window frames 0 and 1 (only step 5 triangulates them, S5).
    truth: the SfM frame's Q / T (camera i to camera l, unit baseline), the landmarks in it, every frame's R / T as the
    all-frame PnP should give them; the alignment problem's truth scale is the baseline in metres."""
    n_frames = n_window + extra
    window = sorted(set(np.linspace(0, n_frames - 1, n_window).round().astype(int).tolist()))
    assert len(window) == n_window
    ap = make_problem(seed=seed, n_frames=n_frames, window_frame=window, cam_dt=cam_dt, imu_per_frame=imu_per_frame, sfm_scale=1.0,
                      acc_noise=acc_noise, gyr_noise=gyr_noise, **kw)
    ric = synth.RIC
    rng = synth.SplitMix64(0x5F3D00000000 + seed)
    l = n_window // 2 if l is None else l
    Rc = [np.array(ap.frames[f].R).reshape(3, 3) @ ric for f in range(n_frames)]   # camera to c0
    Cc = [np.array(ap.frames[f].T) for f in range(n_frames)]                       # camera centres in c0 (metres)
    wl, wlast = window[l], window[-1]
    base = np.linalg.norm(Cc[wlast] - Cc[wl]) or 1.0   # (a hovering body: no baseline)
    to_l = lambda X: Rc[wl].T @ (X - Cc[wl]) / base                                  # noqa: E731
    # landmarks
    tracks, obs, lms, truth_pts = [], [], [], []
    mean_len = (2 + n_window) / 2.5
    n_lm = int(round(per_frame * n_window / mean_len))
    u = rng.uniform(6 * n_lm * 4).reshape(-1, 6)
    nz = rng.normal(2 * n_lm * n_window * 4 + 2 * n_frames * n_lm).tolist()
    ni = iter(nz)
    next_id = 7
    k = 0
    while len(tracks) < n_lm and k < len(u):
        s = int(u[k, 0] * (n_window - 1))
        L = max(2, int(np.sqrt(u[k, 1]) * (n_window + 1)))
        L = min(L, n_window - s)
        d = depth[0] + (depth[1] - depth[0]) * u[k, 2]
        xy = (u[k, 3:5] - 0.5) * 1.2
        X = Rc[window[s]] @ (np.array([xy[0], xy[1], 1.0]) * d) + Cc[window[s]]
        k += 1
        uv = []
        for i in range(s, s + L):
            xc = Rc[window[i]].T @ (X - Cc[window[i]])
            if xc[2] < 0.2 or abs(xc[0] / xc[2]) > 1.2 or abs(xc[1] / xc[2]) > 1.2:
                break
            uv.append(xc[:2] / xc[2])
        if len(uv) < 2 or len(obs) + len(uv) > max_obs:
            continue
        uv = [p + pixel_noise * np.array([next(ni), next(ni)]) for p in uv]
        tracks.append((next_id, s, len(uv)))
        obs.extend(uv)
        lms.append(X)
        truth_pts.append(to_l(X))
        next_id += 1 + int(u[k - 1, 5] * 3)
    for b in range(behind):
        X = Rc[window[0]] @ (np.array([0.1 * b - 0.2, 0.15, -1.0]) * 5.0) + Cc[window[0]]
        uv = [(Rc[window[i]].T @ (X - Cc[window[i]]))[:2] / (Rc[window[i]].T @ (X - Cc[window[i]]))[2] for i in (0, 1)]
        tracks.append((next_id, 0, 2)); obs.extend(uv); lms.append(X); truth_pts.append(to_l(X))
        next_id += 1
    # all_image_frame's points: the window frames' own observations; a non-keyframe sees the tracks alive at both neighbours
    frame_pts = [[] for _ in range(n_frames)]
    off = 0
    for (tid, s, n), X in zip(tracks, lms):
        for i in range(n):
            frame_pts[window[s + i]].append((tid, obs[off + i][0], obs[off + i][1]))
        for f in range(n_frames):
            if f in window:
                continue
            i1 = int(np.searchsorted(window, f))
            if s <= i1 - 1 and i1 < s + n:
                xc = Rc[f].T @ (X - Cc[f])
                if xc[2] > 0.2:
                    p = xc[:2] / xc[2] + pixel_noise * np.array([next(ni), next(ni)])
                    frame_pts[f].append((tid, p[0], p[1]))
        off += n
    for f in range(n_frames):
        frame_pts[f].sort(key=lambda e: e[0])
    # pre-integration delta_v / sum_dt of every frame (stage 0)
    dv, sdt = np.zeros((n_frames, 3)), np.zeros(n_frames)
    for f in range(1, n_frames):
        fr = ap.frames[f]
        rows = ap.imu[fr.imu_begin:fr.imu_begin + fr.imu_count]
        acc = np.vstack([np.array(fr.linearized_acc), rows[:, 1:4]])
        gyr = np.vstack([np.array(fr.linearized_gyr), rows[:, 4:7]])
        pre = synth.preintegrate(rows[0, 0], acc[None], gyr[None], np.zeros((1, 3)), np.zeros((1, 3)))
        dv[f], sdt[f] = pre["delta_v"][0], pre["sum_dt"]
    relR = Rc[wl].T @ Rc[wlast]
    relT = to_l(Cc[wlast])
    if rel_rot_err:
        a = np.array([0.3, -0.5, 0.8]); relR = _rotvec(rel_rot_err * a / np.linalg.norm(a)) @ relR
    if rel_dir_err:
        a = np.cross(relT, [0.2, 0.9, -0.4]); relT = _rotvec(rel_dir_err * a / np.linalg.norm(a)) @ relT
    sp = SfmProblem(n_window, l, relR, relT, ric, tracks, obs, frame_pts, dv, sdt, window)
    sp.truth = dict(Q=np.array([Rc[wl].T @ Rc[w] for w in window]), T=np.array([to_l(Cc[w]) for w in window]),
                    points=np.array(truth_pts).reshape(-1, 3), R=np.array([Rc[wl].T @ Rc[f] @ ric.T for f in range(n_frames)]),
                    Tf=np.array([to_l(Cc[f]) for f in range(n_frames)]), base=base)
    ap.truth["scale"] = base
    return sp, ap


def q_to_R(q):
    """x y z w -> rotation matrix (normalised)"""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sfm_errors(res, sp):
    """errors of an OK SfM result against the scene's truth (the SfM frame is fixed by camera l and the unit baseline, so no
    similarity is left to fit): (max rotation error of Q [Frobenius], max |T - T_gt|, max point error, max all-frame R error,
    max all-frame T error)"""
    tr = sp.truth
    nw, nf = sp.c.n_window, sp.c.n_frames
    eq = max(np.linalg.norm(q_to_R(res.Q[i]) - tr["Q"][i]) for i in range(nw))
    et = np.abs(np.array([list(res.T[i]) for i in range(nw)]) - tr["T"]).max()
    st = sp.state[:sp.c.n_tracks].astype(bool)
    ep = np.abs(sp.position[:sp.c.n_tracks][st] - tr["points"][st]).max() if st.any() else 0.0
    eR = max(np.linalg.norm(np.array(res.R[f]).reshape(3, 3) - tr["R"][f]) for f in range(nf))
    eT = np.abs(np.array([list(res.Tf[f]) for f in range(nf)]) - tr["Tf"]).max()
    return eq, et, ep, eR, eT


# ---------------------------------------------------------------------------------------------------------------------
# The relative-pose stage (is-vins_amd/csrc/isv_relpose.h): IMU excitation, then relativePose's candidates, each a
# findFundamentalMat RANSAC and recoverPose.  It reads the SfM problem and ignores its l / relative_R / relative_T.

RELPOSE_STATUS = {0: "ok", 1: "excitation", 2: "no_relative_pose", 3: "capacity", 4: "input"}


class isv_relpose_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("l", C.c_int32), ("n_candidates", C.c_int32), ("_pad", C.c_int32),
                ("excitation_var", C.c_double), ("relative_R", C.c_double * 9), ("relative_T", C.c_double * 3),
                ("n_corres", C.c_int32 * _W), ("ransac_iters", C.c_int32 * _W), ("ransac_inliers", C.c_int32 * _W),
                ("recover_inliers", C.c_int32 * _W), ("solution", C.c_int32 * _W), ("parallax", C.c_double * _W)]

    def arr(self, name):
        return np.ctypeslib.as_array(getattr(self, name)).copy()


def apply_relpose(res, sp):
    """relativePose's outputs (l, relative_R, relative_T) of an OK result into the SfM problem it was computed from"""
    sp.c.l = res.l
    sp.c.relative_R[:] = list(res.relative_R)
    sp.c.relative_T[:] = list(res.relative_T)


def relpose_batch(be, problems, write=False, masks=False):
    """isv_internal_relpose_batch on the backend handle `be`; returns the results, and with masks=True also a list of
    per-track inlier masks (int32 [n_tracks]: 1 / 0 for the chosen pair's correspondences, -1 elsewhere).  write=True copies
    l / relative_R / relative_T of every OK result into its problem (apply_relpose)."""
    mk, mptr = None, None
    if masks:
        mk = [np.full(max(p.c.n_tracks, 1), -1, dtype=np.int32) for p in problems]
        mptr = (C.POINTER(C.c_int32) * max(len(problems), 1))(*[m.ctypes.data_as(C.POINTER(C.c_int32)) for m in mk])
    out = _run(be, "isv_internal_relpose_batch", isv_sfm_problem_t, isv_relpose_result_t, problems, mptr)
    if write:
        for r, p in zip(out, problems):
            if r.status == 0:
                apply_relpose(r, p)
    return (out, [m[:p.c.n_tracks] for m, p in zip(mk, problems)]) if masks else out


def relpose_last_ms(be):
    """(whole call, kernel) milliseconds of the last relpose_batch on this handle"""
    return _last_ms(be, "relpose")


def initial_structure_from_tracks_batch(be, sfm_problems, align_problems):
    """initialStructure from tracks, pre-integrations and RIC: the relative-pose stage on every problem (its l / relative_R /
    relative_T written into the problem), then initial_structure_batch (SfM, then alignment) on the problems whose relative
    pose was found.  Returns (relpose results, SfM results, alignment results), with None where an earlier stage refused."""
    rr = relpose_batch(be, sfm_problems, write=True)
    ok = [i for i, r in enumerate(rr) if r.status == 0]
    sr = [None] * len(sfm_problems)
    ar = [None] * len(sfm_problems)
    if ok:
        s_ok, a_ok = initial_structure_batch(be, [sfm_problems[i] for i in ok], [align_problems[i] for i in ok])
        for i, s, a in zip(ok, s_ok, a_ok):
            sr[i], ar[i] = s, a
    return rr, sr, ar


def make_relpose_scene(seed=0, n_window=18, outliers=0.0, **kw):
    """make_scene (same arguments; its output is unchanged) with `outliers`: that fraction of the tracks that reach the last
    window frame get a mismatched last observation, a uniform point in [-0.6, 0.6]^2 from a stream of their own.  Far depths
    (low parallax) are make_scene's `depth`.  truth["outliers"]: the indices of the corrupted tracks.  The tracks do not
    depend on l, so make_relpose_scene(seed, l=found, ...) gives the truth for the l the stage finds."""
    sp, ap = make_scene(seed=seed, n_window=n_window, **kw)
    bad = []
    if outliers > 0:
        rng = synth.SplitMix64(0x0E1A7E000000 + seed)
        last = sp.c.n_window - 1
        reach = [j for j in range(sp.c.n_tracks) if sp.tracks[j].start_frame + sp.tracks[j].n_obs - 1 == last]
        u = rng.uniform(3 * len(reach)).reshape(-1, 3)
        bad = [j for j, r in zip(reach, u) if r[0] < outliers]
        wl = sp.c.window_frame[last]
        for j, r in zip(reach, u):
            if r[0] >= outliers:
                continue
            T = sp.tracks[j]
            k = T.obs_off + T.n_obs - 1
            sp.obs[k] = (r[1] - 0.5) * 1.2, (r[2] - 0.5) * 1.2
            a, b = sp.pt_off[wl], sp.pt_off[wl + 1]   # all_image_frame's copy of the same observation
            hit = np.nonzero(sp.pt_id[a:b] == T.id)[0]
            if hit.size:
                sp.pt_uv[a + hit[0]] = sp.obs[k]
    sp.truth["outliers"] = np.array(bad, dtype=np.int64)
    return sp, ap
