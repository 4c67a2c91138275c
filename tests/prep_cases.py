"""The windows on which the solve's input kernels -- k_triangulate, k_imu_prep, k_vector2double -- are held against the 40-digit
statements of tests/prep_highprec.py (tests/test_prep_highprec.py: the CPU oracle and the table itself; tests/test_gpu_prep_highprec.py:
the kernels), and the comparison both files share.

Triangulation.  A RUNG is a list of windows triangulated in one call and judged together.  Every window is built by build_window():
the states of a synthetic window (tests' synth.make_window: perturbed poses, taken as the truth), landmarks placed on rays of their
host camera at chosen depths, every other view the exact projection (rounded once to doubles), optionally with 1/460 of pixel noise.

  ladder_s*_exact / _noisy   positions contracted about frame 0 by s = 1, 1e-1, 1e-2, 1e-3, 2e-4 (baselines 0.5 m .. 0.1 mm at 1..7 m)
  tracks                     k = 2 hosted at frame 0, k = 2 hosted at frame N - 2, k = 3, k = N, eight of each in one window
  clamp                      true depths 0.1 (1 -+ 1e-6), 8 (1 -+ 1e-6), 0.05, 20 and -3 (behind the host camera), three tracks each, in a
                             window contracted by 0.2 (so that a point 0.1 m away stays in front of every view); and 0.1 (1 -+ 4e-9),
                             8 (1 -+ 4e-9): four times the excluded band, 1e4 times the routes' error there (a threshold moved by
                             1e-7 passed the 1e-6 cases unnoticed)
  entry                      depth 0.0, -1.0 and (a third) positive on entry
  norm_plain / _x2p5 / _unit / _varied   one noisy window; its obs_point rows as they are, scaled by 2.5, as unit vectors, and scaled
                             row by row by factors in [0.5, 4]: FeatureManager normalises every point, the depths are the same
  batch                      four windows of 1, 64, 65 and 130 landmarks (260 lanes: five workgroups, the last partial; window
                             boundaries at lanes 1, 65 and 130) with four extrinsics: EuRoC's, identity / zero, EuRoC's turned 180 degrees
                             about x, a random one
  n18                        one (18, 8) window
  degenerate                 [ordinary, all views equal the host's, ordinary, pure rotation about the camera centre]: in the two
                             degenerate windows two singular values vanish and the depth is not determined

What is asserted of a result `got` (judge()):
  decision   got == init_depth exactly  iff  the 40-digit depth d* is outside [0.1, 8]
  value      otherwise e = |got / d* - 1| enters the rung's maximum, unless the landmark is EXCLUDED: (sigma_3 - sigma_4) / sigma_1 < 1e-6
             (not determined), or d* within 1e-9 relative of 0.1 or 8 (a correct route may decide either way).  At most 10 % of a rung
             may be excluded (the degenerate windows apart).
  bound      max e <= TRI_MARGIN * max e_ref over the rung's compared landmarks, e_ref the larger error of two SVD-class float64 routes
             on the same matrix: the oracle's one-sided Jacobi and numpy.linalg.svd.  Neither is the code under test.

The IMU weights and the quaternion cases are described at imu_window() / judge_imu() and quat_window()."""
import ctypes as C

import mpmath as mp
import numpy as np

import prep_highprec as ph
from isvins_amd import abi, synth

INIT_DEPTH = 5.0                      # abi.make_config's default (config/euroc_config.yaml)
D_LO, D_HI = 0.1, 8.0
GAP_MIN, EDGE_REL, EXCLUDED_MAX = 1e-6, 1e-9, 0.10
LADDER = (1.0, 1e-1, 1e-2, 1e-3, 2e-4)

# The margin of the value bound.  Two backward-stable SVDs of one matrix differ by a small factor that cannot be derived (Jacobi order,
# LAPACK's bidiagonalisation); it is MEASURED between the two reference routes, per rung, as max e_oracle / max e_numpy or its inverse,
# whichever is larger (tests/test_prep_highprec.py asserts that the table still measures no more than is recorded here).  TRI_MARGIN is
# twice the largest ratio, and at least 4.  Measured with numpy and the oracle on the CPU (neither route runs on the GPU):
#   ladder  s = 1: 1.60 / 1.92 (exact / noisy)   1e-1: 2.94 / 2.03   1e-2: 2.14 / 1.19   1e-3: 2.77 / 1.11   2e-4: 2.06 / 1.47
#   tracks 1.64   clamp 1.67   entry 3.09   norm_plain 6.58   norm_x2p5 5.78   norm_unit 8.90   norm_varied 5.54   batch 1.03   n18 6.93
#   degenerate (its ordinary windows) 3.04
TRI_ROUTE_RATIO_MEASURED = 8.90        # norm_unit: numpy's SVD at 4.5e-14, the oracle's one-sided Jacobi at 5.1e-15
TRI_MARGIN = 2 * TRI_ROUTE_RATIO_MEASURED


def rot(axis, angle):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def half_turn(axis):
    """the rotation by exactly 180 degrees about `axis`: 2 n n^T - I (exact in doubles for the axes used here)"""
    a = np.asarray(axis, float)
    return 2.0 * np.outer(a, a) / (a @ a) - np.eye(3)


def build_window(seed, hosts, ks, depths, n_frames=11, n_vo=5, contract=1.0, noise=False, ric=None, tic=None, poses=None, entry=None):
    """an abi.Window with the states, IMU records and priors of synth.make_window(seed) and landmarks of its own: landmark l is hosted
    in frame hosts[l], seen in ks[l] consecutive frames, and lies at depths[l] on a ray of the host camera; all other observations are
    its exact projections (+ noise / 460 on x and y when `noise`).  contract: Ps' = Ps[0] + contract (Ps - Ps[0]).  poses: a function
    (Ps, Rs, ric, tic) -> (Ps, Rs) applied after that.  entry[l]: lm_depth on entry (default: 0.0 / -1.0 alternating)."""
    N, L = n_frames, len(hosts)
    base = synth.make_window(seed, n_frames=N, n_vo=n_vo, n_landmarks=4)
    w = abi.Window(N, n_vo, L, int(np.sum(ks)), base.n_rollpitch)
    for name in ("Ps", "Rs", "Vs", "Bas", "Bgs", "tic", "ric"):
        getattr(w, name)[...] = getattr(base, name)
    C.memmove(w.imu, base.imu, C.sizeof(base.imu))
    C.memmove(C.byref(w.pose_prior), C.byref(base.pose_prior), C.sizeof(abi.isv_se3_prior_t))
    C.memmove(C.byref(w.vb_prior), C.byref(base.vb_prior), C.sizeof(abi.isv_linear9_t))
    C.memmove(w.relpose, base.relpose, C.sizeof(base.relpose))
    C.memmove(w.rollpitch, base.rollpitch, C.sizeof(base.rollpitch))
    w.margin_old, w.header0 = base.margin_old, base.header0
    if ric is not None:
        w.ric[...] = ric
    if tic is not None:
        w.tic[...] = tic
    w.Ps[...] = w.Ps[0] + contract * (w.Ps - w.Ps[0])
    if poses is not None:
        P2, R2 = poses(w.Ps.copy(), w.Rs.copy(), w.ric.copy(), w.tic.copy())
        w.Ps[...] = P2; w.Rs[...] = R2
    rng = np.random.default_rng(1000 + seed)
    w.lm_start_frame[:L] = hosts
    w.lm_obs_ptr[1:] = np.cumsum(ks)
    xy = rng.uniform(-0.4, 0.4, size=(L, 2))
    for l in range(L):
        h, o0 = int(hosts[l]), int(w.lm_obs_ptr[l])
        ray = np.array([xy[l, 0], xy[l, 1], 1.0])
        w.obs_point[o0] = ray
        pw = w.Rs[h] @ (w.ric @ (ray * depths[l]) + w.tic) + w.Ps[h]
        for o in range(1, int(ks[l])):
            j = h + o
            pc = w.ric.T @ (w.Rs[j].T @ (pw - w.Ps[j]) - w.tic)
            assert pc[2] * np.sign(depths[l]) > 0.3 * abs(depths[l]), (l, j, pc)          # the view sees the point as the host does
            n = rng.normal(size=2) / 460.0 if noise else np.zeros(2)
            w.obs_point[o0 + o] = [pc[0] / pc[2] + n[0], pc[1] / pc[2] + n[1], 1.0]
    w.lm_depth[:L] = np.where(np.arange(L) % 2 == 0, 0.0, -1.0) if entry is None else entry
    w.planted = np.array(depths, float)
    return w


def _mixed_tracks(rng, L, N, n_vo):
    hosts = rng.integers(0, n_vo, size=L)
    ks = np.array([min(N - h, k) for h, k in zip(hosts, rng.choice([2, 3, 5, N], size=L))])
    return hosts, ks


class Rung:
    def __init__(self, name, windows, shape=(11, 5), degenerate=()):
        self.name, self.windows, self.shape, self.degenerate = name, windows, shape, tuple(degenerate)


def _ladder(s, noisy):
    rng = np.random.default_rng(int(round(-np.log10(s) * 100)) + (7 if noisy else 0))
    hosts, ks = _mixed_tracks(rng, 32, 11, 5)
    return build_window(20 + LADDER.index(s), hosts, ks, rng.uniform(1.0, 7.0, 32), contract=s, noise=noisy)


def _scaled(w, how):
    o = w.clone(); o.planted = w.planted
    rng = np.random.default_rng(5)
    if how == "x2p5":
        o.obs_point *= 2.5
    elif how == "unit":
        o.obs_point /= np.linalg.norm(o.obs_point, axis=1, keepdims=True)
    elif how == "varied":
        o.obs_point *= rng.uniform(0.5, 4.0, size=(len(o.obs_point), 1))
    return o


def _same_views(Ps, Rs, ric, tic):
    return np.tile(Ps[0], (len(Ps), 1)), np.tile(Rs[0], (len(Rs), 1, 1))


def _pure_rotation(Ps, Rs, ric, tic):
    c = Ps[0] + Rs[0] @ tic                                        # the camera centre stays where frame 0 has it
    return np.array([c - R @ tic for R in Rs]), Rs


EXTRINSICS = {"euroc": (synth.RIC, synth.TIC), "identity": (np.eye(3), np.zeros(3)),
              "turned_x": (half_turn([1.0, 0, 0]) @ synth.RIC, synth.TIC * np.array([1.0, -1.0, -1.0])),
              "random": (rot([0.3, -0.5, 0.8], 1.1), np.array([0.05, -0.02, 0.11]))}
_RUNGS = None


def rungs():
    """{name: Rung}, built once"""
    global _RUNGS
    if _RUNGS is not None:
        return _RUNGS
    R = {}
    for s in LADDER:
        for noisy in (False, True):
            name = f"ladder_s{s:g}_{'noisy' if noisy else 'exact'}"
            R[name] = Rung(name, [_ladder(s, noisy)])
    N = 11
    hosts = np.array([0] * 8 + [N - 2] * 8 + [0, 1, 2, 3, 4, 6, 7, 8] + [0] * 8)
    ks = np.array([2] * 8 + [2] * 8 + [3] * 8 + [N] * 8)
    rng = np.random.default_rng(41)
    R["tracks"] = Rung("tracks", [build_window(31, hosts, ks, rng.uniform(1.0, 7.0, 32))])
    planted = [D_LO * (1 - 1e-6), D_LO * (1 + 1e-6), D_HI * (1 - 1e-6), D_HI * (1 + 1e-6), 0.05, 20.0, -3.0,
               D_LO * (1 - 4e-9), D_LO * (1 + 4e-9), D_HI * (1 - 4e-9), D_HI * (1 + 4e-9)]
    depths = np.array([d for d in planted for _ in range(3)] + list(rng.uniform(1.0, 7.0, 12)))
    ks = np.array([3, 5, N] * len(planted) + [4] * 12)
    R["clamp"] = Rung("clamp", [build_window(32, np.zeros(len(ks), int), ks, depths, contract=0.2)])
    hosts, ks = _mixed_tracks(rng, 33, N, 5)
    entry = np.array([(2.0 + 0.37 * l, 0.0, -1.0)[l % 3] for l in range(33)])
    R["entry"] = Rung("entry", [build_window(33, hosts, ks, rng.uniform(1.0, 7.0, 33), entry=entry)])
    hosts, ks = _mixed_tracks(rng, 32, N, 5)
    plain = build_window(34, hosts, ks, rng.uniform(1.0, 7.0, 32), noise=True)
    R["norm_plain"] = Rung("norm_plain", [plain])
    for how in ("x2p5", "unit", "varied"):
        R["norm_" + how] = Rung("norm_" + how, [_scaled(plain, how)])
    ws = []
    for i, (L, ex) in enumerate(zip((1, 64, 65, 130), EXTRINSICS)):
        hosts, ks = _mixed_tracks(rng, L, N, 5)
        entry = np.array([(1.5 + 0.01 * l, 0.0, -1.0)[l % 3] for l in range(1, L + 1)])
        ws.append(build_window(35 + i, hosts, ks, rng.uniform(1.0, 7.0, L), ric=EXTRINSICS[ex][0], tic=EXTRINSICS[ex][1], entry=entry))
    R["batch"] = Rung("batch", ws)
    hosts, ks = _mixed_tracks(rng, 40, 18, 8)
    R["n18"] = Rung("n18", [build_window(40, hosts, ks, rng.uniform(1.0, 7.0, 40), n_frames=18, n_vo=8)], shape=(18, 8))
    ws = []
    for i, (L, poses) in enumerate(((33, None), (10, _same_views), (33, None), (10, _pure_rotation))):
        hosts, ks = _mixed_tracks(rng, L, N, 5)
        ws.append(build_window(41 + i, hosts, ks, rng.uniform(1.0, 7.0, L), poses=poses))
    R["degenerate"] = Rung("degenerate", ws, degenerate=(1, 3))
    _RUNGS = R
    return R


# ---- the 40-digit side and the two float64 routes, once per rung ----------------------------------------------------------------------
class Truth:
    """per window of a rung: d* (mpf), sigma (floats [L][4]), todo (triangulated: depth <= 0 on entry), clamped (d* outside [0.1, 8]),
    excluded, and the float64 routes' depths"""


_TRUTH = {}


def truth(oracle, name):
    if name in _TRUTH:
        return _TRUTH[name]
    rung = rungs()[name]
    cfg = abi.make_config(*rung.shape, max_landmarks=max(w.L for w in rung.windows), max_obs=max(w.n_obs for w in rung.windows))
    out = []
    for wi, w in enumerate(rung.windows):
        t = Truth()
        t.todo = np.array(w.lm_depth[: w.L]) <= 0.0
        t.dstar, t.sigma = [None] * w.L, np.zeros((w.L, 4))
        t.clamped, t.excluded = np.zeros(w.L, bool), np.zeros(w.L, bool)
        t.np_svd = np.full(w.L, np.nan)
        for l in np.flatnonzero(t.todo):
            d, sig = ph.triangulate_mp(w, int(l))
            t.dstar[l], t.sigma[l] = d, [float(x) for x in sig]
            t.clamped[l] = d < mp.mpf(D_LO) or d > mp.mpf(D_HI)
            near_edge = min(abs(d / mp.mpf(D_LO) - 1), abs(d / mp.mpf(D_HI) - 1)) < EDGE_REL
            t.excluded[l] = (t.sigma[l, 2] - t.sigma[l, 3]) / t.sigma[l, 0] < GAP_MIN or bool(near_edge)
            t.np_svd[l] = ph.triangulate_f64(w, int(l))
        o = w.clone()
        assert oracle.isvo_triangulate(C.byref(cfg), C.byref(o.c())) == 0
        t.oracle = np.array(o.lm_depth[: w.L])
        t.degenerate = wi in rung.degenerate
        out.append(t)
    _TRUTH[name] = out
    return out


def errors(t, got):
    """e = |got / d* - 1| of the compared landmarks of one window (NaN elsewhere)"""
    e = np.full(len(got), np.nan)
    for l in np.flatnonzero(t.todo & ~t.clamped & ~t.excluded):
        e[l] = float(abs(mp.mpf(float(got[l])) / t.dstar[l] - 1))
    return e


def decisions_ok(w, t, got):
    """list of the landmarks that break the decision rule, the untouched-bits rule or (degenerate windows) the range rule"""
    bad = []
    for l in range(w.L):
        if not t.todo[l]:
            if got[l].tobytes() != np.float64(w.lm_depth[l]).tobytes():
                bad.append((l, "touched", float(got[l])))
        elif t.degenerate or t.excluded[l]:
            if not (got[l] == INIT_DEPTH or D_LO <= got[l] <= D_HI):
                bad.append((l, "range", float(got[l])))
        elif (got[l] == INIT_DEPTH) != bool(t.clamped[l]):
            bad.append((l, "decision", float(got[l]), float(t.dstar[l])))
    return bad


def ref_error(rung_truth):
    """(max e_oracle, max e_numpy) over a rung's compared landmarks"""
    eo = max(np.nanmax(errors(t, t.oracle), initial=0.0) for t in rung_truth if not t.degenerate)
    en = max(np.nanmax(errors(t, np.where(np.isnan(t.np_svd), 1.0, t.np_svd)), initial=0.0) for t in rung_truth if not t.degenerate)
    return float(eo), float(en)


def judge(oracle, name, results):
    """results: the depths [L] of every window of rung `name` after triangulation by the code under test.
    -> (decision faults, e_max, e_ref, worst sigma_1 / sigma_3 among the compared landmarks), printed"""
    rung, tr = rungs()[name], truth(oracle, name)
    bad, e_max, cond = [], 0.0, 0.0
    for w, t, got in zip(rung.windows, tr, results):
        got = np.asarray(got, float)
        bad += [(rung.windows.index(w),) + b for b in decisions_ok(w, t, got)]
        if t.degenerate:
            continue
        e = errors(t, got)
        ok = ~np.isnan(e) & (got != INIT_DEPTH)
        e_max = max(e_max, float(np.max(e[ok], initial=0.0)))
        cmp = t.todo & ~t.clamped & ~t.excluded
        if cmp.any():
            cond = max(cond, float((t.sigma[cmp, 0] / t.sigma[cmp, 2]).max()))
    e_ref = max(ref_error(tr))
    print(f"TRI {name:22s} sigma1/sigma3 {cond:9.2e}  e_ref {e_ref:.2e}  e {e_max:.2e}  ratio {e_max / e_ref if e_ref else float('inf'):8.2f}  faults {bad}")
    return bad, e_max, e_ref, cond


# ---- IMU weights ------------------------------------------------------------------------------------------------------------------------
IMU_CASES = {"s2": dict(samples=2), "s20": dict(samples=20), "s200": dict(samples=200), "s2000": dict(samples=2000),
             "dt2p5ms": dict(samples=20, dt=0.0025), "gyro_x10": dict(samples=20, gyro=10.0)}
# The two float64 routes against each other, as for TRI_MARGIN (numpy / LAPACK on the CPU): the larger error over the smaller, per case
# and per yardstick.  Each margin is twice the largest ratio, and at least 4.
#   case       cond(cov)   U^T U: route a, b (ratio)          U row-wise: route a, b (ratio)
#   s2         2.56e6      1.82e-16  1.82e-16  (1.00)         8.90e-16  1.10e-15  (1.24)
#   s20        2.57e6      1.84e-16  3.37e-16  (1.83)         6.85e-16  8.89e-16  (1.30)
#   s200       3.27e6      2.29e-16  1.83e-16  (1.25)         2.81e-14  7.45e-15  (3.77)
#   s2000      1.32e8      3.06e-16  2.67e-16  (1.14)         3.39e-15  5.07e-14  (14.95)
#   dt2p5ms    2.56e6      1.84e-16  1.84e-16  (1.00)         5.81e-16  9.13e-16  (1.57)
#   gyro_x10   2.57e6      1.84e-16  1.84e-16  (1.00)         5.84e-16  1.67e-15  (2.85)
IMU_ROUTE_RATIO_INFO_MEASURED, IMU_ROUTE_RATIO_FACTOR_MEASURED = 1.83, 14.95
IMU_MARGIN_INFO = max(4.0, 2 * IMU_ROUTE_RATIO_INFO_MEASURED)
IMU_MARGIN_FACTOR = max(4.0, 2 * IMU_ROUTE_RATIO_FACTOR_MEASURED)
_IMU = None


def _preintegrated(seed, samples, dt=0.005, gyro=1.0):
    """one pre-integration of `samples` IMU samples at `dt` along the synthetic trajectory, EuRoC noise; gyro: the factor on the rate and
    the gyro biases"""
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory(phase=2 * np.pi * rng.uniform())
    ba, bg = 0.02 * rng.normal(size=3), 0.002 * gyro * rng.normal(size=3)
    G = np.array([0, 0, synth.G_NORM])
    acc, gyr = np.zeros((1, samples + 1, 3)), np.zeros((1, samples + 1, 3))
    for s in range(samples + 1):
        t = 3.0 + s * dt
        acc[0, s] = traj.R(t).T @ (traj.acc(t) + G) + ba + synth.ACC_N * rng.normal(size=3)
        gyr[0, s] = gyro * traj.gyro(t) + bg + synth.GYR_N * rng.normal(size=3)
    lin_ba, lin_bg = ba + 0.005 * rng.normal(size=3), bg + 0.0005 * gyro * rng.normal(size=3)
    return synth.preintegrate(dt, acc, gyr, lin_ba[None], lin_bg[None]), lin_ba, lin_bg


def imu_window():
    """-> (an (11, 5) window whose first IMU records are IMU_CASES' pre-integrations, in that order; {case: record index}).  The states are
    not those the records were integrated along: the residuals are large, the weights do not depend on them."""
    global _IMU
    if _IMU is None:
        w = synth.make_window(50, n_landmarks=40)
        for i, (name, kw) in enumerate(IMU_CASES.items()):
            pre, ba, bg = _preintegrated(60 + i, **kw)
            im = w.imu[i]
            im.delta_p[:] = pre["delta_p"][0]; im.delta_v[:] = pre["delta_v"][0]
            q = pre["delta_q"][0]; im.delta_q[:] = [q[1], q[2], q[3], q[0]]
            im.linearized_ba[:] = ba; im.linearized_bg[:] = bg; im.sum_dt = pre["sum_dt"]
            im.jacobian[:] = pre["jacobian"][0].ravel(); im.covariance[:] = pre["covariance"][0].ravel()
        _IMU = (w, {name: i for i, name in enumerate(IMU_CASES)})
    return _IMU


class ImuTruth:
    """cov^-1 and its upper Cholesky factor at 40 digits (as doubles' nearest), and the errors of the two float64 routes"""

    def __init__(self, cov):
        self.cov = np.array(cov, float).reshape(15, 15)
        Inv, U = ph.information_mp(self.cov)
        self.Inv_mp, self.U_mp = Inv, U
        self.Inv, self.U = ph.to_np(Inv), ph.to_np(U)
        self.cond = float(np.linalg.cond(self.cov))
        routes = ph.information_f64(self.cov)
        self.e_info = [self.err_info(u) for _, u in routes]
        self.e_factor = [self.err_factor(u) for _, u in routes]

    def err_info(self, U):
        """U^T U against cov^-1: max-norm distance relative to the largest entry (tests/marg_cases.py's yardstick for information
        matrices).  The product is formed at 40 digits from the doubles of U, so the yardstick adds no rounding of its own."""
        with mp.workdps(40):
            Um = ph._m(np.asarray(U, float))
            D = Um.T * Um - self.Inv_mp
            return float(max(abs(D[a, b]) for a in range(15) for b in range(15)) / max(abs(self.Inv_mp[a, b]) for a in range(15) for b in range(15)))

    def err_factor(self, U):
        """U against the 40-digit factor, row-wise: max over rows of max|row difference| / max|row|"""
        U = np.asarray(U, float)
        with mp.workdps(40):
            worst = mp.mpf(0)
            for a in range(15):
                d = max(abs(mp.mpf(float(U[a, b])) - self.U_mp[a, b]) for b in range(15))
                worst = max(worst, d / max(abs(self.U_mp[a, b]) for b in range(15)))
            return float(worst)


_IMU_TRUTH = {}


def imu_truth(name):
    if name not in _IMU_TRUTH:
        w, idx = imu_window()
        _IMU_TRUTH[name] = ImuTruth(abi.arr(w.imu[idx[name]].covariance))
    return _IMU_TRUTH[name]


def judge_imu(name, U):
    """-> (structure faults, e_info, e_factor, their yardsticks max(route a, route b)) of a 15 x 15 sqrt_info `U`, printed"""
    t = imu_truth(name)
    U = np.asarray(U, float).reshape(15, 15)
    faults = []
    if np.tril(U, -1).any():
        faults.append("nonzero below the diagonal")
    if not (np.diag(U) > 0).all():
        faults.append("diagonal not positive")
    ei, ef = t.err_info(U), t.err_factor(U)
    print(f"IMU {name:9s} cond {t.cond:.2e}  info: e {ei:.2e} routes {t.e_info[0]:.2e} {t.e_info[1]:.2e}   factor: e {ef:.2e} routes {t.e_factor[0]:.2e} {t.e_factor[1]:.2e}")
    return faults, ei, ef, max(t.e_info), max(t.e_factor)


# ---- vector2double ----------------------------------------------------------------------------------------------------------------------
# name: (what frame PIVOT's rotation becomes, exactly or nearly; the arm and tie it must reach)
T_XY, T_YZ = half_turn([1.0, 1.0, 0.0]), half_turn([0.0, 1.0, 1.0])
QUAT_CASES = {"near_pi_x": (rot([1.0, 0.02, -0.03], np.pi - 0.04), False), "near_pi_y": (rot([0.03, 1.0, 0.02], np.pi - 0.05), False),
              "near_pi_z": (rot([-0.02, 0.03, 1.0], np.pi - 0.03), False), "tie_xy": (T_XY, True), "tie_yz": (T_YZ, True)}
PIVOT = 5
RIC_X_ARM = rot([1.0, 0.05, -0.02], np.pi - 0.1)
_QUAT = {}


def quat_window(name):
    """an (11, 5) synthetic window turned as a whole, Ps' = Q Ps, Rs' = Q Rs, with Q chosen so that frame PIVOT's rotation is the case's
    target (the observations stay: relative geometry does not change); on the two tie cases frame PIVOT's rotation is then SET to the
    exact half turn, a change of the last bit.  "ric_x_arm": an unturned window whose camera-IMU rotation lies in the x arm, its
    observations rebuilt for that extrinsic."""
    if name in _QUAT:
        return _QUAT[name]
    if name == "ric_x_arm":
        rng = np.random.default_rng(9)
        hosts, ks = _mixed_tracks(rng, 40, 11, 5)
        depths = rng.uniform(1.0, 7.0, 40)
        w = build_window(52, hosts, ks, depths, noise=True, ric=RIC_X_ARM, entry=depths * rng.uniform(0.9, 1.1, 40))
    else:
        target, exact = QUAT_CASES[name]
        w = synth.make_window(51, n_landmarks=40)
        Q = target @ w.Rs[PIVOT].T
        w.Ps[...] = w.Ps @ Q.T
        w.Rs[...] = np.einsum("ab,nbc->nac", Q, w.Rs)
        if exact:
            w.Rs[PIVOT] = target
    _QUAT[name] = w
    return w
