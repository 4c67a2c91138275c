"""The bundle adjustment of the initialisation's SfM stage (is-vins_amd/csrc/isv_sfm.h, stage 2) and the serial pieces of OpenCV's
iterative PnP (csrc/isv_pnp.h) recomputed at 40 digits in mpmath, on small scenes whose SHAPE is chosen so that k_sfm's strided
loops (csrc/isv_sfm.hip: 64 lanes over nact points, nitems = nw (nw + 1) / 2 * 6 reduced-system items, nc = 6 nw - 9 reduced
columns) take each of their loop-count edges.  Test infrastructure: tests/test_sfm_highprec.py pins this file to the CPU
restatements (tests/native/isv_sfm_oracle.c, isv_loop_oracle.c), tests/test_gpu_sfm_highprec.py compares the kernel with it.

Written from the definitions isv_sfm.h cites, not from the kernel's text:
  residual   ReprojectionError3D: p = QuaternionRotatePoint(q, X) + t (the rotation of q / |q|), r = p.xy / p.z - uv;
  blocks     a quaternion per window frame under QuaternionParameterization (Plus(q, d) = [cos |d|, sin |d| / |d| d] * q), frame l
             constant; a translation per frame, frames l and n_window - 1 constant; a 3-vector per triangulated track;
  Jacobians  chain rule in mpmath: d r / d p, d p / d u (u = q / |q|), d u / d q, and d Plus / d d at d = 0 -- Plus ITSELF is
             differentiated (its 4 x 3 Jacobian), -2 [R X]x is not assumed (check_plus_jacobian compares with central differences
             through Plus);
  iteration  Ceres 2.0.0 TrustRegionMinimizer + LevenbergMarquardtStrategy, default options: Jacobi scaling 1 / (1 + sqrt(column
             norm^2)) taken once at x0, LM diagonal diag(Js^T Js) clamped to [1e-6, 1e32] over the radius (1e4 at first), the step
             from the regularised normal equations, the model cost change, the parameter / function tolerance tests, the step
             accepted when relative_decrease > 1e-3, radius / max(1/3, 1 - (2 rho - 1)^3) capped at 1e16 on accept, the halving with
             a doubling decrease_factor on reject.  The reference takes every decision itself.
  solve      the smallest case densely (mpmath Cholesky of the whole (nc + 3 nact)^2 system); the others by eliminating the
             points first (exact); `routes_agree` asserts on the smallest case that the two agree to 1e-30;
  record     Q = q.inverse() (conjugate / squared norm), T = -(Q * t) by Eigen's _transformVector formula (isv_sfm.h S6),
             both ways, in mpmath on the float64 outputs.
Beside every quantity the same quantity by a float64 route -- the Jacobians rounded to float64, J.T @ J by numpy, the solve by
LAPACK, costs and Plus by the same code at 53 bits: its error against the 40-digit one is the yardstick e64 of the tests.

One iteration is checked at a time: iteration k linearises at the state the code under test stored after k - 1 iterations (its
cap-(k-1) output, read back through the record), with the Jacobi scaling of the cap-0 state and the radius of the reference's own
decisions, and predicts the cap-k output.
"""
import ctypes as C
import functools

import mpmath as mp
import numpy as np

from isvins_amd import initial, synth

mp.mp.dps = 40
mpf = mp.mpf
ZERO, ONE, TWO = mpf(0), mpf(1), mpf(2)
PIXEL = 0.5 / 460
U = 2.0 ** -53


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# name -> (n_window, l, triangulated tracks, seed, relative-pose error [rad]).  What each reaches: see DESIGN.md (SfM section).
CASES = {
    "w3_l0":       (3, 0, 20, 1, 0.0),       # smallest legal shape: nc = 9, nitems = 36 < 64; l = 0; the dense route
    "w4_l2":       (4, 2, 24, 2, 0.0),       # nc = 15; l = n_window - 2
    "w5_n63":      (5, 2, 63, 3, 0.0),       # nitems = 90 > 64; nact one short of the wavefront
    "w5_n64":      (5, 2, 64, 4, 0.0),       # nact = the wavefront
    "w5_n65":      (5, 2, 65, 5, 0.0),       # one lane takes a second point
    "w5_n131":     (5, 3, 131, 6, 0.0),      # three passes of the point loops; l = n_window - 2
    "w11_l5":      (11, 5, 40, 7, 0.0),      # the product's default window: nc = 57
    "w13_l6":      (13, 6, 30, 8, 0.0),      # first nc > 64 (69): the Cholesky's row loop and the column loops wrap
    "w20_l10":     (20, 10, 30, 9, 0.0),     # the cap: nc = 111, nitems = 1260
    # the first step is REJECTED (iteration 2 solves the old linearisation again at half the radius): found by a seed search on the
    # restatement at cap 1 (ba_successful == 0, and == 1 at cap 2) over relative poses turned by 0.026 .. 0.038 rad, 16 tracks, 120
    # seeds per shape; cost at x0 2.2e-3 < 5e-3
    "w13_reject":  (13, 6, 16, 164, 0.026),
    # one point 30 baselines away on camera l's axis, seen from frames l and l + 1: its depth column's norm is ~1e-4, the scaled LM
    # diagonal of that column sits on the 1e-6 clamp, which is the only place where the Jacobi scaling does not cancel from the step
    "w5_far":      (5, 2, 40, 11, 0.0, "far"),
}
NAMES = list(CASES)
SMALLEST = "w3_l0"


def _spans(nw, l, n, rng):
    """frame spans [(start, n_obs)] of n tracks with >= 2 observations: twelve over the whole window first (every solveFrameByPnP
    then has its 10 points), then in turn a two-frame track, one that misses frame l, one that misses the last frame, a seeded
    span and a whole-window one"""
    out = [(0, nw)] * 12
    k = 0
    while len(out) < n:
        kind, k = k % 5, k + 1
        if kind == 0:
            s = int(rng.uniform(1)[0] * (nw - 1)); out.append((s, 2))
        elif kind == 1:
            out.append((0, l) if l >= 2 else (l + 1, nw - l - 1))
        elif kind == 2:
            out.append((0, nw - 1))
        elif kind == 3:
            s = int(rng.uniform(1)[0] * (nw - 1)); L = 2 + int(rng.uniform(1)[0] * (nw - s - 1)); out.append((s, min(L, nw - s)))
        else:
            out.append((0, nw))
    return out[:n]


@functools.lru_cache(maxsize=None)
def _case_data(spec):
    nw, l, n, seed, rel_err = spec[:5]
    far = len(spec) > 5
    base, _ = initial.make_scene(seed=seed, n_window=nw, l=l, per_frame=12, rel_rot_err=rel_err, rel_dir_err=rel_err)
    Q, T = base.truth["Q"], base.truth["T"]                        # camera i to camera l, unit baseline
    rng = synth.SplitMix64(0x5F3E00000000 + seed)
    spans = _spans(nw, l, n, rng)
    assert all(L >= 2 and s >= 0 and s + L <= nw for s, L in spans), spans
    if far:
        spans[-1] = (l, 2)
    mid = n // 2
    spans.insert(mid, (min(1, nw - 1), 1))                          # one observation: never triangulated, act[] is not the identity
    tracks, obs = [], []
    for j, (s, L) in enumerate(spans):
        while True:
            u = rng.uniform(3)
            d = 4.0 + 8.0 * u[0]
            X = Q[s] @ (np.array([(u[1] - 0.5) * 0.8, (u[2] - 0.5) * 0.8, 1.0]) * d) + T[s]
            if far and j == len(spans) - 1:
                X = Q[s] @ np.array([0.01, -0.02, 30.0]) + T[s]
            xc = [Q[i].T @ (X - T[i]) for i in range(s, s + L)]
            if all(p[2] > 1.0 and abs(p[0] / p[2]) < 1.0 and abs(p[1] / p[2]) < 1.0 for p in xc):
                break
        nz = rng.normal(2 * L).reshape(L, 2)
        tracks.append((7 + 3 * j, s, L))
        obs.extend([p[:2] / p[2] + PIXEL * nz[i] for i, p in enumerate(xc)])
    frame_pts = [[] for _ in range(nw)]
    off = 0
    for tid, s, L in tracks:
        for i in range(L):
            frame_pts[s + i].append((tid, obs[off + i][0], obs[off + i][1]))
        off += L
    nf = base.c.n_frames
    assert nf == nw
    # stage 0 is not under test here: pre-integrations that pass checkIMUExcitation at any window length (spread 1 > 0.25)
    sdt = np.full(nf, 0.1)
    dv = np.array([[0.1 * (-1.0) ** f, 0.03 * (f % 3), 0.98] for f in range(nf)])
    args = (nw, l, np.array(base.c.relative_R), np.array(base.c.relative_T), np.array(base.c.RIC), tracks, np.array(obs), frame_pts,
            dv, sdt, list(base.c.window_frame[:nw]))
    return args, n, mid


def make_case(name):
    """-> (a fresh SfmProblem, expected n_triangulated, index of the never-triangulated track)"""
    args, n, mid = _case_data(CASES[name] if isinstance(name, str) else tuple(name))
    return initial.SfmProblem(*args), n, mid


def shape_facts(sp):
    """what the case list is chosen for, from the problem alone"""
    nw, l = sp.c.n_window, sp.c.l
    tr = [sp.tracks[j] for j in range(sp.c.n_tracks)]
    inside = lambda t, f: t.start_frame <= f < t.start_frame + t.n_obs   # noqa: E731
    return dict(nc=6 * nw - 9, nitems=nw * (nw + 1) // 2 * 6, lengths={t.n_obs for t in tr},
                miss_l=sum(t.n_obs >= 2 and not inside(t, l) for t in tr), miss_last=sum(t.n_obs >= 2 and not inside(t, nw - 1) for t in tr))


# ---- quaternions (w x y z), the record <-> the BA's state ----------------------------------------------------------------------------
def q_mul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def q_inverse(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def transform_vector(q, v):
    """Eigen's QuaternionBase::_transformVector: v + w uv + q.vec x uv, uv = 2 q.vec x v (a rotation only when |q| = 1)"""
    uv = [2 * c for c in _cross(q[1:], v)]
    c = _cross(q[1:], uv)
    return [v[k] + q[0] * uv[k] + c[k] for k in range(3)]


def plus(q, d):
    """QuaternionParameterization::Plus"""
    n = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if n == 0:
        return list(q)
    s = mp.sin(n) / n
    return q_mul([mp.cos(n), s * d[0], s * d[1], s * d[2]], q)


def state_to_record(cq, ct):
    """the BA's c_rotation / c_translation -> the record's Q (x y z w) / T"""
    Q, T = [], []
    for q, t in zip(cq, ct):
        qi = q_inverse(q)
        Q.append([qi[1], qi[2], qi[3], qi[0]])
        T.append([-c for c in transform_vector(qi, t)])
    return Q, T


def record_to_state(Q, T, nw):
    """the record's float64 Q / T -> c_rotation / c_translation at 40 digits: q = Q.inverse(), and t from T = -M(Q) t, M the
    (linear) map of _transformVector"""
    cq, ct = [], []
    for f in range(nw):
        qo = [mpf(float(Q[f][3])), mpf(float(Q[f][0])), mpf(float(Q[f][1])), mpf(float(Q[f][2]))]
        cq.append(q_inverse(qo))
        cols = [transform_vector(qo, [ONE if k == c else ZERO for k in range(3)]) for c in range(3)]
        M = mp.matrix(3, 3)
        for c in range(3):
            for r in range(3):
                M[r, c] = cols[c][r]
        t = mp.lu_solve(M, mp.matrix([-mpf(float(T[f][k])) for k in range(3)]))
        ct.append([t[0], t[1], t[2]])
    return cq, ct


class State:
    """cq [nw][4] (w x y z), ct [nw][3], X {track: [3]}"""

    def __init__(self, cq, ct, X):
        self.cq, self.ct, self.X = cq, ct, X

    @staticmethod
    def from_output(res, position, state, nw):
        cq, ct = record_to_state(res.Q, res.T, nw)
        X = {j: [mpf(float(position[j][k])) for k in range(3)] for j in range(len(state)) if state[j]}
        return State(cq, ct, X)

    def record(self):
        Q, T = state_to_record(self.cq, self.ct)
        return Q, T


# ---- the problem ------------------------------------------------------------------------------------------------------------------
def _rot_point(u, X):
    """R(u) X for a unit quaternion: X + 2 w (v x X) + 2 v x (v x X)"""
    c1 = _cross(u[1:], X)
    c2 = _cross(u[1:], c1)
    return [X[k] + 2 * u[0] * c1[k] + 2 * c2[k] for k in range(3)]


def residual(q, t, X, uv):
    n = mp.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    u = [c / n for c in q]
    p = [a + b for a, b in zip(_rot_point(u, X), t)]
    return [p[0] / p[2] - uv[0], p[1] / p[2] - uv[1]]


def plus_jacobian(q):
    """d Plus(q, d) / d d at d = 0 (4 x 3): cos |d| -> 1 and sin |d| / |d| -> 1 to first order, so it is d ([1, d] * q) / d d"""
    w, x, y, z = q
    return [[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]]


def obs_jacobians(q, t, X, uv, half_qjac=False):
    """-> r [2], Jq [2][3] (the quaternion's tangent), Jt [2][3], JX [2][3], unscaled"""
    n = mp.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    u = [c / n for c in q]
    w, v = u[0], u[1:]
    RX = _rot_point(u, X)
    p = [a + b for a, b in zip(RX, t)]
    r = [p[0] / p[2] - uv[0], p[1] / p[2] - uv[1]]
    iz = 1 / p[2]
    Jp = [[iz, ZERO, -p[0] * iz * iz], [ZERO, iz, -p[1] * iz * iz]]
    # d (R(u) X) / d u: column 0 = 2 v x X; columns 1..3 = -2 w [X]x + 2 ((v . X) I + v X^T - 2 X v^T)
    vX = v[0] * X[0] + v[1] * X[1] + v[2] * X[2]
    c0 = _cross(v, X)
    Xx = [[ZERO, -X[2], X[1]], [X[2], ZERO, -X[0]], [-X[1], X[0], ZERO]]
    dpdu = [[2 * c0[a]] + [-2 * w * Xx[a][b] + 2 * ((vX if a == b else ZERO) + v[a] * X[b] - 2 * X[a] * v[b]) for b in range(3)] for a in range(3)]
    dudq = [[((ONE if a == b else ZERO) - u[a] * u[b]) / n for b in range(4)] for a in range(4)]
    P = plus_jacobian(q)
    dudd = [[sum(dudq[a][k] * P[k][c] for k in range(4)) for c in range(3)] for a in range(4)]
    dpdd = [[sum(dpdu[a][k] * dudd[k][c] for k in range(4)) for c in range(3)] for a in range(3)]
    Jq = [[sum(Jp[a][k] * dpdd[k][c] for k in range(3)) for c in range(3)] for a in range(2)]
    if half_qjac:
        Jq = [[e / 2 for e in row] for row in Jq]
    # d (R(u) X) / d X = R(u): its columns are the rotated unit vectors
    Rc = [_rot_point(u, [ONE if k == c else ZERO for k in range(3)]) for c in range(3)]
    JX = [[sum(Jp[a][k] * Rc[c][k] for k in range(3)) for c in range(3)] for a in range(2)]
    return r, Jq, Jp, JX


def check_plus_jacobian(q, t, X, uv, h=mpf("1e-14")):
    """max |Jq - central differences of r(Plus(q, d))| (truncation ~ h^2, rounding ~ 1e-40 / h)"""
    _, Jq, _, _ = obs_jacobians(q, t, X, uv)
    worst = ZERO
    for c in range(3):
        d = [h if k == c else ZERO for k in range(3)]
        rp, rm = residual(plus(q, d), t, X, uv), residual(plus(q, [-e for e in d]), t, X, uv)
        for a in range(2):
            worst = max(worst, abs((rp[a] - rm[a]) / (2 * h) - Jq[a][c]))
    return worst


def _obj(rows):
    a = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, r in enumerate(rows):
        for j, e in enumerate(r):
            a[i, j] = e
    return a


def _chol_solve(A, b):
    """A x = b for a symmetric positive definite object array, by Cholesky"""
    n = len(b)
    L = np.empty((n, n), dtype=object)
    L[:] = ZERO
    for j in range(n):
        s = A[j, j] - (np.dot(L[j, :j], L[j, :j]) if j else ZERO)
        assert s > 0
        L[j, j] = mp.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (np.dot(L[i, :j], L[j, :j]) if j else ZERO)) / L[j, j]
    y = np.empty(n, dtype=object)
    for i in range(n):
        y[i] = (b[i] - (np.dot(L[i, :i], y[:i]) if i else ZERO)) / L[i, i]
    x = np.empty(n, dtype=object)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (np.dot(L[i + 1:, i], x[i + 1:]) if i < n - 1 else ZERO)) / L[i, i]
    return x


def _inv3(A):
    M = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            M[i, j] = A[i, j]
    W = M ** -1
    return _obj([[W[i, j] for j in range(3)] for i in range(3)])


class Control:
    """the trust region's scalars between iterations"""

    def __init__(self):
        self.radius, self.decrease_factor = mpf("1e4"), TWO


class Reference:
    """the BA of one problem: the structure from the problem, the active tracks from its `state` output"""

    def __init__(self, sp, state):
        c = sp.c
        self.nw, self.l = c.n_window, c.l
        self.act = [j for j in range(c.n_tracks) if state[j]]
        self.aidx = {j: a for a, j in enumerate(self.act)}
        self.ncf = [0 if f == self.l else 3 if f == self.nw - 1 else 6 for f in range(self.nw)]
        self.coff = list(np.cumsum([0] + self.ncf[:-1]))
        self.nc = sum(self.ncf)
        self.n = self.nc + 3 * len(self.act)
        self.obs = []                                               # (active index, track, frame, uv) in track order
        for a, j in enumerate(self.act):
            t = sp.tracks[j]
            for k in range(t.n_obs):
                uv = sp.obs[t.obs_off + k]
                self.obs.append((a, j, t.start_frame + k, [mpf(float(uv[0])), mpf(float(uv[1]))]))
        self.nres = 2 * len(self.obs)
        # corruptions of the REFERENCE (negative controls)
        self.half_qjac = False
        self.no_point_lm = False
        self.drop_offdiag = None                                    # (track, fa, fb): that observation pair left out of S[fa][fb]
        self.rescale = False

    # -- costs
    def residuals(self, x):
        return [residual(x.cq[f], x.ct[f], x.X[j], uv) for _, j, f, uv in self.obs]

    def cost(self, x):
        return sum((r[0] * r[0] + r[1] * r[1] for r in self.residuals(x)), ZERO) / 2

    def cost64(self, x):
        with mp.workprec(53):
            return self.cost(x)

    # -- the linearisation: per observation (a, f, r, E 2x3, F 2xncf), unscaled
    def blocks(self, x):
        out = []
        for a, j, f, uv in self.obs:
            r, Jq, Jt, JX = obs_jacobians(x.cq[f], x.ct[f], x.X[j], uv, self.half_qjac)
            F = [(Jq[row] + Jt[row])[:self.ncf[f]] for row in range(2)]
            out.append((a, f, np.array(r, dtype=object), _obj(JX), _obj(F) if self.ncf[f] else None))
        return out

    def scale(self, blocks):
        """Jacobi scaling (camera columns [nc], point columns [nact][3]) from the unscaled column norms"""
        cn = np.array([ZERO] * self.nc, dtype=object)
        pn = np.array([[ZERO] * 3 for _ in self.act], dtype=object)
        for a, f, r, E, F in blocks:
            pn[a] += (E * E).sum(axis=0)
            if F is not None:
                cn[self.coff[f]:self.coff[f] + self.ncf[f]] += (F * F).sum(axis=0)
        one = np.vectorize(lambda v: 1 / (1 + mp.sqrt(v)), otypes=[object])
        return one(cn), one(pn)

    def _scaled(self, blocks, sc):
        csc, psc = sc
        return [(a, f, r, E * psc[a][None, :], None if F is None else F * csc[self.coff[f]:self.coff[f] + self.ncf[f]][None, :]) for a, f, r, E, F in blocks]

    def _lm_diag(self, sb, radius):
        cd = np.array([ZERO] * self.nc, dtype=object)
        pd = np.array([[ZERO] * 3 for _ in self.act], dtype=object)
        for a, f, r, E, F in sb:
            pd[a] += (E * E).sum(axis=0)
            if F is not None:
                cd[self.coff[f]:self.coff[f] + self.ncf[f]] += (F * F).sum(axis=0)
        self.n_clamped = sum(v < mpf("1e-6") for v in cd) + sum(v < mpf("1e-6") for row in pd for v in row)
        clamp = np.vectorize(lambda v: min(max(v, mpf("1e-6")), mpf("1e32")) / radius, otypes=[object])
        cd, pd = clamp(cd), clamp(pd)
        if self.no_point_lm:
            pd[:] = ZERO
        return cd, pd

    def solve_schur(self, sb, cd, pd):
        na = len(self.act)
        Hpp = [np.diag(pd[a]).astype(object) for a in range(na)]
        for a in range(na):
            Hpp[a][Hpp[a] == 0] = ZERO
        gp = [np.array([ZERO] * 3, dtype=object) for _ in range(na)]
        S = np.empty((self.nc, self.nc), dtype=object); S[:] = ZERO
        gc = np.array([ZERO] * self.nc, dtype=object)
        per = [[] for _ in range(na)]                               # per point: (f, F^T E)
        for a, f, r, E, F in sb:
            Hpp[a] = Hpp[a] + E.T @ E
            gp[a] = gp[a] + E.T @ r
            if F is not None:
                o, m = self.coff[f], self.ncf[f]
                S[o:o + m, o:o + m] += F.T @ F
                gc[o:o + m] += F.T @ r
                per[a].append((f, F.T @ E))
        for k in range(self.nc):
            S[k, k] += cd[k]
        W = [_inv3(H) for H in Hpp]
        for a in range(na):                                         # S -= B W B^T, B the point's stacked F^T E blocks
            if not per[a]:
                continue
            idx = np.concatenate([np.arange(self.coff[f], self.coff[f] + self.ncf[f]) for f, _ in per[a]])
            B = np.vstack([Bf for _, Bf in per[a]])
            BW = B @ W[a]
            gc[idx] -= BW @ gp[a]
            S[np.ix_(idx, idx)] -= BW @ B.T
            if self.drop_offdiag is not None and self.act[a] == self.drop_offdiag[0]:
                (fa, Ba), (fb, Bb) = [(f, Bf) for f, Bf in per[a] if f in self.drop_offdiag[1:]]
                blk = Ba @ W[a] @ Bb.T                              # put the dropped pair's contribution back: it was never there
                S[self.coff[fa]:self.coff[fa] + self.ncf[fa], self.coff[fb]:self.coff[fb] + self.ncf[fb]] += blk
                S[self.coff[fb]:self.coff[fb] + self.ncf[fb], self.coff[fa]:self.coff[fa] + self.ncf[fa]] += blk.T
        y = _chol_solve(S, gc)                                      # H dx = -g: dx_c = -y
        dp = []
        for a in range(na):
            v = gp[a].copy()
            for f, Bf in per[a]:
                v = v - Bf.T @ y[self.coff[f]:self.coff[f] + self.ncf[f]]
            dp.append(-(W[a] @ v))
        return -y, np.array(dp, dtype=object)

    def _dense(self, sb, dtype):
        J = np.zeros((self.nres, self.n), dtype=dtype)
        if dtype is object:
            J[:] = ZERO
        r = np.zeros(self.nres, dtype=dtype)
        cv = (lambda v: v) if dtype is object else float
        for i, (a, f, rr, E, F) in enumerate(sb):
            for row in range(2):
                r[2 * i + row] = cv(rr[row])
                for c in range(3):
                    J[2 * i + row, self.nc + 3 * a + c] = cv(E[row, c])
                if F is not None:
                    for c in range(self.ncf[f]):
                        J[2 * i + row, self.coff[f] + c] = cv(F[row, c])
        return J, r

    def solve_dense(self, sb, cd, pd):
        J, r = self._dense(sb, object)
        H = J.T @ J
        D = list(cd) + [e for row in pd for e in row]
        for k in range(self.n):
            H[k, k] += D[k]
        dx = _chol_solve(H, -(J.T @ r))
        return dx[:self.nc], dx[self.nc:].reshape(-1, 3)

    def apply(self, x, dc, dp):
        """x (+) delta"""
        cq, ct = [], []
        for f in range(self.nw):
            o = self.coff[f]
            cq.append(plus(x.cq[f], list(dc[o:o + 3])) if self.ncf[f] >= 3 else list(x.cq[f]))
            ct.append([x.ct[f][k] + dc[o + 3 + k] for k in range(3)] if self.ncf[f] == 6 else list(x.ct[f]))
        X = {j: [x.X[j][k] + dp[a][k] for k in range(3)] for a, j in enumerate(self.act)}
        return State(cq, ct, X)

    def norm2(self, x, y=None):
        """the squared 2-norm of the free ambient state (or of x - y)"""
        s = ZERO
        for j in self.act:
            s += sum((x.X[j][k] - (y.X[j][k] if y else 0)) ** 2 for k in range(3))
        for f in range(self.nw):
            if self.ncf[f] >= 3:
                s += sum((x.cq[f][k] - (y.cq[f][k] if y else 0)) ** 2 for k in range(4))
            if self.ncf[f] == 6:
                s += sum((x.ct[f][k] - (y.ct[f][k] if y else 0)) ** 2 for k in range(3))
        return s

    def iteration(self, x, sc, ctl, route="schur"):
        """one iteration at x with the Jacobi scaling sc and the control state ctl (updated): dict(x1 = the state after it, accepted,
        rho, model, cost, cand_cost, term (None, 'parameter' or 'function'), and the same by the float64 route: x1_64, rho64, model64,
        cost64, cand64)"""
        blocks = self.blocks(x)
        if self.rescale:
            sc = self.scale(blocks)
        sb = self._scaled(blocks, sc)
        cd, pd = self._lm_diag(sb, ctl.radius)
        dc, dp = (self.solve_schur if route == "schur" else self.solve_dense)(sb, cd, pd)
        mcc = ZERO
        for a, f, r, E, F in sb:
            m = E @ dp[a]
            if F is not None:
                m = m + F @ dc[self.coff[f]:self.coff[f] + self.ncf[f]]
            mcc -= m[0] * (r[0] + m[0] / 2) + m[1] * (r[1] + m[1] / 2)
        cand = self.apply(x, dc * sc[0], dp * sc[1])
        cost, cc = self.cost(x), self.cost(cand)
        out = dict(step_c=dc * sc[0], step_p=dp * sc[1], model=mcc, cost=cost, cand_cost=cc, cand=cand, term=None)
        # the float64 route
        J, r = self._dense(sb, np.float64)
        D = np.array([float(e) for e in cd] + [float(e) for row in pd for e in row])
        dx = np.linalg.solve(J.T @ J + np.diag(D), -(J.T @ r))
        m = J @ dx
        s64 = np.array([float(e) for e in sc[0]] + [float(e) for row in sc[1] for e in row])
        de = dx * s64
        with mp.workprec(53):
            cand64 = self.apply(x, [mpf(v) for v in de[:self.nc]], [[mpf(v) for v in row] for row in de[self.nc:].reshape(-1, 3)])
            c64, cc64 = self.cost(x), self.cost(cand64)
        out.update(model64=float(-(m @ (r + m / 2))), cost64=float(c64), cand64=float(cc64), cand_64=cand64)
        out["rho64"] = (out["cost64"] - out["cand64"]) / out["model64"]
        # the decisions
        assert mcc > 0
        out["rho"] = rho = (cost - cc) / mcc
        out["accepted"] = False
        if mp.sqrt(self.norm2(x, cand)) <= mpf("1e-8") * (mp.sqrt(self.norm2(x)) + mpf("1e-8")):
            out["term"] = "parameter"
        elif abs(cost - cc) <= mpf("1e-6") * cost:
            out["term"] = "function"
        elif rho > mpf("1e-3"):
            out["accepted"] = True
            ctl.radius = min(mpf("1e16"), ctl.radius / max(ONE / 3, 1 - (2 * rho - 1) ** 3))
            ctl.decrease_factor = TWO
        else:
            ctl.radius = ctl.radius / ctl.decrease_factor
            ctl.decrease_factor *= 2
        out["x1"] = cand if out["accepted"] else x
        out["x1_64"] = cand64 if out["accepted"] else x
        return out


def routes_agree(ref, x):
    """max |dense - point-eliminated| over the step of one iteration at x (radius 1e4), both in mpmath"""
    blocks = ref.blocks(x)
    sb = ref._scaled(blocks, ref.scale(blocks))
    cd, pd = ref._lm_diag(sb, mpf("1e4"))
    a, b = ref.solve_schur(sb, cd, pd), ref.solve_dense(sb, cd, pd)
    return max(max(abs(e) for e in (a[0] - b[0])), max(abs(e) for e in (a[1] - b[1]).ravel()))


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def _f(v):
    return float(v)


def flat_points(ref, x):
    return np.array([[_f(e) for e in x.X[j]] for j in ref.act])


def flat_record(x):
    Q, T = x.record()
    return np.array([[_f(e) for e in q] for q in Q]), np.array([[_f(e) for e in t] for t in T])


def step_errors(ref, x0, it, res, position):
    """the stored state after an accepted iteration `it` (from x0) against the reference's x1, in max-norm over the 2-norm of the
    reference's step: -> {"position": (err, e64, floor), "QT": (err, e64, floor)}.  The differences are taken at 40 digits.
    floor = 2^-53 max(n, |x0|_inf / |step|_2): the step is read back through stored states.  For Q / T the state went through S6's
    inversion once on the device (x1 -> record) and once in the reference (record -> x0): each is a handful of rounded operations on
    entries of size |x0|_inf, which the same floor with the test's margin covers (the measured Q / T ratios sit below the positions')."""
    nw = ref.nw
    out = {}
    # positions
    d = [it["x1"].X[j][k] - x0.X[j][k] for j in ref.act for k in range(3)]
    sn = mp.sqrt(sum((e * e for e in d), ZERO))
    e = max(abs(mpf(float(position[j][k])) - it["x1"].X[j][k]) for j in ref.act for k in range(3)) / sn
    e64 = max(abs(it["x1_64"].X[j][k] - it["x1"].X[j][k]) for j in ref.act for k in range(3)) / sn
    x0inf = max(abs(x0.X[j][k]) for j in ref.act for k in range(3))
    out["position"] = (_f(e), _f(e64), U * max(ref.n, _f(x0inf / sn)))
    # Q / T
    Q1, T1 = it["x1"].record()
    Q0, T0 = x0.record()
    with mp.workprec(53):
        Q64, T64 = it["x1_64"].record()
    ref1 = [e for q in Q1 for e in q] + [e for t in T1 for e in t]
    ref0 = [e for q in Q0 for e in q] + [e for t in T0 for e in t]
    r64 = [e for q in Q64 for e in q] + [e for t in T64 for e in t]
    got = [mpf(float(res.Q[f][k])) for f in range(nw) for k in range(4)] + [mpf(float(res.T[f][k])) for f in range(nw) for k in range(3)]
    sn = mp.sqrt(sum(((a - b) ** 2 for a, b in zip(ref1, ref0)), ZERO))
    e = max(abs(a - b) for a, b in zip(got, ref1)) / sn
    e64 = max(abs(a - b) for a, b in zip(r64, ref1)) / sn
    out["QT"] = (_f(e), _f(e64), U * max(ref.n, _f(max(abs(v) for v in ref0) / sn)))
    return out


def cost_errors(ref, value, c, c64):
    """a cost of the code under test against the reference's c (relative): (err, e64, floor = number of residuals x 2^-53)"""
    return _f(abs(mpf(float(value)) - c) / c), _f(abs(mpf(c64) - c) / c), ref.nres * U


# ---- OpenCV's serial pieces -----------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """exp([r]x) at 40 digits: R [3][3]"""
    th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    th = mp.sqrt(th2)
    if th < mpf("1e-12"):                                           # Taylor: the next terms are below 1e-48
        A, B = 1 - th2 / 6 + th2 * th2 / 120, ONE / 2 - th2 / 24 + th2 * th2 / 720
    else:
        A, B = mp.sin(th) / th, (1 - mp.cos(th)) / th2
    K = [[ZERO, -r[2], r[1]], [r[2], ZERO, -r[0]], [-r[1], r[0], ZERO]]
    K2 = [[sum(K[i][k] * K[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return [[(ONE if i == j else ZERO) + A * K[i][j] + B * K2[i][j] for j in range(3)] for i in range(3)]


def rodrigues_jacobian(r, h=mpf("1e-13")):
    """d R / d r_i as 3 x 9 (row i: the row-major R differentiated by r_i), by central differences of the exponential itself at 40
    digits (truncation ~ h^2 = 1e-26, rounding ~ 1e-40 / h)"""
    J = []
    for i in range(3):
        rp = [r[k] + (h if k == i else 0) for k in range(3)]
        rm = [r[k] - (h if k == i else 0) for k in range(3)]
        Rp, Rm = rodrigues(rp), rodrigues(rm)
        J.append([(Rp[a][b] - Rm[a][b]) / (2 * h) for a in range(3) for b in range(3)])
    return J


def rodrigues_jacobian_f64(rv):
    """OpenCV's formula (cvRodrigues2, vector to matrix) in numpy float64: the yardstick of the Jacobian test"""
    rv = np.asarray(rv, dtype=np.float64)
    theta = np.sqrt(rv @ rv)
    J = np.zeros((3, 9))
    if theta < np.finfo(np.float64).eps:
        J[0, 5] = J[1, 6] = J[2, 1] = -1.0
        J[0, 7] = J[1, 2] = J[2, 3] = 1.0
        return np.eye(3), J
    c, s = np.cos(theta), np.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    r = rv * it
    rrt = np.outer(r, r)
    rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    R = c * np.eye(3) + c1 * rrt + s * rx
    for i in range(3):
        e = np.zeros(3); e[i] = 1.0
        drrt = np.outer(e, r) + np.outer(r, e)
        drx = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        a0, a1, a2, a3, a4 = -s * r[i], (s - 2 * c1 * it) * r[i], c1 * it, (c - s * it) * r[i], s * it
        J[i] = (a0 * np.eye(3) + a1 * rrt + a2 * drrt + a3 * rx + a4 * drx).ravel()
    return R, J


def pnp_project(rvec, tvec, X, m):
    """cvProjectPoints2 of one point (K = I, no distortion) at 40 digits: err [2], J [2][6] (d / d rvec | d / d tvec)"""
    R, dR = rodrigues(rvec), rodrigues_jacobian(rvec)
    p = [sum(R[a][k] * X[k] for k in range(3)) + tvec[a] for a in range(3)]
    err = [p[0] / p[2] - m[0], p[1] / p[2] - m[1]]
    Jp = [[1 / p[2], ZERO, -p[0] / p[2] ** 2], [ZERO, 1 / p[2], -p[1] / p[2] ** 2]]
    J = []
    for a in range(2):
        dr = [sum(Jp[a][k] * sum(dR[i][3 * k + b] * X[b] for b in range(3)) for k in range(3)) for i in range(3)]
        J.append(dr + Jp[a])
    return err, J


def pnp_step(JtJ, JtE, lg, prev, rank_cut=True):
    """CvLevMarq::step at 40 digits: prev - A^+ JtE, A = JtJ with its diagonal times 1 + 10^lg; the pseudo-inverse drops singular
    values <= 2 DBL_EPSILON sum(w), as cv::solve(DECOMP_SVD) does"""
    A = mp.matrix(6, 6)
    for a in range(6):
        for b in range(6):
            A[a, b] = mpf(float(JtJ[max(a, b)][min(a, b)]))
        A[a, a] *= 1 + mpf(10) ** lg
    Uu, w, V = mp.svd_r(A)
    thr = 2 * mpf(2) ** -52 * sum(w)
    b = mp.matrix([mpf(float(v)) for v in JtE])
    ub = Uu.T * b
    x = V.T * mp.matrix([ub[i] / w[i] if (w[i] > thr or not rank_cut) else ZERO for i in range(6)])
    return [mpf(float(prev[k])) - x[k] for k in range(6)]


# ---- running the restatement / reading outputs ---------------------------------------------------------------------------------------
def bind(lib):
    dp = C.POINTER(C.c_double)
    lib.isvo_sfm_set_ba_max_iterations.argtypes = [C.c_int]; lib.isvo_sfm_set_ba_max_iterations.restype = None
    lib.isvo_sfm_ba_obs.argtypes = [dp] * 8; lib.isvo_sfm_ba_obs.restype = None
    return lib


def oracle_capped(lib, name, cap):
    """the restatement on a case with the BA capped at `cap` iterations -> (problem, result, positions, states)"""
    import sfm_oracle
    sp, n, mid = make_case(name)
    bind(lib).isvo_sfm_set_ba_max_iterations(cap)
    try:
        r, pos, st = sfm_oracle.solve(lib, sp)
    finally:
        lib.isvo_sfm_set_ba_max_iterations(50)
    return sp, r, pos, st


INTS = ("status", "ba_iterations", "ba_successful", "ba_termination", "n_triangulated", "n_ba_cols")


def check_chain(name, outputs, label, margin=None, corrupt=None, route=None):
    """outputs: [(result, positions, states)] of the code under test at caps 0, 1, 2 on case `name`.  Reproduces ba_initial_cost from
    the cap-0 output and every later output from the one before it; prints one RATIO line per quantity and returns
    [(key, err, e64, floor)]; asserts the integer side of every decision.  corrupt(ref): a corruption of the reference."""
    sp, n, mid = make_case(name)
    r0, p0, s0 = outputs[0]
    assert r0.status == 0 and r0.ba_iterations == 0 and r0.n_triangulated == n and not s0[mid] and r0.ba_termination == 4, (name, r0.status, r0.ba_iterations, r0.n_triangulated)
    refs = [Reference(sp, s0)] + ([Reference(sp, s0)] if corrupt else [])
    if corrupt:
        corrupt(refs[1])
    ref = refs[0]
    x0 = State.from_output(r0, p0, s0, ref.nw)
    scs = [r.scale(r.blocks(x0)) for r in refs]
    ctls = [Control() for _ in refs]
    rows = [("cost0",) + cost_errors(ref, r0.ba_initial_cost, refs[-1].cost(x0), ref.cost64(x0))]
    x, nsucc, edges, clamped = x0, 0, [], 0
    for k in (1, 2):
        rk, pk, sk = outputs[k]
        its = [r.iteration(x, sc, ctl, route or ("dense" if name == SMALLEST else "schur")) for r, sc, ctl in zip(refs, scs, ctls)]
        it = its[0]
        clamped = max(clamped, ref.n_clamped)
        assert it["term"] is None, (name, k, it["term"])
        edges.append((k, _f(it["rho"]), abs(it["rho64"] - _f(it["rho"])), _f(it["model"]), abs(it["model64"] - _f(it["model"]))))
        nsucc += it["accepted"]
        assert (rk.status, rk.ba_iterations, rk.ba_successful, rk.ba_termination) == (0, k, nsucc, 4), (name, k, rk.status, rk.ba_iterations, rk.ba_successful, nsucc)
        assert np.array_equal(sk, s0)
        if it["accepted"]:
            # (under a corruption: the corrupted reference's candidate against the output, in the clean reference's yardsticks)
            bad = dict(its[-1], x1=its[-1]["cand"])
            clean = step_errors(ref, x, it, rk, pk)
            for key, v in step_errors(ref, x, bad, rk, pk).items():
                rows.append((f"{key}{k}", v[0]) + clean[key][1:])
            rows.append((f"cost{k}", cost_errors(ref, rk.ba_final_cost, its[-1]["cand_cost"], it["cand64"])[0]) + cost_errors(ref, rk.ba_final_cost, it["cand_cost"], it["cand64"])[1:])
        else:                                                       # a rejected step leaves the state as it was, bit for bit
            prev = outputs[k - 1]
            assert np.array_equal(pk, prev[1]) and bytes(rk.Q) == bytes(prev[0].Q) and bytes(rk.T) == bytes(prev[0].T) and rk.ba_final_cost == prev[0].ba_final_cost
        x = State.from_output(rk, pk, sk, ref.nw)                  # the next iteration linearises where the code under test stands
    for key, e, e64, fl in rows:
        print(f"{label} {name} {key:10s} err {e:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {e / max(e64, fl):.3f}")
    return rows, edges, clamped
