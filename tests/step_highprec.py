"""One Gauss-Newton / dogleg step (DoglegStrategy::ComputeStep + TrustRegionMinimizer's model cost change, Ceres 2.0.0
trust_region_minimizer.cc / dogleg_strategy.cc, as csrc/isv_dogleg.h restates them) recomputed in np.longdouble from Jacobian
STRIPS.  Test infrastructure: tests/test_gpu_step_highprec.py feeds it the strips the GPU's own factor kernels wrote (pinned to the
oracle by tests/test_gpu_linearize.py) and compares the solver's intermediate vectors with the result, so that the comparison sees
the rounding of the solve stage alone; tests/test_step_highprec.py feeds it the oracle's strips and pins it to the oracle and to
a 40-digit mpmath solve.  Plain numpy: no BLAS on the extended-precision path (numpy has none for longdouble), a hand-written
Cholesky, the dense system on the main path; the ill-conditioned part (J^T J, the scalings, the Gauss-Newton solve) in PAIRS of
longdouble (step_dd below), because one longdouble is not enough for it.

Inputs (all float64, exact in longdouble):
  proj strips [F][28]   ISV_PROJ_STRIP: r(2) | J_pose_i 2x6 | J_pose_j 2x6 | J_lambda 2x1, CSR (landmark-major) factor order
  imu strips  [N-1][465] ISV_IMU_STRIP: r(15) | 15x6 pose_i | 15x9 sb_i | 15x6 pose_j | 15x9 sb_j
  prior strip           debug_read(0): [se3 r6 J6x6][lin9 r9 J9x9][relpose k: r6 Ji6x6 Jj6x6]...[rollpitch m: r2 J2x6]
  strip_ex    [F][12]   debug_read(22), free extrinsic only: J_ex 2x6 of every factor
every one Cauchy-corrected and in the 6-dof pose tangent already.

Parameter (column) order = the GPU's: 15 per DEVICE frame (6 pose | 9 speed/bias), frames 0 .. N-1, then -- with a free extrinsic --
the pseudo-frame N (6 extrinsic columns | 9 dummy columns no factor touches), then the L inverse depths.  The `_p` debug vectors
hold window w at [w * np, (w + 1) * np), np = 15 * device frames; the `_l` vectors hold it at [lm_off[w], lm_off[w + 1]), lm_off
the running sum of the windows' landmark counts.

What each debug selector of isv_debug_read holds, in the names of `Step` below (x = the point of the linearisation):
  14 scale_p, 15 scale_l   scale    Jacobi scaling 1 / (1 + ||J col||), J' = J diag(scale)            (>0, dimension of 1 / column norm)
  16 diag_p,  23 diag_l    diag     D = sqrt(clamp(diag(J'^T J'), 1e-6, 1e32))                         (>0)
  12 grad_p,  13 grad_l    gradient D^-1 J'^T r: DoglegStrategy::gradient_, in the dogleg's D-scaled space, sign of +J^T r
  10 gn_p,    11 gn_l      gn       -D y, (J'^T J' + mu D^2) y = J'^T r: gauss_newton_step_, same space, a DESCENT direction
  17 delta_p, 18 delta_l   delta    the dogleg step with both scalings undone, step / D * scale: what Evaluator::Plus adds to x
  19 cost_c                         the cost at Plus(x, delta)
  20 model                 model    (J delta)^T (r + J delta / 2) = -model_cost_change                (<0 for a valid step)
The one ambiguity of this table is the sign of gn (Ceres negates the solve's y in place: "gauss_newton_step_ *= -diagonal_"); `Step`
asserts gradient . gn < 0, which only the descent direction satisfies, so a wrong sign cannot pass by loosening a tolerance.
The dummy columns of a free extrinsic carry no information (the device gives them a unit Hessian diagonal so that every kernel can
treat the pseudo-frame as a frame): `Problem.real_p` masks them out of every comparison; their step must be exactly zero.
"""
import numpy as np

LD = np.longdouble
PR_LIN9, PR_REL0, PR_REL_SZ, PR_RP_SZ = 42, 132, 78, 14
GAUSS_NEWTON, CAUCHY, INTERPOLATED = "gauss_newton", "cauchy", "interpolated"


def prior_strip_size(n_vo, max_rollpitch):
    return PR_REL0 + PR_REL_SZ * (n_vo - 1) + PR_RP_SZ * max_rollpitch


class Problem:
    """the factor blocks of one window in the GPU's column order: blocks[k] = (r [dim], [(col0, J [dim][wid]), ...]) in float64"""

    def __init__(self, w, proj, imu, prior, strip_ex=None):
        N, L, Nvo = w.N, w.L, w.Nvo
        self.est_ex = strip_ex is not None
        self.Nr, self.Nd, self.L = N, N + (1 if self.est_ex else 0), L
        self.np = 15 * self.Nd
        self.ncols = self.np + L
        self.real_p = np.ones(self.np, bool)
        if self.est_ex:
            self.real_p[15 * N + 6:] = False
        self.blocks, self.kinds = [], []
        proj = np.asarray(proj, float).reshape(-1, 28); imu = np.asarray(imu, float).reshape(-1, 465); prior = np.asarray(prior, float)
        for i in range(N - 1):
            if w.imu[i].sum_dt > 10.0:                      # (src/estimator.cpp:1043: left out)
                continue
            s = imu[i]
            self._add("imu", s[:15], [(15 * i, s[15:105].reshape(15, 6)), (15 * i + 6, s[105:240].reshape(15, 9)),
                                      (15 * (i + 1), s[240:330].reshape(15, 6)), (15 * (i + 1) + 6, s[330:465].reshape(15, 9))])
        f = 0
        self.proj_block_of_landmark = [[] for _ in range(L)]
        for l in range(L):
            h, o0, o1 = int(w.lm_start_frame[l]), int(w.lm_obs_ptr[l]), int(w.lm_obs_ptr[l + 1])
            for o in range(o0 + 1, o1):
                s = proj[f]
                cols = [(15 * h, s[2:14].reshape(2, 6)), (15 * (h + o - o0), s[14:26].reshape(2, 6))]
                if self.est_ex:
                    cols.append((15 * N, np.asarray(strip_ex, float).reshape(-1, 12)[f].reshape(2, 6)))
                cols.append((self.np + l, s[26:28].reshape(2, 1)))
                self.proj_block_of_landmark[l].append(len(self.blocks))
                self._add("proj", s[:2], cols)
                f += 1
        assert f == proj.shape[0], (f, proj.shape)
        self._add("se3", prior[0:6], [(0, prior[6:42].reshape(6, 6))])
        self._add("lin9", prior[42:51], [(15 * (Nvo - 1) + 6, prior[51:132].reshape(9, 9))])
        for k in range(Nvo - 1):
            b = PR_REL0 + PR_REL_SZ * k
            self._add("relpose", prior[b:b + 6], [(15 * k, prior[b + 6:b + 42].reshape(6, 6)), (15 * (k + 1), prior[b + 42:b + 78].reshape(6, 6))])
        base = PR_REL0 + PR_REL_SZ * (Nvo - 1)
        for m in range(w.n_rollpitch):
            b = base + PR_RP_SZ * m
            self._add("rollpitch", prior[b:b + 2], [(15 * int(w.rollpitch[m].index), prior[b + 2:b + 14].reshape(2, 6))])
        self.nres = sum(len(r) for r, _ in self.blocks)

    def _add(self, kind, r, cols):
        self.blocks.append((np.array(r, float), [(int(c), np.array(J, float)) for c, J in cols]))
        self.kinds.append(kind)

    def dense(self, dtype=float):
        """J [nres][ncols] and r [nres]"""
        J = np.zeros((self.nres, self.ncols), dtype); r = np.zeros(self.nres, dtype)
        o = 0
        for rb, cols in self.blocks:
            d = len(rb)
            r[o:o + d] = rb
            for c, Jb in cols:
                J[o:o + d, c:c + Jb.shape[1]] += Jb
            o += d
        return J, r

    def normal_equations_ld(self):
        """J^T J and J^T r in longdouble, block by block (what the dense product gives, without its nres * ncols^2 zeros)"""
        H = np.zeros((self.ncols, self.ncols), LD); g = np.zeros(self.ncols, LD)
        for rb, cols in self.blocks:
            r = rb.astype(LD)
            cl = [(c, Jb.astype(LD)) for c, Jb in cols]
            for ca, Ja in cl:
                g[ca:ca + Ja.shape[1]] += (Ja * r[:, None]).sum(0)
                for cb, Jb in cl:
                    H[ca:ca + Ja.shape[1], cb:cb + Jb.shape[1]] += (Ja[:, :, None] * Jb[:, None, :]).sum(0)
        return H, g

    def normal_equations_f64(self):
        J, r = self.dense(float)
        return J.T @ J, J.T @ r


def cholesky_ld(A):
    """lower Cholesky factor, column by column, in A's precision; raises on a non-positive pivot"""
    n = A.shape[0]
    Lc = np.zeros_like(A)
    for j in range(n):
        row = Lc[j, :j]
        p = A[j, j] - (row * row).sum()
        if not p > 0:
            raise np.linalg.LinAlgError("not positive definite")
        p = np.sqrt(p)
        Lc[j, j] = p
        if j + 1 < n:
            Lc[j + 1:, j] = (A[j + 1:, j] - (Lc[j + 1:, :j] * row[None, :]).sum(1)) / p
    return Lc


def cholesky_solve_ld(Lc, b):
    n = len(b)
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - (Lc[i, :i] * y[:i]).sum()) / Lc[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (Lc[i + 1:, i] * x[i + 1:]).sum()) / Lc[i, i]
    return x


def matvec(A, x):
    return (A * x[None, :]).sum(1)


def solve_dense_ld(A, b):
    """hand-written Cholesky + one round of iterative refinement"""
    Lc = cholesky_ld(A)
    x = cholesky_solve_ld(Lc, b)
    return x + cholesky_solve_ld(Lc, b - matvec(A, x))


def solve_f64(A, b):
    """the float64 yardstick's solve: LAPACK potrf / potrs through scipy"""
    import scipy.linalg
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


DENSE_MAX_COLS = 700           # (a longdouble Cholesky of 700 columns takes about a second; beyond: step_dd's eliminated preconditioner)


class Step:
    """everything DoglegStrategy::ComputeStep derives from (J^T J, J^T r) at a fresh linearisation, in the precision of H (float64:
    the yardstick; longdouble: a plain restatement used by the CPU tests).  The reference itself is step_dd -> Step.finish."""

    def __init__(self, H, g, mu, radius, n_p, solver=None):
        dt = H.dtype.type
        if solver is None:
            solver = solve_f64 if dt is np.float64 else solve_dense_ld
        one = dt(1)
        self.scale = scale = one / (one + np.sqrt(np.diag(H)))
        Hs = H * scale[:, None] * scale[None, :]
        gs = g * scale
        self.diag = D = np.sqrt(np.clip(np.diag(Hs), dt(1e-6), dt(1e32)))
        self.gradient = grad = gs / D
        self.alpha = self._alpha(Hs, grad, D)
        A = Hs + np.diag(dt(mu) * D * D)
        y = solver(A, gs)
        self._dogleg(Hs, gs, scale, D, grad, y, -D * y, dt(radius), n_p)

    @staticmethod
    def _alpha(Hs, grad, D):
        """the Cauchy step length |g|^2 / |J' D^-1 g|^2"""
        t = grad / D
        return (grad * grad).sum() / (t * matvec(Hs, t)).sum()

    @classmethod
    def finish(cls, Hs, gs, scale, D, grad, y, gn, radius, n_p):
        self = cls.__new__(cls)
        self.scale, self.diag, self.gradient = scale, D, grad
        self.alpha = cls._alpha(Hs, grad, D)
        self._dogleg(Hs, gs, scale, D, grad, y, gn, Hs.dtype.type(radius), n_p)
        return self

    def _dogleg(self, Hs, gs, scale, D, grad, y, gn, radius, n_p):
        alpha = self.alpha
        self.y, self.gn = y, gn
        assert (grad * gn).sum() < 0, "the Gauss-Newton step is a descent direction: gradient . gn < 0 pins the sign of selectors 10 / 11"
        gn_norm, g_norm = np.sqrt((gn * gn).sum()), np.sqrt((grad * grad).sum())
        self.gn_norm, self.cauchy_norm = gn_norm, g_norm * alpha
        if gn_norm <= radius:
            self.branch, step = GAUSS_NEWTON, gn.copy()
        elif g_norm * alpha >= radius:
            self.branch, step = CAUCHY, -(radius / g_norm) * grad
        else:
            self.branch = INTERPOLATED
            b_dot_a = -alpha * (grad * gn).sum()
            a_sq = (alpha * g_norm) ** 2
            bma_sq = a_sq - 2 * b_dot_a + gn_norm ** 2
            c = b_dot_a - a_sq
            d = np.sqrt(c * c + bma_sq * (radius ** 2 - a_sq))
            beta = (d - c) / bma_sq if c <= 0 else (radius * radius - a_sq) / (d + c)
            step = (-alpha * (1 - beta)) * grad + beta * gn
        self.step = step                        # the dogleg step in the D-scaled space
        sd = step / D
        self.delta = sd * scale                 # both scalings undone
        self.model = (sd * gs).sum() + (sd * matvec(Hs, sd)).sum() / 2       # (J' sd)^T (r + J' sd / 2)
        self.n_p = n_p


# ---- pairs of longdouble ("double-longdouble", ~38 digits) ------------------------------------------------------------------
# The damped scaled system has a condition number of ~2.5e8, so a longdouble solve of a longdouble J^T J is good to ~1e-12 only.
# The reference therefore carries J^T J, the scalings, the system matrix and the residual of the iterative refinement as
# unevaluated sums hi + lo of two longdoubles (error-free transformations: Knuth's two-sum, Dekker's product with Veltkamp's
# split at 32 of the 64 mantissa bits); the longdouble Cholesky factor is the preconditioner of the refinement.
_SPLIT = LD(2.0 ** 32 + 1.0)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = _SPLIT * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a); bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd(a):
    a = np.asarray(a, LD)
    return a, np.zeros_like(a)


def dd_add(a, b):
    s, e = _two_sum(a[0], b[0])
    t, f = _two_sum(a[1], b[1])
    s, e = _fast_two_sum(s, e + t)
    return _fast_two_sum(s, e + f)


def dd_neg(a):
    return -a[0], -a[1]


def dd_sub(a, b):
    return dd_add(a, dd_neg(b))


def dd_mul(a, b):
    p, e = _two_prod(a[0], b[0])
    return _fast_two_sum(p, e + (a[0] * b[1] + a[1] * b[0]))


def dd_div(a, b):
    q1 = a[0] / b[0]
    r = dd_sub(a, dd_mul(b, dd(q1)))
    q2 = r[0] / b[0]
    r = dd_sub(r, dd_mul(b, dd(q2)))
    return dd_add(_fast_two_sum(q1, q2), dd(r[0] / b[0]))


def dd_sqrt(a):
    x = np.sqrt(a[0])
    r = dd_sub(a, _two_prod(x, x))
    return dd_add(dd(x), dd(np.where(x > 0, r[0], 0) / np.where(x > 0, 2 * x, 1)))


def dd_sum(a, axis):
    """sum along an axis by halving (a fixed tree)"""
    h, l = np.moveaxis(a[0], axis, 0), np.moveaxis(a[1], axis, 0)
    while h.shape[0] > 1:
        if h.shape[0] % 2:
            z = np.zeros((1,) + h.shape[1:], LD)
            h, l = np.concatenate([h, z]), np.concatenate([l, z])
        m = h.shape[0] // 2
        h, l = dd_add((h[:m], l[:m]), (h[m:], l[m:]))
    return h[0], l[0]


def dd_segment_sum(idx, v, size):
    """out[k] = sum of v[idx == k]: sorted by destination, neighbours of a segment are added pairwise until one is left of each"""
    order = np.argsort(idx, kind="stable")
    idx, h, l = idx[order], v[0][order].copy(), v[1][order].copy()
    while len(idx):
        start = np.concatenate([[True], idx[1:] != idx[:-1]])
        if start.all():
            break
        pos = np.arange(len(idx))
        odd = (pos - np.maximum.accumulate(np.where(start, pos, 0))) % 2 == 1
        tgt = np.nonzero(odd)[0] - 1
        h[tgt], l[tgt] = dd_add((h[tgt], l[tgt]), (h[odd], l[odd]))
        idx, h, l = idx[~odd], h[~odd], l[~odd]
    oh, ol = np.zeros(size, LD), np.zeros(size, LD)
    oh[idx], ol[idx] = h, l
    return oh, ol


def normal_equations_dd(prob):
    """J^T J and J^T r as pairs of longdouble: every product of two float64 entries exactly, the sums in pair arithmetic"""
    J, r = prob.dense(float)
    n = prob.ncols
    rows, cols = np.nonzero(J)
    cnt = np.bincount(rows, minlength=J.shape[0])
    first = np.concatenate([[0], np.cumsum(cnt)])
    Hi, Hv, gi, gv = [], [], [], []
    for k in np.unique(cnt[cnt > 0]):
        rr = np.nonzero(cnt == k)[0]
        sel = first[rr][:, None] + np.arange(k)[None, :]
        Cc = cols[sel]; V = J[rows[sel], Cc].astype(LD)
        Hi.append((Cc[:, :, None] * n + Cc[:, None, :]).ravel())
        p = _two_prod(V[:, :, None], V[:, None, :])
        Hv.append((p[0].ravel(), p[1].ravel()))
        gi.append(Cc.ravel())
        p = _two_prod(V, r[rr].astype(LD)[:, None])
        gv.append((p[0].ravel(), p[1].ravel()))
    cat = lambda vs: (np.concatenate([v[0] for v in vs]), np.concatenate([v[1] for v in vs]))
    H = dd_segment_sum(np.concatenate(Hi), cat(Hv), n * n)
    g = dd_segment_sum(np.concatenate(gi), cat(gv), n)
    return (H[0].reshape(n, n), H[1].reshape(n, n)), g


def step_dd(prob, mu, radius, route=None):
    """the reference Step: scalings, gradient and the Gauss-Newton solve in pair arithmetic (rounded to longdouble at the end), the
    dogleg formulas -- well conditioned -- in longdouble from those.  route: "dense" | "eliminated" preconditioner (default by size)"""
    H, g = normal_equations_dd(prob)
    n, n_p = prob.ncols, prob.np
    one = dd(np.ones(n))
    Hd = (np.diag(H[0]).copy(), np.diag(H[1]).copy())
    scale = dd_div(one, dd_add(one, dd_sqrt(Hd)))
    Hs = dd_mul(dd_mul(H, (scale[0][:, None], scale[1][:, None])), (scale[0][None, :], scale[1][None, :]))
    gs = dd_mul(g, scale)
    d2 = (np.diag(Hs[0]).copy(), np.diag(Hs[1]).copy())
    lo_, hi_ = d2[0] < LD(1e-6), d2[0] > LD(1e32)
    d2 = (np.where(lo_, LD(1e-6), np.where(hi_, LD(1e32), d2[0])), np.where(lo_ | hi_, LD(0), d2[1]))
    D = dd_sqrt(d2)
    grad = dd_div(gs, D)
    damp = dd_mul(dd(np.full(n, LD(mu))), d2)
    A = (Hs[0].copy(), Hs[1].copy())
    i = np.arange(n)
    A[0][i, i], A[1][i, i] = dd_add((A[0][i, i], A[1][i, i]), damp)
    if route is None:
        route = "dense" if n <= DENSE_MAX_COLS else "eliminated"
    if route == "dense":
        Lc = cholesky_ld(A[0])
        apply = lambda rhs: cholesky_solve_ld(Lc, rhs)
    else:
        App, Apl, all_ = A[0][:n_p, :n_p], A[0][:n_p, n_p:], np.diag(A[0])[n_p:]
        T = Apl / all_[None, :]
        Lc = cholesky_ld(App - np.array([(T[k][None, :] * Apl).sum(1) for k in range(n_p)]))

        def apply(rhs):
            xp = cholesky_solve_ld(Lc, rhs[:n_p] - matvec(T, rhs[n_p:]))
            return np.concatenate([xp, (rhs[n_p:] - matvec(Apl.T, xp)) / all_])
    y = dd(np.zeros(n))
    for _ in range(4):              # (each round gains ~cond * 2^-64 = 1e-11; the residual is formed in pair arithmetic)
        res = dd_sub(gs, dd_sum(dd_mul(A, (y[0][None, :], y[1][None, :])), 1))
        dy = apply(res[0])
        y = dd_add(y, dd(dy))
    last = float(np.sqrt((dy * dy).sum() / (y[0] * y[0]).sum()))
    assert last < 1e-25, f"the refinement of the reference has not converged: last correction {last:.1e} of the solution"
    gn = dd_neg(dd_mul(D, y))
    return Step.finish(Hs[0], gs[0], scale[0], D[0], grad[0], y[0], gn[0], radius, n_p)


def reference_pair(prob, mu, radius):
    """(extended-precision step, plain float64 step of the same strips -- J^T J by numpy's BLAS, the Cholesky solve by LAPACK through
    scipy): the reference and the yardstick"""
    H64, g64 = prob.normal_equations_f64()
    return step_dd(prob, mu, radius), Step(H64, g64, mu, radius, prob.np)


def perturb(w, amp=1.0, seed=0):
    """non-zero prior residuals: tests/test_gpu_linearize.py::test_linearize_at_perturbed_priors, scaled by amp"""
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(seed)
    w.Ps += amp * 0.03 * rng.normal(size=w.Ps.shape); w.Vs += amp * 0.03 * rng.normal(size=w.Vs.shape)
    for i in range(w.N):
        w.Rs[i] = w.Rs[i] @ Rot.from_rotvec(amp * 0.01 * rng.normal(size=3)).as_matrix()
    return w


def err(a, ref):
    """max-norm of the difference relative to the 2-norm of the reference vector (in longdouble)"""
    a, ref = np.asarray(a, LD), np.asarray(ref, LD)
    return float(np.abs(a - ref).max() / np.sqrt((ref * ref).sum()))


def floor_of(n):
    return n * 2.0 ** -53
