"""The loop-closure verification (include/isvins_loop.h: KeyFrame::findConnection) at 40 digits, written from the definitions and not from
is-vins_amd/csrc/isv_loop_common.h: the reference project's src/pose_graph/keyframe.cpp:77-303 (the matching, the gates, PnPRANSAC's tail,
loop_weight, the relative pose and the yaw) and the OpenCV 3.2.0 routines that the header of include/isvins_loop.h cites
(RANSACPointSetRegistrator::run, getSubset, RANSACUpdateNumIters, PnPRansacCallback, epnp::compute_pose, cvFindExtrinsicCameraParams2,
CvLevMarq).  OpenCV's source is not available to this project, so that part is a reading of the citations.  It is the independent
reading that tests/test_loop_highprec.py holds the CPU restatement to, and tests/test_gpu_loop_highprec.py the kernel.  No call into the
C restatement is made here, but for the one basis hook of the EPnP stage test (epnp_from_hook takes what isvo_lp_epnp_basis returned).

Reused, because already independent readings: relpose_highprec.rng_uniform / subset (OpenCV's RNG in Python integers),
loop_cases.brute_force (the matching), sfm_highprec.rodrigues / rodrigues_jacobian (the exponential and its derivative at 40 digits).

Integer layer, decided exactly.  The match list comes from brute_force in point order and carries `src`.  The gates are L1 and
0.6 MIN_LOOP_NUM.  The RANSAC is serial (the kernel's chunks of 64 are the kernel's business): a fresh RNG(2^64 - 1), five distinct draws
per hypothesis, a model kept when g > max(best, 4), RANSACUpdateNumIters(conf, (n - g) / n, 5, niters) with cvRound as round-half-even,
ransac_iterations from the configuration.  A point is an inlier when float32(dx^2 + dy^2) <= float32(thresh^2), in float32 from the
float32-rounded projection (L5): the projection is computed at 40 digits and rounded, and the float32 operations are numpy's (exact
roundings of exactly representable inputs).  A projection within BAND (1e-9, relative) of a float32 rounding boundary whose other side
flips the decision is a violated condition (`round`); so is a 40-digit error within BAND of thresh^2 in doubles (`band`).

EPnP on five points is not a function of its input alone: M^T M has an exact two-dimensional null space, the two eigenvectors a solver
returns for it are an arbitrary basis, and so are the signs of all four eigenvectors and of the control-point axes (an axis sign changes
M itself).  find_betas_approx_1 reads one null vector alone and five Gauss-Newton iterations do not erase the start on noisy data.  So:
  the stage test (epnp_from_hook)  takes the basis the code under test used, projects its null pair onto the exact null space, replaces
        the other eigenvectors by the exact ones they approximate, and runs the rest at 40 digits; e64 is the same from the same basis
        in float64
  the decisions (Ransac)  evaluate every hypothesis over FAMILY admissible bases: eight turns of the null pair (odd ones reflected),
        each with another of the eight sign patterns of the control-point axes and another sign pattern of the four eigenvectors.
        Screen: a hypothesis whose count stays <= max(best, 4) - 3 over the family by the float64 route is decided.  Every other one,
        and the kept one, is solved at 40 digits over the family and must give ONE inlier count, the kept model ONE mask (`basis`).
        One exception, because no output can depend on it: a hypothesis whose count stays <= max(best, 4) over the whole family by
        both routes is kept under no basis, and its count is never read again, so there the counts may differ (an all-outlier pair
        is full of such hypotheses: five wrong matches fit nothing, and 0, 1 or 2 points fall inside 10 px by chance).  The same
        holds for a hypothesis whose largest count c over the family passes the floor, when keeping it would leave niters as it is
        (RANSACUpdateNumIters of c gives no less than the current niters) and a LATER keep of this reference has more than c
        inliers: that keep is then taken under every basis, from the same niters, and overwrites model and count alike.

Float layer, from the mask onward (a function of the inlier set, so no basis enters): the planarity ratio, L^T L summed exactly, its
smallest eigenvector at 40 digits, the determinant's sign, the 3 x 3 SVD, |R| / |RR|, Rodrigues; CvLevMarq (20 iterations, FLT_EPSILON)
with every accept / reject / stop decision taken at 40 digits; then keyframe.cpp:200-227 and :274-292.  Beside every float output stands
the same quantity by a plain float64 route (numpy): its error against the 40-digit value is the yardstick e64.

Conditions (Reference.conditions(); a case that fails one is replaced in tests/loop_highprec_cases.py, never excused):
  round / band   see above
  gates          RANSACUpdateNumIters' quotient off a half-integer, the planarity ratio off 1e-3, the yaw off 30 and the distance off 20,
                 CvLevMarq's stop test (relative change below FLT_EPSILON?) off its edge, all by 1e-9 relative.  Limitation: a
                 convergence test on a relative change near FLT_EPSILON is a decision like any other
  lm_accept      CvLevMarq's accept test (errNorm > prevErrNorm?): d = (errNorm - prevErrNorm) / prevErrNorm is off zero by 1e-9 where
                 that can be.  It cannot in the last iteration of a converged solve, which lowers the error by about the square of
                 its relative step (measured: 7e-13 on noise2, whose float64 route gives the same d to 2e-15).  There the bound is
                 derived from the number format: errNorm is the root of a sum of 2n squares, each carrying about eight roundings, so a
                 float64 evaluation is within (2n + 16) 2^-53 of it; two norms and a factor 4 give 4 (2n + 16) 2^-52
  basis          see above; also: no EPnP branch (the sign of a beta^2, the sign of the first depth, the choice of N among reprojection
                 errors) is tested here -- a branch that depends on the basis shows as a differing count or mask
  dlt            the smallest eigenvalue of L^T L is separated from the next (ratio below 0.5), det(RR) off zero
  routes         the float64 route gives the same planar / iteration / gate decisions as the 40-digit one

Controls (CONTROLS) corrupt this reference, never the code under test."""
import copy
import math

import mpmath as mp
import numpy as np

import loop_cases
import relpose_highprec as rh
import sfm_highprec as sh

mp.mp.dps = 40
mpf = mp.mpf
BAND = 1e-9
NEAR64 = 1e-3                    # a float64 point error within this (relative) of thresh^2 is evaluated again at 40 digits
SCREEN = 3
FAMILY = 8
FLT_EPSILON, DBL_EPSILON = 2.0 ** -23, 2.0 ** -52
CONTROLS = ("keep_ge", "keep_no_floor", "model_points_4", "l5_off", "no_l3", "t_untransposed", "quat_xyzw", "turned_1e-11")
TAIL_CONTROLS = ("no_l3", "t_untransposed", "quat_xyzw", "turned_1e-11")        # act after the final solve: no second RANSAC
(OK, FEW_MATCHES, UNDEFINED_POSE, PNP_FAILED, GATE, PLANAR) = range(6)
_M64 = (1 << 64) - 1
PAIRS6 = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


class Edge(Exception):
    """a decision too close to its edge, or a degenerate solve: the case is inadmissible"""


# ------------------------------------------------------------------------------------------------------------ two arithmetics, one text
class F64:
    """plain float64: Python floats, numpy's LAPACK for the factorisations"""
    name = "f64"
    sqrt = staticmethod(math.sqrt)

    @staticmethod
    def num(v):
        return float(v)

    @staticmethod
    def lstsq(A, b):
        return np.linalg.lstsq(np.array(A, float), np.array(b, float), rcond=None)[0].tolist()

    @staticmethod
    def polar(M):
        U, _, Vt = np.linalg.svd(np.array(M, float))
        return (U @ Vt).tolist()

    @staticmethod
    def eigh(M):
        w, V = np.linalg.eigh(np.array(M, float))
        return w.tolist(), V.T.tolist()


class MP:
    """40 digits: mpmath"""
    name = "mp"
    sqrt = staticmethod(mp.sqrt)

    @staticmethod
    def num(v):
        return v if isinstance(v, mpf) else mpf(float(v))

    @staticmethod
    def lstsq(A, b):
        x = mp.qr_solve(mp.matrix(A), mp.matrix(b))[0]
        return [x[i] for i in range(len(A[0]))]

    @staticmethod
    def polar(M):
        U, _, Vt = mp.svd_r(mp.matrix(M))
        R = U * Vt
        return [[R[i, j] for j in range(3)] for i in range(3)]

    @staticmethod
    def eigh(M):
        w, Q = mp.eigsy(mp.matrix(M))
        n = len(M)
        order = sorted(range(n), key=lambda i: w[i])
        return [w[i] for i in order], [[Q[k, i] for k in range(n)] for i in order]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def inv3(m):
    d = det3(m)
    c = lambda i, j: m[(i + 1) % 3][(j + 1) % 3] * m[(i + 2) % 3][(j + 2) % 3] - m[(i + 1) % 3][(j + 2) % 3] * m[(i + 2) % 3][(j + 1) % 3]   # noqa: E731
    return [[c(j, i) / d for j in range(3)] for i in range(3)]


# ------------------------------------------------------------------------------------------------------------------------------- EPnP
def control_points(X, be, signs=(1, 1, 1)):
    """choose_control_points: the centroid, then centroid + sqrt(lambda_i / n) axis_i, largest lambda first; signs: the axes' signs"""
    n = len(X)
    c0 = [sum(x[k] for x in X) / n for k in range(3)]
    C = [[sum((x[j] - c0[j]) * (x[k] - c0[k]) for x in X) for k in range(3)] for j in range(3)]
    w, V = be.eigh(C)
    return [c0] + [[c0[j] + signs[i] * be.sqrt(w[2 - i] / n) * V[2 - i][j] for j in range(3)] for i in range(3)]


def barycentric(cws, X):
    """compute_barycentric_coordinates: alphas [n][4]"""
    CC = [[cws[j + 1][i] - cws[0][i] for j in range(3)] for i in range(3)]
    ci = inv3(CC)
    out = []
    for x in X:
        d = [x[k] - cws[0][k] for k in range(3)]
        a = [dot(ci[j], d) for j in range(3)]
        out.append([1 - a[0] - a[1] - a[2]] + a)
    return out


def mtm(alphas, uv):
    """fill_M with fu = fv = 1, uc = vc = 0, and M^T M"""
    rows = []
    for a, (u, v) in zip(alphas, uv):
        rows.append([c for j in range(4) for c in (a[j], 0 * a[j], -a[j] * u)])
        rows.append([c for j in range(4) for c in (0 * a[j], a[j], -a[j] * v)])
    return [[sum(r[p] * r[q] for r in rows) for q in range(12)] for p in range(12)], rows


def epnp_from_basis(X, uv, cws, alphas, vv, be):
    """epnp::compute_pose from the control points and the four eigenvectors vv (smallest eigenvalue first) on: L_6x10, rho, the three
    beta approximations, five Gauss-Newton iterations each, R / t by the 3 x 3 SVD, the N of lowest reprojection error.
    -> (R [3][3], t [3], N, the three reprojection errors)"""
    n = len(X)
    dv = [[[vv[i][3 * a + k] - vv[i][3 * b + k] for k in range(3)] for a, b in PAIRS6] for i in range(4)]
    L = []
    for r in range(6):
        d = [dv[i][r] for i in range(4)]
        L.append([dot(d[0], d[0]), 2 * dot(d[0], d[1]), dot(d[1], d[1]), 2 * dot(d[0], d[2]), 2 * dot(d[1], d[2]), dot(d[2], d[2]),
                  2 * dot(d[0], d[3]), 2 * dot(d[1], d[3]), 2 * dot(d[2], d[3]), dot(d[3], d[3])])
    rho = [sum((cws[a][k] - cws[b][k]) ** 2 for k in range(3)) for a, b in PAIRS6]
    zero = 0 * rho[0]
    best = None
    errs = []
    for N, cols in ((1, (0, 1, 3, 6)), (2, (0, 1, 2)), (3, (0, 1, 2, 3, 4))):
        x = be.lstsq([[row[c] for c in cols] for row in L], rho)
        if N == 1:                                  # B11 B12 B13 B14
            b0 = be.sqrt(abs(x[0]))
            sg = -1 if x[0] < 0 else 1
            b = [b0, sg * x[1] / b0, sg * x[2] / b0, sg * x[3] / b0]
        else:                                       # B11 B12 B22 (B13 B23)
            b0 = be.sqrt(abs(x[0]))
            b1 = be.sqrt(abs(x[2])) if (x[2] < 0) == (x[0] < 0) and x[2] != 0 else zero
            if x[1] < 0:
                b0 = -b0
            b = [b0, b1, x[3] / b0 if N == 3 else zero, zero]
        for _ in range(5):                          # gauss_newton
            A, r = [], []
            for l, rh_ in zip(L, rho):
                A.append([2 * l[0] * b[0] + l[1] * b[1] + l[3] * b[2] + l[6] * b[3], l[1] * b[0] + 2 * l[2] * b[1] + l[4] * b[2] + l[7] * b[3],
                          l[3] * b[0] + l[4] * b[1] + 2 * l[5] * b[2] + l[8] * b[3], l[6] * b[0] + l[7] * b[1] + l[8] * b[2] + 2 * l[9] * b[3]])
                r.append(rh_ - (l[0] * b[0] * b[0] + l[1] * b[0] * b[1] + l[2] * b[1] * b[1] + l[3] * b[0] * b[2] + l[4] * b[1] * b[2]
                                + l[5] * b[2] * b[2] + l[6] * b[0] * b[3] + l[7] * b[1] * b[3] + l[8] * b[2] * b[3] + l[9] * b[3] * b[3]))
            dx = be.lstsq(A, r)
            b = [b[k] + dx[k] for k in range(4)]
        # compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t
        ccs = [[sum(b[i] * vv[i][3 * j + k] for i in range(4)) for k in range(3)] for j in range(4)]
        pcs = [[sum(a[j] * ccs[j][k] for j in range(4)) for k in range(3)] for a in alphas]
        if pcs[0][2] < 0:
            pcs = [[-v for v in p] for p in pcs]
        pc0 = [sum(p[k] for p in pcs) / n for k in range(3)]
        pw0 = [sum(x_[k] for x_ in X) / n for k in range(3)]
        ABt = [[sum((p[j] - pc0[j]) * (x_[k] - pw0[k]) for p, x_ in zip(pcs, X)) for k in range(3)] for j in range(3)]
        R = be.polar(ABt)
        if det3(R) < 0:
            R[2] = [-v for v in R[2]]
        t = [pc0[k] - dot(R[k], pw0) for k in range(3)]
        e = zero
        for x_, (u, v) in zip(X, uv):
            pc = [dot(R[k], x_) + t[k] for k in range(3)]
            e += be.sqrt((u - pc[0] / pc[2]) ** 2 + (v - pc[1] / pc[2]) ** 2)
        e = e / n
        errs.append(e)
        if best is None or e < best[3]:
            best = (R, t, N, e)
    return best[0], best[1], best[2], errs


_SIGNS3 = [(1 - 2 * (k & 1), 1 - 2 * ((k >> 1) & 1), 1 - 2 * ((k >> 2) & 1)) for k in range(8)]


def epnp_family(X, uv, be, members=FAMILY):
    """EPnP on the five points X, uv over the FAMILY admissible bases (module docstring): [(R, t)]; None where a solve degenerates"""
    Xn = [[be.num(v) for v in x] for x in X]
    un = [[be.num(v) for v in q] for q in uv]
    out = []
    for k in range(members):
        cws = control_points(Xn, be, _SIGNS3[k])
        al = barycentric(cws, Xn)
        M, _ = mtm(al, un)
        w, V = be.eigh(M)
        th = math.pi * k / FAMILY + 0.1
        c, s = (be.num(math.cos(th)), be.num(math.sin(th))) if be is F64 else (mp.cos(mpf(th)), mp.sin(mpf(th)))
        v0 = [c * a + s * b for a, b in zip(V[0], V[1])]
        v1 = [c * b - s * a for a, b in zip(V[0], V[1])]
        if k & 1:
            v0, v1 = v1, v0
        sg = [1 - 2 * ((5 * k + 3 >> i) & 1) for i in range(4)]
        vv = [[sg[i] * v for v in vec] for i, vec in enumerate((v0, v1, V[2], V[3]))]
        try:
            R, t, _, _ = epnp_from_basis(Xn, un, cws, al, vv, be)
        except (ZeroDivisionError, np.linalg.LinAlgError, ValueError):
            R = t = None
        out.append((R, t))
    return out


def _match_sign(v, like):
    return [-x for x in v] if dot(v, [mpf(float(y)) for y in like]) < 0 else list(v)


def epnp_from_hook(X, uv, cws_hook, vv_hook):
    """the stage test's reference: EPnP at 40 digits from the basis the code under test used (cws_hook [4][3], vv_hook [4][12], smallest
    eigenvalue first) -> dict(R, t, N, R64, t64, N64, null_dim, resid).  The control points are recomputed at 40 digits with the hook's
    axis signs; with five points the hook's null pair is projected onto the exact null space, every other eigenvector is the exact one
    with the hook's sign.  R64 / t64: the same from the hook's own float64 basis by the float64 route."""
    n = len(X)
    Xm = [[mpf(float(v)) for v in x] for x in X]
    um = [[mpf(float(v)) for v in q] for q in uv]
    plain = control_points(Xm, MP)
    signs = tuple(1 if dot([a - b for a, b in zip(plain[i + 1], plain[0])], [mpf(float(a - b)) for a, b in zip(cws_hook[i + 1], cws_hook[0])]) > 0 else -1
                  for i in range(3))
    cws = control_points(Xm, MP, signs)
    al = barycentric(cws, Xm)
    M, _ = mtm(al, um)
    w, V = MP.eigh(M)
    null_dim = 2 if n == 5 else 1
    vv = []
    for i in range(4):
        h = [mpf(float(v)) for v in vv_hook[i]]
        if i < null_dim and null_dim == 2:
            vv.append([dot(h, V[0]) * a + dot(h, V[1]) * b for a, b in zip(V[0], V[1])])
        else:
            vv.append(_match_sign(V[i], vv_hook[i]))
    resid = max(float(abs(mpf(float(a)) - b)) for i in range(4) for a, b in zip(vv_hook[i], vv[i]))
    R, t, N, errs = epnp_from_basis(Xm, um, cws, al, vv, MP)
    X64 = [[float(v) for v in x] for x in X]
    u64 = [[float(v) for v in q] for q in uv]
    c64 = [[float(v) for v in c] for c in cws_hook]
    R64, t64, N64, _ = epnp_from_basis(X64, u64, c64, barycentric(c64, X64), [[float(v) for v in r] for r in vv_hook], F64)
    gaps = sorted(float(abs(a - b) / max(a, b)) for a in errs for b in errs if a is not b)
    return dict(R=R, t=t, N=N, R64=R64, t64=t64, N64=N64, resid=resid, n_gap=gaps[0], gap=float((w[null_dim] - w[null_dim - 1]) / w[11]))


# ------------------------------------------------------------------------------------------------------------------- the inlier test
def _f32_steps(v):
    """the float32 nearest to the float64 v, and the float32 on the other side of the nearer rounding boundary, with the relative
    distance of v from that boundary"""
    f = np.float32(v)
    other = np.nextafter(f, np.float32(np.inf) if v > float(f) else np.float32(-np.inf))
    mid = (float(f) + float(other)) / 2
    return f, other, mid


def _err32(u, v, px, py):
    dx, dy = np.float32(u) - px, np.float32(v) - py
    return np.float32(np.float32(dx * dx) + np.float32(dy * dy))


def inlier_mask(R, t, X, uv, thresh, stats, l5=True):
    """findInliers of the model R, t (mpf) over X [n][3], uv [n][2] (float64 arrays holding float32 values): the bool mask.  l5 False:
    the error formed and compared in doubles (the control)."""
    td = thresh * thresh
    tf = np.float32(td)
    Rf, tv = np.array([[float(v) for v in r] for r in R]), np.array([float(v) for v in t])
    pc = X @ Rf.T + tv
    pr = pc[:, :2] / pc[:, 2:3]
    e = ((uv - pr) ** 2).sum(axis=1)
    mask = e <= td
    for j in np.nonzero(np.abs(e - td) < NEAR64 * td)[0]:
        x = [mpf(float(v)) for v in X[j]]
        p = [dot(R[k], x) + t[k] for k in range(3)]
        px, py = p[0] / p[2], p[1] / p[2]
        em = (mpf(float(uv[j, 0])) - px) ** 2 + (mpf(float(uv[j, 1])) - py) ** 2
        stats["min_band"] = min(stats["min_band"], float(abs(em - td) / td))
        if not l5:
            mask[j] = em <= td
            continue
        fx, ox, mx = _f32_steps(float(px))
        fy, oy, my = _f32_steps(float(py))
        mask[j] = _err32(uv[j, 0], uv[j, 1], fx, fy) <= tf
        if (_err32(uv[j, 0], uv[j, 1], ox, fy) <= tf) != mask[j] or (_err32(uv[j, 0], uv[j, 1], ox, oy) <= tf) != mask[j]:
            stats["min_round"] = min(stats["min_round"], float(abs(px - mx) / abs(px)))
        if (_err32(uv[j, 0], uv[j, 1], fx, oy) <= tf) != mask[j] or (_err32(uv[j, 0], uv[j, 1], ox, oy) <= tf) != mask[j]:
            stats["min_round"] = min(stats["min_round"], float(abs(py - my) / abs(py)))
    return mask


def count64(R, t, X, uv, thresh, l5=True):
    """the float64 route's count (the screen): the projection in doubles, then float32 as the definition has it (l5) or doubles
    throughout; None models count 0"""
    if R is None:
        return 0
    pc = X @ np.array(R).T + np.array(t)
    with np.errstate(all="ignore"):
        pr = pc[:, :2] / pc[:, 2:3]
        if not l5:
            return int((((uv - pr) ** 2).sum(axis=1) <= thresh * thresh).sum())
        d = uv.astype(np.float32) - pr.astype(np.float32)
        return int((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= np.float32(thresh * thresh)).sum())


def update_num_iters(p, g, count, model_points, niters, hp):
    """RANSACUpdateNumIters(p, (count - g) / count, model_points, niters) at 40 digits (hp) or in float64: (niters, the distance of the
    quotient from a half-integer, cvRound's only edge)"""
    if g == count:
        return 0, 1.0                                   # 1 - (1 - 0)^m = 0 < DBL_MIN
    if hp:
        v = mp.log(1 - mpf(p)) / mp.log(1 - (mpf(g) / count) ** model_points)
    else:
        v = math.log(1.0 - p) / math.log(1.0 - (1.0 - (count - g) / count) ** model_points)
    if v >= niters:
        return niters, 1.0
    r = int(mp.nint(v)) if hp else int(round(v))        # both round half to even
    return r, float(abs(v - (mp.floor(v) if hp else math.floor(v)) - 0.5))


class Ransac:
    """RANSACPointSetRegistrator::run with PnPRansacCallback on X, uv (float64 arrays of the float32 points)"""

    def __init__(self, X, uv, thresh, confidence, max_iters, stats, control=None):
        n = len(X)
        state, best, niters, it = _M64, 0, max_iters, 0
        self.R = self.t = self.mask = None
        self.keeps, self.n_mp, self.n_screened, pending = [], 0, 0, []
        floor = (lambda b: b) if control == "keep_no_floor" else (lambda b: max(b, 4))
        keep = (lambda g, b: g >= floor(b)) if control == "keep_ge" else (lambda g, b: g > floor(b))
        l5 = control != "l5_off"
        while it < niters:
            state, idx = rh.subset(state, n, 5)
            fam64 = epnp_family(X[idx].tolist(), uv[idx].tolist(), F64)
            g64 = [count64(R, t, X, uv, thresh, l5) for R, t in fam64]
            if max(g64) <= floor(best) - SCREEN:
                self.n_screened += 1
            else:
                self.n_mp += 1
                fam = epnp_family(X[idx].tolist(), uv[idx].tolist(), MP, FAMILY if control is None else 1)   # (a control asserts no condition)
                if any(R is None for R, _ in fam):
                    raise Edge(f"hypothesis {it}: a 40-digit EPnP solve degenerated")
                masks = [inlier_mask(R, t, X, uv, thresh, stats, l5) for R, t in fam]
                g = [int(m.sum()) for m in masks]
                if control is None and (len(set(g)) != 1 or set(g64) != {g[0]}) and max(g + g64) > floor(best):
                    cmax = max(g + g64)
                    noop = update_num_iters(confidence, cmax, n, 4 if control == "model_points_4" else 5, niters, True)[0] == niters
                    pending.append((it, cmax, noop, g, g64))
                g = g[0]
                if keep(g, best):
                    best, self.R, self.t, self.mask = g, fam[0][0], fam[0][1], masks[0]
                    self.same_mask = all(np.array_equal(m, masks[0]) for m in masks)
                    mpts = 4 if control == "model_points_4" else 5
                    n_mp, edge = update_num_iters(confidence, g, n, mpts, niters, True)
                    n_64, _ = update_num_iters(confidence, g, n, mpts, niters, False)
                    stats["min_gate"] = min(stats["min_gate"], edge)
                    if n_mp != n_64:
                        stats["routes"].append(("niters", it, n_mp, n_64))
                    niters = n_mp
                    self.keeps.append((it, g, niters))
            it += 1
        self.iters, self.inliers = it, best
        for at, cmax, noop, g, g64 in pending:           # basis-dependent, and above the keep rule's floor under some basis
            if not (noop and any(k > at and gk > cmax for k, gk, _ in self.keeps)):
                stats["basis"].append(("count", at, g, g64))
        if self.keeps and not self.same_mask:
            stats["basis"].append(("mask", self.keeps[-1][0]))


# ------------------------------------------------------------------------------------------- solvePnP(SOLVEPNP_ITERATIVE, no guess)
def _edge(stats, value, bound):
    stats["min_gate"] = min(stats["min_gate"], float(abs(value - bound) / abs(bound)))


def planarity(X, be, stats=None):
    """cvFindExtrinsicCameraParams2's test on the scatter of the object points about their mean: W[2] / W[1] < 1e-3"""
    n = len(X)
    mc = [sum(x[k] for x in X) / n for k in range(3)]
    MM = [[sum((x[j] - mc[j]) * (x[k] - mc[k]) for x in X) for k in range(3)] for j in range(3)]
    w, _ = be.eigh(MM)
    ratio = w[0] / w[1]
    if stats is not None:
        _edge(stats, ratio, 1e-3)
    return ratio < 1e-3, ratio


def dlt(X, uv, be, stats=None):
    """the non-planar initialisation: L^T L (rows X Y Z 1 0 0 0 0 -uX -uY -uZ -u and 0 0 0 0 X Y Z 1 -vX -vY -vZ -v), its smallest
    eigenvector as [RR | tt], the sign by det(RR), R by the 3 x 3 SVD, tt scaled by |R| / |RR| -> (R [3][3], t [3])"""
    one, zero = 1 + 0 * X[0][0], 0 * X[0][0]
    rows = []
    for x, (u, v) in zip(X, uv):
        h = [x[0], x[1], x[2], one]
        rows.append(h + [zero] * 4 + [-u * c for c in h])
        rows.append([zero] * 4 + h + [-v * c for c in h])
    LtL = [[sum(r[p] * r[q] for r in rows) for q in range(12)] for p in range(12)]
    w, V = be.eigh(LtL)
    f = V[0]
    RR = [[f[4 * i + j] for j in range(3)] for i in range(3)]
    tt = [f[4 * i + 3] for i in range(3)]
    d = det3(RR)
    sc = be.sqrt(sum(v * v for r in RR for v in r))
    if stats is not None:
        stats["dlt_gap"] = max(stats["dlt_gap"], float(w[0] / w[1]))
        stats["min_det"] = min(stats["min_det"], float(abs(d) / sc ** 3))
    if d < 0:
        RR, tt = [[-v for v in r] for r in RR], [-v for v in tt]
    R = be.polar(RR)
    nr = be.sqrt(sum(v * v for r in R for v in r))
    return R, [v * (nr / sc) for v in tt]


def rot_to_vec(R, be):
    """Rodrigues, matrix to vector, off its special cases (theta well inside (0, pi)): theta axis, axis from the skew part"""
    r = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    s = be.sqrt(dot(r, r) / 4)
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    if not 1e-3 < float(s):
        raise Edge("Rodrigues(matrix) near its special cases")
    th = mp.atan2(s, c) if be is MP else math.atan2(s, c)
    return [v * th / (2 * s) for v in r]


def rodrigues64(r):
    return sh.rodrigues_jacobian_f64(r)


def lm_eval(par, X, uv, be, want_j):
    """cvProjectPoints2 over the points: (|err|^2, J^T J, J^T err)"""
    if be is MP:
        R, dR = sh.rodrigues(par[:3]), (sh.rodrigues_jacobian(par[:3]) if want_j else None)
    else:
        R, dR = rodrigues64(par[:3])
        R, dR = R.tolist(), dR.tolist()
    zero = 0 * par[0]
    e2, JtJ, JtE = zero, [[zero] * 6 for _ in range(6)], [zero] * 6
    for x, m in zip(X, uv):
        p = [dot(R[a], x) + par[3 + a] for a in range(3)]
        iz = 1 / p[2]
        pr = [p[0] * iz, p[1] * iz]
        err = [pr[0] - m[0], pr[1] - m[1]]
        e2 += err[0] * err[0] + err[1] * err[1]
        if not want_j:
            continue
        for a in range(2):
            dp = [[sum(dR[i][3 * k + b] * x[b] for b in range(3)) for k in range(3)] for i in range(3)]
            J = [iz * (dp[i][a] - pr[a] * dp[i][2]) for i in range(3)]
            J += [iz if a == 0 else zero, iz if a == 1 else zero, -pr[a] * iz]
            for i in range(6):
                JtE[i] += J[i] * err[a]
                for k in range(i + 1):
                    JtJ[i][k] += J[i] * J[k]
    for i in range(6):
        for k in range(i):
            JtJ[k][i] = JtJ[i][k]
    return e2, JtJ, JtE


def lm_step(JtJ, JtE, lg, prev, be):
    """CvLevMarq::step: prev - A^+ JtE, A = JtJ with its diagonal times 1 + 10^lg; cv::solve(DECOMP_SVD) drops singular values
    <= 2 DBL_EPSILON sum(w)"""
    if be is MP:
        A = mp.matrix(JtJ)
        for a in range(6):
            A[a, a] *= 1 + mpf(10) ** lg
        U, w, V = mp.svd_r(A)
        thr = 2 * mpf(DBL_EPSILON) * sum(w)
        ub = U.T * mp.matrix(JtE)
        x = V.T * mp.matrix([ub[i] / w[i] if w[i] > thr else mpf(0) for i in range(6)])
        return [prev[k] - x[k] for k in range(6)]
    A = np.array(JtJ, float)
    A[np.diag_indices(6)] *= 1.0 + math.exp(lg * math.log(10.0))
    U, w, Vt = np.linalg.svd(A)
    ub = U.T @ np.array(JtE, float)
    x = Vt.T @ np.where(w > 2 * DBL_EPSILON * w.sum(), ub / w, 0.0)
    return [prev[k] - float(x[k]) for k in range(6)]


def lev_marq(par, X, uv, be, stats=None):
    """CvLevMarq(6, 2n, 20 iterations, FLT_EPSILON) on cvProjectPoints2's residuals from `par`: (par, iterations, the decisions)"""
    lg, iters, prev_err, trail = -3, 0, None, []
    while True:
        e2, JtJ, JtE = lm_eval(par, X, uv, be, True)
        prev = par
        par = lm_step(JtJ, JtE, lg, prev, be)
        if iters == 0:
            prev_err = be.sqrt(e2)
        while True:
            err = be.sqrt(lm_eval(par, X, uv, be, False)[0])
            up = err > prev_err
            trail.append((bool(up), float((err - prev_err) / prev_err) if prev_err != 0 else 1.0))
            if up:
                lg += 1
                if lg <= 16:
                    par = lm_step(JtJ, JtE, lg, prev, be)
                    continue
            break
        lg = max(lg - 1, -16)
        iters += 1
        change = be.sqrt(sum((a - b) ** 2 for a, b in zip(par, prev))) / (be.sqrt(sum(b * b for b in prev)) + DBL_EPSILON)
        if stats is not None and iters < 20:
            stats["min_lm"] = min(stats["min_lm"], float(abs(change - FLT_EPSILON) / FLT_EPSILON))
        if iters >= 20 or change < FLT_EPSILON:
            return par, iters, trail
        prev_err = err


def iterative(X, uv, be, stats=None):
    """solvePnP(SOLVEPNP_ITERATIVE, no guess) -> (planar, rvec + tvec [6] or None, iterations, decisions)"""
    Xn = [[be.num(v) for v in x] for x in X]
    un = [[be.num(v) for v in q] for q in uv]
    if planarity(Xn, be, stats)[0]:
        return True, None, -1, []
    R, t = dlt(Xn, un, be, stats)
    par, iters, trail = lev_marq(rot_to_vec(R, be) + t, Xn, un, be, stats)
    return False, par, iters, trail


# ------------------------------------------------------------------------------------------------ keyframe.cpp:200-227 and :274-292
def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _tr(A):
    return [list(r) for r in zip(*A)]


def _mv(A, v):
    return [dot(r, v) for r in A]


def quaternion(m, be):
    """Eigen's Quaterniond(Matrix3d): w x y z"""
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        t = be.sqrt(t + 1)
        return [t / 2, (m[2][1] - m[1][2]) / (2 * t), (m[0][2] - m[2][0]) / (2 * t), (m[1][0] - m[0][1]) / (2 * t)]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = be.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
    q = [None] * 4
    q[1 + i] = t / 2
    q[0] = (m[k][j] - m[j][k]) / (2 * t)
    q[1 + j] = (m[j][i] + m[i][j]) / (2 * t)
    q[1 + k] = (m[k][i] + m[i][k]) / (2 * t)
    return q


def tail(par, X, uv, cfg, oT, oR, be, control=None, stats=None):
    """from rvec / tvec and the inliers X, uv on: R_pnp, T_w_c_old, PnP_R_old, PnP_T_old (:200-209), res and loop_weight (:211-227),
    relative_t / relative_q / relative_yaw and the gate (:276-282) -> dict"""
    if be is MP:
        R_pnp = sh.rodrigues(par[:3])
        atan2, pi, floor = mp.atan2, mp.pi, mp.floor
    else:
        R_pnp = rodrigues64(par[:3])[0].tolist()
        atan2, pi, floor = math.atan2, math.pi, math.floor
    if control == "turned_1e-11":                   # about (1, 2, 2) / 3, applied to the final pose
        G = sh.rodrigues([mpf("1e-11") / 3, mpf("2e-11") / 3, mpf("2e-11") / 3])
        R_pnp = _mm(R_pnp, _tr(G))
    T_pnp = par[3:]
    R_w_c_old = _tr(R_pnp)
    T_w_c_old = _mv(R_pnp if control == "t_untransposed" else R_w_c_old, [-v for v in T_pnp])
    ric = [[be.num(cfg.ric[3 * i + j]) for j in range(3)] for i in range(3)]
    tic = [be.num(v) for v in cfg.tic]
    PnP_R = _mm(R_w_c_old, _tr(ric))
    PnP_T = [a - b for a, b in zip(T_w_c_old, _mv(PnP_R, tic))]
    f = be.num(cfg.focal_length)
    res = 0 * f
    for x, q in zip(X, uv):
        p = _mv(R_pnp, [be.num(a) - b for a, b in zip(x, T_w_c_old)])
        p = [v / p[2] for v in p]
        d = [be.num(q[0]) - p[0], be.num(q[1]) - p[1], 1 - p[2]]
        res += be.sqrt(dot(d, d)) if control == "no_l3" else be.sqrt(sum((v / f) ** 2 for v in d))
    m = len(X)
    weight = (m - 6) / (res * res) if res > 0 and m > 6 else 0 * f
    oTn = [be.num(v) for v in oT]
    oRn = [[be.num(oR[i][j]) for j in range(3)] for i in range(3)]
    rel_t = _mv(_tr(PnP_R), [a - b for a, b in zip(oTn, PnP_T)])
    q = quaternion(_mm(_tr(PnP_R), oRn), be)
    if control == "quat_xyzw":
        q = q[1:] + q[:1]
    yaw_of = lambda R: atan2(R[1][0], R[0][0]) / pi * 180      # noqa: E731  Utility::R2ypr(R).x()
    a = yaw_of(oRn) - yaw_of(PnP_R)
    yaw = a - 360 * floor((a + 180) / 360) if a > 0 else a + 360 * floor((-a + 180) / 360)      # Utility::normalizeAngle
    dist = be.sqrt(dot(rel_t, rel_t))
    if stats is not None:
        _edge(stats, abs(yaw), cfg.max_yaw_deg)
        _edge(stats, dist, cfg.max_distance)
        stats["min_gate"] = min(stats["min_gate"], float(abs(abs(a) - 180) / 180))
    gate = abs(yaw) < cfg.max_yaw_deg and dist < cfg.max_distance
    return dict(PnP_R_old=sum(PnP_R, []), PnP_T_old=PnP_T, res=res, loop_weight=weight, loop_info=rel_t + q + [yaw], gate=bool(gate))


# ------------------------------------------------------------------------------------------------------------------------- the pair
def matches(pair):
    """searchByBRIEFDes and the first reduceVector, from loop_cases.brute_force: (index, dist, src, X [n][3], uv [n][2]) in point order"""
    bi, bd, ba = loop_cases.brute_force(pair)
    src = np.nonzero(ba)[0]
    X = pair.point_3d[src].astype(np.float64).reshape(-1, 3)
    uv = pair.keypoints_norm[bi[src]].astype(np.float64).reshape(-1, 2)
    return bi, bd, src, X, uv


FLOATS = ("PnP_R_old", "PnP_T_old", "loop_info", "res", "loop_weight")


class Reference:
    """findConnection on one pair: every field of isv_loop_result_t, the three per-point arrays, e64 of every float output and the record
    behind the conditions"""

    def __init__(self, cfg, pair, control=None):
        assert control is None or control in CONTROLS and control not in TAIL_CONTROLS
        self.control, self.cfg = control, cfg
        st = self.stats = dict(min_band=1.0, min_round=1.0, min_gate=1.0, min_lm=1.0, dlt_gap=0.0, min_det=1.0, basis=[], routes=[], lm_accept=[])
        self.n_points = pair.c.n_points
        self.match_index, self.match_dist, self.src, X, uv = matches(pair)
        n = self.n_matched = len(self.src)
        self.ransac_iters, self.ransac_inliers, self.pnp_iterations, self.n_final = -1, 0, -1, n
        self.has_loop, self.loop_index, self.ransac, self.out, self.out64 = 0, -1, None, None, None
        self.inlier = np.full(self.n_points, -1, dtype=np.int32)
        if not n > 0.6 * cfg.min_loop_num:                       # :274
            self.status = FEW_MATCHES
            return
        if not n > cfg.min_loop_num:                             # :262, L1
            self.status = UNDEFINED_POSE
            return
        r = self.ransac = Ransac(X, uv, cfg.ransac_threshold, cfg.ransac_confidence, cfg.ransac_iterations, st, control)
        self.ransac_iters, self.ransac_inliers = r.iters, r.inliers
        self.inlier[self.src] = 0
        if r.inliers <= 0:
            self.status, self.n_final = PNP_FAILED, 0
            return
        self.inlier[self.src] = r.mask.astype(np.int32)
        self.n_final = int(r.mask.sum())
        if not self.n_final > 0.6 * cfg.min_loop_num:
            self.status = PNP_FAILED
            return
        self.Xi, self.uvi = X[r.mask].tolist(), uv[r.mask].tolist()
        planar, self.par, iters, trail = iterative(self.Xi, self.uvi, MP, st)
        planar64, self.par64, iters64, trail64 = iterative(self.Xi, self.uvi, F64)
        if (planar, iters, [u for u, _ in trail]) != (planar64, iters64, [u for u, _ in trail64]):
            st["routes"].append(("iterative", planar, iters, trail, planar64, iters64, trail64))
        else:                                                    # the accept test's edge (module docstring)
            bound = 4 * (2 * self.n_final + 16) * DBL_EPSILON
            st["lm_accept"] = [(d, d64, bound) for (_, d), (_, d64) in zip(trail, trail64) if not abs(d) > min(BAND, bound)]
        if planar:
            self.status = PLANAR
            return
        self.pnp_iterations = iters
        self.oT, self.oR, self.old_index = pair.origin_vio_T, pair.origin_vio_R, pair.c.old_index
        self._finish(None)

    def _finish(self, control):
        self.out = tail(self.par, self.Xi, self.uvi, self.cfg, self.oT, self.oR, MP, control, self.stats if control is None else None)
        if self.par64 is not None and control is None:
            self.out64 = tail(self.par64, self.Xi, self.uvi, self.cfg, self.oT, self.oR, F64)
            if self.out64["gate"] != self.out["gate"]:
                self.stats["routes"].append(("gate",))
            self.e64 = {f: err(_vec(self.out64[f]), _vec(self.out[f])) for f in FLOATS}
        self.status = OK if self.out["gate"] else GATE
        self.has_loop, self.loop_index = (1, self.old_index) if self.out["gate"] else (0, -1)

    def with_tail_control(self, control):
        """a copy whose tail is corrupted by a control that acts after the final solve (no second RANSAC); it keeps e64"""
        assert control in TAIL_CONTROLS and self.out is not None
        o = copy.copy(self)
        o.control = control
        o._finish(control)
        return o

    def conditions(self):
        """the conditions of the module docstring, asserted on the reference alone"""
        st = self.stats
        assert st["min_band"] > BAND and st["min_round"] > BAND, st
        assert st["min_gate"] > 1e-9 and st["min_lm"] > 1e-9, st
        assert not st["basis"], st["basis"]
        assert not st["routes"], st["routes"]
        assert not st["lm_accept"], st["lm_accept"]
        assert st["dlt_gap"] < 0.5 and st["min_det"] > 1e-9, st


def _vec(v):
    return list(v) if isinstance(v, (list, tuple)) else [v]


def err(a, ref):
    """max-norm of the difference relative to the 2-norm of the 40-digit vector"""
    ref = [mpf(v) for v in ref]
    nrm = mp.sqrt(sum(r * r for r in ref))
    return float(max(abs(mpf(float(x)) - r) for x, r in zip(a, ref)) / (nrm if nrm else 1))


INTS = ("status", "n_matched", "ransac_iters", "ransac_inliers", "pnp_iterations", "n_final", "has_loop", "loop_index")


def compare(ref, res, mi, md, inl, floats=FLOATS):
    """a result record and its per-point arrays against the reference: (the integer outputs that differ, {quantity: (error, e64, floor)}).
    loop_info is compared only where the record holds it (status OK), the pose wherever the final solve ran."""
    bad = [f for f in INTS if getattr(res, f) != getattr(ref, f)]
    for name, got, want in (("match_index", mi, ref.match_index), ("match_dist", md, ref.match_dist), ("inlier", inl, ref.inlier)):
        if not np.array_equal(np.asarray(got), np.asarray(want)):
            bad.append(name)
    num = {}
    if ref.out is not None and res.status == ref.status:
        for f in floats:
            if f == "loop_info" and ref.status != OK:
                continue
            got = _vec(getattr(res, f)) if f in ("res", "loop_weight") else list(getattr(res, f))
            n = len(got)
            num[f] = (err(got, _vec(ref.out[f])), ref.e64[f], n * 2.0 ** -53)
    return bad, num


def ratios(num):
    return {k: e / max(e64, fl) for k, (e, e64, fl) in num.items()}
