"""What the solve's input kernels compute -- k_triangulate, k_imu_prep, k_vector2double (is-vins_amd/csrc/isv_linearize.hip) -- restated in
mpmath at 40 digits or more.  Test infrastructure: tests/test_prep_highprec.py holds these statements and the CPU oracle against each
other, tests/test_gpu_prep_highprec.py the kernels; the windows are tests/prep_cases.py's.

Written from the reference's text (src/feature_tracker/feature_manager.cpp:206-258, include/factor/imu_factor.h:44, Eigen's
Quaternion(Matrix3) as used by src/estimator.cpp:474-516), not from the oracle or the kernels: no Jacobi sweep, pivot order or
branch-free form of theirs appears here.  A window's doubles are read as exact numbers."""
import mpmath as mp
import numpy as np

import align_highprec as ah

TRI_DPS = 60        # working digits of triangulate_mp
INFO_DPS = 60       # working digits of information_mp


def _m(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a]) if a.ndim == 2 else mp.matrix([mp.mpf(float(x)) for x in a])


def dlt_matrix(Ps, Rs, ric, tic, host, pts, K=mp.mpf):
    """the 2k x 4 matrix svd_A of feature_manager.cpp:218-241 for one landmark seen from frames host .. host + k - 1 with the points
    `pts` [k][3]; K = mp.mpf builds it exactly-rounded at the working precision, K = float in doubles (numpy, for the float64 route)"""
    if K is float:
        Ps, Rs, ric, tic, pts = (np.asarray(x, dtype=np.float64) for x in (Ps, Rs, ric, tic, pts))
        R0, t0 = Rs[host] @ ric, Ps[host] + Rs[host] @ tic
        A = np.zeros((2 * len(pts), 4))
        for o, pt in enumerate(pts):
            j = host + o
            R1, t1 = Rs[j] @ ric, Ps[j] + Rs[j] @ tic
            t, R = R0.T @ (t1 - t0), R0.T @ R1
            P = np.hstack([R.T, (-R.T @ t)[:, None]])
            f = pt / np.sqrt(pt @ pt)
            A[2 * o], A[2 * o + 1] = f[0] * P[2] - f[2] * P[0], f[1] * P[2] - f[2] * P[1]
        return A
    ric_, tic_ = _m(ric), _m(tic)
    R0, t0 = _m(Rs[host]) * ric_, _m(Ps[host]) + _m(Rs[host]) * tic_
    A = mp.zeros(2 * len(pts), 4)
    for o, pt in enumerate(pts):
        j = host + o
        R1, t1 = _m(Rs[j]) * ric_, _m(Ps[j]) + _m(Rs[j]) * tic_
        t, R = R0.T * (t1 - t0), R0.T * R1
        Rt = R.T
        mt = Rt * t
        p = _m(pt)
        f = p / mp.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2)
        for c in range(4):
            P0, P1, P2 = (Rt[0, c], Rt[1, c], Rt[2, c]) if c < 3 else (-mt[0], -mt[1], -mt[2])
            A[2 * o, c] = f[0] * P2 - f[2] * P0
            A[2 * o + 1, c] = f[1] * P2 - f[2] * P1
    return A


def landmark_views(w, l):
    """(host frame, the k points [k][3]) of landmark l of an abi.Window"""
    o0, o1 = int(w.lm_obs_ptr[l]), int(w.lm_obs_ptr[l + 1])
    return int(w.lm_start_frame[l]), np.array(w.obs_point[o0:o1], dtype=np.float64)


def triangulate_mp(w, l, method="svd"):
    """-> (depth V[2] / V[3] of the right singular vector of svd_A's smallest singular value, [sigma_1 .. sigma_4] descending), as mpf.

    Digits and argument.  svd_A is built at TRI_DPS = 60 digits from the window's doubles (its entries are sums of products of at most
    four of them: an error of a few 1e-60).  mp.svd_r is a backward-stable one-sided Jacobi: the computed V is the exact V of a matrix
    within 1e-59 |A| of svd_A, so the singular vector of sigma_4 moves by at most 1e-59 sigma_1 / (sigma_3 - sigma_4), and the depth, a
    ratio of two of its components, by that divided by |V[3]| (>= 0.1 here: the vector is (X, 1) / |(X, 1)| with |X| <= 10 on compared
    landmarks).  Every landmark whose VALUE is compared has (sigma_3 - sigma_4) / sigma_1 >= 1e-6 (tests/prep_cases.py): the depth is
    good to 1e-52, far inside the 1e-25 asked for.  method = "gram" is the independent second route of tests/test_prep_highprec.py:
    the eigenvectors of svd_A^T svd_A by mp.eigsy at 100 digits, where the 2 log10(sigma_1 / sigma_3) <= 12 digits that squaring costs
    are still spare; the two agree to 1e-40 on every fourth landmark of the table."""
    host, pts = landmark_views(w, l)
    with mp.workdps(TRI_DPS if method == "svd" else 100):
        A = dlt_matrix(w.Ps, w.Rs, w.ric, w.tic, host, pts)
        if method == "svd":
            _, S, V = mp.svd_r(A)                                   # A = U diag(S) V, rows of V are the right singular vectors
            order = sorted(range(4), key=lambda i: S[i], reverse=True)
            v = [V[order[3], c] for c in range(4)]
            sig = [+S[i] for i in order]
        else:
            E, Q = mp.eigsy(A.T * A)
            order = sorted(range(4), key=lambda i: E[i], reverse=True)
            v = [Q[c, order[3]] for c in range(4)]
            sig = [mp.sqrt(abs(E[i])) for i in order]
        return v[2] / v[3], sig


def triangulate_f64(w, l):
    """the same svd_A in doubles and numpy.linalg.svd (LAPACK gesdd): one of the two SVD-class double-precision routes e_ref is taken from"""
    host, pts = landmark_views(w, l)
    A = dlt_matrix(w.Ps, w.Rs, w.ric, w.tic, host, pts, K=float)
    v = np.linalg.svd(A)[2][3]
    return float(v[2] / v[3])


# ---- IMU weight: sqrt_info = LLT(covariance^-1).matrixL().transpose()  (imu_factor.h:44) -----------------------------------------------
def information_mp(cov):
    """-> (cov^-1, U) as mp matrices at INFO_DPS digits: U upper triangular with positive diagonal and U^T U = cov^-1.  Eigen's LLT reads
    the lower triangle of its argument only; cov^-1 of a covariance that is symmetric to the last bit but one is symmetric to
    cond * 2^-52, and the lower triangle is what is factored here too.  cond(cov) <= 2e8 on the cases: 60 digits leave 50."""
    with mp.workdps(INFO_DPS):
        n = len(cov)
        Inv = mp.inverse(_m(cov))
        L = mp.zeros(n, n)
        for j in range(n):
            d = Inv[j, j] - mp.fsum(L[j, k] ** 2 for k in range(j))
            assert d > 0, "cov^-1 is not positive definite"
            L[j, j] = mp.sqrt(d)
            for i in range(j + 1, n):
                L[i, j] = (Inv[i, j] - mp.fsum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
        return Inv, L.T


def to_np(M):
    return np.array([[float(M[a, b]) for b in range(M.cols)] for a in range(M.rows)])


def information_f64(cov):
    """the two double-precision routes to (cov^-1, U): (a) numpy.linalg.inv (LAPACK getrf / getri: LU with partial pivoting) then
    numpy.linalg.cholesky (potrf) of its lower triangle -- the algorithm class of the reference's LLT(cov.inverse()) (Eigen itself is not
    available to the tests); (b) Cholesky of cov, a triangular inversion (trtrs), cov^-1 = C^-T C^-1, and potrf of that"""
    from scipy.linalg import solve_triangular
    cov = np.asarray(cov, dtype=np.float64)
    Ia = np.linalg.inv(cov)
    Ua = np.linalg.cholesky(np.tril(Ia) + np.tril(Ia, -1).T).T
    Ci = solve_triangular(np.linalg.cholesky(cov), np.eye(len(cov)), lower=True)
    Ib = Ci.T @ Ci
    Ub = np.linalg.cholesky(Ib).T
    return (Ia, Ua), (Ib, Ub)


# ---- vector2double: Eigen::Quaterniond(Matrix3d) ----------------------------------------------------------------------------------------
ARMS = ("trace", "x", "y", "z")


def quat_arm(R):
    """(arm, tie) of Eigen's matrix -> quaternion conversion, decided on the EXACT entries of the doubles R [3][3]: arm in ARMS;
    tie = "xy" when m00 == m11 decides between the x and the y arm (>= keeps x), "yz" when m11 == m22 decides between y and z, else None"""
    m = [[mp.mpf(float(R[a][b])) for b in range(3)] for a in range(3)]
    with mp.workdps(60):                                              # (three doubles add exactly at 60 digits)
        if m[0][0] + m[1][1] + m[2][2] > 0:
            return "trace", None
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    tie = None
    if i == 0 and m[0][0] == m[1][1] and m[0][0] >= m[2][2]:
        tie = "xy"
    if i == 1 and m[1][1] == m[2][2]:
        tie = "yz"
    return ARMS[1 + i], tie


def quat_mp(R):
    """Eigen's Quaterniond(Matrix3d) on the doubles R [3][3] -> (x, y, z, w) as mpf, the arm chosen on the exact entries and the signs as
    that arm gives them (no canonical sign).  The arithmetic is tests/align_highprec.py's _q_from_R in its mpmath instance."""
    with mp.workdps(50):
        m = [[mp.mpf(float(R[a][b])) for b in range(3)] for a in range(3)]
        q = ah._q_from_R(ah.MP, m)
        return [+q[1], +q[2], +q[3], +q[0]]


# One arm of the conversion, in rounding units u = 2^-53, on a rotation matrix R (|entries| <= 1).  The radicand s = 4 q_i^2 with q_i the
# arm's own component: on the trace arm w^2 > 1/4, on the others w^2 <= 1/4 and q_i^2 is the largest of three that sum to >= 3/4: s in [1, 4].
#   s = m_ii - m_jj - m_kk + 1 (trace arm: m_00 + m_11 + m_22 + 1): three additions whose results are <= 2, 3 and 4 in size,
#                                each rounded once: (2 + 3 + 4) u absolute, and s >= 1 .............. 9 u relative
#   t = sqrt(s): half the relative error of s, and its own rounding .................................. 5.5 u relative
#   the arm's own component 0.5 t (exact scaling, value <= 1) ......................................... 5.5 u absolute
#   r = 0.5 / t: t's error and the division's rounding ................................................ 6.5 u relative
#   another component (m_ab +- m_ba) * r: the sum rounds by u relative, the product by u: 8.5 u relative
#                                on a quaternion component, <= 1 ...................................... 8.5 u absolute
# QUAT_ATOL is the largest line rounded up to a whole count: 9 u = 1.0e-15, absolute, per component.  (No product feeds an addition here,
# so fused multiply-add contraction changes nothing.)
QUAT_ATOL = 9 * 2.0 ** -53
