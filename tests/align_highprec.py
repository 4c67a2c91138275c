"""The visual-inertial alignment (is-vins_amd/csrc/isv_initial.h: solveGyroscopeBias, LinearAlignment, RefineGravity, g2R and the state
rebuild of visualInitialAlign) recomputed at 40 digits in mpmath, STAGE BY STAGE, with the error float64 allows at each stage.  Test
infrastructure: tests/test_align_highprec.py holds the CPU restatement (tests/native/isv_init_oracle.c) against it, and
tests/test_gpu_align_highprec.py the kernel k_visual_imu_align.  The cases, their conditions and the negative controls are
tests/align_cases.py's.

Written from the reference's equations (src/initial/initial_aligment.cpp:3-208, src/estimator.cpp:357-429, src/utility/utility.cpp:3-13)
with the quirks Q1-Q3 of isv_initial.h -- not from the kernel or the C file: a frame pair is one 6 x m block row H and its right-hand side
z, the normal equations are the sum of H^T H scattered through ONE index list (the pair's six velocity unknowns, then the shared
gravity / scale unknowns), and the solve is an exact one.  No pivoting order, packing or summation order of the kernel appears here.

Every stage is recomputed from the inputs of that stage AS FOUND IN THE RESULT UNDER TEST, read as exact doubles, so the stages' errors
do not compound:

  stage      inputs                                                                  compared outputs
  gyro       frames' R, delta_q, jac_rr                                              delta_bg; Bgs = Bgs_in + the result's delta_bg
  linear     frames' R, T, tic, the result's rp_delta_p / rp_delta_v / rp_sum_dt     g_linear, s_linear
  refine     the same, and the result's g_linear                                     x[:3 nf + 3] (last entry / 100), g_c0
  rebuild    the result's x and g_c0, frames' R, T, tic, window_frame, keyframe map  s, g, R0, Ps, Rs, Vs

The limits.  For a solve A x = b the componentwise first-order limit of float64 is

    lim = 2^-52 (|A^-1| |A| |x| + |A^-1| |b|)

with A, b, x from the 40-digit model (|A^-1| from float64 numpy: a limit need not be exact).  The margin on the three solve stages is 1:
the limit is the bound.

  linear   lim, per component (s_linear = x[n-1] / 100: lim[n-1] / 100).
  refine   x: the LAST pass's lim (Q2: its matrix is 1000 (previous + this pass), so it carries every pass).  g_c0: |lxly| lim[n-3:n-1]
           + 2^-52 * 4 * |G| for the final normalisation and scaling.
  gyro     delta_bg: lim of the 3 x 3 system + 2^-52 * C_QUAT * |A^-1| sum_i |J_i|^T (1,1,1)^T.  The second term is the rounding of
           the residual r_i = -2 vec(q_ij^-1 (x) delta_q): its components are differences of products of unit quaternions and carry an
           ABSOLUTE error whatever their size (they vanish on exact data).  C_QUAT counts the operations on that path in units of
           u = 2^-53 on quantities bounded by 1:
             R_i^T R_j, a 3-term product sum ........................... 3 u per entry
             q_from_R (trace branch): t + 1 from three such entries and three additions 19 u on a value in (1, 4], its root 10.5 u
               relative, 0.5 / root 11.5 u; a vector component (m_ab - m_ba) * (0.5 / root) is (2 * 3 + 2) u * 0.5 + 11.5 u + u
               = 16.5 u, w is 10.5 u: at most 31 u in the 2-norm
             q^-1 = conj / |q|^2: the inversion is an isometry at |q| = 1, its own four products, three additions and division 5 u
             the 4-term quaternion product with the unit delta_q ...... 4 u per component
             the factor -2 (exact) ...................................... (31 + 5 + 4) * 2 = 80 u = 40 * 2^-52
           so C_QUAT = 40.  Bgs: one rounding of the exact sum, in the unit of every other limit: 2^-52 |Bgs_in + delta_bg|.
  rebuild  closed form, no solve: per field 16 x max(error of the float64 evaluation against the 40 digits, 2^-52 max(1, max|field|)).
           16 is one order of magnitude for the difference between two correct float64 orderings of a chain of about 30 operations,
           atan2 / sin / cos included, where the device's and glibc's libm differ in the last bits.

The model follows q_from_R's branch on the exact R_i^T R_j (the trace is near 3 on every case; the kernel's rounded trace takes the same
branch) and, like the kernel, does not normalise q_ij or delta_q.  TangentBasis' `a == (0,0,1)` is tested on the exact a.

Exact solves: mp.lu_solve up to LU_MAX_N unknowns (it would do up to about 70, at a second per solve: too slow for the 5 solves of a
case and the 14 of its controls; at n = 123 / 124 it is out of the question) and iterative refinement above -- the residual in mpmath,
the correction from a float64 numpy.linalg.solve, until the correction is below 1e-35 relative.  tests/test_align_highprec.py shows once
that the two agree to 1e-30 up to n = 64.  Every solve returns its residual |A x - b| / |b| and cond2(A) for the conditions of
tests/align_cases.py.

Beside the 40 digits every stage is evaluated once more in plain float64 (Python floats are IEEE doubles; numpy.linalg.solve for the
systems) from the same stage inputs: its distance from the model in units of the limit says whether the limit FORMULA is adequate
without asking the code under test (tests/test_align_highprec.py: at most 1/2, for it and for the restatement).  It runs the model's own
formulas in the other arithmetic, with another solver: it checks the LIMITS, not the model.  The model is checked by the restatement and
the kernel, which share no line with it, and by the negative controls."""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 40
EPS = 2.0 ** -52
C_QUAT = 40.0
LU_MAX_N = 16
STAGES = ("gyro", "linear", "refine", "rebuild")
# the corruptions of the MODEL that the negative controls use (tests/align_cases.py), and the stages each one reaches
CONTROLS = {"q2_off": ("refine",), "drop_last_pair_tail": ("linear", "refine"), "jac_transposed": ("gyro",),
            "scale_100_dropped": ("linear", "refine"), "q3_frame_index": ("rebuild",)}


class _Arith:
    def __init__(self, num, sqrt, atan2, sin, cos, pi):
        self.num, self.sqrt, self.atan2, self.sin, self.cos, self.pi = num, sqrt, atan2, sin, cos, pi


MP = _Arith(mp.mpf, mp.sqrt, mp.atan2, mp.sin, mp.cos, +mp.pi)
F64 = _Arith(float, math.sqrt, math.atan2, math.sin, math.cos, math.pi)


class Inputs:
    """what the alignment reads of an initial.Problem, as numpy doubles"""

    def __init__(self, p):
        c, fr = p.c, p.frames
        self.nf, self.nw = c.n_frames, c.n_window
        self.R = [np.array(fr[f].R, dtype=np.float64).reshape(3, 3) for f in range(self.nf)]
        self.T = [np.array(fr[f].T, dtype=np.float64) for f in range(self.nf)]
        self.dq = [np.array(fr[f].delta_q, dtype=np.float64) for f in range(self.nf)]            # x y z w
        self.J = [np.array(fr[f].jac_rr, dtype=np.float64).reshape(3, 3) for f in range(self.nf)]
        self.tic, self.G = np.array(c.tic, dtype=np.float64), np.array(c.G, dtype=np.float64)
        self.Bgs = np.array([list(c.Bgs[i]) for i in range(self.nw)], dtype=np.float64)
        self.win = [int(c.window_frame[i]) for i in range(self.nw)]
        # the keyframes after visualInitialAlign marked the window's frames (estimator.cpp:369-376), in all_image_frame order
        self.kf = [f for f in range(self.nf) if f in self.win or fr[f].is_key_frame]


def result_values(inp, res):
    """the compared outputs of a result record, {field: flat float64 array}, and the stage inputs it carries"""
    nf, nw = inp.nf, inp.nw
    v = {k: res.arr(k).ravel() for k in ("delta_bg", "g_linear", "g_c0", "g", "R0")}
    for k in ("Bgs", "Ps", "Rs", "Vs"):
        v[k] = res.arr(k)[:nw].ravel()
    v["x"] = res.arr("x")[:3 * nf + 3]
    v["s_linear"], v["s"] = np.array([res.s_linear]), np.array([res.s])
    v["rp_delta_p"], v["rp_delta_v"], v["rp_sum_dt"] = res.arr("rp_delta_p")[:nf], res.arr("rp_delta_v")[:nf], res.arr("rp_sum_dt")[:nf]
    return v


# ---- small dense helpers on nested lists of either arithmetic ---------------------------------------------------------------------------
def _mat(K, a):
    return [[K.num(float(v)) for v in row] for row in a]


def _vec(K, a):
    return [K.num(float(v)) for v in a]


def _tr(A):
    return [list(r) for r in zip(*A)]


def _mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def _norm(K, v):
    return K.sqrt(sum(c * c for c in v))


def _flat(a):
    return [v for row in a for v in row]


def _f64(a):
    return np.array([float(v) for v in a], dtype=np.float64)


# ---- exact solves and the float64 limit ------------------------------------------------------------------------------------------------
def residual(A, b, x):
    """max |A x - b| / max |b| in mpmath"""
    r = max(abs(mp.fdot(A[i], x) - b[i]) for i in range(len(b)))
    return float(r / max(abs(v) for v in b))


def solve_lu(A, b):
    x = mp.lu_solve(mp.matrix(A), mp.matrix(b))
    return [x[i] for i in range(len(b))]


def solve_refined(A, b, A64=None):
    """iterative refinement: residual in mpmath, correction from numpy.linalg.solve of the float64 matrix, to 1e-35 relative"""
    n = len(b)
    A64 = np.array([[float(v) for v in row] for row in A]) if A64 is None else A64
    x = [mp.mpf(float(v)) for v in np.linalg.solve(A64, _f64(b))]
    nz = [[j for j, v in enumerate(row) if v != 0] for row in A]      # (the velocity rows hold a dozen entries each)
    Anz = [[row[j] for j in cols] for row, cols in zip(A, nz)]
    for it in range(80):
        r = [b[i] - mp.fdot(Anz[i], [x[j] for j in nz[i]]) for i in range(n)]
        scale = max(abs(v) for v in r)
        if scale == 0:
            return x
        d = np.linalg.solve(A64, _f64([v / scale for v in r]))        # (the residual is scaled so that it cannot underflow)
        dx = [scale * mp.mpf(float(v)) for v in d]
        x = [x[i] + dx[i] for i in range(n)]
        if max(abs(v) for v in dx) <= mp.mpf("1e-35") * max(abs(v) for v in x):
            return x
    raise AssertionError("refinement did not converge")


class Solve:
    """A x = b at 40 digits: x (mpf list), lim (the componentwise float64 limit), cond2(A), the residual, |A^-1| in float64"""

    def __init__(self, A, b, method=None):
        n = len(b)
        self.A, self.b = A, b
        self.A64 = np.array([[float(v) for v in row] for row in A])
        self.b64 = _f64(b)
        method = method or ("lu" if n <= LU_MAX_N else "refined")
        self.x = solve_lu(A, b) if method == "lu" else solve_refined(A, b, self.A64)
        self.resid = residual(A, b, self.x)
        self.cond = float(np.linalg.cond(self.A64))
        self.absinv = np.abs(np.linalg.inv(self.A64))
        x64 = _f64(self.x)
        self.lim = EPS * (self.absinv @ (np.abs(self.A64) @ np.abs(x64)) + self.absinv @ np.abs(self.b64))


class Stage:
    """one stage's 40-digit outputs `exact` {field: mpf list}, their limits `lim` {field: array}, the plain float64 evaluation `e64`
    {field: array}, and the Solve records of its systems"""

    def __init__(self, name):
        self.name, self.exact, self.lim, self.e64, self.solves = name, {}, {}, {}, []

    def errors(self, values):
        """{field: |values - exact| as float64 array}"""
        return {k: _f64([abs(mp.mpf(float(values[k][i])) - e) for i, e in enumerate(ex)]) for k, ex in self.exact.items()}

    def ratios(self, values):
        """{field: the worst |values - exact| / lim}; a zero limit allows a zero error only"""
        out = {}
        for k, e in self.errors(values).items():
            lim = np.broadcast_to(self.lim[k], e.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(e == 0.0, 0.0, np.where(lim > 0, e / lim, np.inf))
            out[k] = float(r.max())
        return out

    def moved(self, other):
        """the worst |other.exact - exact| / lim over the fields: how far a corrupted model lies from this one, in limits"""
        w = 0.0
        for k, ex in self.exact.items():
            d = _f64([abs(a - b) for a, b in zip(ex, other.exact[k])])
            lim = np.broadcast_to(self.lim[k], d.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                w = max(w, float(np.where(d == 0.0, 0.0, np.where(lim > 0, d / lim, np.inf)).max()))
        return w


# ---- gyro bias (initial_aligment.cpp:3-37, quirk Q1) -----------------------------------------------------------------------------------
def _q_from_R(K, m):
    """Eigen's matrix -> quaternion (w, x, y, z)"""
    t = m[0][0] + m[1][1] + m[2][2]
    if t > 0:
        s = K.sqrt(t + 1)
        f = 1 / (2 * s)
        return [s / 2, (m[2][1] - m[1][2]) * f, (m[0][2] - m[2][0]) * f, (m[1][0] - m[0][1]) * f]
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    s = K.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
    f = 1 / (2 * s)
    q = [0, 0, 0, 0]
    q[0], q[1 + i], q[1 + j], q[1 + k] = (m[k][j] - m[j][k]) * f, s / 2, (m[j][i] + m[i][j]) * f, (m[k][i] + m[i][k]) * f
    return q


def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def _gyro_system(K, inp, control):
    A, b = [[K.num(0)] * 3 for _ in range(3)], [K.num(0)] * 3
    for i in range(inp.nf - 1):
        q = _q_from_R(K, _mm(_tr(_mat(K, inp.R[i])), _mat(K, inp.R[i + 1])))
        n2 = sum(c * c for c in q)
        d = _vec(K, inp.dq[i + 1])
        e = _qmul([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2], [d[3], d[0], d[1], d[2]])
        r = [-2 * e[1], -2 * e[2], -2 * e[3]]
        J = _mat(K, inp.J[i + 1].T if control == "jac_transposed" else inp.J[i + 1])
        Jt = _tr(J)
        JtJ, Jtr = _mm(Jt, J), _mv(Jt, r)
        A = [[A[a][c] + JtJ[a][c] for c in range(3)] for a in range(3)]
        b = [b[a] + Jtr[a] for a in range(3)]
    return A, b


def stage_gyro(inp, val, control=None):
    st = Stage("gyro")
    A, b = _gyro_system(MP, inp, control)
    sv = Solve(A, b, "lu")
    st.solves.append(sv)
    sumJ = sum(np.abs((J.T if control == "jac_transposed" else J).T) @ np.ones(3) for J in inp.J[1:])
    st.exact["delta_bg"], st.lim["delta_bg"] = sv.x, sv.lim + EPS * C_QUAT * (sv.absinv @ sumJ)
    dbg = _vec(MP, val["delta_bg"])
    st.exact["Bgs"] = [mp.mpf(float(inp.Bgs[i][k])) + dbg[k] for i in range(inp.nw) for k in range(3)]
    st.lim["Bgs"] = EPS * np.abs(_f64(st.exact["Bgs"]))
    A64, b64 = _gyro_system(F64, inp, control)
    st.e64["delta_bg"] = np.linalg.solve(np.array(A64), np.array(b64))
    st.e64["Bgs"] = (inp.Bgs + np.asarray(val["delta_bg"])[None, :]).ravel()
    return st


# ---- the frame pairs of LinearAlignment (:128-181) and of a RefineGravity pass (:70-114) ------------------------------------------------
def _pair(K, inp, val, i, lxly, g0, control):
    """(H, z): the 6 x m block row of frame pair (i, i+1) on its unknowns [v_i, v_j, gravity (3, or 2 on the tangent basis), 100 s]"""
    j = i + 1
    dt = K.num(float(val["rp_sum_dt"][j]))
    dp, dv = _vec(K, val["rp_delta_p"][j]), _vec(K, val["rp_delta_v"][j])
    RiT = _tr(_mat(K, inp.R[i]))
    Rij = _mm(RiT, _mat(K, inp.R[j]))
    tic = _vec(K, inp.tic)
    Ti, Tj = _vec(K, inp.T[i]), _vec(K, inp.T[j])
    sc = _mv(RiT, [Tj[k] - Ti[k] for k in range(3)])
    if control != "scale_100_dropped":
        sc = [v / 100 for v in sc]
    ctic = _mv(Rij, tic)
    half = dt * dt / 2
    B = RiT if lxly is None else _mm(RiT, lxly)          # the gravity unknowns' basis, seen from body i
    ng = len(B[0])
    m = 6 + ng + 1
    H = [[K.num(0)] * m for _ in range(6)]
    z = [K.num(0)] * 6
    Rg = [K.num(0)] * 3 if g0 is None else _mv(RiT, g0)
    for a in range(3):
        H[a][a], H[3 + a][a] = -dt, K.num(-1)
        for c in range(3):
            H[3 + a][3 + c] = Rij[a][c]
        for c in range(ng):
            H[a][6 + c], H[3 + a][6 + c] = B[a][c] * half, B[a][c] * dt
        H[a][m - 1] = sc[a]
        z[a] = dp[a] + ctic[a] - tic[a] - Rg[a] * half
        z[3 + a] = dv[a] - Rg[a] * dt
    return H, z


def _add_pairs(K, inp, val, A, b, lxly, g0, control):
    """A += sum of H^T H, b += sum of H^T z over the frame pairs, through the pair's index list"""
    n = len(b)
    for i in range(inp.nf - 1):
        H, z = _pair(K, inp, val, i, lxly, g0, control)
        m = len(H[0])
        idx = list(range(3 * i, 3 * i + 6)) + list(range(n - (m - 6), n))
        cut = control == "drop_last_pair_tail" and i == inp.nf - 2
        cols = _tr(H)
        rows = [[r for r in range(6) if c[r] != 0] for c in cols]     # (a velocity column holds one or three entries)
        for p in range(m):
            for q in range(m):
                if not (cut and p >= 6 and q >= 6):
                    A[idx[p]][idx[q]] += sum(cols[p][r] * cols[q][r] for r in rows[p] if cols[q][r] != 0)
            if not (cut and p >= 6):
                b[idx[p]] += sum(cols[p][r] * z[r] for r in rows[p])


def _zeros(K, n):
    return [[K.num(0)] * n for _ in range(n)], [K.num(0)] * n


def _times_1000(A, b):
    return [[v * 1000 for v in row] for row in A], [v * 1000 for v in b]


def stage_linear(inp, val, control=None):
    st = Stage("linear")
    n = 3 * inp.nf + 4
    out = {}
    for K in (MP, F64):
        A, b = _zeros(K, n)
        _add_pairs(K, inp, val, A, b, None, None, control)
        A, b = _times_1000(A, b)
        if K is MP:
            sv = Solve(A, b)
            st.solves.append(sv)
            st.exact["g_linear"], st.lim["g_linear"] = sv.x[n - 4:n - 1], sv.lim[n - 4:n - 1]
            st.exact["s_linear"], st.lim["s_linear"] = [sv.x[n - 1] / 100], sv.lim[n - 1:] / 100
        else:
            x = np.linalg.solve(np.array(A), np.array(b))
            st.e64["g_linear"], st.e64["s_linear"] = x[n - 4:n - 1], x[n - 1:] / 100
    return st


# ---- RefineGravity (:55-123, quirk Q2) -------------------------------------------------------------------------------------------------
def _tangent_basis(K, g0):
    """lxly (3 x 2): an orthonormal basis of the plane across g0 (TangentBasis, :40-53)"""
    na = _norm(K, g0)
    a = [v / na for v in g0]
    tmp = [K.num(0), K.num(0), K.num(1)]
    if a == tmp:
        tmp = [K.num(1), K.num(0), K.num(0)]
    d = sum(a[k] * tmp[k] for k in range(3))
    t = [tmp[k] - a[k] * d for k in range(3)]
    nt = _norm(K, t)
    bb = [v / nt for v in t]
    cc = [a[1] * bb[2] - a[2] * bb[1], a[2] * bb[0] - a[0] * bb[2], a[0] * bb[1] - a[1] * bb[0]]
    return [[bb[k], cc[k]] for k in range(3)]


def _refine(K, inp, val, control, st=None):
    n = 3 * inp.nf + 3
    Gn = _norm(K, _vec(K, inp.G))
    g = _vec(K, val["g_linear"])
    ng = _norm(K, g)
    g0 = [v / ng * Gn for v in g]
    A, b = _zeros(K, n)
    for k in range(4):
        if control == "q2_off":
            A, b = _zeros(K, n)
        lxly = _tangent_basis(K, g0)
        _add_pairs(K, inp, val, A, b, lxly, g0, control)
        A, b = _times_1000(A, b)
        if K is MP:
            sv = Solve(A, b)
            st.solves.append(sv)
            x = sv.x
        else:
            x = [float(v) for v in np.linalg.solve(np.array(A), np.array(b))]
        gn = [g0[a] + lxly[a][0] * x[n - 3] + lxly[a][1] * x[n - 2] for a in range(3)]
        nn = _norm(K, gn)
        g0 = [v / nn * Gn for v in gn]
    return x[:n - 1] + [x[n - 1] / 100], g0, lxly, Gn


def stage_refine(inp, val, control=None):
    st = Stage("refine")
    n = 3 * inp.nf + 3
    x, g0, lxly, Gn = _refine(MP, inp, val, control, st)
    lim = st.solves[-1].lim
    st.exact["x"], st.lim["x"] = x, np.concatenate([lim[:n - 1], lim[n - 1:] / 100])
    L = np.abs(np.array([[float(v) for v in row] for row in lxly]))
    st.exact["g_c0"], st.lim["g_c0"] = g0, L @ lim[n - 3:n - 1] + EPS * 4 * float(Gn)
    x64, g64, _, _ = _refine(F64, inp, val, control)
    st.e64["x"], st.e64["g_c0"] = np.array(x64), np.array(g64)
    return st


# ---- g2R (utility.cpp:3-13) and the state rebuild (estimator.cpp:367-429, quirk Q3) ----------------------------------------------------
def _remove_yaw(K, R, of):
    """ypr2R(-yaw(of), 0, 0) * R, the yaw in degrees as Utility::R2ypr returns it"""
    yaw = K.atan2(of[1][0], of[0][0]) / K.pi * 180
    y = -yaw / 180 * K.pi
    c, s = K.cos(y), K.sin(y)
    return _mm([[c, -s, K.num(0)], [s, c, K.num(0)], [K.num(0), K.num(0), K.num(1)]], R)


def _rebuild(K, inp, val, control):
    nf, nw = inp.nf, inp.nw
    x, g = _vec(K, val["x"]), _vec(K, val["g_c0"])
    s = x[3 * nf + 2]
    R = [_mat(K, inp.R[f]) for f in range(nf)]
    tic = _vec(K, inp.tic)
    # the rotation that takes g / |g| to z (Quaterniond::FromTwoVectors), then its yaw removed
    ng = _norm(K, g)
    v0 = [v / ng for v in g]
    sq = K.sqrt((1 + v0[2]) * 2)
    w, qx, qy, qz = sq / 2, v0[1] / sq, -v0[0] / sq, K.num(0)
    R0 = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * w), 2 * (qx * qz + qy * w)],
          [2 * (qx * qy + qz * w), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * w)],
          [2 * (qx * qz - qy * w), 2 * (qy * qz + qx * w), 1 - 2 * (qx * qx + qy * qy)]]
    R0 = _remove_yaw(K, R0, R0)
    R0 = _remove_yaw(K, R0, _mm(R0, R[inp.win[0]]))
    cam = [[s * K.num(float(inp.T[f][k])) - rt for k, rt in enumerate(_mv(R[f], tic))] for f in inp.win]
    Ps = [_mv(R0, [cam[i][k] - cam[0][k] for k in range(3)]) for i in range(nw)]
    Rs = [_flat(_mm(R0, R[f])) for f in inp.win]
    Vs = []
    for kv, f in enumerate(inp.kf):
        o = 3 * (f if control == "q3_frame_index" else kv)       # Q3: the keyframe COUNTER indexes x
        Vs.append(_mv(R0, _mv(R[f], x[o:o + 3])))
    return {"s": [s], "g": _mv(R0, g), "R0": _flat(R0), "Ps": _flat(Ps), "Rs": _flat(Rs), "Vs": _flat(Vs)}


def stage_rebuild(inp, val, control=None):
    st = Stage("rebuild")
    st.exact = _rebuild(MP, inp, val, control)
    st.yardstick = {}
    for k, v in _rebuild(F64, inp, val, control).items():
        st.e64[k] = np.array(v)
    for k, e in st.errors(st.e64).items():
        st.yardstick[k] = max(float(e.max()), EPS * max(1.0, float(np.abs(_f64(st.exact[k])).max())))
        st.lim[k] = np.float64(16.0 * st.yardstick[k])
    return st


_STAGE_FN = {"gyro": stage_gyro, "linear": stage_linear, "refine": stage_refine, "rebuild": stage_rebuild}


def model(inp, val, stages=STAGES, control=None):
    """{stage: Stage} recomputed from the stage inputs in `val` (result_values of the result under test); `control`: one of CONTROLS"""
    return {s: _STAGE_FN[s](inp, val, control) for s in stages}

