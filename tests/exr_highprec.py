"""A 40-digit (mpmath) reading of the rotation calibration's definitions (include/isvins_exrot.h), stage by stage from the inputs the
code actually used, after the method of tests/align_highprec.py and tests/relpose_highprec.py.  Each check returns (error, limit):
`error` is the code's distance from the 40-digit value and `limit` is the float64 limit of that solve WITHOUT its constant K, so that
error / limit is the ratio tests/test_exr_highprec.py measures on the CPU and exr_cases.K bounds for the CPU and the GPU alike.

  fundamental    the kept F, as a unit 9-vector, against the exact null space of the 7 x 9 system of the subset it came from (the
                 float32 correspondences, which are exact inputs): the norm of its component in the row space.  The limit of a null
                 space is eps * sigma_1 / sigma_7 of that system.
  rotation       Rc^T against the four matrices +-U W Vt, +-U Wt Vt of the exact SVD of the code's own F (decomposeE takes no care of
                 the sign): the smallest largest-entry difference.  The limit is eps * sigma_1 / (sigma_2 - sigma_3): the products U W Vt
                 and U Wt Vt do not see the gap between the two large singular values (W commutes with a rotation of the plane of
                 u1, u2, which a near-essential F leaves almost free), only the one to the third.  Where the scene is clean and the estimator took the true root, Rc is
                 also within float32's reach of the true relative rotation.
  rows           Rimu and Rc_g = ric^-1 Rimu ric from delta_q and the ric from BEFORE the call; the angle between Rc and Rc_g and the
                 weight.  Limits: eps * (|ric^-1| |Rimu| |ric|) for the matrices' entries, eps * max(angle, 180 / pi) for the angle
                 in degrees, a fifth of that for the weight (d(5 / a) <= da / 5 beyond 5 degrees).
  svd            singular[] and ric against the exact SVD of the A the code built (exr_oracle.build_A of the slot's history, read
                 back with read_slot): limits eps * sigma_1 for the values, eps * sigma_1 / (sigma_3 - sigma_4) for the vector; ric's
                 entries are quadratic in the unit vector, which costs a factor 4.  A single frame's A has its singular values in
                 equal pairs: the vector is then not determined, the limit is infinite and nothing is asserted of ric.
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 40
EPS = 2.0 ** -52
W = mp.matrix([[0, -1, 0], [1, 0, 0], [0, 0, 1]])          # initial_ex_rotation.cpp:131-133, not solve_5pts.cpp's


def M(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a.reshape(a.shape[0], -1)])


def maxabs(X):
    return max(abs(v) for v in X)


def q_from_R(m):
    """Eigen 3.3's matrix-to-quaternion, (w, x, y, z), in 40 digits"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = [mp.mpf(0)] * 4
    if t > 0:
        t = mp.sqrt(t + 1)
        q[0] = t / 2
        t = 1 / (2 * t)
        q[1], q[2], q[3] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = mp.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        q[1 + i] = t / 2
        t = 1 / (2 * t)
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def q_to_R(q):
    w, x, y, z = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def q_mul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def check_F(F, pts7):
    """F [3][3] the code kept; pts7 [7][4] the float32 correspondences of its subset, as doubles"""
    rows = mp.matrix(9, 9)
    for i, (x0, y0, x1, y1) in enumerate(np.asarray(pts7, np.float64)):
        x0, y0, x1, y1 = (mp.mpf(float(v)) for v in (x0, y0, x1, y1))
        for k, v in enumerate((x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, mp.mpf(1))):
            rows[i, k] = v
    U, S, V = mp.svd_r(rows)                                    # rows = U diag(S) V, V's rows the right singular vectors
    f = M(np.asarray(F).reshape(9, 1))
    f = f / mp.norm(f)
    comp = [sum(V[r, k] * f[k] for k in range(9)) for r in range(7)]
    return float(mp.sqrt(sum(c * c for c in comp))), float(EPS * S[0] / S[6])


def rotations_of(F):
    """the exact U W Vt, U Wt Vt of F and its singular values"""
    U, S, V = mp.svd_r(M(F))
    return U * W * V, U * W.T * V, S


def check_Rc(Rc, F, control=None):
    """Rc [3][3] of the result against the exact decomposition of the code's F.  control "transposed": Rc is taken without the
    transpose of initial_ex_rotation.cpp:92-94."""
    R1, R2, S = rotations_of(F)
    got = M(Rc) if control == "transposed" else M(Rc).T
    err = min(maxabs(got - s * R) for R in (R1, R2) for s in (1, -1))
    gap = S[1] - S[2]
    return float(err), float(EPS * S[0] / gap)


def check_rows(ric_before, dq, Rc, Rimu, Rc_g, angle_deg, huber):
    """one frame's rows from the ric before the call: {name: (error, limit)}"""
    ric = M(ric_before)
    q = [mp.mpf(float(v)) for v in dq]
    Ri = q_to_R(q)
    inv = ric ** -1
    Rg = inv * Ri * ric
    scale = mp.norm(inv, mp.inf) * mp.norm(Ri, mp.inf) * mp.norm(ric, mp.inf)
    out = {"Rimu": (float(maxabs(M(Rimu) - Ri)), float(EPS * mp.norm(Ri, mp.inf))), "Rc_g": (float(maxabs(M(Rc_g) - Rg)), float(EPS * scale))}
    # the angle and the weight from the matrices the code stored (its own inputs to this stage)
    r1, r2 = q_from_R(M(Rc)), q_from_R(M(Rc_g))
    d = q_mul(r1, [r2[0], -r2[1], -r2[2], -r2[3]])
    ang = 180 / mp.pi * 2 * mp.atan2(mp.sqrt(d[1] ** 2 + d[2] ** 2 + d[3] ** 2), abs(d[0]))
    hub = 5 / ang if ang > 5 else mp.mpf(1)
    lim = EPS * max(float(ang), 180 / np.pi)
    out["angle"] = (float(abs(ang - mp.mpf(float(angle_deg)))), lim)
    out["huber"] = (float(abs(hub - mp.mpf(float(huber)))), lim / 5)
    out["near_5"] = abs(float(ang) - 5.0) < 1e-9               # the weight's branch is then not decided in float64
    return out


def check_svd(A, singular, ric):
    """A [rows][4] as the code built it: {"sigma": (error, limit), "ric": (error, limit)}; ric's limit is inf for an undetermined vector"""
    U, S, V = mp.svd_r(M(A))
    s = [S[k] for k in range(4)]
    out = {"sigma": (float(max(abs(mp.mpf(float(singular[k])) - s[k]) for k in range(4))), float(EPS * s[0]) if s[0] > 0 else EPS)}
    x = [V[3, k] for k in range(4)]                            # (x, y, z, w)
    R = q_to_R([x[3], x[0], x[1], x[2]]) ** -1
    gap = s[2] - s[3]
    lim = float("inf") if gap <= 16 * EPS * s[0] else float(4 * EPS * s[0] / gap)
    out["ric"] = (float(maxabs(M(np.asarray(ric, np.float64).reshape(3, 3)) - R)), lim)
    return out


def swapped_A(hist):
    """the control "swapped L / R sign": A from a slot's history with L = w I - skew and R = w I + skew (huber 1)"""
    def blk(q, sign):
        w, x, y, z = q
        S = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        m = np.zeros((4, 4))
        m[:3, :3] = w * np.eye(3) + sign * S
        m[:3, 3] = (x, y, z); m[3, :3] = (-x, -y, -z); m[3, 3] = w
        return m
    out = []
    for Rc, Rimu, _ in hist:
        q1 = [float(v) for v in q_from_R(M(Rc))]
        q2 = [float(v) for v in q_from_R(M(Rimu))]
        out.append(blk(q1, -1.0) - blk(q2, 1.0))
    return np.concatenate(out)
