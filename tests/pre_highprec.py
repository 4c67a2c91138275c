"""The IMU pre-integration at 50 digits: IntegrationBase's constructor and propagate -> midPointIntegration (reference
include/factor/integration_base.h:13-158) and processIMU's propagation of the newest frame (src/estimator.cpp:109-122), written down
once more in mpmath from the reference's text -- dense F (15 x 15) and V (15 x 18), dense F J and F C F^T + V N V^T, no block masks and
no summation order of is-vins_amd/csrc/isv_preint.h.  Doubles are read as exact numbers.  What the reference leaves unnormalised stays
so: F and V use result_delta_q.toRotationMatrix() of the unnormalised product, the nav rotation is multiplied by
deltaQ(un_gyr dt).toRotationMatrix() with deltaQ = (1, theta / 2), so R drifts off the orthogonal matrices as the reference's does.
delta_q is normalised after the step, without a sign change.

`integrate_mp` is the statement, `bias_derivative_mp` an independent derivation of the jacobian's bias columns (central differences of
the deltas at 60 digits), `errors` the measures a float64 result is judged in.  Cases, routes and the margin: tests/pre_highprec_cases.py."""
import mpmath as mp
import numpy as np

DPS = 50
U = 2.0 ** -53                        # one rounding unit of a double
O_P, O_R, O_V, O_BA, O_BG = 0, 3, 6, 9, 12


def _mpv(a):
    """doubles as exact numbers (mpf entries pass through)"""
    if isinstance(a, np.ndarray):
        a = a.ravel().tolist()
    return [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in a]


def _hat(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _qmul(a, b):                      # (w, x, y, z)
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def _qmat(q):
    """Eigen's toRotationMatrix(): the polynomial in (w, x, y, z), with no division by the norm.  q * v is the same polynomial
    (Eigen's _transformVector, v + 2w (u x v) + 2 u x (u x v)), so rotations of vectors go through this matrix as well."""
    w, x, y, z = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _set(M, r0, c0, B):
    for a in range(3):
        for b in range(3):
            M[r0 + a, c0 + b] = B[a, b]


def _col(v):
    return mp.matrix([[x] for x in v])


def integrate_mp(dt, acc, gyr, acc_0, gyr_0, ba, bg, noise, nav=None, gravity=None, dps=DPS, matrices=True):
    """The samples dt [n], acc [n][3], gyr [n][3] pushed onto IntegrationBase(acc_0, gyr_0, ba, bg); noise = (ACC_N, GYR_N, ACC_W, GYR_W).
    nav = (R, P, V, Ba, Bg) with gravity: processIMU's Rs / Ps / Vs beside every sample.  -> dict of mpf: delta_p [3], delta_q [4]
    (x y z w, as the record has it), delta_v [3], sum_dt, J and C (mp.matrix 15 x 15; None without `matrices`), and with nav R
    (mp.matrix 3 x 3), P, V."""
    with mp.workdps(dps):
        dt = _mpv(np.asarray(dt, float))
        n = len(dt)
        acc, gyr = _mpv(np.asarray(acc, float)), _mpv(np.asarray(gyr, float))
        acc_0, gyr_0, ba, bg = _mpv(acc_0), _mpv(gyr_0), _mpv(ba), _mpv(bg)
        an, gn, aw, gw = _mpv(noise)
        N = mp.zeros(18, 18)
        for k, s in enumerate((an, gn, an, gn, aw, gw)):
            for a in range(3):
                N[3 * k + a, 3 * k + a] = s * s
        dp, dv, dq, sum_dt = mp.zeros(3, 1), mp.zeros(3, 1), [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)], mp.mpf(0)
        J, C = mp.eye(15), mp.zeros(15, 15)
        I3, half, quarter = mp.eye(3), mp.mpf(1) / 2, mp.mpf(1) / 4
        if nav is not None:
            R = mp.matrix(3, 3)
            Rin = _mpv(np.asarray(nav[0], float))
            for a in range(3):
                for b in range(3):
                    R[a, b] = Rin[3 * a + b]
            P, Vn, Ba, Bg, g = _col(_mpv(nav[1])), _col(_mpv(nav[2])), _col(_mpv(nav[3])), _col(_mpv(nav[4])), _col(_mpv(gravity))
        for i in range(n):
            h, a1, g1 = dt[i], acc[3 * i: 3 * i + 3], gyr[3 * i: 3 * i + 3]
            if nav is not None:                                             # estimator.cpp:113-120, acc_0 / gyr_0 before the step
                un_acc_0 = R * (_col(acc_0) - Ba) - g
                un_gyr = half * (_col(gyr_0) + _col(g1)) - Bg
                R = R * _qmat([mp.mpf(1), un_gyr[0] * h / 2, un_gyr[1] * h / 2, un_gyr[2] * h / 2])
                un_acc_1 = R * (_col(a1) - Ba) - g
                un_acc = half * (un_acc_0 + un_acc_1)
                P = P + h * Vn + half * h * h * un_acc
                Vn = Vn + h * un_acc
            # midPointIntegration, integration_base.h:63-71
            a_0_x = [acc_0[k] - ba[k] for k in range(3)]
            a_1_x = [a1[k] - ba[k] for k in range(3)]
            w_x = [half * (gyr_0[k] + g1[k]) - bg[k] for k in range(3)]
            Rd = _qmat(dq)
            rq = _qmul(dq, [mp.mpf(1), w_x[0] * h / 2, w_x[1] * h / 2, w_x[2] * h / 2])
            Rr = _qmat(rq)
            un_acc = half * (Rd * _col(a_0_x) + Rr * _col(a_1_x))
            rp = dp + dv * h + half * un_acc * h * h
            rv = dv + un_acc * h
            if matrices:                                                    # :75-125
                R_w_x, R_a_0_x, R_a_1_x = _hat(w_x), _hat(a_0_x), _hat(a_1_x)
                F, V = mp.zeros(15, 15), mp.zeros(15, 18)
                _set(F, 0, 0, I3)
                _set(F, 0, 3, -quarter * Rd * R_a_0_x * h * h + -quarter * Rr * R_a_1_x * (I3 - R_w_x * h) * h * h)
                _set(F, 0, 6, I3 * h)
                _set(F, 0, 9, -quarter * (Rd + Rr) * h * h)
                _set(F, 0, 12, -quarter * Rr * R_a_1_x * h * h * -h)
                _set(F, 3, 3, I3 - R_w_x * h)
                _set(F, 3, 12, -1 * I3 * h)
                _set(F, 6, 3, -half * Rd * R_a_0_x * h + -half * Rr * R_a_1_x * (I3 - R_w_x * h) * h)
                _set(F, 6, 6, I3)
                _set(F, 6, 9, -half * (Rd + Rr) * h)
                _set(F, 6, 12, -half * Rr * R_a_1_x * h * -h)
                _set(F, 9, 9, I3)
                _set(F, 12, 12, I3)
                _set(V, 0, 0, quarter * Rd * h * h)
                _set(V, 0, 3, quarter * -Rr * R_a_1_x * h * h * half * h)
                _set(V, 0, 6, quarter * Rr * h * h)
                _set(V, 0, 9, V[0:3, 3:6])
                _set(V, 3, 3, half * I3 * h)
                _set(V, 3, 9, half * I3 * h)
                _set(V, 6, 0, half * Rd * h)
                _set(V, 6, 3, half * -Rr * R_a_1_x * h * half * h)
                _set(V, 6, 6, half * Rr * h)
                _set(V, 6, 9, V[6:9, 3:6])
                _set(V, 9, 12, I3 * h)
                _set(V, 12, 15, I3 * h)
                J = F * J
                C = F * C * F.T + V * N * V.T
            # propagate, :148-156
            dp, dv = rp, rv
            nq = mp.sqrt(sum(c * c for c in rq))
            dq = [c / nq for c in rq]
            sum_dt += h
            acc_0, gyr_0 = a1, g1
        out = dict(delta_p=list(dp), delta_q=[dq[1], dq[2], dq[3], dq[0]], delta_v=list(dv), sum_dt=sum_dt,
                   J=J if matrices else None, C=C if matrices else None)
        if nav is not None:
            out.update(R=R, P=list(P), V=list(Vn))
        return out


def bias_derivative_mp(dt, acc, gyr, acc_0, gyr_0, ba, bg, step="1e-20", dps=60):
    """d (delta_p, 2 vec(dq0^-1 * dq), delta_v) / d (ba, bg) by central differences with a 1e-20 step at 60 digits (truncation about
    1e-40 relative): an mp.matrix 9 x 6, rows p / the local rotation vector / v, columns ba / bg.  It shares no algebra with F."""
    with mp.workdps(dps):
        h = mp.mpf(step)
        ba, bg = _mpv(ba), _mpv(bg)
        run = lambda a, g: integrate_mp(dt, acc, gyr, acc_0, gyr_0, a, g, (0, 0, 0, 0), dps=dps, matrices=False)
        q0 = run(ba, bg)["delta_q"]
        q0inv = [q0[3], -q0[0], -q0[1], -q0[2]]                            # (w, x, y, z) of the conjugate; q0 is unit
        D = mp.zeros(9, 6)

        def value(a, g):
            o = run(a, g)
            q = o["delta_q"]
            dq = _qmul(q0inv, [q[3], q[0], q[1], q[2]])
            return o["delta_p"] + [2 * dq[1], 2 * dq[2], 2 * dq[3]] + o["delta_v"]
        for k in range(6):
            pa, pg, ma, mg = list(ba), list(bg), list(ba), list(bg)
            if k < 3:
                pa[k] += h; ma[k] -= h
            else:
                pg[k - 3] += h; mg[k - 3] -= h
            vp, vm = value(pa, pg), value(ma, mg)
            for r in range(9):
                D[r, k] = (vp[r] - vm[r]) / (2 * h)
        return D


# ---- the measures ---------------------------------------------------------------------------------------------------------------------
def _f(x):
    return mp.mpf(float(x))


def _rel_max(got, ref):
    """max |x - x*| / max |x*| (0 where both are all zero; inf where only the reference is)"""
    d = max(abs(_f(a) - b) for a, b in zip(got, ref))
    s = max(abs(b) for b in ref)
    return float(d / s) if s != 0 else (0.0 if d == 0 else float("inf"))


def blocks(got, ref):
    """a 15 x 15 float array against its 50-digit value, per 3 x 3 block: -> (e [5][5], max |B - B*| / max |B*| and NaN where B* is
    exactly zero; the list of blocks that are exactly zero at 50 digits and not all 0.0 in `got`; the number of non-zero blocks)"""
    got = np.asarray(got, float).reshape(15, 15)
    e, bad, nz = np.full((5, 5), np.nan), [], 0
    for rb in range(5):
        for cb in range(5):
            idx = [(3 * rb + a, 3 * cb + b) for a in range(3) for b in range(3)]
            s = max(abs(ref[i, j]) for i, j in idx)
            if s == 0:
                if any(got[i, j] != 0.0 for i, j in idx):
                    bad.append((rb, cb))
                continue
            nz += 1
            e[rb, cb] = float(max(abs(_f(got[i, j]) - ref[i, j]) for i, j in idx) / s)
    return e, bad, nz


MEASURES = ("delta_p", "delta_q", "delta_v", "sum_dt", "J", "C")
NAV_MEASURES = ("R", "P", "V")


def errors(ref, got):
    """`got`: dict of float arrays (delta_p, delta_q (x y z w), delta_v, sum_dt, and where present J, C [15][15], R [3][3], P, V) against
    integrate_mp's `ref`.  -> (e: measure -> error, faults: list).  delta_p, delta_v, P, V: max |x - x*| / max |x*|; delta_q per
    component with its sign and R per entry: absolute; sum_dt: relative; J and C: the worst 3 x 3 block, each max |B - B*| / max |B*|
    (e["J_blocks"], e["C_blocks"] keep all 25).  Faults: a non-finite entry; a block that is exactly zero at 50 digits and not 0.0."""
    with mp.workdps(DPS):
        e, faults = {}, []
        for k, v in got.items():
            if not np.isfinite(np.asarray(v, float)).all():
                faults.append((k, "not finite"))
        if faults:
            return {k: float("inf") for k in got}, faults
        for k in ("delta_p", "delta_v", "P", "V"):
            if k in got:
                e[k] = _rel_max(np.asarray(got[k], float).ravel(), ref[k])
        e["delta_q"] = float(max(abs(_f(a) - b) for a, b in zip(np.asarray(got["delta_q"], float).ravel(), ref["delta_q"])))
        e["sum_dt"] = _rel_max([got["sum_dt"]], [ref["sum_dt"]])
        if "R" in got:
            R = np.asarray(got["R"], float).reshape(3, 3)
            e["R"] = float(max(abs(_f(R[a, b]) - ref["R"][a, b]) for a in range(3) for b in range(3)))
        for k in ("J", "C"):
            if k in got:
                eb, bad, nz = blocks(got[k], ref[k])
                e[k + "_blocks"], e[k + "_nonzero"] = eb, nz
                e[k] = float(np.nanmax(eb)) if nz else 0.0
                faults += [(k, "zero block not 0.0", b) for b in bad]
        return e, faults

