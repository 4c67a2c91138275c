"""The 40-digit statements of tests/prep_highprec.py held against independent facts, the CPU oracle held against the statements, and the
case table of tests/prep_cases.py held to what it is meant to reach.  No GPU: the kernels' side is tests/test_gpu_prep_highprec.py,
with the same judge() / judge_imu() and the same margins.

What pins the statements (none of it is the oracle or a kernel):
  triangulate_mp   on exact geometry the depth is the planted one to the rounding of the observations times sigma_1 / sigma_3; and a
                   second route at 100 digits (eigenvectors of A^T A) agrees to 1e-40
  information_mp   cov^-1 cov = I and U^T U = cov^-1 at 40 digits, U upper triangular with a positive diagonal
  quat_mp          the rotation matrix of the quaternion is the input, the quaternion is a unit one, the arm's own component is positive
                   and the largest of x, y, z (the trace arm: w > 1/2)
The margins of the value bounds are measured here between the two float64 reference routes (prep_cases.TRI_ROUTE_RATIO_MEASURED,
IMU_ROUTE_RATIO_*_MEASURED): these tests fail when the table measures more than is recorded."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import prep_cases as pc
import prep_highprec as ph
from isvins_amd import abi

dp = C.POINTER(C.c_double)
RUNGS = list(pc.rungs())


def P(a):
    return a.ctypes.data_as(dp)


def oracle_sqrt_info(oracle, im):
    so = np.zeros(225); r = np.zeros(15)
    G = np.array([0, 0, 9.81007]); p7 = np.array([0, 0, 0, 0, 0, 0, 1.0]); z9 = np.zeros(9)
    oracle.isvo_x_imu(C.byref(im), P(G), P(p7), P(z9), P(p7), P(z9), 1, P(r), None, None, None, None, P(so))
    return so.reshape(15, 15)


# ---- triangulation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUNGS)
def test_triangulate_statement_and_table(oracle, name):
    rung, tr = pc.rungs()[name], pc.truth(oracle, name)
    exact = "noisy" not in name and not name.startswith("norm_")
    for w, t in zip(rung.windows, tr):
        todo = np.flatnonzero(t.todo)
        assert len(todo) > 0
        if t.degenerate:
            # two vanishing singular values: nothing to compare, every landmark excluded by the gap rule
            assert t.excluded[todo].all() and (t.sigma[todo, 2] / t.sigma[todo, 0]).max() < 1e-12
            continue
        for l in todo[::4]:
            d2, s2 = ph.triangulate_mp(w, int(l), method="gram")
            assert abs(d2 / t.dstar[l] - 1) < mp.mpf(10) ** -40, (name, l)
            assert max(abs(float(a) / b - 1) for a, b in zip(s2[:3], t.sigma[l, :3])) < 1e-12
        if exact:
            # the observations are the planted point's projections rounded to doubles: d* is the planted depth to 2^-52 sigma_1 / sigma_3
            # times a small count (64).  The projections invert ric by its transpose, as the reference does, but in another place of the
            # chain; EuRoC's ric is given to 12 digits and is orthonormal to 1e-12 only, which enters the same way (count 8).
            skew = float(np.abs(w.ric.T @ w.ric - np.eye(3)).max())
            for l in todo:
                lim = (64 * 2.0 ** -52 + 8 * skew) * t.sigma[l, 0] / t.sigma[l, 2]
                assert abs(float(t.dstar[l] / mp.mpf(float(w.planted[l])) - 1)) < lim, (name, l, float(t.dstar[l]), w.planted[l], lim)
    n = sum(int(t.todo.sum()) for t in tr if not t.degenerate)
    n_ex = sum(int((t.todo & t.excluded).sum()) for t in tr if not t.degenerate)
    assert n_ex <= pc.EXCLUDED_MAX * n, (name, n_ex, n)


def test_triangulate_table_reaches_what_it_names(oracle):
    R = pc.rungs()
    conds = []
    for s in pc.LADDER:
        for kind in ("exact", "noisy"):
            name = f"ladder_s{s:g}_{kind}"
            w, t = R[name].windows[0], pc.truth(oracle, name)[0]
            assert w.L >= 30 and t.todo.all() and (np.array(w.lm_depth[: w.L]) == 0.0).any() and (np.array(w.lm_depth[: w.L]) == -1.0).any()
            if kind == "exact":
                conds.append(float((t.sigma[:, 0] / t.sigma[:, 2]).max()))
    print("ladder, exact: largest sigma1/sigma3 per rung", ["%.1e" % c for c in conds])
    assert conds[0] < 2e2 and min(conds[2:]) > 2e3          # the Gram route's u cond^2 reaches 1e-9 from the third rung down
    w = R["tracks"].windows[0]
    k = np.diff(w.lm_obs_ptr)
    N = w.N
    assert {(int(h), int(kk)) for h, kk in zip(w.lm_start_frame[: w.L], k)} >= {(0, 2), (N - 2, 2), (0, N)} and (k == 3).sum() == 8
    w, t = R["clamp"].windows[0], pc.truth(oracle, "clamp")[0]
    for l, d in enumerate(w.planted[:33]):
        assert bool(t.clamped[l]) == (d < pc.D_LO or d > pc.D_HI) and not t.excluded[l], (l, d)
        assert abs(float(t.dstar[l]) / d - 1) < 1e-9                   # d* is the planted depth to a quarter of the nearest planted distance, 4e-9
    assert t.clamped[:33].sum() == 21 and (w.planted < 0).sum() == 3 and float(t.dstar[18]) < 0
    w, t = R["entry"].windows[0], pc.truth(oracle, "entry")[0]
    e = np.array(w.lm_depth[: w.L])
    assert (e > 0).sum() == 11 and (e == 0.0).sum() == 11 and (e == -1.0).sum() == 11 and not t.todo[e > 0].any()
    ws = R["batch"].windows
    assert [w.L for w in ws] == [1, 64, 65, 130] and len({w.ric.tobytes() for w in ws}) == 4 and len({w.tic.tobytes() for w in ws}) == 4
    assert not ws[1].tic.any() and np.array_equal(ws[1].ric, np.eye(3))
    assert R["n18"].windows[0].N == 18
    plain = pc.truth(oracle, "norm_plain")[0]
    for how in ("x2p5", "unit", "varied"):
        w, t = R["norm_" + how].windows[0], pc.truth(oracle, "norm_" + how)[0]
        assert (w.obs_point[:, 2] != 1.0).all()
        # the same depths as the unscaled window: the scaling rounds every coordinate once, sigma_1 / sigma_3 <= 50 carries that into d*
        worst = max(abs(float(a / b - 1)) for a, b in zip(t.dstar, plain.dstar))
        print("norm_" + how, "d* against the unscaled window's", worst)
        assert worst < 50 * 16 * 2.0 ** -52


@pytest.mark.parametrize("name", RUNGS)
def test_oracle_triangulate_against_40_digits(oracle, name):
    """the oracle alone meets the decision rule on every rung, and the two reference routes differ by no more than what TRI_MARGIN was
    taken from"""
    tr = pc.truth(oracle, name)
    bad, e, e_ref, cond = pc.judge(oracle, name, [t.oracle for t in tr])
    assert not bad, bad
    bad_np = []
    for w, t in zip(pc.rungs()[name].windows, tr):
        got = np.where(t.todo, t.np_svd, np.array(w.lm_depth[: w.L]))
        got = np.where(t.todo & ((got < pc.D_LO) | (got > pc.D_HI)), pc.INIT_DEPTH, got)
        bad_np += pc.decisions_ok(w, t, got)
    assert not bad_np, bad_np
    eo, en = pc.ref_error(tr)
    ratio = max(eo, en) / min(eo, en)
    print(f"ROUTES {name}: oracle {eo:.2e} numpy {en:.2e} ratio {ratio:.2f}")
    assert ratio <= 1.01 * pc.TRI_ROUTE_RATIO_MEASURED
    assert e <= pc.TRI_MARGIN * e_ref


def test_margins_are_what_the_measurements_give():
    assert pc.TRI_MARGIN == max(4.0, 2 * pc.TRI_ROUTE_RATIO_MEASURED)
    assert pc.IMU_MARGIN_INFO == max(4.0, 2 * pc.IMU_ROUTE_RATIO_INFO_MEASURED)
    assert pc.IMU_MARGIN_FACTOR == max(4.0, 2 * pc.IMU_ROUTE_RATIO_FACTOR_MEASURED)


# ---- IMU weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.IMU_CASES))
def test_information_statement_and_oracle(oracle, name):
    w, idx = pc.imu_window()
    t = pc.imu_truth(name)
    with mp.workdps(ph.INFO_DPS):
        I = t.Inv_mp * ph._m(t.cov)
        assert max(abs(I[a, b] - (a == b)) for a in range(15) for b in range(15)) < mp.mpf(10) ** -40
        D = t.U_mp.T * t.U_mp - t.Inv_mp
        scale = max(abs(t.Inv_mp[a, b]) for a in range(15) for b in range(15))
        assert max(abs(D[a, b]) for a in range(15) for b in range(a + 1)) < scale * mp.mpf(10) ** -40     # (the lower triangle is what LLT reads)
        assert all(t.U_mp[a, a] > 0 for a in range(15)) and all(t.U_mp[a, b] == 0 for a in range(15) for b in range(a))
    assert abs(w.imu[idx[name]].sum_dt - pc.IMU_CASES[name]["samples"] * pc.IMU_CASES[name].get("dt", 0.005)) < 1e-12
    assert not w.imu[idx[name]].sum_dt > 10.0                        # (2000 samples: the gate's edge, still weighted)
    ri, rf = max(t.e_info) / min(t.e_info), max(t.e_factor) / min(t.e_factor)
    print(f"ROUTES {name}: cond {t.cond:.2e} info {ri:.2f} factor {rf:.2f}")
    assert ri <= 1.01 * pc.IMU_ROUTE_RATIO_INFO_MEASURED and rf <= 1.01 * pc.IMU_ROUTE_RATIO_FACTOR_MEASURED
    faults, ei, ef, yi, yf = pc.judge_imu(name, oracle_sqrt_info(oracle, w.imu[idx[name]]))
    assert not faults, faults
    assert ei <= pc.IMU_MARGIN_INFO * yi, (ei, yi)
    assert ef <= pc.IMU_MARGIN_FACTOR * yf, (ef, yf)


def test_imu_condition_numbers_are_the_documented_ones():
    conds = {n: pc.imu_truth(n).cond for n in pc.IMU_CASES}
    print(conds)
    assert 2e6 < conds["s2"] < 3e6 and 2e6 < conds["s20"] < 3e6 and 3e6 < conds["s200"] < 4e6 and 1e8 < conds["s2000"] < 2e8


# ---- vector2double --------------------------------------------------------------------------------------------------------------------------
def _q_to_R_mp(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def test_quaternion_statement_and_table():
    reached, ties = set(), set()
    for name in list(pc.QUAT_CASES) + ["ric_x_arm"]:
        w = pc.quat_window(name)
        for R in list(w.Rs) + [w.ric]:
            arm, tie = ph.quat_arm(R)
            reached.add(arm); ties.add(tie)
            q = ph.quat_mp(R)
            # R is a rotation matrix to a few 2^-53 (products of doubles; EuRoC's ric, given to 12 digits: to 2e-13), so is the quaternion's
            tol = 1e-14 + 4 * float(np.abs(R.T @ R - np.eye(3)).max())
            assert abs(float(sum(c * c for c in q)) - 1) < tol
            M = _q_to_R_mp(q)
            assert max(abs(float(M[a][b]) - R[a][b]) for a in range(3) for b in range(3)) < tol
            qf = [float(c) for c in q]
            own = {"trace": qf[3], "x": qf[0], "y": qf[1], "z": qf[2]}[arm]
            assert own > 0 and (own > 0.5 if arm == "trace" else own >= max(abs(qf[0]), abs(qf[1]), abs(qf[2])))
    assert reached == set(ph.ARMS) and ties >= {"xy", "yz"}, (reached, ties)
    assert ph.quat_arm(pc.quat_window("ric_x_arm").ric)[0] == "x"
    for name, arm in (("near_pi_x", "x"), ("near_pi_y", "y"), ("near_pi_z", "z")):
        assert {ph.quat_arm(R)[0] for R in pc.quat_window(name).Rs} == {arm}
    assert ph.quat_arm(pc.quat_window("tie_xy").Rs[pc.PIVOT]) == ("x", "xy")
    assert ph.quat_arm(pc.quat_window("tie_yz").Rs[pc.PIVOT]) == ("y", "yz")
    # both sides of each tie are present beside it
    assert {ph.quat_arm(R)[0] for R in pc.quat_window("tie_xy").Rs} == {"x", "y"}
    assert {ph.quat_arm(R)[0] for R in pc.quat_window("tie_yz").Rs} == {"y", "z"}
    assert ph.QUAT_ATOL == 9 * 2.0 ** -53
