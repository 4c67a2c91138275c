"""Pins tests/sfm_highprec.py -- the 40-digit restatement of the SfM stage's bundle adjustment and of OpenCV's serial PnP pieces, and
the case list of the GPU test -- to the CPU restatements (tests/native/isv_sfm_oracle.c, isv_loop_oracle.c), before
tests/test_gpu_sfm_highprec.py trusts it; and pins the restatements' Jacobians, which share their text with the kernels, to mpmath.

Capped BA.  The restatement runs every case with the BA capped at 0, 1 and 2 iterations (isvo_sfm_set_ba_max_iterations).  The
reference reproduces ba_initial_cost from the cap-0 output, and from each output the next one: positions, Q / T, ba_final_cost and the
accept / reject decision (ba_successful).  err <= MARGIN_ORACLE * max(e64, floor); e64 and the floors are sfm_highprec's (cost: number
of residuals x 2^-53; state: 2^-53 max(n, |x0|_inf / |step|_2), max-norm over the reference step's 2-norm).  Measured worst ratio
err / max(e64, floor) per case, over cost0 | position | Q T | cost of iterations 1 and 2:
  w3_l0    4.45 (position1)     w5_n65   2.46 (position2)     w13_l6      4.96 (QT1)
  w4_l2    8.47 (QT2)           w5_n131  2.42 (QT1)           w20_l10     2.55 (QT1)
  w5_n63   4.23 (QT2)           w11_l5   5.40 (QT2)           w13_reject  0.80 (QT2)
  w5_n64   1.04 (QT1)           w5_far   2.59 (QT2)
worst 8.47 (w4_l2) -> MARGIN_ORACLE = 4 x 8.47 = 33.9 -> 64.  No ratio is near 100, which would be a finding.

Decision edges.  For every case and iteration the reference's rho is at least 1e3 of its own float64 error away from 1e-3 and its
model cost change from 0 (rho sits within 2 % of 1 on the accepted cases, its e64 is at most 1.4e-10; w13_reject: rho -0.064, then 0.185).

The rejected first step.  A seed search on the restatement at cap 1 (the relative pose turned through make_scene's rel_rot_err /
rel_dir_err) found, at 40 tracks and 5 frames, rejected first steps only from 0.12 rad on, where the cost at x0 is 0.045 and more: above
the 5e-3 under which a capped BA still writes Q / T.  With 16 tracks over 11 or 13 frames the first step is rejected at 0.026 rad and a
cost of 2.2e-3: w13_reject (seed 164), whose second iteration -- the old linearisation at half the radius -- is accepted.

w5_far has the one column of the list whose scaled LM diagonal sits on the 1e-6 clamp: the only place where the Jacobi scaling does not
cancel from the step, and so the case of the GPU test's last negative control.

The mpmath work is 1 .. 3 s per iteration and case, 7 s at n_window = 20 (pure-Python mpmath; 111 reduced columns).
"""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import loop_oracle
import sfm_highprec as sh
import sfm_oracle

mpf = mp.mpf
MARGIN_ORACLE = 64.0         # 4 x 8.47 = 33.9 -> 64
_dp = C.POINTER(C.c_double)


def _d(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sh.bind(sfm_oracle.build(tmp_path_factory.mktemp("sfm_oracle")))


@pytest.fixture(scope="module")
def llib(tmp_path_factory):
    lib = loop_oracle.build(tmp_path_factory.mktemp("loop_oracle"))
    lib.isvo_rodrigues_v2m_J.argtypes = [_dp, _dp, _dp]; lib.isvo_rodrigues_v2m_J.restype = None
    lib.isvo_rodrigues_m2v.argtypes = [_dp, _dp]; lib.isvo_rodrigues_m2v.restype = None
    lib.isvo_pnp_project.argtypes = [_dp] * 6; lib.isvo_pnp_project.restype = None
    lib.isvo_pnp_step.argtypes = [_dp, _dp, C.c_int, _dp, _dp]; lib.isvo_pnp_step.restype = None
    return lib


def _mp(v):
    return [mpf(float(e)) for e in v]


# ---- ReprojectionError3D and its Jacobians -------------------------------------------------------------------------------------------
def _obs_points():
    """(q w x y z, t, X, uv): unit quaternions and |q| = 1 +- 1e-3 (S6: the BA never renormalises), depths 0.5 .. 50 and a point
    behind the camera (S5)"""
    rng = np.random.RandomState(7)
    out = []
    for scale in (1.0, 1.0 + 1e-3, 1.0 - 1e-3):
        for depth in (0.5, 2.0, 10.0, 50.0, -3.0):
            q = rng.normal(size=4); q = q / np.linalg.norm(q) * scale
            t = rng.normal(size=3) * 0.3
            pc = np.array([0.3 * depth * rng.uniform(-1, 1), 0.3 * depth * rng.uniform(-1, 1), depth])   # in the camera; turned back by q below
            u = _mp(q / np.linalg.norm(q))
            ui = [u[0], -u[1], -u[2], -u[3]]
            X = np.array([float(e) for e in sh._rot_point(ui, _mp(pc - t))])
            out.append((q, t, X, pc[:2] / pc[2] + 1e-3 * rng.normal(size=2), depth))
    return out


def test_ba_obs_against_40_digit_derivative(lib):
    """isvo_sfm_ba_obs (the kernel's ba_obs, the same text) against the chain rule through QuaternionParameterization::Plus in mpmath.
    Bound: an entry is a sum of at most 9 products, fewer than 40 rounded operations on intermediates no larger than
    max |J| (1 + |p| / |p_z|): 40 x 2^-53 of that.  Measured worst err / bound 0.03."""
    worst = 0.0
    for q, t, X, uv, depth in _obs_points():
        r, Jq, Jt, JX = np.zeros(2), np.zeros(6), np.zeros(6), np.zeros(6)
        lib.isvo_sfm_ba_obs(_d(q), _d(t), _d(X), _d(uv), _d(r), _d(Jq), _d(Jt), _d(JX))
        rm, Jqm, Jtm, JXm = sh.obs_jacobians(_mp(q), _mp(t), _mp(X), _mp(uv))
        assert sh.check_plus_jacobian(_mp(q), _mp(t), _mp(X), _mp(uv)) < mpf("1e-20")      # the chain rule IS the derivative of Plus
        ref = np.array([[float(e) for e in row] for row in (Jqm + Jtm + JXm)]).reshape(3, 6)
        got = np.array([Jq, Jt, JX])
        u = _mp(q / np.linalg.norm(q))
        p = np.array([float(e) for e in sh._rot_point(u, _mp(X))]) + t
        assert np.sign(p[2]) == np.sign(depth) and abs(p[2] - depth) < 1e-9 * abs(depth)
        bound = 40 * sh.U * np.abs(ref).max() * (1 + np.linalg.norm(p) / abs(p[2]))
        err = max(float(abs(mpf(float(g)) - e)) for g, e in zip(got.ravel(), [e for row in (Jqm + Jtm + JXm) for e in row]))
        er = max(float(abs(mpf(float(g)) - e)) for g, e in zip(r, rm))
        worst = max(worst, err / bound)
        assert err <= bound, (depth, np.linalg.norm(q), err, bound)
        assert er <= 40 * sh.U * (1 + np.linalg.norm(p) / abs(p[2])), (depth, er)
    print(f"RATIO ba_obs worst err / bound {worst:.3f}")


# ---- Rodrigues -----------------------------------------------------------------------------------------------------------------------
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
THETAS = [("0", 0.0), ("eps/4", 2.0 ** -54), ("1e-12", 1e-12), ("1e-8", 1e-8), ("1e-4", 1e-4), ("1", 1.0), ("3", 3.0),
          ("pi-1e-9", np.pi - 1e-9), ("pi", np.pi), ("4", 4.0)]
MARGIN_ROD = 4.0


@pytest.mark.parametrize("label,theta", THETAS, ids=[t[0] for t in THETAS])
def test_rodrigues_jacobian(llib, label, theta):
    """isvo_rodrigues_v2m_J's R and 3 x 9 J against the exponential and its derivative at 40 digits.  OpenCV's formula loses digits in
    (s - 2 (1 - c) / theta) and (c - s / theta) at small theta -- the reference's behaviour, restated as it is -- so every entry
    passes against MARGIN_ROD * max(e64, 2^-52), e64 the worst entry error of the same formula evaluated in numpy float64 at this
    theta.  Digits kept by J (C code | numpy), measured:
      theta   0      eps/4   1e-12   1e-8   1e-4   1      3      pi-1e-9   pi     4
      C       exact  16.3    12.4    8.4    12.7   15.9   15.6   15.8      15.9   15.9
      numpy   exact  16.3    12.4    8.4    12.7   15.9   15.6   15.8      15.9   15.9
    (the two agree to the last bit.  (1 - c) / theta carries an absolute error of 2^-53 / theta while 1 - c is rounding noise, 4e-9 at
    1e-8; below that 1 - c is exactly zero and the lost term, theta / 2, is the error; below DBL_EPSILON the generators are returned,
    exact to theta.  R keeps 16 digits at every theta.)"""
    rv = theta * AXIS
    R, J = np.zeros(9), np.zeros(27)
    llib.isvo_rodrigues_v2m_J(_d(rv), _d(R), _d(J))
    Rm = [e for row in sh.rodrigues(_mp(rv)) for e in row]
    Jm = [e for row in sh.rodrigues_jacobian(_mp(rv)) for e in row]
    R64, J64 = sh.rodrigues_jacobian_f64(rv)
    for name, got, ref, f64 in (("R", R, Rm, R64.ravel()), ("J", J, Jm, J64.ravel())):
        err = [float(abs(mpf(float(g)) - e)) for g, e in zip(got, ref)]
        e64 = max(float(abs(mpf(float(g)) - e)) for g, e in zip(f64, ref))
        scale = max(float(abs(e)) for e in ref)
        digits = [(-np.log10(max(v) / scale) if max(v) > 0 else np.inf) for v in (err, [e64])]
        print(f"RATIO rodrigues theta {label:8s} {name} err {max(err):.3e} e64 {e64:.3e} ratio {max(err) / max(e64, 2 * sh.U):.3f} digits C {digits[0]:.1f} numpy {digits[1]:.1f}")
        assert max(err) <= MARGIN_ROD * max(e64, 2 * sh.U), (label, name, max(err), e64)


def _m2v(llib, R):
    v = np.zeros(3)
    llib.isvo_rodrigues_m2v(_d(np.ascontiguousarray(R, dtype=np.float64).ravel()), _d(v))
    return v


def _R64(rv):
    return np.array([[float(e) for e in row] for row in sh.rodrigues(_mp(rv))])


@pytest.mark.parametrize("theta", [1e-3, 0.5, 1.0, 2.0, 3.0])
def test_rodrigues_round_trip(llib, theta):
    """v -> R (40 digits, rounded) -> isvo_rodrigues_m2v, s >= 1e-5 and away from the branch edges.  acos' argument carries three
    roundings of entries of size 1, so theta moves by 3 x 2^-53 / sin(theta); the axis 2 s n carries one rounding per entry, theta x
    2^-53 / (2 s) on v: |v - v0|_inf <= 8 x 2^-53 (1 + theta) / sin(theta)"""
    v0 = theta * AXIS
    v = _m2v(llib, _R64(v0))
    err = np.abs(v - v0).max()
    bound = 8 * sh.U * (1 + theta) / np.sin(theta)
    print(f"RATIO m2v theta {theta} err {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_rodrigues_m2v_small_angle_branch(llib):
    """s < 1e-5 with c > 0: OpenCV returns the zero vector (the rotation, up to 1e-5 rad, is dropped: the reference's behaviour)"""
    for theta in (0.0, 1e-9, 9e-6):
        assert np.array_equal(_m2v(llib, _R64(theta * AXIS)), np.zeros(3))
    assert np.abs(_m2v(llib, _R64(1.1e-5 * AXIS)) - 1.1e-5 * AXIS).max() < 1e-5 * 1e-5      # just past the edge: the general branch


@pytest.mark.parametrize("axis", [(0.5, 0.6, 0.62), (0.5, -0.6, 0.62), (0.5, 0.6, -0.62), (0.5, -0.6, -0.62), (0.1, 0.7, 0.7), (0.1, 0.7, -0.7),
                                  (0.1, -0.7, 0.7), (0.0, 0.6, -0.8), (0.0, 0.6, 0.8), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)])
def test_rodrigues_m2v_near_pi_branch(llib, axis):
    """s < 1e-5 with c <= 0: the axis from R's diagonal, the signs of its second and third entries from R[1], R[2], and the fix through
    R[5] when the first entry is the smallest (isv_pnp.h:71).  The branch takes R = 2 n n^T - I, which holds to O(pi - theta), and
    acos near -1 keeps half the digits: the result is +-theta n (the two are the same rotation at pi) within
    4 ((pi - theta) + sqrt(2^-52)), the first entry of the axis not negative."""
    n = np.array(axis) / np.linalg.norm(axis)
    for theta in (np.pi, np.pi - 1e-7, np.pi - 5e-6):
        v = _m2v(llib, _R64(theta * n))
        err = min(np.abs(v - theta * n).max(), np.abs(v + theta * n).max())
        assert err <= 4 * ((np.pi - theta) + 2.0 ** -26), (axis, theta, v, err)
        assert v[0] >= 0
        if n[0] > 0.05:
            assert np.abs(v - theta * n).max() <= 4 * ((np.pi - theta) + 2.0 ** -26)      # the signs come out as n's


# ---- the projection and CvLevMarq's step ---------------------------------------------------------------------------------------------
def test_pnp_project_against_40_digit_derivative(llib):
    """isvo_pnp_project (Rodrigues, then cvProjectPoints2 with K = I) against the same at 40 digits, the Jacobian through the 40-digit
    dR/dr.  Angles of 0.05 .. 2 rad (where Rodrigues' Jacobian keeps its digits).  Bound as for ba_obs: 64 x 2^-53 max |J| (1 + |p| / p_z)
    (dR/dr adds some twenty operations per entry).  Measured worst err / bound 0.03."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for theta in (0.05, 0.4, 1.0, 2.0):
        for depth in (0.5, 5.0, 50.0):
            rv = theta * AXIS
            tv = rng.normal(size=3) * 0.2 + np.array([0, 0, depth])
            X = rng.uniform(-1, 1, size=3) * min(depth, 2.0) * 0.4
            m = rng.normal(size=2) * 0.1
            err, J = np.zeros(2), np.zeros(12)
            llib.isvo_pnp_project(_d(rv), _d(tv), _d(X), _d(m), _d(err), _d(J))
            em, Jm = sh.pnp_project(_mp(rv), _mp(tv), _mp(X), _mp(m))
            p = _R64(rv) @ X + tv
            ref = np.array([[float(e) for e in row] for row in Jm])
            bound = 64 * sh.U * np.abs(ref).max() * (1 + np.linalg.norm(p) / abs(p[2]))
            e = max(float(abs(mpf(float(g)) - r)) for g, r in zip(J, [v for row in Jm for v in row]))
            worst = max(worst, e / bound)
            assert e <= bound, (theta, depth, e, bound)
            assert max(float(abs(mpf(float(g)) - r)) for g, r in zip(err, em)) <= 64 * sh.U * (1 + np.linalg.norm(p) / abs(p[2]))
    print(f"RATIO pnp_project worst err / bound {worst:.3f}")


def _step(llib, JtJ, JtE, lg, prev):
    out = np.zeros(6)
    llib.isvo_pnp_step(_d(np.ascontiguousarray(JtJ).ravel()), _d(JtE), lg, _d(prev), _d(out))
    return out


def _step64(JtJ, JtE, lg, prev):
    A = JtJ.copy()
    A[np.diag_indices(6)] *= 1.0 + 10.0 ** lg
    Uu, w, Vt = np.linalg.svd(A)
    ub = Uu.T @ JtE
    return prev - Vt.T @ np.where(w > 2 * np.finfo(float).eps * w.sum(), ub / np.where(w > 0, w, 1.0), 0.0)


@pytest.mark.parametrize("rank", [6, 5])
def test_pnp_step_against_40_digits(llib, rank):
    """isvo_pnp_step against the damped pseudo-inverse solve at 40 digits, on a well-conditioned JtJ and on a rank-5 one.  The damping
    multiplies the diagonal, so it lifts every singular value but one that belongs to a (numerically) zero row and column: parameter 3
    has JtJ[3][3] = 1e-20 and nothing else, its singular value is below the cut-off 2 DBL_EPSILON sum(w) and cv::solve(DECOMP_SVD)
    leaves that parameter where it was, although JtErr[3] = 1.  Yardstick: the same solve by numpy's SVD;
    err <= 8 max(e64, 2^-53 cond |x|), cond over the five kept singular values."""
    rng = np.random.RandomState(5 + rank)
    Vs = rng.normal(size=(12, 6))
    if rank == 5:
        Vs[:, 3] = 0.0
    JtJ = Vs.T @ Vs
    if rank == 5:
        JtJ[3, 3] = 1e-20
    JtE = JtJ @ rng.normal(size=6)
    if rank == 5:
        JtE[3] = 1.0
    prev = rng.normal(size=6)
    for lg in (-3, 0, 2):
        got = _step(llib, JtJ, JtE, lg, prev)
        ref = sh.pnp_step(JtJ, JtE, lg, prev)
        e64 = max(float(abs(mpf(float(g)) - r)) for g, r in zip(_step64(JtJ, JtE, lg, prev), ref))
        err = max(float(abs(mpf(float(g)) - r)) for g, r in zip(got, ref))
        w = np.linalg.svd(JtJ, compute_uv=False)
        fl = sh.U * w[0] / w[rank - 1] * max(float(abs(mpf(float(p)) - r)) for p, r in zip(prev, ref))
        print(f"RATIO pnp_step rank {rank} lg {lg} err {err:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {err / max(e64, fl):.3f}")
        assert err <= 8 * max(e64, fl), (rank, lg, err, e64, fl)
        if rank == 5:                                                # the cut-off is what is tested: without it parameter 3 moves by 1e20
            assert got[3] == prev[3] and abs(ref[3] - mpf(float(prev[3]))) < mpf("1e-35")
            assert abs(sh.pnp_step(JtJ, JtE, lg, prev, rank_cut=False)[3] - ref[3]) > 1e15


# ---- the capped BA ---------------------------------------------------------------------------------------------------------------------
def test_the_case_list_reaches_the_loop_edges(lib):
    """the shapes the case list is there for (SfM section), asserted from the problems and n_triangulated"""
    seen_nc, seen_n, ls = set(), set(), set()
    for name in sh.NAMES:
        sp, r, pos, st = sh.oracle_capped(lib, name, 0)
        _, n, mid = sh.make_case(name)
        f = sh.shape_facts(sp)
        nw = sp.c.n_window
        assert r.status == 0 and r.n_triangulated == n and r.n_ba_cols == f["nc"] and not st[mid] and st[mid - 1] and st[mid + 1]
        assert {2, nw} <= f["lengths"] and f["miss_l"] > 0 and f["miss_last"] > 0, (name, f)
        assert r.ba_initial_cost < 5e-3                             # a capped BA must still write Q / T
        seen_nc.add(f["nc"]); seen_n.add(n); ls.add((sp.c.l == 0, sp.c.l == nw - 2))
    assert {9, 15, 21, 57, 69, 111} <= seen_nc and {63, 64, 65} <= seen_n and max(seen_n) >= 129
    assert (True, False) in ls and any(b for _, b in ls)


def test_dense_and_eliminated_routes_agree(lib):
    sp, r, pos, st = sh.oracle_capped(lib, sh.SMALLEST, 0)
    ref = sh.Reference(sp, st)
    assert sh.routes_agree(ref, sh.State.from_output(r, pos, st, ref.nw)) < mpf("1e-30")


@pytest.mark.parametrize("name", sh.NAMES)
def test_reference_against_the_restatement(lib, name):
    outs = [sh.oracle_capped(lib, name, cap)[1:] for cap in (0, 1, 2)]
    rows, edges, clamped = sh.check_chain(name, outs, "RATIO")
    assert (clamped > 0) == (name == "w5_far")                      # the one case where the 1e-6 clamp of the LM diagonal is active
    assert any(not (rho > 1e-3) for _, rho, _, _, _ in edges) == (name == "w13_reject")
    for k, rho, rho_e64, model, model_e64 in edges:                 # decision edges: 1e3 yardsticks away from each threshold
        print(f"EDGE {name} iteration {k} rho {rho:.6f} (e64 {rho_e64:.1e}) model {model:.3e} (e64 {model_e64:.1e})")
        assert abs(rho - 1e-3) >= 1e3 * max(rho_e64, sh.U) and model >= 1e3 * max(model_e64, sh.U * model)
    print(f"WORST {name} {max(e / max(e64, fl) for _, e, e64, fl in rows):.3f}")
    for key, e, e64, fl in rows:
        assert e <= MARGIN_ORACLE * max(e64, fl), (name, key, e, e64, fl)
