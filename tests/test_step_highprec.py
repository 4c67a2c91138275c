"""Pins tests/step_highprec.py (the extended-precision Gauss-Newton / dogleg step the GPU solve stage is compared with) on the CPU:
fed the ORACLE's strips it must reproduce the oracle's normal equations and its DENSE_SCHUR solve, agree with a 40-digit mpmath
solve of the same strips, and give the same step through its landmark-eliminated route as through the dense one."""
import ctypes as C

import numpy as np
import pytest

import step_highprec as sh
from isvins_amd import abi, synth

dp = C.POINTER(C.c_double)
LD = np.longdouble


def P(a):
    return a.ctypes.data_as(dp)


def oracle_strips(oracle, cfg, w):
    """the oracle's strips in the product's layouts; the prior strip (residual AND Jacobian, Cauchy-corrected like ceres' Corrector)
    from the oracle's factor exports"""
    F, N = w.n_factors, w.N
    ps = np.zeros((max(F, 1), 28)); im = np.zeros((N - 1, 465)); cost = np.zeros(1)
    assert oracle.isvo_linearize(C.byref(cfg), C.byref(w.c()), P(ps), P(im), None, P(cost)) == 0
    pose = np.zeros((N, 7)); sb = np.zeros((N, 9))
    for i in range(N):
        pose[i, :3] = w.Ps[i]; oracle.isvo_x_R2q(P(np.ascontiguousarray(w.Rs[i])), P(pose[i, 3:]))
        sb[i] = np.concatenate([w.Vs[i], w.Bas[i], w.Bgs[i]])
    strip = np.zeros(sh.prior_strip_size(w.Nvo, w.n_rollpitch))

    def put(off, r, Js):
        sc = 1.0 / np.sqrt(1.0 + r @ r)
        strip[off:off + len(r)] = r * sc
        off += len(r)
        for J in Js:
            strip[off:off + J.size] = (J * sc).ravel(); off += J.size

    r6 = np.zeros(6); J7 = np.zeros((6, 7)); K7 = np.zeros((6, 7))
    oracle.isvo_x_se3prior(C.byref(w.pose_prior), 1, P(pose[0]), P(r6), P(J7)); put(0, r6, [J7[:, :6]])
    r9 = np.zeros(9); J9 = np.zeros((9, 9))
    oracle.isvo_x_linear9(C.byref(w.vb_prior), 1, P(sb[w.Nvo - 1]), P(r9), P(J9)); put(sh.PR_LIN9, r9, [J9])
    for k in range(w.Nvo - 1):
        oracle.isvo_x_relpose(C.byref(w.relpose[k]), 1, P(pose[k]), P(pose[k + 1]), P(r6), P(J7), P(K7))
        put(sh.PR_REL0 + sh.PR_REL_SZ * k, r6, [J7[:, :6], K7[:, :6]])
    r2 = np.zeros(2); J2 = np.zeros((2, 7))
    for m in range(w.n_rollpitch):
        oracle.isvo_x_rollpitch(C.byref(w.rollpitch[m]), 1, P(pose[w.rollpitch[m].index]), P(r2), P(J2))
        put(sh.PR_REL0 + sh.PR_REL_SZ * (w.Nvo - 1) + sh.PR_RP_SZ * m, r2, [J2[:, :6]])
    return ps[:F], im, strip


perturb = sh.perturb


SHAPES = [(4, 2, 40, 30), (11, 5, 65, 31)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"N{s[0]}_L{s[2]}")
def case(request, oracle):
    N, Nvo, L, wid = request.param
    w = perturb(synth.make_window(wid, n_frames=N, n_vo=Nvo, n_landmarks=L))
    cfg = abi.make_config(N, Nvo)
    prob = sh.Problem(w, *oracle_strips(oracle, cfg, w))
    H, g = prob.normal_equations_ld()
    return w, cfg, prob, H, g


def test_normal_equations_match_oracle(oracle, case):
    """J^T J and J^T r from the strips, in the helper's column order = isvo_normal_equations.  Both sum the same float64 products, the
    oracle in float64 in ceres' block order: n * 2^-53 of the largest entry of a row's terms bounds the difference (n residual rows)"""
    w, cfg, prob, H, g = case
    n = prob.ncols
    Ho = np.zeros((n, n)); go = np.zeros(n); nn = C.c_int(0)
    oracle.isvo_normal_equations(C.byref(cfg), C.byref(w.c()), P(Ho), P(go), C.byref(nn))
    assert nn.value == n == 15 * w.N + w.L
    tol = prob.nres * 2.0 ** -53
    d = np.sqrt(np.diag(Ho))
    assert np.abs((H - Ho) / np.outer(d, d)).max() < tol            # |H_ab| <= sqrt(H_aa H_bb): the scale of a row's terms
    J, r = prob.dense(LD)
    gabs = (np.abs(J) * np.abs(r)[:, None]).sum(0)
    assert (np.abs(g - go) <= tol * gabs).all()
    H64, g64 = prob.normal_equations_f64()
    assert np.abs((H64 - Ho) / np.outer(d, d)).max() < tol


def test_step_matches_oracle_schur_solve(oracle, case):
    """the Gauss-Newton solve of the SCALED system is the oracle's DENSE_SCHUR solve of the unscaled one with
    D = sqrt(mu) diag / scale, y_unscaled = scale * y: to the tolerance tests/test_oracle_solver.py uses for Schur == dense"""
    w, cfg, prob, H, g = case
    st = sh.Step(H, g, 1e-8, 1e4, prob.np)
    D = np.array(np.sqrt(LD(1e-8)) * st.diag / st.scale, float)
    y = np.zeros(prob.ncols)
    assert oracle.isvo_schur_solve(C.byref(cfg), C.byref(w.c()), P(D), P(y)) == 0
    y_ref = np.array(st.scale * st.y, float)
    assert np.allclose(y, y_ref, rtol=1e-7, atol=1e-9 * np.abs(y_ref).max())


def test_eliminated_route_equals_dense(case):
    """the landmark-eliminated preconditioner (long windows) against the dense one: the refinement in pair arithmetic converges to
    the same solution through either, each within 1e-17 of the exact one (test_smallest_window_matches_mpmath), so within 2e-17 of
    one another; the whole step likewise"""
    w, cfg, prob, H, g = case
    a = sh.step_dd(prob, 1e-8, 1e4, route="dense")
    b = sh.step_dd(prob, 1e-8, 1e4, route="eliminated")
    print("eliminated vs dense:", sh.err(b.gn, a.gn), sh.err(b.step, a.step))
    assert sh.err(b.gn, a.gn) < 2e-17 and sh.err(b.step, a.step) < 2e-17 and a.branch == b.branch
    assert abs(b.model - a.model) < 2e-17 * abs(a.model)


def test_pair_arithmetic_normal_equations_round_to_the_longdouble_ones(case):
    """J^T J in pairs of longdouble, rounded, is the plain longdouble sum to its rounding: nres * 2^-64 of a row's scale"""
    w, cfg, prob, H, g = case
    Hd, gd = sh.normal_equations_dd(prob)
    d = np.sqrt(np.diag(H))
    assert np.abs((Hd[0] - H) / np.outer(d, d)).max() < prob.nres * 2.0 ** -64
    assert np.abs(Hd[1]).max() <= np.abs(Hd[0]).max() * 2.0 ** -63


@pytest.fixture(scope="module")
def mp_errors(oracle):
    """N = 4, L = 40: scaling, diagonal, gradient and the Gauss-Newton step recomputed at 40 digits from the same strips (the strips'
    entries are float64, exact in both); errors of the longdouble helper as max-norm over 2-norm"""
    import mpmath as mp
    mp.mp.dps = 40
    N, Nvo, L, wid = SHAPES[0]
    w = perturb(synth.make_window(wid, n_frames=N, n_vo=Nvo, n_landmarks=L))
    prob = sh.Problem(w, *oracle_strips(oracle, abi.make_config(N, Nvo), w))
    st, _ = sh.reference_pair(prob, 1e-8, 1e4)
    n = prob.ncols
    H = mp.zeros(n, n); g = mp.zeros(n, 1)
    for rb, cols in prob.blocks:
        for ca, Ja in cols:
            for a in range(Ja.shape[1]):
                g[ca + a] += mp.fsum(mp.mpf(Ja[e, a]) * mp.mpf(rb[e]) for e in range(len(rb)))
                for cb, Jb in cols:
                    for b in range(Jb.shape[1]):
                        H[ca + a, cb + b] += mp.fsum(mp.mpf(Ja[e, a]) * mp.mpf(Jb[e, b]) for e in range(len(rb)))
    scale = [1 / (1 + mp.sqrt(H[i, i])) for i in range(n)]
    D = [mp.sqrt(min(max(scale[i] ** 2 * H[i, i], mp.mpf("1e-6")), mp.mpf("1e32"))) for i in range(n)]
    A = mp.zeros(n, n); gs = mp.zeros(n, 1)
    for i in range(n):
        gs[i] = g[i] * scale[i]
        for j in range(n):
            A[i, j] = H[i, j] * scale[i] * scale[j]
        A[i, i] += mp.mpf(1e-8) * D[i] ** 2          # (mu is the float64 1e-8 of k_init_state, not the decimal)
    y = mp.cholesky_solve(A, gs)

    def e(a, ref):          # (a longdouble as the exact sum of two float64)
        a = [mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v)))) for v in a]
        return float(max(abs(x - r) for x, r in zip(a, ref)) / mp.sqrt(mp.fsum(r * r for r in ref)))

    errs = dict(scale=e(st.scale, scale), diag=e(st.diag, D), gradient=e(st.gradient, [gs[i] / D[i] for i in range(n)]),
                gn=e(st.gn, [-D[i] * y[i] for i in range(n)]))
    print("longdouble against 40 digits:", errs)
    return errs


def test_smallest_window_sums_match_mpmath(mp_errors):
    """the sums of products (scaling, diagonal, gradient): 1e-17 relative; measured 2.0e-20, 9.7e-21, 8.3e-20"""
    assert max(mp_errors[k] for k in ("scale", "diag", "gradient")) < 1e-17, mp_errors


def test_smallest_window_matches_mpmath(mp_errors):
    """the Gauss-Newton step: 1e-17 relative.  (One longdouble misses this by five orders -- the damped scaled system has a condition
    number of 2.3e8 -- which is why the helper solves in pairs of longdouble.)"""
    assert mp_errors["gn"] < 1e-17, mp_errors


def test_corrupted_problem_moves_the_step(case):
    """what the GPU module's negative control relies on: dropping one landmark's factors moves the step by far more than any
    rounding yardstick"""
    w, cfg, prob, H, g = case
    a = sh.Step(H, g, 1e-8, 1e4, prob.np)
    J, r = prob.dense(LD)
    o = 0; keep = np.ones(prob.nres, bool)
    for k, (rb, _) in enumerate(prob.blocks):
        if k in prob.proj_block_of_landmark[prob.L - 1]:
            keep[o:o + len(rb)] = False
        o += len(rb)
    Jc, rc = J[keep], r[keep]
    Hc = np.array([(Jc * Jc[:, i][:, None]).sum(0) for i in range(prob.ncols)])
    b = sh.Step(Hc, (Jc * rc[:, None]).sum(0), 1e-8, 1e4, prob.np)
    assert sh.err(b.gn, a.gn) > 1e-6
