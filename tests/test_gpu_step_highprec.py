"""The solve stage of ONE iteration slot on the MI355X -- Gram products, landmark elimination, speed/bias chain elimination, reduced
pose solve, back-substitution and DoglegStrategy::ComputeTraditionalDoglegStep -- against tests/step_highprec.py: the same step
recomputed in extended precision (pairs of longdouble, pinned to a 40-digit solve at 1e-17) from the GPU's OWN Jacobian strips
(pinned to the oracle by tests/test_gpu_linearize.py), so the comparison sees the rounding of this stage alone and names the vector that is wrong.

Every case: a handle with num_iterations = 1 and windows with margin_old = 0 runs exactly one slot at x0; nothing after it writes
the step vectors (k_finalize reads delta_p only, the marginalisation kernels touch none of them), so isv_debug_read's selectors
10-20 and 23 hold that slot's values (tests/step_highprec.py's docstring maps them).

Tolerance.  Yardstick e64: the error of a plain float64 computation (J^T J by numpy's BLAS, the Cholesky solve by LAPACK through scipy) of the same vector from the
same strips against the extended-precision one -- what FP64 can do on this system (condition number ~2.5e8 in the scaled space), from
the reference side alone.  Errors: max-norm over the 2-norm of the reference vector, steps in Ceres' scaled space, floor n * 2^-53.
A vector passes when  err_gpu <= MARGIN * max(e64, floor);  MARGIN = 4 x the worst measured ratio, rounded up to a power of two
(one for the vectors, one for the scalar model); the table is below.  cost_c: against isvo_cost at x0 + the GPU's own step, 1e-11 relative.
Measured on one MI355X, worst ratio err_gpu / max(e64, floor) per case (documentation: the margins below are derived from it by hand) --
over the vectors scale, diag, gradient, gn, step | of the scalar model:
  n3_l25                      0.83   0.04    ragged_batch_st             0.80  62.76
  n4_l40                      1.42   0.00    mu_retry                    1.28   0.00
  n11_l63                     1.10   1.58    chain_split_n11             0.58   0.00
  n11_l64                     1.19   0.00    chain_split_n18             0.35   6.67
  n11_l65                     1.88   5.00    solve_st_n11                0.58   0.00
  n11_l150                    1.36   4.69    solve_st_n18                0.35   6.85
  n12_l100                    0.56   0.54    no_pose_dogleg_n11          0.57   0.00
  n18_l120                    0.82   6.98    no_pose_dogleg_n18          0.35   6.38
  n20_l100                    3.10   8.03    legacy_visual_n11           0.57   0.00
  n21_l60_dense               0.89   0.00    legacy_visual_n18           0.35   6.38
  tracks_two_frames           0.82   0.95    split_control_n11           0.57   0.00
  tracks_whole_window         0.95   7.57    split_control_n18           0.35   6.38
  frames_without_landmarks    1.12   1.39    generic_n_n11               0.57   0.00
  ex_n11_l100                 2.35   3.24    generic_n_n18               0.35   6.38
  ex_n19_l80                  1.00   0.08    lg_batch_waves_n11          0.57   0.00
  split_l193                  0.47   0.34    lg_batch_waves_n18          0.35   6.38
  backsub_split_l1025         3.09   7.51
scale, diag and gradient sit at the floor (ratios <= 0.46: the GPU's sums are as good as numpy's); gn and step are conditioning-limited
on both sides (e64 1e-10 .. 6e-9), worst 3.10 -> MARGIN 16.  model: off the Gauss-Newton branch it inherits the step's error to first
order, on the GPU (1.5e-11 .. 3.3e-11 relative in every interpolated case) and in numpy alike (e64 typically 2e-12 .. 2e-11).  The 62.76 is
window 0 (L = 37, interpolated branch) of ragged_batch_st: the GPU's error there is an ordinary 3.26e-11, numpy's e64 an unusually
small 5.05e-13; every other case is at most 8.03.  62.76 is below the 100 that would make it a finding -> MARGIN_MODEL 256.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import step_highprec as sh
from step_cases import CASES, DEFAULT, MU0, expected_path      # (shared with tests/test_solve_plan.py, which runs the path rules on the CPU)
from isvins_amd import abi, backend, synth

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
LD = np.longdouble
RADIUS = 1e4                 # initial_trust_region_radius (k_init_state)

MARGIN = 16.0                # vectors: 4 x 3.10 = 12.4 -> 16
MARGIN_MODEL = 256.0         # model: 4 x 62.76 = 251 -> 256 (no ratio reaches the 100 that would make it a finding)


def margin_of(k):
    return MARGIN_MODEL if k == "model" else MARGIN


SEEN = {}                    # case id -> dogleg branch of its (first) window


def P(a):
    return a.ctypes.data_as(dp)


# ---- states ---------------------------------------------------------------------------------------------------------------
def converged(oracle, w, est_ex=0):
    """tests/test_oracle_solver.py::test_converged_solution_is_stationary: the oracle's solution with the ORIGINAL priors"""
    from scipy.spatial.transform import Rotation as Rot
    cfg = abi.make_config(w.N, w.Nvo, num_iterations=60, estimate_extrinsic=est_ex)
    o = w.clone(); s = abi.isv_summary_t(); mg = abi.isv_marg_result_t()
    assert oracle.isvo_optimize(C.byref(cfg), C.byref(o.c()), C.byref(s), C.byref(mg)) == 0
    c = w.clone()
    for i in range(w.N):
        c.Ps[i] = o.para_Pose[i, :3]; c.Rs[i] = Rot.from_quat(o.para_Pose[i, 3:]).as_matrix()
        c.Vs[i] = o.para_SpeedBias[i, :3]; c.Bas[i] = o.para_SpeedBias[i, 3:6]; c.Bgs[i] = o.para_SpeedBias[i, 6:]
    c.lm_depth[: w.L] = 1.0 / o.para_Feature[: w.L]
    return c


def make_state(oracle, spec):
    kw = dict(spec.get("make", {}))
    ws = []
    for k, L in enumerate(spec.get("Ls", [spec["L"]])):
        w = synth.make_window(spec["wid"] + k, n_frames=spec["N"], n_vo=spec["Nvo"], n_landmarks=L, margin_old=0, **kw)
        if spec.get("ex"):
            from scipy.spatial.transform import Rotation as Rot
            w.ric[:] = w.ric @ Rot.from_rotvec((0.01, -0.008, 0.012)).as_matrix(); w.tic[:] = w.tic + np.array((0.01, -0.01, 0.005))
        state = spec.get("state", "x0")
        if state == "converged":
            w = converged(oracle, w, spec.get("ex", 0))
        elif state != "x0":
            w = sh.perturb(w, float(state))
        ws.append(w)
    return ws


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- one case -------------------------------------------------------------------------------------------------------------
def gpu_strips(be, w, est_ex):
    ps, im, cost = be.linearize(w)
    prior = be.debug_read(0, sh.prior_strip_size(w.Nvo, be.cfg.max_rollpitch))
    jex = be.debug_read(22, w.n_factors * 12) if est_ex else None
    return ps, im, prior, jex


def candidate_window(oracle, w, delta_p, delta_l, est_ex):
    """Evaluator::Plus(x0, delta) as a window (the oracle's own pose Plus)"""
    from scipy.spatial.transform import Rotation as Rot
    c = w.clone()

    def plus(p3, R, d6):
        x = np.zeros(7); xp = np.zeros(7)
        x[:3] = p3; oracle.isvo_x_R2q(P(np.ascontiguousarray(R)), P(x[3:]))
        oracle.isvo_x_pose_plus(P(x), P(np.ascontiguousarray(d6)), P(xp))
        return xp[:3], Rot.from_quat(xp[3:]).as_matrix()
    for i in range(w.N):
        d = delta_p[15 * i: 15 * i + 15]
        c.Ps[i], c.Rs[i] = plus(w.Ps[i], w.Rs[i], d[:6])
        c.Vs[i] = w.Vs[i] + d[6:9]; c.Bas[i] = w.Bas[i] + d[9:12]; c.Bgs[i] = w.Bgs[i] + d[12:15]
    if est_ex:
        t, R = plus(w.tic, w.ric, delta_p[15 * w.N: 15 * w.N + 6])
        c.tic[:] = t; c.ric[:] = R
    c.lm_depth[: w.L] = 1.0 / (1.0 / w.lm_depth[: w.L] + delta_l)
    return c


def compare(ref, f64, got, prob, nres):
    """{vector: (err_gpu, e64, floor)} in the norm of the module docstring.  Steps (delta) go back to the scaled space with the
    REFERENCE's scalings; the dummy columns of a free extrinsic's pseudo-frame are left out (and their step must be zero)."""
    n_p = prob.np
    real = np.concatenate([prob.real_p, np.ones(prob.L, bool)])
    out = {}

    def both(name, g_p, g_l, r, e):
        g = np.concatenate([g_p, g_l])[real]
        out[name] = (sh.err(g, r[real]), sh.err(e[real], r[real]), sh.floor_of(int(real.sum())))
    both("scale", got["scale_p"], got["scale_l"], ref.scale, f64.scale)
    both("diag", got["diag_p"], got["diag_l"], ref.diag, f64.diag)
    both("gradient", got["grad_p"], got["grad_l"], ref.gradient, f64.gradient)
    both("gn", got["gn_p"], got["gn_l"], ref.gn, f64.gn)
    to_scaled = ref.diag / ref.scale
    gd = np.concatenate([got["delta_p"], got["delta_l"]])
    assert not np.any(gd[:n_p][~prob.real_p]), "the dummy columns of the extrinsic's pseudo-frame moved"
    both("step", (gd * to_scaled)[:n_p], (gd * to_scaled)[n_p:], ref.step, f64.step)
    out["model"] = (abs(float((LD(got["model"]) - ref.model) / ref.model)), abs(float((LD(f64.model) - ref.model) / ref.model)), sh.floor_of(nres))
    return out


def run_case(name, oracle, capfd, corrupt=None):
    """runs one case; returns [(window, Problem, reference Step, float64 Step, GPU vectors)], asserting the kernel path"""
    spec = CASES[name]
    est_ex = spec.get("ex", 0)
    ws = make_state(oracle, spec)
    N, Nvo = spec["N"], spec["Nvo"]
    backend.build()
    env = dict(spec.get("env", {}), ISV_DEBUG_PATH="1")
    capfd.readouterr()
    with environment(env):
        be = backend.Backend(N, Nvo, max_landmarks=max(w.L for w in ws), max_obs=max(w.n_obs for w in ws),
                             max_batch=spec.get("max_batch", 1), num_iterations=1, estimate_extrinsic=est_ex)
    path = capfd.readouterr().err
    try:
        strips = [gpu_strips(be, w, est_ex) for w in ws]
        gs = [w.clone() for w in ws]
        capfd.readouterr()
        sums, _ = be.optimize_batch(gs)
        run_err = capfd.readouterr().err
        cnt = be.last_counts()
        npd = 15 * (N + est_ex)
        Ltot = sum(w.L for w in ws)
        sel = dict(gn_p=10, gn_l=11, grad_p=12, grad_l=13, scale_p=14, scale_l=15, diag_p=16, delta_p=17, delta_l=18, cost_c=19, model=20, diag_l=23)
        raw = {k: be.debug_read(s, len(ws) * npd if k.endswith("_p") else Ltot if k.endswith("_l") else len(ws)) for k, s in sel.items()}
        with pytest.raises(backend.BackendError):                   # a count beyond the buffer is refused, not read
            be.debug_read(10, spec.get("max_batch", 1) * npd + 1)
    finally:
        be.close()
    # the intended kernels really ran: the counters, and the library's own account of the handle and of the enqueue
    exp = dict(DEFAULT, **spec.get("expect", {}))
    lds_T = int(re.search(r"lds_T=(\d)", path).group(1))
    assert lds_T == exp["lds_T"], path
    if lds_T:
        assert cnt[4] == exp["fused_visual"], cnt
        if exp["fused_control"] is not None:
            assert cnt[5] == exp["fused_control"], cnt
        assert cnt[6] == exp["solve_st"] == int(re.search(r"solve_st=(\d)", path).group(1)), (cnt, path)
        assert (cnt[7] > 0) == bool(exp["split"]), cnt
    said = {}
    for line in (path + run_err).splitlines():
        if line.startswith("isv: handle ") or line.startswith("isv: enqueue "):
            said.update({k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)})
    want = expected_path(spec, lds_T, len(ws), max(w.L for w in ws))
    print(f"PATH  {name} {said}")
    assert {k: said.get(k) for k in want} == want, (name, said, want)
    assert cnt[0] == cnt[1] == 1, cnt                               # one slot: one linearisation, one solve
    out = []
    lm_off = np.concatenate([[0], np.cumsum([w.L for w in ws])])
    for b, (w, (ps, im, prior, jex), s) in enumerate(zip(ws, strips, sums)):
        assert s.iterations == 1
        prob = sh.Problem(w, ps, im, prior, jex)
        if corrupt is not None:
            corrupt(prob)
        ref, f64 = sh.reference_pair(prob, spec.get("mu", MU0), RADIUS)
        got = {k: (v[b * npd:(b + 1) * npd] if k.endswith("_p") else v[lm_off[b]:lm_off[b + 1]] if k.endswith("_l") else v[b]) for k, v in raw.items()}
        out.append((w, prob, ref, f64, got))
    return out, be.cfg


def worst_ratio(cmp):
    return max(e / max(e64, fl) for e, e64, fl in cmp.values())


@pytest.mark.parametrize("name", list(CASES))
def test_step_against_extended_precision(oracle, capfd, name):
    spec = CASES[name]
    res, cfg = run_case(name, oracle, capfd)
    worst = 0.0
    for b, (w, prob, ref, f64, got) in enumerate(res):
        cmp = compare(ref, f64, got, prob, prob.nres)
        for k, (e, e64, fl) in cmp.items():
            print(f"RATIO {name} w{b} {k:9s} err_gpu {e:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {e / max(e64, fl):.3f} [{ref.branch}]")
        worst = max(worst, worst_ratio(cmp))
        # the candidate cost against the oracle at x0 + the GPU's own step
        cand = candidate_window(oracle, w, got["delta_p"], got["delta_l"], spec.get("ex", 0))
        c_o = oracle.isvo_cost(C.byref(cfg), C.byref(cand.c()))
        print(f"COST  {name} w{b} cost_c {got['cost_c']:.15e} oracle {c_o:.15e} rel {abs(got['cost_c'] - c_o) / c_o:.2e}")
        if b == 0:
            SEEN[name] = ref.branch
        if name == "tracks_two_frames":
            assert set(np.diff(w.lm_obs_ptr[: w.L + 1])) == {2}
        if name == "tracks_whole_window":
            assert np.diff(w.lm_obs_ptr[: w.L + 1]).max() == w.N and not w.lm_start_frame[: w.L].any()
        if name == "frames_without_landmarks":
            assert w.lm_start_frame[: w.L].max() == 2
        if name == "backsub_split_l1025":
            assert prob.ncols > sh.DENSE_MAX_COLS                   # (the reference's eliminated preconditioner)
        assert abs(got["cost_c"] - c_o) < 1e-11 * c_o, (got["cost_c"], c_o)
        for k, (e, e64, fl) in cmp.items():
            assert e <= margin_of(k) * max(e64, fl), (name, b, k, e, e64, fl)
    print(f"WORST {name} {worst:.3f}")


def test_all_three_dogleg_branches_were_seen(oracle, capfd):
    """the cases above reach the Gauss-Newton step inside the radius, the scaled gradient (Cauchy) step and the interpolation;
    run alone, this test runs the three cases that do"""
    for name in ("n3_l25", "n11_l65", "n21_l60_dense"):
        if name not in SEEN:
            SEEN[name] = run_case(name, oracle, capfd)[0][0][2].branch
    assert set(SEEN.values()) == {sh.GAUSS_NEWTON, sh.CAUCHY, sh.INTERPOLATED}, SEEN


# ---- the check must be able to fail ---------------------------------------------------------------------------------------
def _drop_last_landmark(prob):
    drop = set(prob.proj_block_of_landmark[prob.L - 1])
    prob.blocks = [b for k, b in enumerate(prob.blocks) if k not in drop]
    prob.nres = sum(len(r) for r, _ in prob.blocks)


def _negate_chain_off_diagonal(prob):
    k = prob.kinds.index("imu") + 4                                  # the fifth IMU factor: its speed/bias_i block (columns 15 i + 6 ..)
    prob.blocks[k][1][1] = (prob.blocks[k][1][1][0], -prob.blocks[k][1][1][1])


def _scale_one_jlambda(prob):
    for k in prob.proj_block_of_landmark[prob.L // 2]:
        c, J = prob.blocks[k][1][-1]
        prob.blocks[k][1][-1] = (c, J * (1.0 + 1e-6))


@pytest.mark.parametrize("corruption", [_drop_last_landmark, _negate_chain_off_diagonal, _scale_one_jlambda], ids=lambda f: f.__name__[1:])
def test_corrupted_reference_is_rejected(oracle, capfd, corruption):
    """negative control on (11, 5, 65): the REFERENCE is corrupted (no fault goes into a kernel), and the comparison that passes
    above must reject it: the last landmark's factors dropped from J (measured: step off by 1.2e5 yardsticks), the speed/bias_i
    Jacobian block of one IMU factor negated -- which negates that factor's off-diagonal chain block of J^T J (4e8), one landmark's
    J_lambda scaled by 1 + 1e-6 (the step moves by only 2 yardsticks -- the system is that ill-conditioned -- but diag by 5e5)"""
    res, _ = run_case("n11_l65", oracle, capfd, corrupt=corruption)
    w, prob, ref, f64, got = res[0]
    cmp = compare(ref, f64, got, prob, prob.nres)
    for k, (e, e64, fl) in cmp.items():
        print(f"CORRUPT {corruption.__name__[1:]} {k:9s} err_gpu {e:.3e} e64 {e64:.3e} ratio {e / max(e64, fl):.3f}")
    assert any(e > margin_of(k) * max(e64, fl) for k, (e, e64, fl) in cmp.items()), cmp
