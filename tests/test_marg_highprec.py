"""The CPU oracle's MargForward / MargBackward against the 40-digit recomputation (tests/marg_highprec.py), LIVE on the suite's own
synthetic windows -- the windows on which tests/test_gpu_solve.py::check_marg holds the GPU to the oracle at 1e-6.  The cases, the
yardstick and the conditions are tests/marg_cases.py's; tests/test_gpu_marg_highprec.py runs the same comparison on the HIP kernels.

Measured (max-norm relative error of the information matrix | float64_limit | err / max(e64, float64_limit, floor)):

  case            forward_pose_prior        combined_relpose          backward_relpose          backward_vb               backward_rollpitch
  n6_l25          2.0e-11 1.3e-13 150.17    4.7e-13 1.3e-13  3.49     3.5e-7 5.7e-7 0.62        2.3e-7 5.7e-7 0.41        1.0e-8 5.7e-7 0.018
  n11_l40         2.0e-11 1.7e-13 117.15    3.7e-13 1.7e-13  2.18     2.2e-7 5.6e-7 0.40        1.4e-7 5.6e-7 0.26        6.3e-9 5.6e-7 0.011
  n18_l40         9.5e-12 8.6e-14 111.17    3.4e-13 8.6e-14  3.96     4.8e-7 5.5e-7 0.88        3.3e-7 5.5e-7 0.60        1.7e-8 5.5e-7 0.030
  n11_l300        2.5e-11 8.2e-13  30.68    4.2e-13 8.2e-13  0.52     4.3e-7 5.5e-7 0.78        2.8e-7 5.5e-7 0.51        1.5e-8 5.5e-7 0.027
  n11_host0_l33   3.6e-11 5.1e-13  70.43    4.9e-13 5.1e-13  0.96     2.9e-7 5.5e-7 0.32        2.0e-7 5.5e-7 0.32        2.0e-9 5.5e-7 0.004
  n11_host0_l65   3.0e-11 8.5e-13  35.09    4.2e-13 8.5e-13  0.49     2.7e-7 5.5e-7 0.49        1.8e-7 5.5e-7 0.34        4.0e-9 5.5e-7 0.007
  n11_none        3.6e-16 4.6e-14   0.01    1.3e-15 4.6e-14  0.03     2.0e-7 5.8e-7 0.34        1.3e-7 5.8e-7 0.22        9.6e-9 5.8e-7 0.016
  n11_l40_ex      2.5e-14 1.9e-13   0.13    6.9e-16 1.9e-13  0.004    3.4e-7 5.8e-7 0.52        2.2e-7 5.8e-7 0.38        6.0e-9 5.8e-7 0.010

e64 (not shown) is 2e-16 .. 1e-14 forward and 1e-9 .. 9e-7 backward: a plain float64 MargBackward is no closer than the oracle.
Backward: the oracle sits at 0.88 of the cancellation limit at worst -> MARGIN_CPU_BWD = 4 (4 x 0.875 = 3.5).  Forward: the 150 is the
oracle's full-pivot LU inverse of the (landmarks + 6)^2 block Lamda_mm, which restates the reference's `Lamda_mm.inverse()`
(tests/test_marg_third_opinion.py; the closed-form elimination is at e64 ~ 1e-15) -> MARGIN_CPU_FWD = 1024 (4 x 150.17 = 601).  Two margins,
not one: a single 1024 would let the backward factors drift to 5e-4.

The measurement parts (delta_t, delta_R, VB, R, t) are plain functions of the states: 1e-12 against the 40-digit values (measured 2e-16)."""
import numpy as np
import pytest

import marg_cases as mc
import marg_highprec as mh
from isvins_amd import abi

MARGIN_CPU_FWD = 1024.0
MARGIN_CPU_BWD = 4.0


@pytest.mark.parametrize("name", list(mc.CASES))
def test_oracle_marginalisation_against_40_digits(oracle, name):
    n_marg = mc.CASES[name][6]
    o, cfg0 = mc.solved_case(oracle, name)
    o2, s, mo = mc.oracle_run(oracle, cfg0, o)
    assert s.iterations == 0 and mo.valid == 1 and mo.n_marg_landmarks == n_marg
    ins = mh.inputs_from_window(cfg0, o2)
    assert len(ins["lam"]) == n_marg
    ref = mc.Reference(ins)
    ref.check_conditions(n_marg)
    res = ref.ratios(mo)
    for k, (e, e64, lim, r) in res.items():
        print(f"RATIO {name} {k:20s} err {e:.2e} e64 {e64:.2e} limit {lim:.2e} ratio {r:.3f}")
    for k, (e, e64, lim, r) in res.items():
        assert r <= (MARGIN_CPU_BWD if k in mc.BWD else MARGIN_CPU_FWD), (name, k, e, e64, lim)
    want = ref.measurements(ins)
    for k, v in mc.measured_parts(mo).items():
        assert np.abs(abi.arr(v) - want[k]).max() < 1e-12, (name, k)


def test_float64_limit_is_the_cancellation_bound():
    """2^-52 max|Lam| / min(kept), and e64_backward really meets a matrix that cancels: a 30 x 30 Lam whose 9 x 9 block couples at 1e11
    into a marginal of order 1e2 loses what the bound says (within 100x either way), not the 1e-16 of a well-scaled one"""
    assert mh.float64_limit(np.diag([2e11, 1.0]), [80.0, 1e9]) == 2.0 ** -52 * 2e11 / 80.0
    rng = np.random.default_rng(0)
    import mpmath as mp
    G = rng.standard_normal((30, 30))
    Lam = G @ np.diag(np.concatenate([np.full(15, 1e2), np.zeros(6), np.full(9, 1e11)])) @ G.T
    Lm = mp.matrix(Lam.tolist())
    A, Bm, Dm = mh.sub(Lm, 0, 21, 0, 21), mh.sub(Lm, 0, 21, 21, 30), mh.sub(Lm, 21, 30, 21, 30)
    Lp = A - Bm * mp.inverse(Dm) * Bm.T
    U, Dv, Eall = mh.eig_truncate(Lp, mp.mpf("0.1"))
    assert len(Dv) == 15
    Jr = mp.eye(21)
    b = {"_bwd_Lam": Lm, "_bwd_Jr": Jr, "backward_relpose": mh.project_info(mh.sub(Jr, 0, 6, 0, 21), U, Dv),
         "backward_vb": mh.project_info(mh.sub(Jr, 6, 15, 0, 21), U, Dv), "backward_rollpitch": mh.project_info(mh.sub(Jr, 15, 17, 0, 21), U, Dv)}
    e = max(mh.e64_backward(b, 0.1).values())
    lim = mh.float64_limit(Lam, [float(d) for d in Dv])
    print(f"e64 {e:.2e} limit {lim:.2e}")
    assert 1e-2 * lim < e < 1e2 * lim and e > 1e-12
