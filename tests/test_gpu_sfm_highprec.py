"""k_sfm's bundle adjustment (csrc/isv_sfm.hip, stage 2) on the cases of tests/sfm_highprec.py -- one small scene per loop-count edge of
its strided loops -- against the problem recomputed at 40 digits (pinned to the CPU restatement by tests/test_sfm_highprec.py, never to
the kernel).  Three handles, created with ISV_DEBUG_SFM_BA_ITERS = 0, 1 and 2, each solve the whole case list in ONE batch (three
launches); the reference is computed on the CPU from the GPU's own outputs:
  a. the integer outputs (status, ba_iterations, ba_successful, ba_termination, n_triangulated, n_ba_cols) are the restatement's at
     the same cap;
  b. ba_initial_cost against cost(x0), x0 read from the cap-0 output; then per iteration k = 1, 2, linearised at the GPU's own cap-(k-1)
     state: the accept / reject decision, the stored positions and Q / T against Plus(x, step), ba_final_cost against the candidate's
     cost; a rejected iteration must leave the state bit for bit;
  c. every case alone == in the mixed batch, bitwise (the LDS carve-up follows the batch's largest problem, so the n_window = 3 case
     runs under the n_window = 20 layout);
  d. negative controls: the REFERENCE corrupted (never the kernel) must be rejected by (b).

Tolerance.  Yardstick e64: the error of the reference's own float64 route (Jacobians rounded to float64, J.T @ J by numpy, LAPACK's
solve, costs and Plus by the same code at 53 bits) against its 40-digit route.  Norms: cost relative, floor (number of residuals) 2^-53;
positions and [Q | T]: max-norm of the difference over the 2-norm of the reference's step in that quantity, floor
2^-53 max(n, |x0|_inf / |step|_2), n = nc + 3 nact (the step is read back through stored states; Q / T pass S6's inversion once on the
device and once in the reference, a handful of rounded operations on entries of size |x0|_inf, inside the same floor).
A quantity passes when err_gpu <= MARGIN * max(e64, floor); MARGIN = 4 x the worst measured ratio, rounded up to a power of two.
Measured on one MI355X, ratio err_gpu / max(e64, floor) per case:
  case         cost0  position1   QT1  cost1  position2   QT2  cost2
  w3_l0         0.03       4.45  2.18   0.66       2.14  1.90   0.40
  w4_l2         0.06       1.03  3.84   0.44       0.83  8.47   0.37
  w5_n63        0.01       0.76  1.75   0.10       1.06  4.23   0.08
  w5_n64        0.00       0.33  1.04   0.00       0.56  0.48   0.08
  w5_n65        0.03       0.82  0.87   0.06       2.46  1.86   0.07
  w5_n131       0.03       0.62  2.42   0.01       0.77  1.20   0.02
  w11_l5        0.00       0.64  0.40   0.03       1.82  3.91   0.05
  w13_l6        0.03       0.39  0.32   0.01       0.64  1.46   0.02
  w20_l10       0.01       0.52  2.74   0.08       3.03  3.41   0.00
  w13_reject    0.01          -     -      -       3.63  0.99   3.51   (iteration 1 is rejected: the state is unchanged, bit for bit)
  w5_far        0.00       0.32  1.15   0.10       0.35  2.59   0.10
The costs sit under their floor; the states are conditioning-limited on both sides (e64 1e-14 .. 6e-13 of the step's norm).  Worst 8.47
(w4_l2, Q / T of iteration 2; the restatement has the same figure there) -> MARGIN = 4 x 8.47 = 33.9 -> 64.  No case stands apart from the rest
(every ratio is below 9; 100 would be a finding), and none needed a kernel change.
Negative controls on w5_far (the reference corrupted), off by, in yardsticks max(e64, floor), at the worst quantity:
  the quaternion tangent Jacobian scaled by 1/2                             1.7e13 (cost1)
  the LM diagonal left off the point blocks                                 1.9e12 (QT2)
  one observation dropped from one off-diagonal block of the reduced system 2.5e12 (position2)
  the Jacobi scaling recomputed at x1 instead of kept from x0               2.2e4  (position2)
"""
import numpy as np
import pytest

import sfm_highprec as sh
import sfm_oracle
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

MARGIN = 64.0                # 4 x 8.47 = 33.9 -> 64
CAPS = (0, 1, 2)
CONTROL_CASE = "w5_far"


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sh.bind(sfm_oracle.build(tmp_path_factory.mktemp("sfm_oracle")))


@pytest.fixture(scope="module")
def runs():
    """{cap: {"batch": [(result, positions, states)] in sh.NAMES order, "single": the same, every case in a call of its own}}"""
    out = {}
    for cap in CAPS:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("ISV_DEBUG_SFM_BA_ITERS", str(cap))
            be = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)     # the cap is read when the handle is created
        try:
            ps = [sh.make_case(n)[0] for n in sh.NAMES]
            rs = initial.sfm_batch(be, ps)
            out[cap] = {"batch": [(r, p.position.copy(), p.state.copy()) for r, p in zip(rs, ps)], "single": []}
            if cap == 2:
                for n in sh.NAMES:
                    p = sh.make_case(n)[0]
                    r = initial.sfm_batch(be, [p])[0]
                    out[cap]["single"].append((r, p.position.copy(), p.state.copy()))
        finally:
            be.close()
    return out


def _outs(runs, name):
    i = sh.NAMES.index(name)
    return [runs[cap]["batch"][i] for cap in CAPS]


# ---- a ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sh.NAMES)
def test_integer_outputs_are_the_restatements(lib, runs, name):
    for cap, (rg, pg, sg) in zip(CAPS, _outs(runs, name)):
        sp, ro, po, so = sh.oracle_capped(lib, name, cap)
        assert [getattr(rg, k) for k in sh.INTS] == [getattr(ro, k) for k in sh.INTS], (name, cap)
        assert rg.ba_iterations == cap and rg.ba_residuals == ro.ba_residuals and np.array_equal(sg, so)


# ---- b ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sh.NAMES)
def test_capped_ba_against_extended_precision(runs, name):
    rows, edges, _ = sh.check_chain(name, _outs(runs, name), "RATIO")
    print(f"WORST {name} {max(e / max(e64, fl) for _, e, e64, fl in rows):.3f}")
    for key, e, e64, fl in rows:
        assert e <= MARGIN * max(e64, fl), (name, key, e, e64, fl)


# ---- c ------------------------------------------------------------------------------------------------------------------------
def test_alone_is_bitwise_the_mixed_batch(runs):
    for name, (rb, pb, sb), (r1, p1, s1) in zip(sh.NAMES, runs[2]["batch"], runs[2]["single"]):
        assert bytes(rb) == bytes(r1) and np.array_equal(pb, p1) and np.array_equal(sb, s1), name
        assert rb.status == 0 and rb.ba_iterations == 2


# ---- d ------------------------------------------------------------------------------------------------------------------------
def _half_quaternion_jacobian(ref):
    ref.half_qjac = True


def _no_lm_diagonal_on_the_points(ref):
    ref.no_point_lm = True


def _one_observation_dropped_from_an_offdiagonal_block(ref):
    sp = sh.make_case(CONTROL_CASE)[0]
    j = next(j for j in ref.act if sp.tracks[j].n_obs == ref.nw)      # a whole-window track: it couples every pair of frames
    free = [f for f in range(ref.nw) if ref.ncf[f]]
    ref.drop_offdiag = (j, free[0], free[1])


def _jacobi_scaling_recomputed_at_x1(ref):
    ref.rescale = True


@pytest.mark.parametrize("corruption", [_half_quaternion_jacobian, _no_lm_diagonal_on_the_points, _one_observation_dropped_from_an_offdiagonal_block,
                                        _jacobi_scaling_recomputed_at_x1], ids=lambda f: f.__name__[1:])
def test_corrupted_reference_is_rejected(runs, corruption):
    """negative control on `w5_far`: the REFERENCE is corrupted (no fault goes into a kernel) and comparison (b), which passes above,
    must reject it.  The Jacobi scaling cancels from an LM step exactly unless a scaled diagonal entry sits on the 1e-6 clamp
    ((S J^T J S + diag(S J^T J S) / radius) y = -S J^T r with delta = S y is (J^T J + diag(J^T J) / radius) delta = -J^T r), so the
    last control can only be caught on a case with a clamped column: w5_far has one (the depth of its far point), and the control
    bites at iteration 2, the first that is not linearised at x0.  Measured sizes: the module docstring."""
    rows, _, clamped = sh.check_chain(CONTROL_CASE, _outs(runs, CONTROL_CASE), "CORRUPT " + corruption.__name__[1:], corrupt=corruption)
    assert clamped > 0
    worst = max(rows, key=lambda t: t[1] / max(t[2], t[3]))
    print(f"CORRUPT {corruption.__name__[1:]} off by {worst[1] / max(worst[2], worst[3]):.3e} yardsticks ({worst[0]})")
    assert any(e > MARGIN * max(e64, fl) for _, e, e64, fl in rows)
