"""Pins tests/pgo_highprec.py -- the 40-digit restatement of the pose-graph problem and the loop topologies of the GPU test -- to the
CPU oracle (oracle/isv_pgo_oracle.c), before tests/test_gpu_pgo_highprec.py trusts it.  Per topology: the builder's claims hold (it
asserts them itself); the reference's cost at x0 is the oracle's trace_cost[0] to 1e-12; the oracle ACCEPTS the first step (the
one-step GPU comparison would compare nothing otherwise: the perturbations in pgo_highprec.SPECS were chosen so); the oracle's poses
after one iteration and its covariances after the full solve, at the oracle's own final poses, agree with the reference.

Tolerance: err <= MARGIN_ORACLE * max(e64, floor), e64 the error of the reference's own float64 route (numpy / LAPACK) against its
40-digit one, floor = 2^-53 max(n, |x0|_inf / |step|_2) for the step (the step is read back through the stored pose) and n 2^-53 for
a covariance block, n = 6 nf.  Measured worst ratio err / max(e64, floor) per topology (oracle: dense Cholesky and a dense inverse):
  chain_k2              0.26      onto_first_free       2.31      ring_pos0             5.63
  chain_k3              1.93      nested                3.52      ring_pos1             8.40
  chain_k9              1.91      crossing              5.69      ring_pos2             6.37
  chain_k10             1.62      back_to_back          6.29      ring_pos3             5.37
  span2                 4.87      adjacent_rows         4.32      ring_pos4             5.76
  span3                 4.94      shared_match          4.07      ring_pos5             4.06
  span9                 2.63      cur_in_the_middle     5.33      ring_pos6             4.78
  span10                6.82      seq0_prefix           1.50      ring_pos7             7.24
  span18                6.92      sparse_rollpitch      5.67      ring_pos8             4.07
  onto_constant_first   8.36      forward               4.07
worst 8.40 (ring_pos1) -> MARGIN_ORACLE = 4 x 8.40 = 33.6 -> 64.
"""
import pytest

import pgo_highprec as ph
from isvins_amd import abi
from test_oracle_pgo import oracle_pgo

MARGIN_ORACLE = 64.0         # 4 x 8.40 = 33.6 -> 64


@pytest.mark.parametrize("name", ph.TOPOLOGIES)
def test_reference_against_the_oracle(oracle, name):
    kf, first, cur = ph.make_topology(name)
    o1, r1 = oracle_pgo(oracle, kf, first, cur, max_iterations=1)
    o10, r10 = oracle_pgo(oracle, kf, first, cur)
    ref, st = ph.first_step(name)
    assert r1.status == 0 and r10.status == 0
    assert (r1.n_poses, r1.n_free, r1.n_loop_edges) == (len(ref.local), ref.nf, len(ref.loop_edges))
    c0 = float(ref.cost(ref.x))
    assert abs(r1.trace_cost[0] - c0) <= 1e-12 * c0, (r1.trace_cost[0], c0)
    assert r1.iterations == 1 and r1.trace_accepted[1] == 1 and r10.trace_accepted[1] == 1          # the first step is accepted
    assert float(st["model"]) > 0
    e, e64, fl = ph.step_errors(ref, st, ph.keyframe_TR(o1, first, cur))
    print(f"RATIO {name} step err_oracle {e:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {e / max(e64, fl):.3f}")
    worst = e / max(e64, fl)
    assert e <= MARGIN_ORACLE * max(e64, fl), (name, e, e64, fl)
    x = ph.poses_of(o10, first, cur, "opt")
    cov, cov64 = ph.reference(kf, first, cur, x).covariance(x)
    assert all(o10[k].cov_computed == 1 for k in ref.local[:-1]) and o10[cur].cov_computed == 0
    fl = 6 * ref.nf * 2.0 ** -53
    errs = ph.cov_errors(cov, cov64, [abi.arr(o10[k].cov) for k in ref.local[:-1]])
    assert len(errs) == ref.nf - 1                    # every free pose before cur; the constant ones are zero (cov_errors asserts it)
    if errs:
        k, ec, ec64 = max(errs, key=lambda t: t[1] / max(t[2], fl))
        print(f"RATIO {name} cov  err_oracle {ec:.3e} e64 {ec64:.3e} floor {fl:.1e} ratio {ec / max(ec64, fl):.3f} (block {k})")
        worst = max(worst, ec / max(ec64, fl))
    print(f"WORST {name} {worst:.3f}  iterations {r10.iterations} accepted {list(r10.trace_accepted[1: r10.iterations + 1])} termination {r10.termination}")
    for k, ec, ec64 in errs:
        assert ec <= MARGIN_ORACLE * max(ec64, fl), (name, k, ec, ec64, fl)


def test_the_list_reaches_both_huber_regions_and_a_longer_solve(oracle):
    """across the topologies: loop residuals inside and outside the Huber radius at x0, and at least one default (10 iteration) solve
    with a rejected step or more than two accepted ones"""
    regions, long_runs = [], []
    for name in ph.TOPOLOGIES:
        kf, first, cur = ph.make_topology(name)
        regions += list(ph.loop_regions(kf, first, cur).values())
        _, r = oracle_pgo(oracle, kf, first, cur)
        acc = list(r.trace_accepted[1: r.iterations + 1])
        if r.num_successful > 2 or (0 in acc[:-1]) or (acc and acc[-1] == 0 and r.termination not in (2, 3)):
            long_runs.append(name)
    assert min(regions) < 1.0 < max(regions), (min(regions), max(regions))
    assert long_runs, "no topology takes more than two accepted steps or rejects one"
