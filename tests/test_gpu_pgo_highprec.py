"""k_pgo (csrc/isv_posegraph.hip) on the loop topologies of tests/pgo_highprec.py -- one small graph per branch of its hand-scheduled
factorisation, substitution and selected inversion -- against the problem recomputed at 40 digits (pinned to the CPU oracle by
tests/test_pgo_highprec.py, never to the kernel):
  a. the full solve (10 iterations) against the dense CPU oracle, tests/test_gpu_pgo.py's check_graph with its tolerances;
  b. ONE Levenberg-Marquardt step (a handle with max_iterations = 1; the oracle accepts every topology's first step, so the poses
     written back are Plus(x0, step)): trace_cost[0] against cost(x0), T_w_i / R_w_i against x1;
  c. the stored covariances after the full solve against (J^T J)^-1 at the GPU's OWN final poses, every stored entry;
  d. the dispatch forms on these topologies: batch == single calls, k_pgo<1> == k_pgo<4>, LDS == global index arrays, bitwise;
  e. negative controls: the REFERENCE corrupted (never the kernel) must be rejected by (b) or (c).
Two module-scoped handles carry every topology: the 10-iteration one and the one-iteration one (max_iterations is a handle setting).

Tolerance.  Yardstick e64: the error of the reference's own float64 route (Jacobians rounded to float64, J.T @ J by numpy, solve and
inverse by LAPACK, the cost by the same residual code at 53 bits) against its 40-digit route: what FP64 can do on this system, from
the reference side alone.  Norms: cost relative, floor (number of residuals) 2^-53; step: max-norm of the pose difference [T | R] over
the 2-norm of the reference step, floor 2^-53 max(n, |x0|_inf / |step|_2) (the step is read back through the stored pose); covariance:
per block, max-abs over the block's largest reference entry, floor n 2^-53; n = 6 nf.  A quantity passes when
err_gpu <= MARGIN * max(e64, floor); margins = 4 x the worst measured ratio, rounded up to a power of two.
Measured on one MI355X, worst ratio err_gpu / max(e64, floor) per topology, cost | step | covariance (worst block):
  chain_k2              2.78  0.26  0.00  shared_match          0.97  4.01  5.45
  chain_k3              1.15  3.91  0.40  cur_in_the_middle     1.33  5.79  3.49
  chain_k9              0.67  1.55  0.38  seq0_prefix           0.29  2.17  2.16
  chain_k10             0.58  2.02  1.04  sparse_rollpitch      0.40  7.79  1.58
  span2                 5.53  5.85  2.94  forward               0.67  5.14  3.29
  span3                 0.09  5.26  3.50  ring_pos0             0.59  6.04  2.92
  span9                 2.18  5.07  1.14  ring_pos1             0.40  7.98  7.03
  span10                0.56  6.34  1.74  ring_pos2             1.62  6.37  2.67
  span18                0.14  5.26  2.81  ring_pos3             0.83  5.37  0.83
  onto_constant_first   0.84  1.48  6.53  ring_pos4             0.18  7.55  3.15
  onto_first_free       0.28  1.79  0.73  ring_pos5             0.53  7.16  3.30
  nested                3.08  4.71  2.02  ring_pos6             0.18  4.81  1.16
  crossing              0.09  2.91  5.41  ring_pos7             0.02  5.94  0.98
  back_to_back          0.17  4.92  1.66  ring_pos8             0.25  6.77  2.60
  adjacent_rows         0.95  4.72  3.80
(chain_k2 has one free pose, cur's: no covariance block is stored for it, its 0.00 is not a measurement.)  The cost sits at the floor
(worst 5.53, span2); the step is conditioning-limited on both sides (e64 1e-14 .. 3e-13 of the step's norm), worst 7.98 (ring_pos1) -> MARGIN
32; covariance worst 7.03 (ring_pos1) -> MARGIN_COV 32.  No topology stands apart from the rest (every ratio is below 8; 100 would be a finding),
and none needed a kernel change.
"""
import pytest

import pgo_highprec as ph
from isvins_amd import abi, posegraph as pg
from test_gpu_pgo import check_graph
from test_oracle_pgo import oracle_pgo

pytestmark = pytest.mark.gpu

MARGIN = 32.0                # cost and step: 4 x 7.98 = 31.9 -> 32
MARGIN_COV = 32.0            # 4 x 7.03 = 28.1 -> 32


@pytest.fixture(scope="module")
def opt():
    from isvins_amd import backend
    backend.build()
    o = pg.PoseGraphOptimizer(32, max_graphs=16, max_loop_blocks=8 * 32)
    yield o
    o.close()


@pytest.fixture(scope="module")
def opt1():
    from isvins_amd import backend
    backend.build()
    o = pg.PoseGraphOptimizer(32, max_graphs=16, max_loop_blocks=8 * 32, max_iterations=1)
    yield o
    o.close()


def solve(opt, name):
    kf, first, cur = ph.make_topology(name)
    g = pg.clone_keyframes(kf)
    r = opt.optimize(g, first, cur)
    assert r.status == 0
    return kf, first, cur, g, r


# ---- a ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ph.TOPOLOGIES)
def test_full_solve_matches_the_oracle(oracle, opt, name):
    """(the forward loops of `forward` and `ring_pos0` are accepted by the oracle and by the library alike, status 0: check_graph
    asserts it -- they are cases like the others)"""
    kf, first, cur, g, rg = solve(opt, name)
    o, ro = oracle_pgo(oracle, kf, first, cur)
    check_graph(o, ro, g, rg, first, cur)
    assert rg.n_loop_edges == len(ph.structure(kf, first, cur)["loops"])


# ---- b ------------------------------------------------------------------------------------------------------------------------
def step_quantities(ref, st, g, rg, first, cur):
    return {"cost": ph.cost_errors(ref, ref.x, rg.trace_cost[0]), "step": ph.step_errors(ref, st, ph.keyframe_TR(g, first, cur))}


@pytest.mark.parametrize("name", ph.TOPOLOGIES)
def test_first_step_against_extended_precision(opt1, name):
    kf, first, cur, g, rg = solve(opt1, name)
    assert rg.iterations == 1 and rg.trace_accepted[1] == 1 and rg.num_successful == 1
    ref, st = ph.first_step(name)
    assert (rg.n_poses, rg.n_free) == (len(ref.local), ref.nf)
    q = step_quantities(ref, st, g, rg, first, cur)
    for k, (e, e64, fl) in q.items():
        print(f"RATIO {name} {k:5s} err_gpu {e:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {e / max(e64, fl):.3f}")
    for k, (e, e64, fl) in q.items():
        assert e <= MARGIN * max(e64, fl), (name, k, e, e64, fl)


# ---- c ------------------------------------------------------------------------------------------------------------------------
def cov_quantities(ref, g, first, cur):
    """[(block, err, e64, floor)] of the stored covariances against the reference at the GPU's own final poses"""
    x = ph.poses_of(g, first, cur, "opt")
    cov, cov64 = ref.covariance(x)
    for k in ref.local[:-1]:
        assert g[k].cov_computed == 1
    fl = 6 * ref.nf * 2.0 ** -53
    return [(k, e, e64, fl) for k, e, e64 in ph.cov_errors(cov, cov64, [abi.arr(g[k].cov) for k in ref.local[:-1]])]


@pytest.mark.parametrize("name", ph.TOPOLOGIES)
def test_covariances_against_extended_precision(opt, name):
    kf, first, cur, g, rg = solve(opt, name)
    ref = ph.reference(kf, first, cur, ph.poses_of(kf, first, cur, "vio"))
    q = cov_quantities(ref, g, first, cur)
    assert len(q) == ref.nf - 1                       # every free pose before cur; the constant ones are zero (cov_errors asserts it)
    if q:
        k, e, e64, fl = max(q, key=lambda t: t[1] / max(t[2], t[3]))
        print(f"RATIO {name} cov   err_gpu {e:.3e} e64 {e64:.3e} floor {fl:.1e} ratio {e / max(e64, fl):.3f} (block {k} of {len(q)})")
    for k, e, e64, fl in q:
        assert e <= MARGIN_COV * max(e64, fl), (name, k, e, e64, fl)


# ---- d ------------------------------------------------------------------------------------------------------------------------
def same_bits(a, ra, b, rb):
    assert bytes(a) == bytes(b)
    assert bytes(ra) == bytes(rb)
    assert ra.status == 0 and ra.iterations > 0


def test_ring_position_batch_is_bitwise_the_single_calls(opt):
    """the nine ring-position graphs in ONE optimize_batch call (nine workgroups, one launch) against their single calls"""
    tops = [ph.make_topology(n) for n in ph.RING]
    singles = []
    for kf, first, cur in tops:
        g = pg.clone_keyframes(kf)
        singles.append((g, opt.optimize(g, first, cur)))
    batch = [pg.clone_keyframes(kf) for kf, _, _ in tops]
    res = opt.optimize_batch(batch, [f for _, f, _ in tops], [c for _, _, c in tops])
    for (gs, rs), gb, rb in zip(singles, batch, res):
        same_bits(gs, rs, gb, rb)


def test_four_wavefronts_are_bitwise_the_one_wavefront_form(opt, monkeypatch):
    for name in ph.TOPOLOGIES:
        kf, first, cur = ph.make_topology(name)
        out = []
        for waves in ("1", "4"):
            monkeypatch.setenv("ISV_PGO_WAVES", waves)
            g = pg.clone_keyframes(kf)
            out.append((g, opt.optimize(g, first, cur)))
        try:
            same_bits(out[0][0], out[0][1], out[1][0], out[1][1])
        except AssertionError as err:
            raise AssertionError(name) from err


@pytest.mark.parametrize("name", ["nested", "crossing", "adjacent_rows"])
def test_global_index_path_is_bitwise_the_lds_one(opt, monkeypatch, name):
    kf, first, cur = ph.make_topology(name)
    a = pg.clone_keyframes(kf)
    ra = opt.optimize(a, first, cur)
    monkeypatch.setenv("ISV_PGO_IDX_GLOBAL", "1")
    b = pg.clone_keyframes(kf)
    rb = opt.optimize(b, first, cur)
    same_bits(a, ra, b, rb)


# ---- e ------------------------------------------------------------------------------------------------------------------------
def _drop_inner_loop_edge(ref):
    ref.drop = {ref.loop_edges[0]}                    # keyframe 8's loop (free row 7): the inner one


def _leave_out_one_fill_block(ref):
    r = max(r for r in range(ref.nf) if ref.start[r] < r - 1)
    ref.drop_fill = (r, (ref.start[r] + r) // 2)      # L(10, 5): an interior column of the outer loop row


def _scale_one_sqrt_rho(ref):
    ref.rho_scale = {ref.loop_edges[1]: 1 + ph.mp.mpf("1e-6")}


@pytest.mark.parametrize("corruption", [_drop_inner_loop_edge, _leave_out_one_fill_block, _scale_one_sqrt_rho], ids=lambda f: f.__name__[1:])
def test_corrupted_reference_is_rejected(opt, opt1, corruption):
    """negative control on `nested`: the REFERENCE is corrupted (no fault goes into a kernel) and the comparisons (b) and (c), which
    pass above, must reject it.  Measured, in yardsticks max(e64, floor) -- cost | step | worst covariance block:
    the inner loop edge (keyframe 8's) dropped from J                      3.1e11 | 1.6e12 | 3.4e13
    L(10, 5), one interior block of the outer loop row's fill, left out      3.09 |   4.72 | 1.2e13   (the covariance alone uses it)
    sqrt(rho') of the outer loop edge scaled by 1 + 1e-6                     3.09 | 1.5e6  | 5.9e7    (the cost does not use the corrector)"""
    name = "nested"
    kf, first, cur, g1, r1 = solve(opt1, name)
    _, _, _, g, _ = solve(opt, name)
    x0 = ph.poses_of(kf, first, cur, "vio")
    ref = ph.reference(kf, first, cur, x0)
    assert [r for r in range(ref.nf) if ref.start[r] < r - 1] == [7, 10] and ref.start[7] > ref.start[10]
    corruption(ref)
    q = step_quantities(ref, ref.lm_step(x0), g1, r1, first, cur)
    over = []
    for k, (e, e64, fl) in q.items():
        print(f"CORRUPT {corruption.__name__[1:]} {k:5s} err_gpu {e:.3e} e64 {e64:.3e} ratio {e / max(e64, fl):.3e}")
        over.append(e > MARGIN * max(e64, fl))
    k, e, e64, fl = max(cov_quantities(ref, g, first, cur), key=lambda t: t[1] / max(t[2], t[3]))
    print(f"CORRUPT {corruption.__name__[1:]} cov   err_gpu {e:.3e} e64 {e64:.3e} ratio {e / max(e64, fl):.3e} (block {k})")
    over.append(e > MARGIN_COV * max(e64, fl))
    assert any(over), (q, e, e64)
