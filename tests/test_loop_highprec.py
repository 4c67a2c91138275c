"""The CPU restatement of the loop-closure verification (tests/native/isv_loop_oracle.c, which compiles the kernel's own text
is-vins_amd/csrc/isv_loop_common.h) against the independent 40-digit reading tests/loop_highprec.py, on the cases of
tests/loop_highprec_cases.py: EPnP alone from the basis the restatement used, the DLT + CvLevMarq alone, the whole pair (all integer
fields and the three per-point arrays identical, the floats by ratio), the case list's edges, and every negative control with its power.

Measured ratios error / max(e64, n 2^-53) of the restatement (this file, one x86-64 host; the table per case is in
tests/test_gpu_loop_highprec.py next to the kernel's):
  EPnP stage     worst 1.76 over 5 (exact, noisy, one outlier), 6, 16 and 60 points       -> MARGIN_EPNP 8
  DLT + LM       worst 9.54 over 6, 16 and 60 noisy points, the iteration counts identical -> MARGIN_ITERATIVE 64
  whole pair     worst 5.59 (out30_noise, res)                                            -> loop_highprec_cases.MARGIN 32
Each margin is 4 x the worst ratio, rounded up to a power of two; a ratio of 100 or more would be a finding, not a margin."""
import numpy as np
import pytest

import loop_cases
import loop_highprec as lh
import loop_highprec_cases as lc
import loop_oracle
from isvins_amd import loop

MARGIN_EPNP = 8.0
MARGIN_ITERATIVE = 64.0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return loop_oracle.build(tmp_path_factory.mktemp("loop_oracle"))


@pytest.fixture(scope="module")
def records(lib):
    """the restatement's answers for the case list, computed once"""
    return {n: loop_oracle.verify(lib, lc.config(lc.CASES[n][1]), lc.pair(n)) for n in lc.names()}


def _points(seed, n, noise=0.0, outlier=False):
    """n non-planar points in front of a camera, their projections (+ noise, + one gross outlier), everything rounded to float32 as the
    RANSAC's points are"""
    rng = np.random.Generator(np.random.PCG64(0x10E9_0000 + seed))
    R = loop.synth._rot_zyx(0.4 - 0.1 * seed, 0.2, -0.3)
    t = np.array([0.3, -0.2, 0.5])
    z = rng.uniform(2, 8, n)
    pc = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    X = ((pc - t) @ R).astype(np.float32).astype(np.float64)
    uv = pc[:, :2] / pc[:, 2:3] + noise * rng.standard_normal((n, 2))
    if outlier:
        uv[n // 2] += [0.2, -0.15]
    return X, uv.astype(np.float32).astype(np.float64)


EPNP_CASES = [(5, 0.0, False), (5, loop_cases.NOISE, False), (5, loop_cases.NOISE, True), (6, loop_cases.NOISE, False),
              (16, loop_cases.NOISE, False), (60, loop_cases.NOISE, False)]


@pytest.mark.parametrize("n,noise,outlier", EPNP_CASES)
def test_epnp_stage(lib, n, noise, outlier):
    """lp_epnp against epnp::compute_pose at 40 digits from the basis lp_epnp used (five points: its null pair projected onto the exact
    null space): R and t within MARGIN_EPNP max(e64, n 2^-53), the same N chosen"""
    for seed in range(3):
        X, uv = _points(seed + 10 * n, n, noise, outlier)
        R, t, cws, vv = loop_oracle.epnp_basis(lib, X, uv)
        ref = lh.epnp_from_hook(X.tolist(), uv.tolist(), cws.tolist(), vv.tolist())
        assert ref["resid"] < 1e-6, (n, seed, ref["resid"])      # the hook's basis is the exact one to rounding (five points: in its span)
        for name, got, want, w64 in (("R", R.ravel(), sum(ref["R"], []), sum(ref["R64"], [])), ("t", t, ref["t"], ref["t64"])):
            e, e64 = lh.err(list(got), want), lh.err(list(w64), want)
            ratio = e / max(e64, len(got) * 2.0 ** -53)
            print(f"RATIO epnp n={n} noise={noise > 0} outlier={outlier} seed={seed} {name}: err {e:.2e} e64 {e64:.2e} ratio {ratio:.3g}")
            assert ratio <= MARGIN_EPNP, (n, seed, name, e, e64)


@pytest.mark.parametrize("n", [6, 16, 60])
def test_dlt_and_levmarq_alone(lib, n):
    """the planarity test, the DLT and the CvLevMarq trajectory on noisy points: the iteration count identical, the pose by ratio; the
    reference's own decisions off their edges"""
    for seed in range(3):
        X, uv = _points(seed + 100 * n, n, loop_cases.NOISE)
        st = dict(min_gate=1.0, min_lm=1.0, dlt_gap=0.0, min_det=1.0)
        planar, par, iters, trail = lh.iterative(X.tolist(), uv.tolist(), lh.MP, st)
        planar64, par64, iters64, trail64 = lh.iterative(X.tolist(), uv.tolist(), lh.F64)
        assert not planar and not planar64 and iters == iters64 and [u for u, _ in trail] == [u for u, _ in trail64]
        assert st["min_gate"] > 1e-9 and st["dlt_gap"] < 0.5 and st["min_det"] > 1e-9, st
        pl, Rg, tg, it = loop_oracle.iterative(lib, X, uv)
        assert pl == 0 and it == iters, (n, seed, it, iters)
        Rm, R64 = lh.sh.rodrigues(par[:3]), lh.rodrigues64(par64[:3])[0]
        for name, got, want, w64 in (("R", Rg.ravel(), sum(Rm, []), R64.ravel()), ("t", tg, par[3:], par64[3:])):
            e, e64 = lh.err(list(got), want), lh.err(list(w64), want)
            ratio = e / max(e64, len(got) * 2.0 ** -53)
            print(f"RATIO iterative n={n} seed={seed} {name}: iterations {iters} err {e:.2e} e64 {e64:.2e} ratio {ratio:.3g}")
            assert ratio <= MARGIN_ITERATIVE, (n, seed, name, e, e64)


@pytest.mark.parametrize("name", lc.names())
def test_restatement_against_reference(records, name):
    ref = lc.reference(name)
    ref.conditions()
    r, mi, md, inl = records[name]
    bad, ratios = lc.measure(name, ref, r, mi, md, inl)
    print(f"RATIO {name}: status {r.status} n_matched {r.n_matched} ransac_iters {r.ransac_iters} ransac_inliers {r.ransac_inliers} n_final {r.n_final} "
          f"pnp_iterations {r.pnp_iterations} solved at 40 digits {ref.ransac.n_mp if ref.ransac else 0}; "
          + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert lc.failures(name, ref, r, mi, md, inl, lc.MARGIN) == []


def test_edges_are_taken():
    """the events the cases are named after, on the reference"""
    ref = {n: lc.reference(n) for n in lc.names()}
    last_keep = lambda n: ref[n].ransac.keeps[-1][0]      # noqa: E731
    assert (ref["stop64"].n_matched, ref["stop64"].n_final, ref["stop64"].ransac_iters) == (29, 17, 64) and last_keep("stop64") < 64
    assert (ref["stop65"].n_matched, ref["stop65"].n_final, ref["stop65"].ransac_iters) == (41, 24, 65) and last_keep("stop65") < 64
    assert ref["keep2_f63"].ransac_iters == 100 and 64 <= last_keep("keep2_f63") < 100 and len(ref["keep2_f63"].ransac.keeps) > 1
    assert ref["keep2_f63"].ransac.keeps[0][0] < 64                       # Lbest holds a first-chunk model when the second chunk is drawn
    assert ref["out60_noise"].ransac_iters == 100 and last_keep("out60_noise") < 64 and ref["out60_noise"].status == lh.OK
    for n, iters in (("all_outliers", 100), ("floor4", 100), ("none129", 129)):
        assert (ref[n].ransac_iters, ref[n].ransac_inliers, ref[n].n_final, ref[n].status) == (iters, 0, 0, lh.PNP_FAILED)
    assert ref["late129"].ransac_iters == 129 and last_keep("late129") == 128 and ref["late129"].status == lh.OK
    assert [ref[n].n_final for n in ("keep2_f63", "f64", "f65", "f129")] == [63, 64, 65, 129]
    for n in ("stop64", "stop65", "keep2_f63", "late129", "f64", "f65", "f129"):          # src differs from the list position
        assert not np.array_equal(ref[n].src, np.arange(ref[n].n_matched)) and ref[n].n_points > ref[n].n_matched
    assert [ref[n].status for n in ("yaw40", "far25", "planar")] == [lh.GATE, lh.GATE, lh.PLANAR]
    assert ref["l5"].ransac_inliers == 40 and lc.reference("l5", "l5_off").ransac_inliers == 39


@pytest.mark.parametrize("control", lh.CONTROLS)
def test_every_control_is_rejected(records, control):
    """a corrupted reference must reject the restatement's record on the cases the control is meant for"""
    assert lc.CONTROL_CASES[control], control
    for name in lc.CONTROL_CASES[control]:
        r, mi, md, inl = records[name]
        assert lc.failures(name, lc.reference(name), r, mi, md, inl, lc.MARGIN) == []
        bad = lc.reference(name, control)
        p = lc.power(name, bad, r, mi, md, inl, lc.MARGIN)
        print(f"CONTROL {control} on {name}: power {p:.3g}; {lc.failures(name, bad, r, mi, md, inl, lc.MARGIN)}")
        assert p >= lc.POWER, (control, name, p)
