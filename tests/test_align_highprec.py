"""The CPU restatement of the visual-inertial alignment (tests/native/isv_init_oracle.c) against the 40-digit model of tests/align_highprec.py,
stage by stage, and the conditions that the model, its limits and its negative controls must meet WITHOUT the kernel.  The cases are
tests/align_cases.py's; tests/test_gpu_align_highprec.py runs the same comparison on k_visual_imu_align.

The bound on the three solve stages is the float64 limit itself (margin 1).  Whether the limit FORMULAS are adequate is decided here,
not on the GPU: two float64 evaluations that share no code -- the restatement (pivoted LDLT, serial sums) and a plain one (numpy.linalg.solve)
-- must both stay within 1/2 of every limit.  Measured, worst ratio per stage (the rebuild's limit is 16 yardsticks):

  case           restatement: gyro linear refine rebuild      plain float64: gyro linear refine rebuild
  nf4                         0.000 0.034 0.314 0.045                        0.000 0.066 0.392 0.045
  nf11                        0.000 0.060 0.196 0.062                        0.000 0.022 0.100 0.062
  nf11_noisy                  0.248 0.078 0.056 0.062                        0.248 0.061 0.103 0.062
  nf16_nonkey                 0.000 0.010 0.094 0.062                        0.000 0.040 0.126 0.062
  nf20                        0.001 0.032 0.348 0.059                        0.001 0.087 0.364 0.059
  nf21_nonkey                 0.001 0.048 0.205 0.062                        0.001 0.023 0.219 0.062
  nf40_cap                    0.001 0.042 0.260 0.062                        0.001 0.032 0.262 0.062
  discrete                    0.000 0.013 0.340 0.062                        0.000 0.115 0.357 0.062
  wide_slow                   0.000 0.042 0.059 0.062                        0.000 0.054 0.043 0.062

The gyro stage's delta_bg sits at 1e-3 of its limit: the count C_QUAT = 40 is a worst case over some forty roundings that in fact cancel
like noise; it is a count, not a fit, and stays.  nf11_noisy's 0.248 is the one rounding of Bgs = Bgs_in + delta_bg.

Control powers (how far the corrupted model lies from the true one, in limits; it must be 8 at least): q2_off 40 (nf20) .. 8.7e6,
drop_last_pair_tail 1.4e9 .. 3.1e12, scale_100_dropped 7.3e7 .. 7.2e10, jac_transposed 1.1e5 .. 4.2e10, q3_frame_index 3.2e12 .. 4.3e13."""
import pytest

import align_cases as ac
import align_highprec as ah
import align_oracle

HALF = 0.5
_REFS = {}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


def reference(lib, name):
    """the case's problem solved by the restatement and the 40-digit model of that record, once per case"""
    if name not in _REFS:
        p = ac.problem(name)
        r = align_oracle.solve(lib, p)
        assert r.status == 0, (name, r.status)
        _REFS[name] = ac.Reference(name, p, r)
    return _REFS[name]


@pytest.mark.parametrize("name", list(ac.CASES))
def test_restatement_and_float64_within_half_of_every_limit(lib, name):
    ref = reference(lib, name)
    ref.check_conditions()
    for tag, ratios in (("restatement", ref.ratios()), ("float64", ref.e64_ratios())):
        worst = ac.report(tag, name, ratios)
        for s, r in worst.items():
            assert r <= HALF, (tag, name, s, ratios[s])
    lin, rfn = ref.stage("linear").lim, ref.stage("refine").lim
    print(f"LIMIT {name:12s} g_linear {lin['g_linear'].max():.1e} s_linear {lin['s_linear'][0]:.1e} g_c0 {rfn['g_c0'].max():.1e} "
          f"s {rfn['x'][-1]:.1e} delta_bg {ref.stage('gyro').lim['delta_bg'].max():.1e}")


def test_worst_ratio_per_stage(lib):
    """over all cases, for the record: both float64 routes within 1/2 of the limit at every stage"""
    for tag in ("restatement", "float64"):
        per_case = [reference(lib, n).ratios() if tag == "restatement" else reference(lib, n).e64_ratios() for n in ac.CASES]
        worst = {s: max(max(r[s].values()) for r in per_case) for s in ah.STAGES}
        print(f"WORST {tag:12s} " + " ".join(f"{s} {w:.3f}" for s, w in worst.items()))
        assert max(worst.values()) <= HALF, (tag, worst)


def test_refinement_agrees_with_lu_solve(lib):
    """every system of the 4- and 11-frame cases (n = 3, 15, 16, 36, 37) and LinearAlignment's at 20 frames (n = 64): 1e-30"""
    systems = [sv for name in ("nf4", "nf11") for s in ("gyro", "linear", "refine") for sv in reference(lib, name).stage(s).solves]
    systems.append(reference(lib, "nf20").stage("linear").solves[0])
    for sv in systems:
        lu, it = ah.solve_lu(sv.A, sv.b), ah.solve_refined(sv.A, sv.b)
        scale = max(abs(v) for v in lu)
        assert max(abs(a - b) for a, b in zip(lu, it)) <= ah.mp.mpf("1e-30") * scale, len(sv.b)


@pytest.mark.parametrize("control,name", [(c, n) for c, names in ac.CONTROL_CASES.items() for n in names])
def test_control_has_power_and_is_rejected(lib, control, name):
    """the corrupted model lies at least POWER limits from the true one, and the restatement's record, held against the corrupted model,
    is outside a limit"""
    ref = reference(lib, name)
    power, rej = ref.power(control), ref.rejects(control)
    print(f"CONTROL {control:20s} {name:12s} power {power:.3g} restatement / corrupted model {rej:.3g}")
    assert power >= ac.POWER, (control, name, power)
    assert rej > 1.0, (control, name, rej)


def test_control_cases_leave_out_only_no_ops(lib):
    """a case is missing from a control only where the control does nothing: q3_frame_index without frames outside the window gives the same
    model to the last digit; jac_transposed and q2_off on exact data move it by less than one limit"""
    for name in set(ac.CASES) - set(ac.CONTROL_CASES["q3_frame_index"]):
        inp = ah.Inputs(ac.problem(name))
        assert inp.kf == list(range(inp.nf))
    ref = reference(lib, "discrete")
    assert set(ac.CASES) - set(ac.CONTROL_CASES["jac_transposed"]) == {"discrete"} == set(ac.CASES) - set(ac.CONTROL_CASES["q2_off"])
    assert ref.power("jac_transposed") < 1.0 and ref.power("q2_off") < 1.0
    assert all(set(ac.CONTROL_CASES[c]) == set(ac.CASES) for c in ("drop_last_pair_tail", "scale_100_dropped"))
