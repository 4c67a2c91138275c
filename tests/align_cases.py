"""Cases, conditions and negative controls of the 40-digit comparison of the visual-inertial alignment (tests/align_highprec.py), shared by
tests/test_align_highprec.py (the CPU restatement) and tests/test_gpu_align_highprec.py (k_visual_imu_align).

Cases (initial.make_problem): the smallest shapes at which the kernel can still go wrong, and the capacity.  n is the number of unknowns
of LinearAlignment / RefineGravity.
  nf4            4 frames, n = 16 / 15: the smallest non-singular system (2 and 3 frames have 6 (nf - 1) rows < 3 nf + 4 unknowns), cond2 ~ 1e12
  nf11           the default window
  nf11_noisy     IMU noise, a gyro bias and a non-zero Bgs on entry: the only case whose delta_bg is far from zero
  nf16_nonkey    five frames of all_image_frame outside the window: quirk Q3
  nf20           n = 64 / 63: exactly one stride of the 64 lanes
  nf21_nonkey    n = 67 / 66: the first wrap of the row- and entry-strided loops; frame 10 is outside the window (20 is ISV_ALIGN_MAX_WINDOW)
  nf40_cap       n = 124 / 123: ISV_ALIGN_MAX_FRAMES, the LDS maximum; every second frame is a keyframe
  discrete       poses that follow the pre-integration exactly: residuals near zero, the limit's |A^-1| |b| term carries it
  wide_slow      a 3 m circle at 0.5 m/s
Singular inputs (2 and 3 frames, hover, the refusals) have no exact answer to compare with; they stay in the parity and bitwise tests.

Controls are corruptions of the MODEL (align_highprec.CONTROLS), never of the code under test.  Q2 makes pass k of RefineGravity enter the
final matrix with weight 1000^(k - 4): a corruption of the last pass alone moves x by a fraction of the limit and cannot be seen, so every
control acts in every pass (or in a stage without passes).  A case is left out of a control only where the control does nothing there:
  q3_frame_index   needs frames outside the window (with none, the keyframe counter IS the frame index);
  jac_transposed   needs a residual to act on: on `discrete` the gyro residuals are zero to rounding (|b| ~ 1e-16) and delta_bg with them;
  q2_off           needs passes that disagree: on `discrete` every pass's equations hold exactly, so every pass, and any weighting of the
                   passes, has the same solution (measured: the model moves by 0.04 limits).
Before a control is used, tests/test_align_highprec.py shows that it moves some compared output by at least POWER limits."""
import numpy as np

import align_highprec as ah
from isvins_amd import initial

POWER = 8.0                      # a control must move the model by at least this many limits where it is used
MAX_COND = 1e13                  # cond2 of every solved matrix: the 40-digit solve keeps more than 25 digits
MAX_RESIDUAL = 1e-30             # |A x - b| / |b| of every 40-digit solve
TIGHTER = 10.0                   # the limits on g_linear, g_c0, s_linear, s against test_gpu_align.py's tolerances, nf >= 11
GPU_ALIGN_RTOL = 1e-8            # tests/test_gpu_align.py: |a - b| <= 1e-8 max(1, max|b|) on g_linear, g_c0, g, s_linear, s
# The one place where the limits are NOT tighter than test_gpu_align.py's tolerances: on the wide, slow circle (cond2 3e12, as bad as 4
# frames) float64 itself allows 6.8e-8 on s_linear and 4.0e-8 on RefineGravity's s, where that test grants 2.7e-8.  Its two sides do the
# same operations, so it passes there; the limit, not the round tolerance, is what the format supports.  Asserted as found.
SCALE_NOT_TIGHTER = ("wide_slow",)

CASES = {
    "nf4": dict(n_frames=4),
    "nf11": dict(),
    "nf11_noisy": dict(seed=1, acc_noise=0.01, gyr_noise=0.001, bg=(0.01, -0.02, 0.005), Bgs0=np.full((11, 3), 0.002)),
    "nf16_nonkey": dict(n_frames=16, window_frame=[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 15]),
    "nf20": dict(n_frames=20, cam_dt=0.05),
    "nf21_nonkey": dict(n_frames=21, cam_dt=0.05, window_frame=[f for f in range(21) if f != 10]),
    "nf40_cap": dict(n_frames=initial.ISV_ALIGN_MAX_FRAMES, window_frame=list(range(0, 40, 2)), cam_dt=0.05, imu_per_frame=5),
    "discrete": dict(discrete=True),
    "wide_slow": dict(radius=3.0, speed=0.5),
}
ALONE = ("nf4", "nf21_nonkey", "nf40_cap")      # also solved in a batch of one: bytewise the mixed batch's result

_NONKEY = ("nf16_nonkey", "nf21_nonkey", "nf40_cap")
CONTROL_CASES = {
    "q2_off": tuple(c for c in CASES if c != "discrete"),
    "drop_last_pair_tail": tuple(CASES),
    "scale_100_dropped": tuple(CASES),
    "jac_transposed": tuple(c for c in CASES if c != "discrete"),
    "q3_frame_index": _NONKEY,
}
# bytewise fields of the GPU result against the restatement, if "operation by operation" holds: everything before libm
BYTEWISE_FIELDS = ("delta_bg", "Bgs", "rp_delta_p", "rp_delta_q", "rp_delta_v", "rp_sum_dt", "g_linear", "s_linear", "x", "g_c0")


def problem(name):
    p = initial.make_problem(**CASES[name])
    assert p.c.n_window <= initial.ISV_ALIGN_MAX_WINDOW and p.c.n_frames <= initial.ISV_ALIGN_MAX_FRAMES
    return p


class Reference:
    """the 40-digit model of one case for one result record, its stages computed on demand and kept"""

    def __init__(self, name, p, res):
        self.name, self.inp = name, ah.Inputs(p)
        self.val = ah.result_values(self.inp, res)
        self._stages = {}

    def stage(self, s, control=None):
        if (s, control) not in self._stages:
            self._stages[s, control] = ah.model(self.inp, self.val, (s,), control)[s]
        return self._stages[s, control]

    def ratios(self, control=None, stages=ah.STAGES):
        """{stage: {field: worst |result - model| / limit}} of the record this reference was built for"""
        return {s: self.stage(s, control).ratios(self.val) for s in stages}

    def e64_ratios(self):
        """the same for the plain float64 evaluation of every stage"""
        return {s: self.stage(s).ratios(self.stage(s).e64) for s in ah.STAGES}

    def check_conditions(self):
        """what the reference alone must meet (module docstring of align_highprec / the constants above)"""
        for s in ("gyro", "linear", "refine"):
            for sv in self.stage(s).solves:
                assert sv.cond < MAX_COND, (self.name, s, sv.cond)
                assert sv.resid < MAX_RESIDUAL, (self.name, s, sv.resid)
        if self.inp.nf >= 11:
            for s, k in (("linear", "g_linear"), ("refine", "g_c0"), ("rebuild", "g")):
                tol = GPU_ALIGN_RTOL * max(1.0, float(np.abs(self.val[k]).max()))
                assert np.all(TIGHTER * self.stage(s).lim[k] <= tol), (self.name, k, self.stage(s).lim[k], tol)
            n = 3 * self.inp.nf + 3
            for lim, v in ((self.stage("linear").lim["s_linear"][0], self.val["s_linear"][0]),
                           (self.stage("refine").lim["x"][n - 1], self.val["x"][n - 1]), (self.stage("rebuild").lim["s"], self.val["s"][0])):
                tol = GPU_ALIGN_RTOL * max(1.0, abs(v))
                if self.name in SCALE_NOT_TIGHTER and lim > 1e-12:       # (the two solved scales; the rebuild's s is a copy)
                    assert tol < lim < 4.0 * tol, (self.name, lim, tol)
                else:
                    assert TIGHTER * lim <= tol, (self.name, lim, v)

    def power(self, control):
        """how far the corrupted model lies from the true one, in limits of the true one (the worst over the stages it reaches)"""
        return max(self.stage(s).moved(self.stage(s, control)) for s in ah.CONTROLS[control])

    def rejects(self, control):
        """the worst ratio of the record against the corrupted model over the stages the control reaches: above 1 is a rejection"""
        return max(max(r.values()) for r in self.ratios(control, ah.CONTROLS[control]).values())


def report(tag, name, ratios):
    """one line per stage: the worst ratio and its field (the rebuild's also in yardsticks: its limit is 16 of them)"""
    worst = {}
    for s, r in ratios.items():
        k = max(r, key=r.get)
        worst[s] = r[k]
        extra = f" = {16.0 * r[k]:.3f} yardsticks" if s == "rebuild" else ""
        print(f"RATIO {tag:12s} {name:12s} {s:8s} worst {r[k]:.3f} ({k}){extra}")
    return worst
