"""Cases, limits and negative controls of the 40-digit comparison of the loop-closure verification (tests/loop_highprec.py), shared by
tests/test_loop_highprec.py (the CPU restatement) and tests/test_gpu_loop_highprec.py (k_loop_match / k_loop_pnp).

Every pair is built with loop.make_loop_scene (through loop_cases.make_scene, which puts the unmatchable window points between the
matchable ones, so that a point's window index `src` differs from its position in the match list).  The new seeds were searched with the
CPU restatement for the event each case is named after (the pair counts give RANSACUpdateNumIters' value by the formula; the search
only had to place the first all-inlier subset), then confirmed with the reference, whose conditions every case meets.  The events are
asserted by tests/test_loop_highprec.py::test_edges_are_taken.  k_loop_pnp draws its hypotheses in chunks of 64.

  name          config  matches  data                       event
  stop64        100     29       12 outliers, exact         17 inliers: log(0.01) / log(1 - (17/29)^5) = 64.196 -> stops at 64, the last
                                                            hypothesis of the first chunk
  stop65        100     41       17 outliers, 0.5 px        24 inliers: 64.675 -> 65, the second chunk is drawn with one hypothesis
  keep2_f63     100     158      95 outliers, 0.5 px        the final model is first kept at hypothesis 81 (0-based), in the second chunk, over
                                                            a model of 7 kept in the first; runs to the cap; 63 final inliers
  out60_noise   100     (loop_cases)                        the cap of 100 with a model kept in the first chunk
  all_outliers  100     (loop_cases)                        the cap with no model at all
  none129       129     all_outliers' pair                  chunks of 64, 64 and 1; no model
  late129       129     48       26 outliers, 0.5 px        the final model is first kept at hypothesis 128, the third chunk's only one
  floor4        100     16       12 outliers, exact         4 inliers: no model (the cap, PNP_FAILED); the keep rule's floor, see keep_ge
  f64 f65 f129  100     70 72 142  6 7 13 outliers, 0.5 px  64, 65 and 129 final inliers: the mask / compaction / pnp_solve lane loops at, one
                                                            past, and two passes past the wavefront (63: keep2_f63)
  noise2 out30_noise m17 m200   (loop_cases)                the default noisy shapes
  yaw40 far25 planar            (loop_cases)                one case per non-OK status that the float layer decides
  l5            0.02    40       exact, one corner moved    the L5 control's case, built like test_quirk_l5_changes_a_pair: point 7's corner is
                                                            moved by 0.02 and the threshold 0.020000014056714158 lies between its float32
                                                            error (the same float32 number under every basis of the family) and its error in
                                                            doubles (which moves by some 1e-6 over the family and stays on the other side): an
                                                            inlier in float32 (40 inliers) and an outlier in doubles (39)

Limits: PnP_R_old, PnP_T_old, loop_info, res, loop_weight: max-norm error over the 2-norm of the 40-digit value, against
MARGIN * max(e64, n 2^-53); e64 is the plain float64 route's own error, n the vector's length.  res / loop_weight are compared on the
noisy cases only (NOISY): on exact data the residual is float32 rounding noise.  Each margin is 4 x the worst ratio measured, rounded up
to a power of two (the tables: tests/test_gpu_loop_highprec.py and DESIGN.md section 14).

Controls corrupt the reference; CONTROL_CASES names where each has power (shown by tests/test_loop_highprec.py on the CPU):
  keep_ge          >= in the keep rule: `floor4`, where hypothesis 81 has exactly 4 inliers under every basis of the family and no
                   hypothesis has more, so that 4 >= max(0, 4) keeps a model where 4 > 4 keeps none (ransac_inliers 4 against 0).  A tie
                   ABOVE the floor has no admissible case: two models with equal counts and different masks need points at the
                   threshold, and with such points the counts depend on the EPnP basis (tried: 19 scenes with planted 8.5 .. 11.5 px
                   corners, every one failed the `basis` condition); with equal masks the final solve, hence every output, is the same
  keep_no_floor    g > best without the floor of 4: all_outliers / none129 keep a model of one or two chance inliers (ransac_inliers 0)
  model_points_4   RANSACUpdateNumIters with 4 model points: every case that stops by it (stop64 -> 36, stop65 -> 37)
  l5_off           the threshold compared in doubles: `l5`
  no_l3            loop_weight without the extra division by FOCAL_LENGTH: res by 460, loop_weight by 460^2
  t_untransposed   T_w_c_old = R_pnp (-T_pnp)
  quat_xyzw        loop_info's quaternion as x y z w
  turned_1e-11     the final pose turned by 1e-11 rad"""
import numpy as np

import loop_cases
import loop_highprec as lh
from isvins_amd import loop

L5_THRESHOLD = 0.020000014056714158
CONFIGS = {"100": dict(), "129": dict(ransac_iterations=129), "l5": dict(ransac_threshold=L5_THRESHOLD)}
FROM_LOOP_CASES = ("stop64", "stop65", "keep2_f63", "out60_noise", "all_outliers", "floor4", "f64", "f65", "f129", "noise2", "out30_noise", "m17", "m200",
                   "yaw40", "far25", "planar")
CASES = {n: (n, "100") for n in FROM_LOOP_CASES}
CASES.update(none129=("all_outliers", "129"), late129=("late129", "129"), l5=(None, "l5"))
NOISY = ("stop65", "keep2_f63", "out60_noise", "late129", "f64", "f65", "f129", "noise2", "out30_noise", "m17", "m200")
NEW = ("stop64", "stop65", "keep2_f63", "floor4", "none129", "late129", "f64", "f65", "f129", "l5")


def names():
    return list(CASES)


def config(key, max_pairs=1):
    c = loop_cases.config(max_pairs)
    for k, v in CONFIGS[key].items():
        setattr(c, k, v)
    return c


def l5_pair():
    pair, tr = loop.make_loop_scene(seed=62, n_points=40, n_keypoints=100, old_pose=loop_cases.OLD_POSE)
    pair.keypoints_norm[int(tr["counterpart"][7]), 0] += np.float32(0.02)
    return pair


_pairs = {}


def pair(name):
    if name not in _pairs:
        scene = CASES[name][0]
        _pairs[name] = l5_pair() if scene is None else loop_cases.make_scene(dict(loop_cases.scene_cases())[scene])[0]
    return _pairs[name]


# ------------------------------------------------------------------------------------------------------------------ limits and controls
POWER = 8.0                      # a control must change an integer output or move a compared vector by at least this many limits
MARGIN = 32.0                    # the restatement: 4 x the worst measured ratio (5.59, out30_noise's res), rounded up to a power of two
MARGIN_GPU = 32.0                # k_loop_pnp on the MI355X, by the same rule, kept separate
CONTROL_CASES = {
    "keep_ge": ("floor4",),
    "keep_no_floor": ("all_outliers", "none129"),
    "model_points_4": ("stop64", "stop65"),
    "l5_off": ("l5",),
    "no_l3": tuple(n for n in NOISY if n != "late129"),
    "t_untransposed": ("stop64", "f65", "noise2", "yaw40"),
    "quat_xyzw": ("stop64", "f65", "noise2", "m17"),
    "turned_1e-11": ("stop64", "f65", "noise2", "yaw40", "far25"),
}
_refs = {}


def reference(name, control=None):
    """the 40-digit reference of a case, computed once per process (it depends on the pair alone, not on the result under test)"""
    if (name, control) not in _refs:
        if control in lh.TAIL_CONTROLS:
            _refs[name, control] = reference(name).with_tail_control(control)
        else:
            _refs[name, control] = lh.Reference(config(CASES[name][1]), pair(name), control)
    return _refs[name, control]


def floats_of(name):
    return lh.FLOATS if name in NOISY else lh.FLOATS[:3]


def measure(name, ref, res, mi, md, inl):
    """(the integer outputs and per-point arrays that differ, {quantity: error / its limit without the margin})"""
    bad, num = lh.compare(ref, res, mi, md, inl, floats_of(name))
    return bad, lh.ratios(num)


def failures(name, ref, res, mi, md, inl, margin):
    """what an assertion against `ref` would report: the differing integer outputs and the quantities beyond their limits"""
    bad, ratios = measure(name, ref, res, mi, md, inl)
    return bad + [f"{k} {r:.3g}" for k, r in ratios.items() if r > margin]


def power(name, ref, res, mi, md, inl, margin):
    """how strongly a corrupted reference rejects a record: inf for a differing integer output, else the worst error in limits"""
    bad, ratios = measure(name, ref, res, mi, md, inl)
    return float("inf") if bad else max(r / margin for r in ratios.values())
