"""Cases, limits and negative controls of the 40-digit comparison of the relative-pose stage (tests/relpose_highprec.py), shared by
tests/test_relpose_highprec.py (the CPU restatement) and tests/test_gpu_relpose_highprec.py (k_relpose).

make() builds a problem directly, so that the counts are exact: the frames and pre-integrations of an initial.make_scene problem, and tracks
from a generator that projects random points through known cameras.  `span` tracks are seen in every window frame (a correspondence of
every candidate), `from1` more from window frame 1 on (n_window = 4: a correspondence of candidate 1 only), the first `outliers` spanning
tracks (in a shuffled order) have a uniform point of [-0.6, 0.6]^2 for their last observation, `noise` is white noise on every observation.
`lead` tracks that are no correspondence of any candidate stand in front and `every` of them after each counted track (alternately one
that ends before the last frame and one that starts after the last candidate), so that the kernel's 64-track ballot compaction carries a
non-zero prefix from pass to pass.  far0 puts camera 0 two hundredths of a baseline from the last one, turned by 0.15 rad: candidate 0 has
its correspondences and 69 px of parallax, its RANSAC keeps a model, and recoverPose refuses every point (250 baselines deep, dist = 50).

The seeds were searched with the CPU restatement (0.1 s a problem) for the event each case is named after, then confirmed with the
reference, whose conditions every case meets.  The events are asserted by tests/test_relpose_highprec.py::test_edges_are_taken.

  name            n_window  correspondences  data                    event
  c21_exact       3         21               exact                   the least the > 20 gate admits; stops at iteration 1 (ep = 0)
  c63_stop64      3         63               20 outliers             43 inliers: RANSACUpdateNumIters gives 64, the whole first chunk
  c64_noise       3         64               0.2 px                  one full pass of the 64-lane mask loop
  c65_noise       3         65               0.5 px                  one lane into the second pass
  c65_exact       3         65               exact                   kept deliberately: F's two singular values agree to 1e-7
  c129_stop65     3         129 (of 264)     41 outliers             88 inliers: 65, one hypothesis into the second chunk; third pass
  c129_mixed      3         129 (of 264)     26 outliers, 0.2 px     spanning tracks beyond index 128, others between them
  c40_late        3         40               20 outliers             the final model is first kept in a later chunk than the first
  c29_cap         3         29               16 outliers             13 inliers: the fewest correspondences that run to the 1000 cap
                                                                     with a pose (13 > 12 needs count >= 13 / 0.4636)
  c30_stop_early  3         30               6 outliers              stops inside the first chunk after a keep
  far0_then1      4         30, then 42      8 outliers              candidate 0 keeps a model and fails recoverPose; candidate 1
                                                                     restarts the RNG (R4)
and CASES of tests/test_gpu_relpose.py (old_0 .. old_12), r5 and its first three refusals (excitation, too few correspondences, low parallax), so that the
old cases get the new check.

Limits: parallax, a sum of `count` positive terms and a division, (count + 4) 2^-53 relative, margin 1 (derived).  excitation_var,
relative_R, relative_T: max-norm error over the 2-norm of the 40-digit value, against MARGIN * max(e64, n 2^-53); e64 is the plain float64
route's own error, n the vector's length.  Where the kept model comes from solveCubic's one-real-root branch the quantity is named
relative_R_cv / relative_T_cv and the yardstick is max(e64, ecv, n 2^-53) under MARGIN_CV: ecv is the spread of the DEFINITION there
(relpose_highprec.cv_single_root_model).  Each margin is 4 x the worst ratio measured, rounded up to a power of two.

Controls corrupt the reference; CONTROL_CASES names where each has power (shown by tests/test_relpose_highprec.py on the CPU):
  rng_carried        the RNG carried over between candidates: needs a candidate before l that ran a RANSAC
  keep_ge            >= in the keep rule: acts where a later model ties the last keep (it replaces the kept F; the integers may stay)
  t_not_transposed   Translation = -R t
  wrong_null_pair    the null space from the singular vectors 7 and 8 of 9, not 8 and 9 (on two small cases: nothing fits, so all is screened)
  turned_1e-11       the pose turned by 1e-11 rad: 62 limits on a three-root model, 4 where ecv sets the limit (c21_exact, left out)
Left out for want of power: W transposed in the decomposition swaps R1 and R2, which renames the four cameras and changes no compared
output; the threshold compared in doubles needs a point error in the float32 gap above thresh^2 (6e-8 wide), which no case has."""
import numpy as np

import relpose_highprec as rh
import test_relpose_oracle
from isvins_amd import initial, synth

PX = 1.0 / 460
NOISE = 0.5 * PX
OLD = [dict(seed=0), dict(seed=1), dict(seed=2), dict(seed=3), dict(seed=0, pixel_noise=NOISE), dict(seed=1, pixel_noise=NOISE),
       dict(seed=0, outliers=0.3), dict(seed=5, outliers=0.3, pixel_noise=NOISE), dict(seed=6, outliers=0.2, pixel_noise=0.2 / 460),
       dict(seed=0, n_window=5, per_frame=30), dict(seed=0, n_window=4, extra=4, per_frame=60), dict(seed=4, extra=6, n_window=18),
       dict(seed=7, n_window=20, extra=20, cam_dt=0.05, imu_per_frame=5, per_frame=400)]     # tests/test_gpu_relpose.py's CASES

NEW = {
    "c21_exact": dict(span=21, every=1, seed=0),
    "c63_stop64": dict(span=63, outliers=20, lead=3, every=1, seed=1),
    "c64_noise": dict(span=64, noise=0.2 * PX, every=2, seed=0),
    "c65_noise": dict(span=65, noise=0.5 * PX, lead=1, every=1, seed=91),
    "c65_exact": dict(span=65, lead=2, every=1, seed=0),
    "c129_stop65": dict(span=129, outliers=41, lead=6, every=1, seed=0),
    "c129_mixed": dict(span=129, outliers=26, noise=0.2 * PX, lead=6, every=1, seed=0),
    "c40_late": dict(span=40, outliers=20, every=1, seed=7),
    "c29_cap": dict(span=29, outliers=16, every=1, seed=6),
    "c30_stop_early": dict(span=30, outliers=6, lead=1, every=1, seed=1),
    "far0_then1": dict(n_window=4, span=30, from1=12, outliers=8, far0=True, every=1, seed=0),
}


def make(n_window=3, span=21, from1=0, outliers=0, noise=0.0, lead=0, every=0, far0=False, seed=0):
    base, _ = initial.make_scene(seed=0, n_window=n_window, extra=11 - n_window, per_frame=4)
    rng = synth.SplitMix64(0x7E1A905E0000 + seed)
    last = n_window - 1
    # camera k: centre C[k] and camera-to-last rotation R[k], in the last camera's frame
    C = [np.array([-0.45 * (last - k), 0.05 * (last - k), 0.02 * (last - k)]) for k in range(n_window)]
    R = [initial._rotvec(0.03 * (last - k) * np.array([0.5, -1.0, 0.3])) for k in range(n_window)]
    if far0:
        C[0], R[0] = np.array([0.02, 0.0, 0.0]), initial._rotvec(np.array([0.0, 0.15, 0.0]))
    counted = sorted([((j + 0.5) / span, "S") for j in range(span)] + [((j + 0.25) / from1, "F") for j in range(from1)])
    kinds = ["N"] * lead
    for _, kind in counted:
        kinds += [kind] + ["N"] * every
    n = len(kinds)
    u = rng.uniform(5 * n).reshape(-1, 5)
    nz = rng.normal(2 * n_window * n).reshape(n, n_window, 2)
    order = np.argsort(rng.uniform(span))
    bad = set(order[:outliers].tolist())
    tracks, obs, frame_pts, s_index, n_index = [], [], [[] for _ in range(11)], 0, 0
    window = [base.c.window_frame[k] for k in range(n_window)]
    for j, kind in enumerate(kinds):
        d = 4.0 + 6.0 * u[j, 0]
        X = np.array([(u[j, 1] - 0.5) * d, (u[j, 2] - 0.5) * d, d])
        if kind == "S":
            s, L = 0, n_window
        elif kind == "F":
            s, L = 1, n_window - 1
        else:
            s, L = ((0, n_window - 1), (n_window - 2, 2))[n_index % 2]
            n_index += 1
        uv = []
        for k in range(s, s + L):
            xc = R[k].T @ (X - C[k])
            uv.append(xc[:2] / xc[2] + noise * nz[j, k])
        if kind == "S":
            if s_index in bad:
                uv[-1] = (u[j, 3:5] - 0.5) * 1.2
            s_index += 1
        tid = 7 + 2 * j
        tracks.append((tid, s, L))
        for k, p in zip(range(s, s + L), uv):
            frame_pts[window[k]].append((tid, p[0], p[1]))
        obs.extend(uv)
    sp = initial.SfmProblem(n_window, 0, np.eye(3), np.zeros(3), np.array(base.c.RIC).reshape(3, 3), tracks, obs, frame_pts,
                            base.delta_v, base.sum_dt, window)
    sp.truth = dict(kinds=kinds, R=R, C=C)
    return sp


def names():
    return list(NEW) + [f"old_{k}" for k in range(len(OLD))] + ["r5"] + [f"refusal_{k}" for k in range(3)]


def problem(name):
    if name in NEW:
        return make(**NEW[name])
    if name.startswith("old_"):
        return initial.make_relpose_scene(**OLD[int(name[4:])])[0]
    if name == "r5":
        return test_relpose_oracle.r5_scene()
    sp = [c for c in test_relpose_oracle.refusal_cases() if c[2] in (1, 2)][int(name[8:])]
    return sp[1]


# ------------------------------------------------------------------------------------------------------------------ limits and controls
POWER = 8.0                      # a control must change an integer output or move a compared vector by at least this many limits
MARGIN = 64.0                    # the restatement: 4 x the worst measured ratio, rounded up to a power of two (table: DESIGN.md section 13)
MARGIN_CV = 4.0                  # one-root models against max(e64, ecv, floor): worst 0.90 (old_0) -> 3.6 -> 4, the same on both sides
MARGIN_GPU = 64.0                # k_relpose on the MI355X, by the same rule, kept separate (worst 15.5, old_2's relative_T, on both sides)
CONTROL_CASES = {
    "rng_carried": ("far0_then1", "old_5"),
    "keep_ge": ("c40_late", "old_4", "old_5", "old_8"),
    "t_not_transposed": tuple(NEW),
    "wrong_null_pair": ("c21_exact", "c30_stop_early"),
    "turned_1e-11": tuple(n for n in NEW if n != "c21_exact"),   # (c21_exact keeps a one-root model: its limit is 4 ecv, 2e-12)
}
_refs = {}


def reference(name, control=None):
    """the 40-digit reference of a case, computed once per process (it depends on the problem alone, not on the result under test)"""
    if (name, control) not in _refs:
        if control in rh.TAIL_CONTROLS:
            _refs[name, control] = reference(name).with_tail_control(control)
        else:
            _refs[name, control] = rh.Reference(problem(name), control)
    return _refs[name, control]


def measure(ref, res, mask):
    """(the integer outputs that differ, {quantity: error / its limit without the margin})"""
    bad, num = rh.compare(ref, res, mask)
    return bad, rh.ratios(num)


def margin_of(quantity, margin):
    return 1.0 if quantity.startswith("parallax") else MARGIN_CV if quantity.endswith("_cv") else margin


def failures(ref, res, mask, margin):
    """what an assertion against `ref` would report: the differing integer outputs and the quantities beyond their limits"""
    bad, ratios = measure(ref, res, mask)
    return bad + [f"{k} {r:.3g}" for k, r in ratios.items() if r > margin_of(k, margin)]


def power(ref, res, mask, margin):
    """how strongly a corrupted reference rejects a record: inf for a differing integer output, else the worst error in limits"""
    bad, ratios = measure(ref, res, mask)
    return float("inf") if bad else max(r / margin_of(k, margin) for k, r in ratios.items())
