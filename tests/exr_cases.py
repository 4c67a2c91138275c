"""The case table of the rotation calibration's tests (tests/test_exr_oracle.py, test_exr_highprec.py, test_gpu_exr.py,
test_gpu_exr_highprec.py): synthetic two-view scenes from a true ric, true body rotations and camera translations, and points at depth
2 .. 20.  A CASE is one frame on a fresh slot (frame_count 0, ric = I); a SEQUENCE is a list of frames on one slot under its own
configuration.  Each is named for what it reaches; tests/test_exr_oracle.py asserts from the restatement's own outputs that it does.

Every scene keeps each depth away from zero (no |depth| within 1e-3 of the point's norm), so the front counts do not depend on the
float32 reading of testTriangulation (X4): test_exr_oracle.py checks the counts with the hook off and on.

K_MEASURED is the restatement's worst ratio (error against the 40-digit reading) / (float64 limit of the solve) over this table, per
stage, as tests/test_exr_highprec.py measures and prints it; K is that times 8, for the libm and ordering slack between host and
device.  The GPU is held to the same K."""
import numpy as np

from isvins_amd import exrot as exr

RIC_TRUE_AXIS, RIC_TRUE_DEG = (0.3, -0.5, 0.8), 35.0
CFG = dict(max_slots=40, max_frames=12, max_corres=160, vo_size=8)        # the cases and most sequences

# stage -> the measured worst ratio on the CPU; the bound's K is 8 x that
# as printed by tests/test_exr_highprec.py: F at vo2[3], Rc at huber_over, row at excited[9], sigma at excited[3], ric at excited[6]
K_MEASURED = {"F": 0.450, "Rc": 3.993, "row": 1.222, "sigma": 5.279, "ric": 0.508}
K = {stage: 8 * v for stage, v in K_MEASURED.items()}


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * S @ S


def quat(axis, deg):
    """(w, x, y, z)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([[np.cos(h)], np.sin(h) * a])


RIC_TRUE = rot(RIC_TRUE_AXIS, RIC_TRUE_DEG)


def scene(seed, n, axis, deg, t_c, mismatch=0.0, ric=RIC_TRUE):
    """n correspondences of a body rotation (axis, deg) and a camera translation t_c (camera k+1 in camera k) -> (corres [n][4],
    delta_q (w x y z), the true Rc)"""
    rng = np.random.default_rng(seed)
    Rimu = rot(axis, deg)
    Rc = ric.T @ Rimu @ ric
    z = rng.uniform(2.0, 20.0, n)
    X = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], 1)
    X2 = (X - np.asarray(t_c, np.float64)) @ Rc          # rows: Rc^T (X - t)
    assert n == 0 or (X2[:, 2] > 0.5).all()
    c = np.concatenate([X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]], 1)
    bad = rng.permutation(n)[:int(round(mismatch * n))]
    c[bad, 2] = rng.uniform(-0.5, 0.5, len(bad)); c[bad, 3] = rng.uniform(-0.35, 0.35, len(bad))
    return np.ascontiguousarray(c), quat(axis, deg), Rc


def junk(seed, n):
    """unrelated points on both sides"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.35, 0.35, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.35, 0.35, n)], 1)
    return np.ascontiguousarray(c), quat((0.2, 0.9, -0.1), 7.0), None


class Frame:
    def __init__(self, corres, dq, Rc_true=None):
        self.corres, self.dq, self.Rc_true = corres, dq, Rc_true

    def item(self, slot):
        return exr.ExrItem(slot, self.corres, self.dq)


T0 = (0.25, -0.08, 0.1)
# name -> Frame.  The seeds of `negated`, `not_negated` and `tie` were searched for on the restatement (which branch the Jacobi SVD's
# signs give is not predictable from the scene); test_exr_oracle.py asserts they still reach their edge.
CASES = {
    "n0": Frame(np.zeros((0, 4)), quat((0, 0, 1), 9.0)),
    "n8_identity": Frame(*scene(1, 8, (0.1, 1, 0.2), 9.0, T0)),
    "n9_lmeds": Frame(*scene(2, 9, (0.1, 1, 0.2), 9.0, T0)),
    "n14_lmeds": Frame(*scene(3, 14, (1, 0.2, -0.3), 7.0, T0)),
    "n15_ransac": Frame(*scene(4, 15, (0.1, 1, 0.2), 9.0, T0)),
    "n63": Frame(*scene(5, 63, (0.4, -1, 0.2), 6.0, T0)),
    "n64": Frame(*scene(6, 64, (0.4, -1, 0.2), 6.0, T0)),
    "n65": Frame(*scene(7, 65, (0.4, -1, 0.2), 6.0, T0)),
    "n129": Frame(*scene(8, 129, (0.2, 0.3, 1), 8.0, T0)),
    "n150": Frame(*scene(9, 150, (0.2, 0.3, 1), 8.0, T0)),
    "n150_mismatch": Frame(*scene(10, 150, (0.2, 0.3, 1), 8.0, T0, mismatch=0.10)),
    "negated": Frame(*scene(11, 40, (0.1, 1, 0.2), 9.0, T0)),
    "not_negated": Frame(*scene(13, 40, (0.1, 1, 0.2), 9.0, T0)),
    "tie": Frame(*junk(5, 10)),
    "pure_translation": Frame(*scene(14, 60, (0, 0, 1), 0.0, (0.3, 0.05, -0.1))),
    "huber_over": Frame(*scene(15, 50, (1, 0.1, 0.1), 16.0, T0)),
    "huber_under": Frame(*scene(16, 50, (1, 0.1, 0.1), 8.25, T0)),
}

AXES = [(1, 0.1, 0.2), (0.1, 1, -0.2), (0.2, -0.1, 1), (1, 1, 0.1), (-0.3, 1, 1), (1, -0.2, -1), (0.5, 1, 0.3), (1, 0.4, -0.6), (0.2, 0.7, 1), (-1, 0.3, 0.2)]


def _frames(seed0, n_frames, n, deg, axes, ric=RIC_TRUE, reseed=None):
    seeds = [(reseed or {}).get(f, seed0 + f) for f in range(n_frames)]
    return [Frame(*scene(seeds[f], n, axes[f % len(axes)], deg, (0.2 + 0.02 * f, -0.05, 0.08), ric=ric)) for f in range(n_frames)]


class Sequence:
    def __init__(self, cfg, frames):
        self.cfg, self.frames = dict(CFG, **cfg), frames


SEQUENCES = {
    "excited": Sequence({}, _frames(100, 9, 40, 12.0, AXES)),                                 # calibrated: false at 7, true at 8
    "one_axis": Sequence({}, _frames(200, 10, 30, 12.0, [(0.2, 1, 0.1)])),                     # singular[2] < 0.25 at 8 and later
    "vo2": Sequence(dict(vo_size=2, max_slots=2), _frames(300, 3, 30, 40.0, AXES, ric=np.eye(3))),   # vo_size = 2: a true ric of I, so no
                                                                                               # huber weight: calibrated at frame 2
    # the ninth frame is refused.  Frame 8's seed was replaced once (407 -> 417): F is singular, so the sign of det(R1), and with it
    # `negated`, is decided by rounding noise in F; with seed 407 the device's and the host's libm round a root of the 7-point cubic an
    # ulp apart and the flag flips (Rc itself agreed to 4e-16).  DESIGN section 22 records it.
    "fill": Sequence(dict(max_frames=8, max_slots=2), _frames(400, 9, 20, 10.0, AXES, reseed={7: 417})),
}
