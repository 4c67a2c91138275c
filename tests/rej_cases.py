"""The case table of the outlier rejection (include/isvins_reject.h), shared by tests/test_rej_oracle.py and tests/test_gpu_rej.py: a
deterministic scene generator with fixed seeds (3-D points in front of two poses, projected through the distorted pinhole of the
tracker tests' camera, optional pixel noise, a given number of planted outliers), the named cases, the degenerate inputs, recorded
error vectors for the LMedS median, and a numpy statement of the lift.

A planted outlier is a cur point moved 5 .. 40 px (of the virtual camera) off its epipolar line.  An "exact" scene has no noise: its
pixels are refined until the lift of the code under test (eight fixed-point steps of the distortion model, not its exact inverse)
returns the intended normalised point, so what remains is the float32 rounding of the pixel and of the lifted coordinates, some 1e-4
px."""
import numpy as np

from isvins_amd import reject as rej, tracker as trk

WIDTH, HEIGHT = 752, 480
MAX_POINTS = rej.MAX_POINTS          # the table's rejector: the header's limit, so that the largest case fills the kernel's LDS budget
R_CFG = dict(max_points=MAX_POINTS)
T_CFG = dict(max_points=MAX_POINTS)  # the tracker the rejector sits on


def tracker_config(**kw):
    return trk.make_config(**dict(T_CFG, **kw))


def rejector_config(**kw):
    return rej.make_config(**dict(R_CFG, **kw))


# ------------------------------------------------------------------------------------------------------------------ the lift, in numpy
def _distortion(c, x, y):
    mx2_u, my2_u, mxy_u = x * x, y * y, x * y
    rho2_u = mx2_u + my2_u
    rad_dist_u = c.k1 * rho2_u + c.k2 * rho2_u * rho2_u
    dx = x * rad_dist_u + 2.0 * c.p1 * mxy_u + c.p2 * (rho2_u + 2.0 * mx2_u)
    dy = y * rad_dist_u + 2.0 * c.p2 * mxy_u + c.p1 * (rho2_u + 2.0 * my2_u)
    return dx, dy


def lift_projective(c, px):
    """PinholeCamera::liftProjective (PinholeCamera.cc:461-521) of pixels [n][2] in float64, operation by operation -> [n][2]"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    inv_K11, inv_K13, inv_K22, inv_K23 = 1.0 / c.fx, -c.cx / c.fx, 1.0 / c.fy, -c.cy / c.fy
    mx_d, my_d = inv_K11 * px[:, 0] + inv_K13, inv_K22 * px[:, 1] + inv_K23
    mx_u, my_u = mx_d, my_d
    if not (c.k1 == 0.0 and c.k2 == 0.0 and c.p1 == 0.0 and c.p2 == 0.0):
        for _ in range(8):
            dx, dy = _distortion(c, mx_u, my_u)
            mx_u, my_u = mx_d - dx, my_d - dy
    return np.stack([mx_u, my_u], axis=1)


def lift(c, px, focal=rej.FOCAL_LENGTH, width=WIDTH, height=HEIGHT):
    """rejectWithF's lift (feature_tracker_simple.cpp:161-165) of float32 pixels [n][2] -> [n][2] float32"""
    b = lift_projective(c, np.asarray(px, np.float32))
    x = focal * b[:, 0] / 1.0 + width / 2.0
    y = focal * b[:, 1] / 1.0 + height / 2.0
    return np.stack([x, y], axis=1).astype(np.float32)


def unlift(c, xn):
    """the pixels whose lift_projective is xn [n][2]: the distortion model forward, then fixed-point steps on the lift itself"""
    dx, dy = _distortion(c, xn[:, 0], xn[:, 1])
    px = np.stack([c.fx * (xn[:, 0] + dx) + c.cx, c.fy * (xn[:, 1] + dy) + c.cy], axis=1)
    for _ in range(40):
        px = px + (xn - lift_projective(c, px)) * np.array([c.fx, c.fy])
    return px


# ------------------------------------------------------------------------------------------------------------------------- the scenes
class Case:
    """one item: prev, cur [n][2] float32 pixels, planted [n] bool (the planted outliers), noise in px"""

    def __init__(self, prev, cur, planted, noise=0.0, width=WIDTH, height=HEIGHT):
        self.prev, self.cur = np.ascontiguousarray(prev, np.float32).reshape(-1, 2), np.ascontiguousarray(cur, np.float32).reshape(-1, 2)
        self.planted, self.noise, self.width, self.height = np.asarray(planted, bool), noise, width, height

    @property
    def n(self):
        return len(self.prev)

    def item(self):
        return rej.RejItem(self.width, self.height, self.prev, self.cur)


def _rotation(rv):
    th = np.linalg.norm(rv)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(n, seed, outliers=0, noise=0.0, cam=None):
    """n points at 2 .. 8 m in front of the first pose, seen again after a turn of some 3 degrees and a step of 0.3 m; `outliers` of
    them (drawn by the seed) displaced in cur; gaussian pixel noise of `noise` px on both sides"""
    c = tracker_config() if cam is None else cam
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    x1 = np.stack([rng.uniform(-0.55, 0.55, n), rng.uniform(-0.38, 0.38, n)], axis=1)
    depth = rng.uniform(2.0, 8.0, n)
    R = _rotation(np.array([0.02, -0.045, 0.015]) * rng.uniform(0.8, 1.2))
    t = np.array([0.28, -0.05, 0.09]) * rng.uniform(0.8, 1.2)
    X = np.concatenate([x1, np.ones((n, 1))], axis=1) * depth[:, None]
    X2 = X @ R.T + t
    x2 = X2[:, :2] / X2[:, 2:]
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:outliers]] = True
    if outliers:
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        lines = np.concatenate([x1, np.ones((n, 1))], axis=1) @ (tx @ R).T          # E x1, the epipolar lines in cur
        normal = lines[:, :2] / np.linalg.norm(lines[:, :2], axis=1, keepdims=True)
        d = rng.uniform(5.0, 40.0, n) * rng.choice([-1.0, 1.0], n) / rej.FOCAL_LENGTH
        x2 = np.where(planted[:, None], x2 + d[:, None] * normal, x2)
    prev, cur = unlift(c, x1), unlift(c, x2)
    if noise:
        prev, cur = prev + rng.normal(0.0, noise, (n, 2)), cur + rng.normal(0.0, noise, (n, 2))
    both = np.concatenate([prev, cur, np.array([[WIDTH / 2.0, HEIGHT / 2.0]])])
    assert cam is not None or (both.min() > 1 and both[:, 0].max() < WIDTH - 1 and both[:, 1].max() < HEIGHT - 1)
    return Case(prev, cur, planted, noise)


def unrelated(n, seed):
    """random pixels on both sides: no epipolar geometry at all"""
    rng = np.random.Generator(np.random.PCG64(9500 + seed))
    box = np.array([WIDTH - 40.0, HEIGHT - 40.0])
    return Case(20 + rng.random((n, 2)) * box, 20 + rng.random((n, 2)) * box, np.zeros(n, bool))


# name -> (builder, arguments); the seeds are chosen so that tests/test_rej_oracle.py's assertions on the table hold
TABLE = {
    "n0": (scene, dict(n=0, seed=1)),
    "n7": (scene, dict(n=7, seed=2, outliers=2)),
    "lmeds8_exact": (scene, dict(n=8, seed=3)),
    "lmeds8_interpolated": (scene, dict(n=8, seed=3, outliers=1)),             # UNDECIDABLE, below
    "lmeds14_exact": (scene, dict(n=14, seed=4, outliers=3)),
    "lmeds8_noise": (scene, dict(n=8, seed=5, noise=0.3)),
    "lmeds14_noise": (scene, dict(n=14, seed=101, outliers=2, noise=0.3)),
    "ransac15_exact": (scene, dict(n=15, seed=7, outliers=2)),
    "ransac63_noise": (scene, dict(n=63, seed=8, outliers=6, noise=0.3)),
    "ransac64_noise": (scene, dict(n=64, seed=9, outliers=6, noise=0.3)),
    "ransac65_exact": (scene, dict(n=65, seed=10, outliers=7)),
    "ransac129_third": (scene, dict(n=129, seed=11, outliers=45)),             # 64 < iters <= 128
    "ransac150_noise": (scene, dict(n=150, seed=12, outliers=15, noise=0.3)),  # the benchmark's item: iters < 64
    "ransac150_half": (scene, dict(n=150, seed=221, outliers=75)),             # 128 < iters < 1000, keeps in the second and third chunk
    "ransac150_half_late": (scene, dict(n=150, seed=227, outliers=75)),        # the last keep ends the loop inside the eleventh chunk
    "ransac40_unrelated": (unrelated, dict(n=40, seed=14)),                    # iters == 1000
    "ransac100_all_inliers": (scene, dict(n=100, seed=15)),                    # niters falls to 0 at the first keep
    "ransac_max_points": (scene, dict(n=MAX_POINTS, seed=16, outliers=MAX_POINTS // 10, noise=0.3)),
}
# A 7-point model passes through any 7 of 8 points, the outlier among them: every model's median of 8 errors is rounding noise, and
# LMedS cannot tell the outlier.  The case stays in the table (the GPU has to agree on it); the tests assert the reason, not the mask.
UNDECIDABLE = ("lmeds8_interpolated",)
COUNTS = (0, 7, 8, 14, 15, 63, 64, 65, 129, 150, MAX_POINTS)


def case(name):
    f, kw = TABLE[name]
    return f(**kw)


def degenerate():
    """inputs whose 7-point systems are rank deficient: name -> Case (LMedS and RANSAC sizes of each)"""
    out = {}
    base = scene(20, 30, outliers=2)
    for n in (8, 14, 20):
        out[f"all_equal{n}"] = Case(np.full((n, 2), 200.5), np.full((n, 2), 200.5), np.zeros(n, bool))
        out[f"prev_is_cur{n}"] = Case(base.prev[:n], base.prev[:n], np.zeros(n, bool))
        s = np.arange(n, dtype=np.float64)[:, None]
        out[f"collinear{n}"] = Case(np.array([100.0, 80.0]) + s * np.array([21.0, 13.0]), np.array([104.0, 83.0]) + s * np.array([21.0, 13.0]), np.zeros(n, bool))
    prev, cur = base.prev[:8].copy(), base.cur[:8].copy()
    prev[:7], cur[:7] = prev[0], cur[0]
    out["seven_coincident8"] = Case(prev, cur, np.zeros(8, bool))
    return out


# recorded float32 error vectors for the LMedS median: name -> list (the NaN has a clear sign bit: J4 sorts it above +inf)
ERROR_VECTORS = {
    "odd": [0.25, 3.0, 0.001, 17.5, 0.5, 2.25, 0.0, 9.0, 1.0],
    "even": [0.3, 4.1, 0.007, 12.5, 0.55, 2.2, 0.0, 9.75, 1.1, 0.42],
    "even_inexact_sum": [1.0000001, 0.1, 3.0, 0.33333334, 7.0, 0.2, 0.7, 5.0],
    "nan_first": [float("nan"), 5.0, 1.0, 3.0, 2.0, 8.0, 0.5, 6.0, 4.0],
    "inf_and_nan": [2.0, float("inf"), 1.0, float("nan"), 3.0, 0.5, 0.25, 4.0],
}
