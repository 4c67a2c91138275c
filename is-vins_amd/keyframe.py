"""Host-side mirror of include/isvins_keyframe.h: the batched keyframe extraction, what the KeyFrame constructor computes from
the image (reference src/pose_graph/keyframe.cpp:43-69: cv::FAST, BRIEF at the corners and at the window points, liftProjective of
every corner) for many 8-bit images in one call.  `KeyframeExtractor(...)` raises when the HIP extension is missing or there is no
GPU: no CPU path.  Its arrays go into bow.BowItem and loop.LoopPair as they are.

`load_brief_pattern` reads a pattern file of the reference's layout, `default_pattern` the copy of the reference's pattern under
tests/golden, `make_image` a deterministic synthetic image for the tests and scripts/kf_bench.py."""
import ctypes as C
import os

import numpy as np

from . import _stage, synth
from ._stage import filled, untouched

ISV_KF_OK, ISV_KF_CAPACITY, ISV_KF_INPUT = range(3)
PATTERN_BITS, PATTERN_RADIUS = 256, 24
MAX_KEYPOINTS = 8192                      # bow's ISV_BOW_MAX_FEATURES
# config/euroc_config.yaml:9-17
EUROC = dict(fx=4.616e+02, fy=4.603e+02, cx=3.630e+02, cy=2.481e+02, k1=-2.917e-01, k2=8.228e-02, p1=5.333e-05, p2=-1.578e-04)

_u8p, _u64p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_float)


class isv_kf_config_t(C.Structure):
    _fields_ = [("max_items", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32), ("max_keypoints", C.c_int32),
                ("max_points", C.c_int32), ("fast_threshold", C.c_int32), ("x1", C.c_int8 * 256), ("y1", C.c_int8 * 256),
                ("x2", C.c_int8 * 256), ("y2", C.c_int8 * 256), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class isv_kf_item_t(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("n_points", C.c_int32), ("image", _u8p),
                ("point_2d_uv", _f32p)]


class isv_kf_result_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_keypoints", C.c_int32), ("n_points", C.c_int32), ("_pad", C.c_int32)]


EXPORTS = ["isv_kf_create", "isv_kf_destroy", "isv_kf_last_error", "isv_kf_extract_batch", "isv_kf_last_ms"]


def load_brief_pattern(path):
    """the four lists x1, y1, x2, y2 of a pattern file in the reference's layout (config/brief_pattern.yml: `%YAML:1.0`, then four
    top-level keys, each followed by `- value` lines) as a dict of int8 arrays.  ValueError for anything else, for a list that is
    not 256 long and for a value outside [-24, 24]."""
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or lines[0].strip() != "%YAML:1.0":
        raise ValueError(f"{path}: not a %YAML:1.0 file")
    lists, key = {}, None
    for ln, line in enumerate(lines[1:], 2):
        s = line.strip()
        if not s or s.startswith("#"):
            continue
        if s.startswith("-"):
            if key is None:
                raise ValueError(f"{path}:{ln}: a value before any key")
            try:
                v = int(s[1:].strip())
            except ValueError:
                raise ValueError(f"{path}:{ln}: not an integer: {s!r}") from None
            if not -PATTERN_RADIUS <= v <= PATTERN_RADIUS:
                raise ValueError(f"{path}:{ln}: {v} is outside [-{PATTERN_RADIUS}, {PATTERN_RADIUS}]")
            lists[key].append(v)
        elif s.endswith(":") and not line[0].isspace():
            key = s[:-1]
            if key in lists:
                raise ValueError(f"{path}:{ln}: duplicate key {key}")
            lists[key] = []
        else:
            raise ValueError(f"{path}:{ln}: unexpected line {s!r}")
    if sorted(lists) != ["x1", "x2", "y1", "y2"]:
        raise ValueError(f"{path}: the keys are {sorted(lists)}, expected x1, x2, y1, y2")
    for k, v in lists.items():
        if len(v) != PATTERN_BITS:
            raise ValueError(f"{path}: {k} has {len(v)} values, expected {PATTERN_BITS}")
    return {k: np.array(v, dtype=np.int8) for k, v in lists.items()}


def default_pattern():
    """the reference's config/brief_pattern.yml, from the fixture tests/golden/brief_pattern.npz"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "brief_pattern.npz")
    with np.load(path) as z:
        return {k: np.array(z[k], dtype=np.int8) for k in ("x1", "y1", "x2", "y2")}


def make_config(max_items=1, max_width=752, max_height=480, max_keypoints=MAX_KEYPOINTS, max_points=256, fast_threshold=20, pattern=None,
                fx=EUROC["fx"], fy=EUROC["fy"], cx=EUROC["cx"], cy=EUROC["cy"], k1=EUROC["k1"], k2=EUROC["k2"], p1=EUROC["p1"], p2=EUROC["p2"]):
    """the reference's constants as defaults (keyframe.cpp:58, config/euroc_config.yaml, config/brief_pattern.yml)"""
    c = isv_kf_config_t()
    c.max_items, c.max_width, c.max_height, c.max_keypoints, c.max_points = max_items, max_width, max_height, max_keypoints, max_points
    c.fast_threshold = fast_threshold
    pattern = default_pattern() if pattern is None else pattern
    for k in ("x1", "y1", "x2", "y2"):
        v = np.asarray(pattern[k])
        if v.shape != (PATTERN_BITS,) or v.min() < -128 or v.max() > 127:
            raise ValueError(f"pattern list {k}: 256 values of int8 are required")
        getattr(c, k)[:] = [int(x) for x in v]
    c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2 = fx, fy, cx, cy, k1, k2, p1, p2
    return c


class KfItem:
    """one image with its window points: numpy arrays (kept alive here) behind an isv_kf_item_t (`.c`).  `image` is [height][stride]
    uint8; `width` defaults to the array's."""

    def __init__(self, image, points=None, width=None):
        self.image = np.ascontiguousarray(image, dtype=np.uint8)
        assert self.image.ndim == 2
        self.points = np.ascontiguousarray(np.zeros((0, 2)) if points is None else points, dtype=np.float32).reshape(-1, 2)
        c = self.c = isv_kf_item_t()
        c.height, c.stride = self.image.shape
        c.width = c.stride if width is None else width
        c.n_points = len(self.points)
        c.image = self.image.ctypes.data_as(_u8p)
        c.point_2d_uv = self.points.ctypes.data_as(_f32p)

    @property
    def pixels(self):
        return self.image[:, :self.c.width]


class KfArrays:
    """an item's output arrays: brief [n][4] uint64, keypoints_uv / keypoints_norm [n][2] float32, score [n] uint8, window_brief
    [n_points][4] uint64, cut to what was written (empty for a refused item)"""

    def __init__(self, brief, keypoints_uv, keypoints_norm, score, window_brief):
        self.brief, self.keypoints_uv, self.keypoints_norm, self.score, self.window_brief = brief, keypoints_uv, keypoints_norm, score, window_brief


@_stage.bind_once("kf")
def _bind(lib):
    vp = C.c_void_p
    lib.isv_kf_create.argtypes = [C.POINTER(isv_kf_config_t), C.POINTER(vp)]
    lib.isv_kf_destroy.argtypes = [vp]; lib.isv_kf_destroy.restype = None
    lib.isv_kf_last_error.argtypes = [vp]; lib.isv_kf_last_error.restype = C.c_char_p
    lib.isv_kf_extract_batch.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(isv_kf_item_t)), C.POINTER(isv_kf_result_t), C.POINTER(_u64p),
                                         C.POINTER(_f32p), C.POINTER(_f32p), C.POINTER(_u8p), C.POINTER(_u64p)]
    lib.isv_kf_last_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.isv_internal_kf_read_back.argtypes = [vp, C.c_int32, _u8p, _u8p]


def keypoint_capacity(cfg, item):
    """the length an item's corner arrays must have: min(max_keypoints, its candidate pixels)"""
    w, h = item.c.width, item.c.height
    return min(cfg.max_keypoints, max(w - 6, 0) * max(h - 6, 0))


class KeyframeExtractor(_stage.StageHandle):
    """KeyFrame's constructor on the MI355X: FAST, BRIEF and the lift for many images per call"""
    PREFIX, N_MS = "isv_kf", 7

    def __init__(self, max_items=1, max_width=752, max_height=480, **kw):
        self.cfg = make_config(max_items, max_width, max_height, **kw)
        self._create(_bind, C.byref(self.cfg), why=" (a MI355X and the HIP extension are required; there is no CPU path)")

    def extract_batch(self, items):
        """items: KfItem list -> (isv_kf_result_t list, KfArrays list).  The arrays are pre-filled with FILL bytes; a refused item's
        are checked to be untouched and come back empty."""
        n = len(items)
        res = (isv_kf_result_t * max(n, 1))()
        ptrs = (C.POINTER(isv_kf_item_t) * max(n, 1))(*[C.pointer(it.c) for it in items])
        caps = [keypoint_capacity(self.cfg, it) for it in items]
        br = [filled(c, 4, np.uint64) for c in caps]
        uv = [filled(c, 2, np.float32) for c in caps]
        nm = [filled(c, 2, np.float32) for c in caps]
        sc = [filled(c, 1, np.uint8).reshape(-1) for c in caps]
        wb = [filled(it.c.n_points, 4, np.uint64) for it in items]
        arr = lambda t, xs: (t * max(n, 1))(*[a.ctypes.data_as(t) for a in xs])
        rc = self.lib.isv_kf_extract_batch(self.h, n, ptrs, res, arr(_u64p, br), arr(_f32p, uv), arr(_f32p, nm), arr(_u8p, sc), arr(_u64p, wb))
        self._check(rc, "isv_kf_extract_batch", with_last_error=True)
        out = list(res)[:n]
        arrays = []
        for i, r in enumerate(out):
            k, p = (r.n_keypoints, r.n_points) if r.status == ISV_KF_OK else (0, 0)
            for a in (br[i], uv[i], nm[i], sc[i]):
                assert untouched(a, k), "written past an item's count"
            assert untouched(wb[i], p), "written past an item's points"
            arrays.append(KfArrays(br[i][:k], uv[i][:k], nm[i][:k], sc[i][:k], wb[i][:p]))
        return out, arrays

    def read_back(self, index, width, height):
        """the blurred image and the FAST score map of item `index` of the last call (debug entry, csrc/isv_keyframe.h)"""
        blur, smap = np.zeros((height, width), np.uint8), np.zeros((height, width), np.uint8)
        self._check(self.lib.isv_internal_kf_read_back(self.h, index, blur.ctypes.data_as(_u8p), smap.ctypes.data_as(_u8p)), "isv_internal_kf_read_back")
        return blur, smap

    def last_ms(self):
        """(whole call, k_kf_blur, k_kf_fast, k_kf_select, k_kf_brief, the upload, the host's packing) milliseconds of the last successful
        call"""
        return super().last_ms()


# ---------------------------------------------------------------------------------------------------------------------
def _box3(a):
    """3 x 3 box mean in integers, edges replicated"""
    p = np.pad(a.astype(np.int32), 1, mode="edge")
    s = sum(p[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(3) for dx in range(3))
    return (s // 9).astype(np.int32)


def make_image(seed, width, height, noise=True, shapes=True, smooth=2, contrast=87):
    """A deterministic [height][width] uint8 image, integers only (SplitMix64 counter stream seeded 0x4B46000000000000 + seed):
    noise box-smoothed `smooth` times and stretched to [128 - contrast, 128 + contrast], and on it, where `shapes`: axis-aligned rectangles, rectangles rotated by the
    3-4-5 angle, a checkerboard of 8-pixel cells, a saturated 0 and a saturated 255 region, and flat two-pixel-wide bars ending on a
    flat ground (their two end pixels see mirrored circles: equal neighbouring scores, quirk K2)."""
    rng = synth.SplitMix64(0x4B46000000000000 + int(seed))
    W, H = int(width), int(height)
    if noise:
        a = (rng.u64(W * H) >> np.uint64(56)).astype(np.int32).reshape(H, W)
        for _ in range(smooth):
            a = _box3(a)
        lo, hi = int(a.min()), int(a.max())
        img = 128 - contrast + (a - lo) * (2 * contrast) // max(hi - lo, 1)
    else:
        img = np.full((H, W), 128, np.int32)
    if shapes and W >= 32 and H >= 32:
        yy, xx = np.mgrid[0:H, 0:W]
        n_each = max(1, W * H // 20000)
        d = iter((rng.u64(10 * n_each) >> np.uint64(33)).astype(np.int64).tolist())
        for _ in range(n_each):       # axis-aligned rectangles
            x0, y0, w, h, v = next(d) % W, next(d) % H, 6 + next(d) % 30, 6 + next(d) % 30, next(d) % 256
            img[(xx >= x0) & (xx < x0 + w) & (yy >= y0) & (yy < y0 + h)] = v
        for _ in range(n_each):       # rotated: u = 4 x + 3 y, v = -3 x + 4 y (five times the rotated coordinates)
            x0, y0, w, h, v = next(d) % W, next(d) % H, 5 * (8 + next(d) % 30), 5 * (8 + next(d) % 30), next(d) % 256
            u, t = 4 * (xx - x0) + 3 * (yy - y0), -3 * (xx - x0) + 4 * (yy - y0)
            img[(u >= 0) & (u < w) & (t >= 0) & (t < h)] = v
        # a checkerboard, the saturated regions, the bars on a flat ground
        cx, cy = W // 8, H // 8
        m = (xx >= cx) & (xx < cx + 32) & (yy >= cy) & (yy < cy + 24)
        img[m] = np.where((((xx - cx) // 8 + (yy - cy) // 8) % 2) == 0, 30, 220)[m]
        img[(xx >= W // 2) & (xx < W // 2 + 14) & (yy >= H // 2) & (yy < H // 2 + 10)] = 0
        img[(xx >= W // 2 + 14) & (xx < W // 2 + 28) & (yy >= H // 2) & (yy < H // 2 + 10)] = 255
        gx, gy = W - W // 3, H // 6
        img[(xx >= gx) & (xx < gx + 20) & (yy >= gy) & (yy < gy + 20)] = 60
        img[(xx >= gx + 6) & (xx < gx + 8) & (yy >= gy) & (yy < gy + 10)] = 200
        img[(xx >= gx + 10) & (xx < gx + 16) & (yy >= gy + 12) & (yy < gy + 14)] = 10
    return np.clip(img, 0, 255).astype(np.uint8)
