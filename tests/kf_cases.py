"""The scenario list of the keyframe extraction (include/isvins_keyframe.h), shared by tests/test_kf_oracle.py (which asserts that
the list covers the ground it is meant to cover) and tests/test_gpu_kf.py (which runs it in one batched call): the sizes 7 x 7,
6 x 40, 64 x 48, 97 x 61 with stride 104, 130 x 67 and 752 x 480; images without a corner; corners on the first and the last
candidate row and column; window points at, across and far beyond the border; items over each capacity and malformed items, placed
between good ones."""
import functools

import numpy as np

from isvins_amd import keyframe as kf, synth

MAX_W, MAX_H, MAX_KEYPOINTS, MAX_POINTS = 752, 480, 700, 40


def config(distorted=True, **kw):
    """the handle's configuration for the scenario list: EuRoC's intrinsics, or the same camera without distortion"""
    cam = {} if distorted else dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    return kf.make_config(len(scenarios()), MAX_W, MAX_H, max_keypoints=MAX_KEYPOINTS, max_points=MAX_POINTS, **cam, **kw)


def window_points(seed, w, h, n=24):
    """n sub-pixel points inside the image, then the border cases: a coordinate in (-1, 0) (K1), in [W - 1, W) and [H - 1, H), just
    outside, far outside, and beyond the range of int"""
    rng = synth.SplitMix64(0x4B46AA0000000000 + seed)
    p = rng.uniform(2 * n).reshape(n, 2) * [w, h]
    edge = [[-0.5, h * 0.5], [w * 0.5, -0.25], [w - 0.4, h - 0.7], [w - 1.0, 0.0], [w + 0.5, h * 0.5], [-1.0, -1.0], [1.0e6, -1.0e6],
            [3.0e9, 5.0], [5.0, -3.0e9], [-0.75, -0.75], [0.25, 0.5]]
    return np.vstack([p, edge]).astype(np.float32)


def _dots(img):
    """flat 8 x 8 patches in the first and the last corner of the image, each with one bright pixel on the outermost candidate"""
    h, w = img.shape
    img[:8, :8] = 100; img[3, 3] = 250
    img[h - 8:, w - 8:] = 90; img[h - 4, w - 4] = 5
    return img


@functools.lru_cache(maxsize=1)
def scenarios():
    """list of dicts: name, item (kf.KfItem), want (the status the item must get)"""
    out = []

    def add(name, image, points=None, want=kf.ISV_KF_OK, width=None):
        out.append(dict(name=name, item=kf.KfItem(image, points, width), want=want))
        return out[-1]["item"]

    tiny = np.full((7, 7), 50, np.uint8); tiny[3, 3] = 200
    add("tiny7", tiny, window_points(1, 7, 7, 4))
    bad = add("bad_stride", kf.make_image(2, 64, 48), want=kf.ISV_KF_INPUT)
    bad.c.stride = 63
    add("thin", kf.make_image(3, 6, 40), window_points(3, 6, 40, 6))
    add("over_keypoints", kf.make_image(4, 130, 67, shapes=False, smooth=0, contrast=127), window_points(4, 130, 67), want=kf.ISV_KF_CAPACITY)
    add("constant", np.full((48, 64), 77, np.uint8), window_points(5, 64, 48, 3))
    add("small", _dots(kf.make_image(6, 64, 48)), window_points(6, 64, 48))
    nan = window_points(7, 64, 48, 5); nan[2, 1] = np.nan
    add("nan_point", kf.make_image(7, 64, 48), nan, want=kf.ISV_KF_INPUT)
    strided = np.full((61, 104), 0xEE, np.uint8); strided[:, :97] = _dots(kf.make_image(8, 97, 61))
    add("strided", strided, window_points(8, 97, 61), width=97)
    add("over_points", kf.make_image(9, 64, 48), window_points(9, 64, 48, MAX_POINTS), want=kf.ISV_KF_CAPACITY)
    add("mid", _dots(kf.make_image(10, 130, 67)), window_points(10, 130, 67))
    add("too_wide", kf.make_image(11, MAX_W + 1, 10), want=kf.ISV_KF_CAPACITY)
    null = add("null_image", kf.make_image(12, 64, 48), want=kf.ISV_KF_INPUT)
    null.c.image = None
    add("big", _dots(kf.make_image(13, 752, 480, contrast=35)), window_points(13, 752, 480, 29))
    inf = window_points(14, 64, 48, 2); inf[0, 0] = -np.inf
    add("inf_point", kf.make_image(14, 64, 48), inf, want=kf.ISV_KF_INPUT)
    return out


def texture_crops(seed=21, size=(120, 100), offsets=((10, 8), (23, 17))):
    """two crops of one larger texture: (crop_a, crop_b, (dx, dy)) with crop_b's origin at crop_a's + (dx, dy)"""
    tex = kf.make_image(seed, 200, 160)
    (ax, ay), (bx, by) = offsets
    w, h = size
    return tex[ay:ay + h, ax:ax + w].copy(), tex[by:by + h, bx:bx + w].copy(), (bx - ax, by - ay)
