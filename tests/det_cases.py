"""The scenario list of the feature detection (include/isvins_detect.h), shared by tests/test_det_oracle.py (which asserts that the
list covers the ground it is meant to cover) and tests/test_gpu_det.py (which runs it in one batched call per min_dist): images of
3 x 3 (a single interior pixel), 2 x 5 (none), 24 x 23, 64 x 48, 97 x 61 with stride 104, 200 x 120 and 752 x 480 analytic textures,
a constant image, checkerboards of 2-pixel cells (tied maxima; the 200 x 150 one has more candidates than the selection kernel keeps
in registers), bright rectangles on a flat background; 0, 1, a few and 30
surviving points with equal and distinct track_cnt, some inside each other's discs, some on the image's edge; max_new of 0, 1,
exactly the uncapped count ("exact": tests/det_oracle.py resolves it per min_dist), and more than it; malformed items and items
over each capacity, placed between good ones.  Scenario k uses slot k."""
import functools

import numpy as np

from isvins_amd import detect as det, synth, tracker as trk

MAX_W, MAX_H, MAX_POINTS, MAX_CORNERS = 752, 480, 40, 400
MIN_DISTS = (1, 3, 30)
EXACT = "exact"


def textured(w, h, stride, seed):
    """[h][stride], the padding beyond the width holds 0xEE"""
    img = np.full((h, stride), 0xEE, np.uint8)
    img[:, :w] = trk.analytic_image(w, h, (0.0, 0.0), seed)
    return img


def checkerboard(w=64, h=48):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // 2) + (yy // 2)) % 2 == 0, 60, 190).astype(np.uint8)


RECTS = [(20, 18, 60, 50), (130, 24, 190, 60), (30, 120, 75, 160), (150, 130, 215, 175)]       # x0, y0, x1, y1 (inclusive), 70 or more apart


def rectangles(w=260, h=200):
    """bright axis-aligned rectangles on a flat background; every pair of rectangle corners is more than 2 * 30 apart except along a
    rectangle's own sides, which are at least 32 long"""
    img = np.full((h, w), 40, np.uint8)
    for x0, y0, x1, y1 in RECTS:
        img[y0:y1 + 1, x0:x1 + 1] = 200
    return img


def rect_corners():
    return [(x, y) for x0, y0, x1, y1 in RECTS for x in (x0, x1) for y in (y0, y1)]


def points(seed, w, h, n, cluster=True):
    """n sub-pixel points whose rounded pixels are inside the image: random ones, then (when n allows) pairs 2 pixels apart, a point on
    each of two edges and one in a corner; track_cnt has equal and distinct values"""
    rng = synth.SplitMix64(0x444554000000000 + seed)
    p = rng.uniform(2 * n).reshape(n, 2) * [w - 1, h - 1]
    if cluster and n >= 8:
        p[1] = p[0] + [2.0, 0.25]
        p[3] = p[2] + [-0.75, 2.0]
        p[4] = [0.25, h * 0.5]
        p[5] = [w * 0.5, h - 1.0]
        p[6] = [w - 1.25, 0.5]            # 0.5 rounds to 0 (half to even)
        p[7] = [1.5, 2.5]                 # both round to 2
    p = np.clip(p, [0, 0], [w - 1, h - 1]).astype(np.float32)
    cnt = (rng.uniform(n) * 4).astype(np.int32) + 1
    if n >= 4:
        cnt[0], cnt[1] = 7, 9             # the later point wins the pair's pixel
    return p, cnt


@functools.lru_cache(maxsize=1)
def scenarios():
    """list of dicts: name, image ([h][stride] uint8 or None: an empty slot), width, item (det.DetItem, slot = its index; max_new may
    still be EXACT in `max_new`), want (the status the item must get)"""
    out = []

    def add(name, image, n=0, max_new=0, want=det.ISV_DET_OK, width=None, seed=None, pts=None, cnt=None):
        k = len(out)
        w = None if image is None else (image.shape[1] if width is None else width)
        if pts is None and n > 0:
            pts, cnt = points(k if seed is None else seed, w, image.shape[0], n)
        item = det.DetItem(k, pts, cnt, 0 if max_new == EXACT else max_new)
        out.append(dict(name=name, image=image, width=w, item=item, max_new=max_new, want=want))
        return item

    s64 = textured(64, 48, 64, 2)
    add("s3x3", textured(3, 3, 3, 11), 0, 5)
    add("s2x5", textured(2, 5, 2, 12), 0, 5, pts=[[0.2, 3.4]], cnt=[1])
    add("s24", textured(24, 23, 24, 1), 5, EXACT)
    nan = add("nan_point", s64, 9, 10, det.ISV_DET_INPUT)
    nan.points[4, 1] = np.nan
    add("s64", s64, 30, MAX_CORNERS)
    add("over_points", s64, MAX_POINTS + 1, 10, det.ISV_DET_CAPACITY)
    add("s97", textured(97, 61, 104, 3), 12, 1, width=97)
    outside = add("outside_point", s64, 9, 10, det.ISV_DET_INPUT)
    outside.points[2] = [63.6, 10.0]      # rounds to x = 64
    add("s200", textured(200, 120, 200, 4), 30, 0)
    add("const", np.full((48, 64), 77, np.uint8), 0, 10)
    add("over_corners", s64, 9, MAX_CORNERS + 1, det.ISV_DET_CAPACITY)
    add("checker", checkerboard(), 0, MAX_CORNERS, pts=[[10.0, 10.0], [40.5, 20.25], [41.0, 21.0]], cnt=[2, 2, 2])
    add("rects", rectangles(), 0, 150)
    neg = add("negative_count", s64, 0, 10, det.ISV_DET_INPUT)
    neg.c.n_points = -1
    add("big", textured(752, 480, 752, 6), 30, 120)
    add("empty_slot", None, 0, 10, det.ISV_DET_INPUT)
    add("negative_max_new", s64, 9, -1, det.ISV_DET_INPUT)
    add("s64_first", s64, 0, EXACT)
    add("covered", textured(24, 23, 24, 1), 0, 10, pts=[[12.0, 11.0]], cnt=[1])
    null = add("null_points", s64, 3, 10, det.ISV_DET_INPUT)
    null.c.cur_pts = None
    add("s64_one", s64, 0, 5, pts=[[30.0, 20.0]], cnt=[3])
    # more candidates (every pixel of every plateau) than the selection keeps on chip: 16384
    add("checker_big", checkerboard(200, 150), 0, 40, pts=[[100.0, 75.0], [3.0, 140.0]], cnt=[1, 4])
    return out


def trk_config(distorted=True):
    """the tracker handle's configuration for the scenario list: EuRoC's intrinsics, or the same camera without distortion"""
    cam = {} if distorted else dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    n = len(scenarios())
    return trk.make_config(n, n, MAX_W, MAX_H, max_points=MAX_POINTS, **cam)


def det_config(min_dist):
    return det.make_config(len(scenarios()), MAX_POINTS, MAX_CORNERS, min_dist, det.QUALITY)
