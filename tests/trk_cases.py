"""The scenario list of the feature tracking (include/isvins_tracker.h), shared by tests/test_trk_oracle.py (which asserts that the
list covers the ground it is meant to cover) and tests/test_gpu_trk.py (which runs it in one batched call): image pairs of 24 x 23
(one level), 64 x 48, 97 x 61 with stride 104 (two), 200 x 120 (three), 181 x 179 (four, the top one 23 x 23) and 752 x 480 (four),
each an analytic texture and the same texture shifted; a checkerboard of 2-pixel cells whose upper levels are flat; points inside,
on, at and beyond every edge, beyond the range of int, and points picked because their iteration ends in each possible way;
malformed items and items over each capacity, placed between good ones.  Every scenario carries its prev image: the restatement has
no slots, and tests/test_gpu_trk.py drops it where it tests the resident path.  Scenario k uses slot k."""
import functools

import numpy as np

from isvins_amd import synth, tracker as trk

MAX_W, MAX_H, MAX_POINTS = 752, 480, 40

# name, width, height, stride, shift of cur against prev, and the points whose iteration ends in a rare way on this pair (found by a
# search over the quarter-pixel grid; tests/test_trk_oracle.py asserts that each way occurs, whichever point shows it)
PAIRS = [
    ("s24", 24, 23, 24, (0.75, -0.5), [(25.75, -4.75), (-8.5, -6.75), (-0.25, -9.5), (-8.0, -6.5), (4.25, -10.75), (26.5, 3.5)]),
    ("s64", 64, 48, 64, (-6.75, 4.5), [(9.0, 9.5), (54.25, 50.5), (66.0, 51.0), (4.25, 13.25), (18.0, 38.5), (30.25, -17.5), (5.0, 14.75), (-0.75, -10.75)]),
    ("s97", 97, 61, 104, (2.5, 1.25), [(95.25, 60.75), (95.5, 10.75), (59.75, -9.5), (88.25, 64.5), (96.5, 22.0), (51.5, -18.25), (-19.0, 29.0)]),
    ("s200", 200, 120, 200, (-6.75, 4.5), [(202.0, 115.25), (10.5, 23.25), (88.25, 112.0), (183.5, -9.5), (-6.0, 4.75), (-0.25, 29.25), (-14.0, -16.0), (11.0, -23.0)]),
    ("s181", 181, 179, 181, (11.6, -9.3), [(166.5, 33.0), (-5.25, 12.25), (14.5, 3.25), (40.75, -3.75), (2.75, 9.0), (5.75, 149.25), (64.5, -10.5)]),
    ("big", 752, 480, 752, (11.6, -9.3), [(736.0, 119.0), (230.0, 3.5), (585.75, 6.5), (740.75, 331.5), (395.5, -9.5), (625.0, 438.25)]),
]


def config(distorted=True, **kw):
    """the handle's configuration for the scenario list: EuRoC's intrinsics, or the same camera without distortion"""
    cam = {} if distorted else dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    n = len(scenarios())
    return trk.make_config(n, n, MAX_W, MAX_H, max_points=MAX_POINTS, **cam, **kw)


def pair(k):
    """(prev, cur) of PAIRS[k], [height][stride] each; the padding beyond the width holds 0xEE"""
    name, w, h, stride, shift, _ = PAIRS[k]
    out = []
    for s in ((0.0, 0.0), shift):
        img = np.full((h, stride), 0xEE, np.uint8)
        img[:, :w] = trk.analytic_image(w, h, s, k + 1)
        out.append(img)
    return out


def points(seed, w, h, special=(), n=16):
    """n sub-pixel points within 24 pixels of the image, the edge cases (ip.x = -21 kept and -22 rejected, ip.x = W - 1 kept and W
    rejected, beyond the range of int, far outside), then the special ones"""
    rng = synth.SplitMix64(0x544B000000000000 + seed)
    p = rng.uniform(2 * n).reshape(n, 2) * [w + 28, h + 28] - 24.0
    edge = [[-10.5, h * 0.5], [-11.5, h * 0.5], [w + 9.5, h * 0.5], [w + 10.0, h * 0.5], [3.0e9, 5.0], [5.0, -3.0e9], [1.0e6, -1.0e6], [w * 0.5, h + 9.75]]
    return np.vstack([p, edge] + ([np.array(special, np.float64)] if len(special) else [])).astype(np.float32)


def checkerboard(w=200, h=120):
    """2-pixel cells: level 1 is a 1-pixel checkerboard (its central differences vanish), levels 2 and up are constant"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // 2) + (yy // 2)) % 2 == 0, 60, 190).astype(np.uint8)


@functools.lru_cache(maxsize=1)
def scenarios():
    """list of dicts: name, item (trk.TrkItem, prev given, slot = its index), want (the status the item must get)"""
    out = []

    def add(name, cur, prev, pts=None, want=trk.ISV_TRK_OK, width=None):
        out.append(dict(name=name, item=trk.TrkItem(len(out), cur, prev, pts, width), want=want))
        return out[-1]["item"]

    def add_pair(k):
        name, w, h, stride, shift, special = PAIRS[k]
        prev, cur = pair(k)
        add(name, cur, prev, points(k, w, h, special), width=w)

    a64, b64 = pair(1)
    add_pair(0)
    bad = add("bad_stride", b64, a64, points(20, 64, 48), want=trk.ISV_TRK_INPUT)
    bad.c.stride = 63
    add_pair(1)
    nan = points(21, 64, 48); nan[2, 1] = np.nan
    add("nan_point", b64, a64, nan, want=trk.ISV_TRK_INPUT)
    add_pair(2)
    add("over_points", b64, a64, points(22, 64, 48, n=MAX_POINTS), want=trk.ISV_TRK_CAPACITY)
    add_pair(3)
    wide = trk.analytic_image(MAX_W + 1, 30)
    add("too_wide", wide, wide, want=trk.ISV_TRK_CAPACITY)
    ch = checkerboard()
    add("checker", ch, ch, [[100, 60], [50.5, 30.25], [150.25, 90.5], [30, 100], [3.0, 117.5], [-11.5, 7.0], [197.0, 4.0], [120.75, 61.5]])
    null = add("null_cur", b64, a64, points(23, 64, 48), want=trk.ISV_TRK_INPUT)
    null.c.cur = None
    add_pair(4)
    inf = points(24, 64, 48); inf[0, 0] = -np.inf
    add("inf_point", b64, a64, inf, want=trk.ISV_TRK_INPUT)
    add("no_points", b64, a64)
    slot = add("bad_slot", b64, a64, points(25, 64, 48), want=trk.ISV_TRK_INPUT)
    slot.c.slot = 1 << 20
    add_pair(5)
    neg = add("negative_count", b64, a64, want=trk.ISV_TRK_INPUT)
    neg.c.n_points = -1
    return out


def texture_crops(size=(168, 168), offsets=((8, 8), (24, 16))):
    """two (prev, cur) pairs cut from one larger pair at two origins: ((prev_a, cur_a), (prev_b, cur_b), (dx, dy)) with crop b's
    origin at crop a's + (dx, dy).  168 -> 84 -> 42: three levels, so origins that differ by multiples of 4 see the same pyramid away
    from the borders."""
    prev, cur = trk.analytic_image(200, 190, (0, 0), 31), trk.analytic_image(200, 190, (1.75, -2.5), 31)
    (ax, ay), (bx, by) = offsets
    w, h = size
    cut = lambda im, x, y: im[y:y + h, x:x + w].copy()
    return (cut(prev, ax, ay), cut(cur, ax, ay)), (cut(prev, bx, by), cut(cur, bx, by)), (bx - ax, by - ay)
