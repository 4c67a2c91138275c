"""The serial restatement of CLAHE (tests/native/isv_eq_oracle.c, include/isvins_equalize.h) against an independent numpy statement of
the same definitions -- np.bincount, np.cumsum, np.float32 operations, np.rint, np.pad(mode="reflect") where the pad is smaller than
the axis -- bitwise for the LUTs, the redistributed histograms and the image; then checks derived from the definitions, and the
restatement's counters, which show that every branch ran: clipping with and without a residual, no clipping, padding in x only, in
y only and in both.  No GPU."""
import numpy as np
import pytest

import eq_oracle as eo
from isvins_amd import equalize as eq, tracker as trk

SIZES = [(1, 1, None), (1, 7, None), (7, 1, None), (3, 3, None), (8, 8, None), (9, 9, None), (15, 17, None), (64, 48, None), (97, 61, 104),
         (752, 480, None)]                     # (width, height, stride)
F = np.float32


def _reflect_index(n_ext, n):
    """BORDER_REFLECT_101 of 0 .. n_ext - 1 into an axis of length n, the general loop"""
    out = []
    for p in range(n_ext):
        while n > 1 and not 0 <= p < n:
            p = -p if p < 0 else 2 * (n - 1) - p
        out.append(0 if n == 1 else p)
    return np.array(out)


def _extend(img, ew, eh):
    h, w = img.shape
    if ew - w < w and eh - h < h:
        return np.pad(img, ((0, eh - h), (0, ew - w)), mode="reflect")
    return img[_reflect_index(eh, h)][:, _reflect_index(ew, w)]


def np_clahe(img, clip_limit, tiles_x, tiles_y):
    """-> (out, luts, bins) as eq_oracle.apply gives them"""
    h, w = img.shape
    ext = img
    if w % tiles_x or h % tiles_y:
        ext = _extend(img, w + tiles_x - w % tiles_x, h + tiles_y - h % tiles_y)
    tw, th = ext.shape[1] // tiles_x, ext.shape[0] // tiles_y
    area = tw * th
    lut_scale = F(255) / F(area)
    clip = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    bins = np.zeros((tiles_y, tiles_x, 256), np.int32)
    for j in range(tiles_y):
        for i in range(tiles_x):
            hist = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(hist - clip, 0).sum())
                hist = np.minimum(hist, clip) + clipped // 256
                residual = clipped % 256
                if residual:
                    hist[np.arange(0, 256, max(256 // residual, 1))[:residual]] += 1
            bins[j, i] = hist
            luts[j, i] = np.clip(np.rint(np.cumsum(hist).astype(F) * lut_scale), 0, 255).astype(np.uint8)

    def axis(n, t, tiles):
        f = np.arange(n).astype(F) * (F(1) / F(t)) - F(0.5)
        t1 = np.floor(f).astype(np.int32)
        a = f - t1.astype(F)
        return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, F(1) - a

    tx1, tx2, xa, xa1 = axis(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = axis(h, th, tiles_y)
    L = luts.astype(F)
    y1, y2, x1, x2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    res = (L[y1, x1, img] * xa1 + L[y1, x2, img] * xa) * ya1[:, None] + (L[y2, x1, img] * xa1 + L[y2, x2, img] * xa) * ya[:, None]
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8), luts, bins


def _cfg(p):
    return eq.make_config(*p)


@pytest.mark.parametrize("p", eo.PARAMS, ids=str)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_numpy_statement(size, p):
    lib = eo.load()
    w, h, stride = size
    kinds = ("dark", "random") if w * h > 100000 else ("const", "checker", "ramp", "dark", "random")
    for name, img in eo.images(w, h, stride).items():
        if name not in kinds:
            continue
        got = eo.apply(lib, _cfg(p), img, w)
        out, luts, bins = np_clahe(np.ascontiguousarray(img[:, :w]), *p)
        assert np.array_equal(got.bins, bins), (name, "bins", np.argwhere(got.bins != bins)[:4])
        assert np.array_equal(got.luts, luts), (name, "luts", np.argwhere(got.luts != luts)[:4])
        assert np.array_equal(got.out, out), (name, "image", np.argwhere(got.out != out)[:4])
        g = eo.Grid(lib, _cfg(p), w, h)
        assert (got.bins.sum(axis=2) == g.area).all() and g.area == g.tw * g.th          # the redistribution loses nothing
        assert (np.diff(got.luts.astype(np.int32), axis=2) >= 0).all() and (got.luts[:, :, 255] == 255).all()
        if name == "const":
            assert (got.out == got.out[0, 0]).all()


def test_grid_and_clip():
    lib = eo.load()
    g = eo.Grid(lib, _cfg((3.0, 8, 8)), 752, 480)
    assert (g.tw, g.th, g.ew, g.eh, g.clip, g.area) == (94, 60, 752, 480, 66, 5640) and g.lut_scale == F(255) / F(5640)
    g = eo.Grid(lib, _cfg((3.0, 8, 8)), 97, 61)
    assert (g.tw, g.th, g.ew, g.eh, g.clip) == (13, 8, 104, 64, 1)                       # 3 * 104 / 256 = 1.2
    g = eo.Grid(lib, _cfg((3.0, 8, 8)), 9, 8)                                            # K1: the axis that divides gets a whole grid more
    assert (g.tw, g.th, g.ew, g.eh, g.clip) == (2, 2, 16, 16, 1)
    assert eo.Grid(lib, _cfg((0.0, 8, 8)), 64, 48).clip == 0
    assert eo.Grid(lib, _cfg((0.001, 1, 1)), 8, 8).clip == 1                             # never below 1 once clipping is on
    assert eo.Grid(lib, _cfg((1e300, 1, 1)), 8, 8).clip == 64                            # E3
    import ctypes as C
    g6, s = (C.c_int32 * 6)(), C.c_float()
    for bad in ((-1.0, 8, 8), (float("nan"), 8, 8), (float("inf"), 8, 8), (3.0, 0, 8), (3.0, 8, 33)):
        assert lib.isvo_eq_grid(C.byref(_cfg(bad)), 64, 48, g6, C.byref(s)) == -1, bad
    assert lib.isvo_eq_grid(C.byref(_cfg((3.0, 8, 8))), 0, 48, g6, C.byref(s)) == -1


def test_tile_centre_reads_its_own_lut():
    lib = eo.load()
    for (w, h), p in (((64, 64), (3.0, 8, 8)), ((64, 48), (40.0, 2, 3)), ((64, 48), (0.0, 8, 8))):
        g = eo.Grid(lib, _cfg(p), w, h)
        assert g.tw % 2 == 0 and g.th % 2 == 0
        img = eo.images(w, h)["random"]
        got = eo.apply(lib, _cfg(p), img)
        fx = np.arange(w).astype(F) * (F(1) / F(g.tw)) - F(0.5)
        fy = np.arange(h).astype(F) * (F(1) / F(g.th)) - F(0.5)
        xs, ys = np.flatnonzero(fx == np.floor(fx)), np.flatnonzero(fy == np.floor(fy))
        xs, ys = xs[fx[xs] >= 0], ys[fy[ys] >= 0]
        assert len(xs) >= 2 and len(ys) >= 2 and (xs % g.tw == g.tw // 2).all() and (ys % g.th == g.th // 2).all()
        for y in ys:
            for x in xs:
                assert got.out[y, x] == got.luts[y // g.th, x // g.tw, img[y, x]], (w, h, p, x, y)


def test_uniform_histogram_without_clipping_is_the_identity_scaled():
    lib = eo.load()
    rng = np.random.Generator(np.random.PCG64(5))
    img = rng.permutation(np.repeat(np.arange(256), 4)).astype(np.uint8).reshape(32, 32)
    got = eo.apply(lib, _cfg((0.0, 1, 1)), img)
    want = np.rint((np.arange(256) + 1) * 255.0 / 256.0).astype(np.uint8)                # exact in double; half to even
    assert np.array_equal(got.luts[0, 0], want) and got.counters["unclipped"] == 1 and got.counters["clipped"] == 0
    assert np.array_equal(got.out, want[img])                                           # one tile: every pixel reads the one LUT


def test_counters_show_every_branch():
    lib = eo.load()
    # clipping with a residual: the smooth texture at the benchmark's size clips at 66
    big = eo.apply(lib, _cfg((3.0, 8, 8)), trk.analytic_image(752, 480, (0, 0), 3))
    assert eo.Grid(lib, _cfg((3.0, 8, 8)), 752, 480).clip == 66
    assert big.counters["clipped"] == 64 and big.counters["residual"] > 0 and big.counters["pad_cols"] == big.counters["pad_rows"] == 0
    # clipping without a residual: 32 x 32 in one tile, clip 12; one bin holds 12 + 256, 63 bins hold 12: clipped = 256 exactly
    flat = np.concatenate([np.zeros(268, np.uint8), np.repeat(np.arange(1, 64), 12).astype(np.uint8)])
    even = eo.apply(lib, _cfg((3.0, 1, 1)), flat.reshape(32, 32))
    assert even.counters == dict(clipped=1, residual=0, even=1, unclipped=0, pad_cols=0, pad_rows=0)
    assert even.bins[0, 0, 0] == 13 and (even.bins[0, 0, 1:64] == 13).all() and (even.bins[0, 0, 64:] == 1).all()
    # E1: a residual of 100 goes to every second bin from 0, not to the first 100
    flat = np.concatenate([np.zeros(12 + 100, np.uint8), np.repeat(np.arange(1, 77), 12).astype(np.uint8)])
    assert len(flat) == 1024
    res = eo.apply(lib, _cfg((3.0, 1, 1)), flat.reshape(32, 32))
    assert res.counters["residual"] == 1 and res.counters["even"] == 0
    assert res.bins[0, 0, 0] == 13 and res.bins[0, 0, 1] == 12 and res.bins[0, 0, 198] == 1 and res.bins[0, 0, 199] == 0 and res.bins[0, 0, 200] == 0
    # no clipping: the limit 0, and a limit no bin reaches
    off = eo.apply(lib, _cfg((0.0, 8, 8)), eo.images(64, 48)["random"])
    assert off.counters["unclipped"] == 64 and off.counters["clipped"] == 0
    high = eo.apply(lib, _cfg((40.0, 2, 3)), eo.images(64, 48)["random"])
    assert high.counters["unclipped"] == 6
    # padding in x only, in y only (K1: the other axis gets a whole grid more), in both, in neither
    for (w, h), (pc, pr) in (((9, 8), (7, 8)), ((8, 9), (8, 7)), ((9, 9), (7, 7)), ((97, 61), (7, 3)), ((8, 8), (0, 0)), ((1, 1), (7, 7))):
        c = eo.apply(lib, _cfg((3.0, 8, 8)), eo.images(w, h)["ramp"]).counters
        assert (c["pad_cols"], c["pad_rows"]) == (pc, pr), (w, h)


def test_stride_and_checks():
    lib = eo.load()
    imgs = eo.images(97, 61, 104)
    packed = np.ascontiguousarray(imgs["random"][:, :97])
    a, b = eo.apply(lib, _cfg((3.0, 8, 8)), imgs["random"], 97), eo.apply(lib, _cfg((3.0, 8, 8)), packed)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.luts, b.luts)               # the bytes behind the width are never read
    tcfg = trk.make_config(1, 1, 100, 80)
    st = lambda im, w=None: eo.check(lib, tcfg, eq.EqImage(im, w))
    z = np.zeros((61, 104), np.uint8)
    assert st(z, 97) == trk.ISV_TRK_OK and st(z, 100) == trk.ISV_TRK_OK and st(z, 101) == trk.ISV_TRK_CAPACITY
    assert st(np.zeros((81, 10), np.uint8)) == trk.ISV_TRK_CAPACITY and st(z, 0) == trk.ISV_TRK_INPUT and st(z, 105) == trk.ISV_TRK_INPUT
    it = eq.EqImage(z, 97)
    it.c.height = 0
    assert eo.check(lib, tcfg, it) == trk.ISV_TRK_INPUT
    it.c.height, it.c.data = 61, None
    assert eo.check(lib, tcfg, it) == trk.ISV_TRK_INPUT
