"""CPU checks that pin tests/native/isv_trk_oracle.c, the serial restatement of include/isvins_tracker.h, independently of the
GPU: pyrDown and the Scharr derivatives against separable numpy convolutions over np.pad(mode="reflect"), the window values, the
five sums and a step against Python integers and np.float32 operations, the lift, shift invariance between two crops of one
texture, known sub-pixel translations of an analytic texture (the physical check), the kept quirks T1..T4, and the conditions the
scenario list of tests/trk_cases.py must meet so that tests/test_gpu_trk.py cannot pass on empty ground."""
import numpy as np
import pytest

import trk_cases
import trk_oracle as to
from isvins_amd import tracker as trk
from test_kf_oracle import py_lift

f32 = np.float32
K5 = [1, 4, 6, 4, 1]
# The physical check: the largest error of the restatement's flow over PHYS_SHIFTS on the fixture of test_known_translations, as
# measured (pixels), and the bound the test asserts: twice that.  (The fixture is 8-bit: the flow of a quantised, resampled texture
# is not the translation to better than a few hundredths of a pixel.)
PHYS_SHIFTS = [(0.3, -0.4), (2.5, 1.25), (-6.75, 4.5), (11.6, -9.3), (-12.0, 8.2), (0.0, 12.0)]
PHYS_MEASURED = 0.0979               # 0.09788 at the shift (-12, 8.2); 0.052 .. 0.065 at the other sub-pixel shifts
PHYS_BOUND = 2 * PHYS_MEASURED


@pytest.fixture(scope="module")
def lib():
    return to.load()


@pytest.fixture(scope="module")
def ref():
    return to.reference(True)


def np_pyrdown(img):
    a = img.astype(np.int64)
    h, w = a.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    p = np.pad(a, ((0, 0), (2, 2)), mode="reflect")
    rows = sum(K5[k] * p[:, k::2][:, :dw] for k in range(5))
    p = np.pad(rows, ((2, 2), (0, 0)), mode="reflect")
    return ((sum(K5[k] * p[k::2, :][:dh, :] for k in range(5)) + 128) >> 8).astype(np.uint8)


def np_scharr(img):
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    t0 = 3 * (p[:-2, :] + p[2:, :]) + 10 * p[1:-1, :]
    t1 = p[2:, :] - p[:-2, :]
    return t0[:, 2:] - t0[:, :-2], 3 * (t1[:, :-2] + t1[:, 2:]) + 10 * t1[:, 1:-1]


def np_weights(a, b):
    one = f32(1)
    iw00 = int(np.rint((one - a) * (one - b) * f32(16384)))
    iw01 = int(np.rint(a * (one - b) * f32(16384)))
    iw10 = int(np.rint((one - a) * b * f32(16384)))
    return iw00, iw01, iw10, 16384 - iw00 - iw01 - iw10


def np_bilinear(padded, pad, ix, iy, iw, n):
    """DESCALE(bilinear, n) over the 21 x 21 window at (ix, iy) of an image padded by `pad`"""
    y0, x0 = iy + pad, ix + pad
    c = lambda dy, dx: padded[y0 + dy:y0 + dy + 21, x0 + dx:x0 + dx + 21]
    return (c(0, 0) * iw[0] + c(0, 1) * iw[1] + c(1, 0) * iw[2] + c(1, 1) * iw[3] + (1 << (n - 1))) >> n


def np_probe(prev, cur, p, q):
    """the window of prev at p - (10, 10) and one step of cur from q - (10, 10), from the definitions"""
    PAD = 24
    P = np.pad(prev.astype(np.int64), PAD, mode="reflect")
    J = np.pad(cur.astype(np.int64), PAD, mode="reflect")
    gx, gy = (np.pad(g, PAD) for g in np_scharr(prev))                   # zero outside the level
    px, py, qx, qy = f32(p[0]) - f32(10), f32(p[1]) - f32(10), f32(q[0]) - f32(10), f32(q[1]) - f32(10)
    ipx, ipy, iqx, iqy = (int(np.floor(v)) for v in (px, py, qx, qy))
    iw = np_weights(px - f32(ipx), py - f32(ipy))
    I, dIx, dIy = np_bilinear(P, PAD, ipx, ipy, iw, 9), np_bilinear(gx, PAD, ipx, ipy, iw, 14), np_bilinear(gy, PAD, ipx, ipy, iw, 14)
    S11, S12, S22 = (int(v.sum()) for v in (dIx * dIx, dIx * dIy, dIy * dIy))
    diff = np_bilinear(J, PAD, iqx, iqy, np_weights(qx - f32(iqx), qy - f32(iqy)), 9) - I
    T1, T2, Tabs = int((diff * dIx).sum()), int((diff * dIy).sum()), int(np.abs(diff).sum())
    scale = f32(2.0 ** -20)
    A11, A12, A22, b1, b2 = (f32(v) * scale for v in (S11, S12, S22, T1, T2))
    D = A11 * A22 - A12 * A12
    minEig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + f32(4) * A12 * A12)) / f32(882)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Dinv = f32(1) / D
        delta = ((A12 * b2 - A22 * b1) * Dinv, (A12 * b1 - A11 * b2) * Dinv)
    return dict(I=I, dIx=dIx, dIy=dIy, sums=[S11, S12, S22, T1, T2, Tabs], f=np.array([A11, A12, A22, D, minEig, delta[0], delta[1]], f32))


def test_pyramid_against_numpy(lib, ref):
    cfg, scen, res = ref
    seen = set()
    for s, t in zip(scen, res):
        if t.pyr_cur is None:
            continue
        it = s["item"]
        for img, pyr in ((it.prev, t.pyr_prev), (it.cur, t.pyr_cur)):
            want = [img[:, :it.c.width]]
            for w, h in trk.levels(it.c.width, it.c.height)[1:]:
                want.append(np_pyrdown(want[-1]))
                assert want[-1].shape == (h, w)
            assert len(pyr) == len(want) == t.r.n_levels, s["name"]
            for l, (g, w) in enumerate(zip(pyr, want)):
                assert np.array_equal(g, w), (s["name"], l)
        seen.add(t.r.n_levels)
    assert seen == {1, 2, 3, 4}
    # odd and even sizes, down to the smallest source a level can have
    rng = np.random.Generator(np.random.PCG64(7))
    for w, h in ((43, 44), (44, 43), (45, 87), (50, 46)):
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        pyr = to.pyramid(lib, img)
        assert len(pyr) == len(trk.levels(w, h)) >= 2 and np.array_equal(pyr[1], np_pyrdown(img)), (w, h)
    edges = ((42, 100), (43, 43), (84, 85), (85, 85), (168, 169), (169, 169), (8192, 8192), (1, 1))
    assert [len(trk.levels(w, h)) for w, h in edges] == [1, 2, 2, 3, 3, 4, 4, 1]
    for w, h in edges:
        assert [s[:2] for s in to.level_shapes(lib, w, h)[0]] == trk.levels(w, h)


def test_scharr_against_numpy(lib, ref):
    cfg, scen, res = ref
    rng = np.random.Generator(np.random.PCG64(8))
    imgs = [rng.integers(0, 256, (h, w)).astype(np.uint8) for w, h in ((2, 2), (3, 7), (24, 23), (64, 48))]
    imgs += [t.pyr_prev[-1] for t in res if t.pyr_prev is not None]
    step = np.zeros((9, 10), np.uint8); step[:, 5:] = 255                   # a full-contrast edge: the largest derivative, 16 * 255
    imgs += [np.full((9, 9), 255, np.uint8), np.tile(np.array([[0, 255]], np.uint8), (8, 4)), step, step.T.copy(), 255 - step]
    big = 0
    for img in imgs:
        ix, iy = to.scharr(lib, img)
        wx, wy = np_scharr(img)
        assert np.array_equal(ix, wx) and np.array_equal(iy, wy), img.shape
        big = max(big, int(np.abs(wx).max()), int(np.abs(wy).max()))
    assert big == 4080                                      # 16 * 255: the largest derivative occurs


def test_window_sums_and_step_against_numpy(lib):
    prev, cur = trk_cases.pair(1)
    prev, cur = prev[:, :64].copy(), cur[:, :64].copy()
    cases = [((30.25, 22.5), (31.0, 21.75)), ((12.0, 12.0), (12.0, 12.0)), ((-10.5, 20.0), (-3.25, 18.5)), ((70.9, 55.3), (60.1, 50.7)),
             ((33.333, 7.777), (30.123, 9.876)), ((0.0, 0.0), (73.99, 57.99)), ((52.6, 40.2), (-10.99, -10.01))]
    n = 0
    for p, q in cases:
        g, w = to.probe(lib, prev, cur, p, q), np_probe(prev, cur, p, q)
        assert g is not None, (p, q)
        for k in ("I", "dIx", "dIy"):
            assert np.array_equal(g[k], w[k]), (p, q, k)
        assert g["sums"].tolist() == w["sums"], (p, q)
        ok = np.isfinite(w["f"])
        assert g["f"][ok].tobytes() == w["f"][ok].tobytes() and ok[:5].all(), (p, q, g["f"], w["f"])
        n += int(ok.all())
    assert n >= 5
    assert to.probe(lib, prev, cur, (-11.5, 20.0), (20.0, 20.0)) is None and to.probe(lib, prev, cur, (20.0, 20.0), (74.0, 20.0)) is None
    assert to.probe(lib, prev, cur, (3.0e9, 20.0), (20.0, 20.0)) is None                  # D2


def test_lift_against_python(lib):
    for distorted in (True, False):
        cfg = trk_cases.config(distorted)
        uv = np.array([[0, 0], [363.0, 248.1], [751.5, 479.25], [-20.5, 500.0], [100.125, 33.3]], f32)
        want = np.array([py_lift(cfg, u, v) for u, v in uv], f32)
        assert to.lift(lib, cfg, uv).tobytes() == want.tobytes()


def test_shift_invariance(lib):
    """Two crops of one pair whose origins differ by a multiple of 4 (three levels): the integers of a window do not depend on the
    crop, bit for bit; the tracked flow agrees to two termination thresholds (0.01 pixel each: the float32 coordinates differ between
    the crops, so the two iterations may end a step apart)."""
    cfg = trk.make_config(1, 1, 400, 400, max_points=4096)
    (pa, ca), (pb, cb), (dx, dy) = trk_cases.texture_crops()
    assert dx % 4 == 0 and dy % 4 == 0 and len(trk.levels(pa.shape[1], pa.shape[0])) == 3
    h, w = pa.shape
    m = 64                                                  # 12 level-2 pixels of window, 2 of border influence, the flow
    xs, ys = np.arange(m + dx, w - m, 3.25), np.arange(m + dy, h - m, 2.75)
    pts = np.array([(x, y) for y in ys for x in xs], f32)
    assert len(pts) >= 20
    off = np.array([dx, dy], f32)
    for p in pts[:12]:
        q = p + f32(1.5)
        a, b = to.probe(lib, pa, ca, p, q), to.probe(lib, pb, cb, p - off, q - off)
        for k in ("I", "dIx", "dIy", "sums", "f"):
            assert np.array_equal(a[k], b[k]), (p, k)
    ta, tb = to.track(lib, cfg, trk.TrkItem(0, ca, pa, pts)), to.track(lib, cfg, trk.TrkItem(0, cb, pb, pts - off))
    assert (ta.arrays.flags == 3).all() and (tb.arrays.flags == 3).all()
    d = np.abs((ta.arrays.cur_pts - pts) - (tb.arrays.cur_pts - (pts - off)))
    print("shift invariance: largest difference of the two flows", d.max())
    assert d.max() <= 0.02


def test_known_translations(lib):
    """the physical check: the flow between an analytic texture and the same texture sampled at shifted coordinates is the shift"""
    cfg = trk.make_config(1, 1, 320, 240, max_points=4096)
    w, h = 320, 240
    assert len(trk.levels(w, h)) == 4
    prev = trk.analytic_image(w, h, (0, 0), 40)
    pts = np.array([(x, y) for y in np.arange(60.0, h - 60, 11.3) for x in np.arange(60.0, w - 60, 13.7)], f32)
    worst = 0.0
    for shift in PHYS_SHIFTS:
        t = to.track(lib, cfg, trk.TrkItem(0, trk.analytic_image(w, h, shift, 40), prev, pts))
        assert (t.arrays.flags == 3).all() and t.r.n_kept == len(pts) and t.r.n_levels == 4, shift
        e = float(np.abs(t.arrays.cur_pts.astype(np.float64) - pts - np.array(shift)).max())
        print("known translation", shift, "largest error", e)
        worst = max(worst, e)
    print("known translations: largest error", worst, "bound", PHYS_BOUND)
    assert worst <= PHYS_BOUND


def _by_name(ref):
    cfg, scen, res = ref
    return {s["name"]: (s, t) for s, t in zip(scen, res)}


def test_quirks_change_results(lib, ref):
    cfg = ref[0]
    by = _by_name(ref)
    # T1: the checkerboard's upper levels are rejected, and its points end with status 1
    s, t = by["checker"]
    assert ((t.term[:, 1:] == to.TERM_MINEIG).any(axis=1) & (t.arrays.flags & 1 == 1)).sum() >= 4
    t1 = to.track(lib, cfg, s["item"], to.T1)
    assert ((t.arrays.flags & 1) > (t1.arrays.flags & 1)).sum() >= 4 and t1.r.n_kept < t.r.n_kept
    changed = {q: 0 for q in (to.T2, to.T3, to.T4)}
    for name, (s, t) in by.items():
        if t.r.status != trk.ISV_TRK_OK or not t.r.n_points:
            continue
        # T2: where the err pass cleared status, it stays 1 without it
        e = (t.term[:, 0] & to.TERM_ERRPASS) != 0
        t2 = to.track(lib, cfg, s["item"], to.T2)
        assert ((t2.arrays.flags[e] & 1) == 1).all() and ((t.arrays.flags[e] & 1) == 0).all()
        assert np.array_equal(t2.arrays.flags[~e], t.arrays.flags[~e]) and np.array_equal(t2.arrays.cur_pts, t.arrays.cur_pts)
        changed[to.T2] += int(e.sum())
        # T3: a point whose level 0 ended by the half-step ends elsewhere without it
        o = (t.term[:, 0] & 15) == to.TERM_OSC
        t3 = to.track(lib, cfg, s["item"], to.T3)
        assert (t3.term & 15 != to.TERM_OSC).all()
        changed[to.T3] += int((t3.arrays.cur_pts[o] != t.arrays.cur_pts[o]).any(axis=1).sum())
        same = ((t.term & 15) != to.TERM_OSC).all(axis=1)
        assert np.array_equal(t3.arrays.cur_pts[same], t.arrays.cur_pts[same])
        # T4: a window that hangs outside the image is refused without it
        t4 = to.track(lib, cfg, s["item"], to.T4)
        changed[to.T4] += int(((t.arrays.flags & 1) > (t4.arrays.flags & 1)).sum())
    assert changed[to.T2] >= 2 and changed[to.T3] >= 2 and changed[to.T4] >= 10, changed


def test_scenario_list_covers_the_ground(ref):
    cfg, scen, res = ref
    by = _by_name(ref)
    for s, t in zip(scen, res):
        assert t.r.status == s["want"], s["name"]
        assert [s["item"].c.slot for s in scen if s["name"] != "bad_slot"] == [i for i, s in enumerate(scen) if s["name"] != "bad_slot"]
    good = [(s, t) for s, t in zip(scen, res) if t.r.status == trk.ISV_TRK_OK]
    sizes = {(s["item"].c.width, s["item"].c.height, s["item"].c.stride): t.r.n_levels for s, t in good}
    want = {(24, 23, 24): 1, (64, 48, 64): 2, (97, 61, 104): 2, (200, 120, 200): 3, (181, 179, 181): 4, (752, 480, 752): 4}
    assert {k: sizes.get(k) for k in want} == want
    assert trk.levels(181, 179)[-1] == (23, 23)
    assert sum(s["item"].c.width == 752 for s, _ in good) == 1
    assert {t.r.status for t in res} == {trk.ISV_TRK_OK, trk.ISV_TRK_CAPACITY, trk.ISV_TRK_INPUT}
    assert all(s["item"].c.n_points <= 40 for s, _ in good) and sum(8 <= s["item"].c.n_points <= 40 for s, _ in good) >= 7
    assert by["no_points"][1].r.n_points == 0 and by["no_points"][1].r.n_levels == 2
    term = np.vstack([t.term for _, t in good if len(t.term)])
    flags = np.concatenate([t.arrays.flags for _, t in good])
    l0 = term[:, 0] & 15
    # every way a level-0 iteration can end, the rejections, the err pass
    for code in (to.TERM_EPS, to.TERM_CAP, to.TERM_OSC, to.TERM_RANGE, to.TERM_MINEIG, to.TERM_IP):
        assert (l0 == code).sum() >= 2, code
    assert ((term[:, 0] & to.TERM_ERRPASS) != 0).sum() >= 2
    assert (flags[(term[:, 0] & to.TERM_ERRPASS) != 0] & 1 == 0).all()
    # ... and above level 0: the cap, the half-step, the range break; a rejection above level 0 followed by status 1
    for code in (to.TERM_CAP, to.TERM_OSC, to.TERM_RANGE):
        assert (term[:, 1:] == code).any(), code
    assert (((term[:, 1:] == to.TERM_MINEIG) | (term[:, 1:] == to.TERM_IP)).any(axis=1) & (flags & 1 == 1)).sum() >= 4
    # bit 1 clear with bit 0 set, both set, both clear
    assert (flags == 1).sum() >= 3 and (flags == 3).sum() >= 40 and (flags == 0).sum() >= 10 and (flags == 2).sum() >= 1
    # ip.x == -21 is kept (the range test passes), -22 is rejected; the same at the other edge; beyond int's range (D2)
    for s, t in good:
        if s["item"].c.n_points < 24:
            continue
        w = s["item"].c.width
        p = s["item"].points
        assert np.floor(p[16, 0] - 10) == -21 and np.floor(p[17, 0] - 10) == -22 and np.floor(p[18, 0] - 10) == w - 1 and np.floor(p[19, 0] - 10) == w
        assert (t.term[16, 0] & 15) != to.TERM_IP and (t.term[17, 0] & 15) == to.TERM_IP, s["name"]
        assert (t.term[18, 0] & 15) != to.TERM_IP and (t.term[19, 0] & 15) == to.TERM_IP, s["name"]
        assert (np.abs(p[20:22]) > 2.0 ** 31).any() and (t.term[20:23, 0] == to.TERM_IP).all() and (t.arrays.flags[20:23] == 0).all()
    # status 0 leaves err and the lifted point 0; status 1 lifts the point
    for _, t in good:
        dead = (t.arrays.flags & 1) == 0
        assert (t.arrays.err[dead] == 0).all() and (t.arrays.cur_un_pts[dead] == 0).all()
        assert np.array_equal(t.arrays.cur_un_pts[~dead], to.lift(to.load(), cfg, t.arrays.cur_pts[~dead]))
        assert t.r.n_kept == int((t.arrays.flags == 3).sum())
        assert len(t.arrays.kept()[0]) == t.r.n_kept
    assert (np.concatenate([t.arrays.err for _, t in good]) > 0).sum() >= 40
    # the two cameras differ in the lift only
    und = to.reference(False)[2]
    big = [i for i, s in enumerate(scen) if s["name"] == "big"][0]
    assert np.array_equal(und[big].arrays.cur_pts, res[big].arrays.cur_pts) and not np.array_equal(und[big].arrays.cur_un_pts, res[big].arrays.cur_un_pts)
