"""The serial restatement of the feature detection (tests/native/isv_det_oracle.c) against independent numpy statements of the
definitions in include/isvins_detect.h: the Sobel pair and the box sums as integer convolutions over reflected padding (exact), the
response in np.float32 operations (bitwise), the disc against a transcription of the midpoint recurrence and against the Euclidean
disc where the two agree, setMask's order, the candidates by brute force, the properties of the greedy selection, the physical
check on bright rectangles, and the conditions the scenario list (tests/det_cases.py) is meant to reach, read from the restatement's
counters.  No GPU."""
import numpy as np
import pytest

import det_cases
import det_oracle as do
import trk_oracle
from isvins_amd import detect as det, tracker as trk


@pytest.fixture(scope="module")
def lib():
    return do.load()


def reflect(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def pad101(a, p=1):
    """np.pad(a, p, mode="reflect"), also for an axis shorter than the padding"""
    h, w = a.shape
    iy, ix = [reflect(i, h) for i in range(-p, h + p)], [reflect(i, w) for i in range(-p, w + p)]
    out = a[np.ix_(iy, ix)]
    if h > p and w > p:
        assert np.array_equal(out, np.pad(a, p, mode="reflect"))
    return out


def box3(a):
    h, w = a.shape[0] - 2, a.shape[1] - 2
    return sum(a[j:j + h, i:i + w] for j in range(3) for i in range(3))


def numpy_sums(img):
    P = pad101(img.astype(np.int64))
    h, w = img.shape
    win = lambda j, i: P[j:j + h, i:i + w]
    dx = (win(0, 2) - win(0, 0)) + 2 * (win(1, 2) - win(1, 0)) + (win(2, 2) - win(2, 0))
    dy = (win(2, 0) - win(0, 0)) + 2 * (win(2, 1) - win(0, 1)) + (win(2, 2) - win(0, 2))
    return dx, dy, box3(pad101(dx * dx)), box3(pad101(dx * dy)), box3(pad101(dy * dy))


def numpy_response(sxx, sxy, syy):
    f = np.float32
    k = f(1.0 / (3060.0 * 3060.0))
    a, b, c = sxx.astype(f) * k * f(0.5), sxy.astype(f) * k, syy.astype(f) * k * f(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def images():
    rng = np.random.Generator(np.random.PCG64(7))
    tiny = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((1, 1), (7, 1), (1, 7), (5, 2), (2, 5), (3, 3), (2, 2), (17, 33), (33, 34))]
    extreme = [np.where(rng.integers(0, 2, (9, 11)) == 0, 0, 255).astype(np.uint8)]
    return tiny + extreme + [s["image"][:, :s["width"]] for s in det_cases.scenarios() if s["image"] is not None and s["name"] != "big"]


def test_sums_and_response_against_numpy(lib):
    for img in images():
        img = np.ascontiguousarray(img)
        got = do.sums(lib, img)
        want = numpy_sums(img)
        for g, w, name in zip(got, want, ("Dx", "Dy", "Sxx", "Sxy", "Syy")):
            assert np.array_equal(g, w), (img.shape, name)
        assert max(np.abs(w).max() for w in want[2:]) < 2 ** 24
        e = do.response(lib, img)
        assert e.tobytes() == numpy_response(*want[2:]).astype(np.float32).tobytes(), img.shape
    # a stride is honoured
    s = det_cases.scenarios()[6]
    assert s["name"] == "s97" and np.array_equal(do.response(lib, s["image"], 97), do.response(lib, np.ascontiguousarray(s["image"][:, :97])))


def recurrence_disc(w, h, cx, cy, r):
    m = np.full((h, w), 255, np.uint8)

    def row(y, xa, xb):
        if 0 <= y < h:
            m[y, max(xa, 0):min(xb, w - 1) + 1] = 0
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        row(cy - dy, cx - dx, cx + dx); row(cy + dy, cx - dx, cx + dx); row(cy - dx, cx - dy, cx + dy); row(cy + dx, cx - dy, cx + dy)
        dy += 1; err += plus; plus += 2
        if err > 0:
            err -= minus; dx -= 1; minus -= 2
    return m


def test_disc_raster(lib):
    for r in range(1, 41):
        n = 2 * r + 5
        m, clipped = do.disc(lib, n, n, r + 2, r + 2, r)
        assert not clipped and np.array_equal(m, recurrence_disc(n, n, r + 2, r + 2, r)), r
        assert (m[0] == 255).all() and (m[:, 0] == 255).all() and (m[-2:] == 255).all() and (m[:, -2:] == 255).all()
        if r in (1, 2, 3, 5, 10, 30):
            yy, xx = np.mgrid[0:n, 0:n]
            assert np.array_equal(m == 0, (xx - r - 2) ** 2 + (yy - r - 2) ** 2 <= r * r), r
    # clipped at every edge and corner: the unclipped disc, cropped
    w, h, r = 20, 15, 5
    for cx in (0, 1, 4, 5, 10, 14, 15, 18, 19):
        for cy in (0, 2, 5, 7, 9, 10, 13, 14):
            full, _ = do.disc(lib, w + 2 * r, h + 2 * r, cx + r, cy + r, r)
            m, clipped = do.disc(lib, w, h, cx, cy, r)
            assert np.array_equal(m, full[r:r + h, r:r + w]), (cx, cy)
            assert clipped == (cx < r or cy < r or cx + r > w - 1 or cy + r > h - 1), (cx, cy)


def model_set_mask(lib, pts, cnt, w, h, r):
    order = sorted(range(len(pts)), key=lambda i: -int(cnt[i]))            # sorted is stable: ties keep the input order
    mask = np.full((h, w), 255, np.uint8)
    kept = []
    for i in order:
        x, y = int(np.rint(pts[i][0])), int(np.rint(pts[i][1]))           # np.rint rounds half to even
        if mask[y, x] == 255:
            kept.append(i)
            mask = np.minimum(mask, recurrence_disc(w, h, x, y, r))
    return kept, mask


def test_set_mask_order_and_ties(lib):
    cam = trk.make_config()
    img = det_cases.textured(40, 30, 40, 5)
    pts = np.array([[5, 5], [6.5, 5.5], [20, 20], [20.4, 20.4], [35, 5], [5.5, 25.5], [39, 29], [0, 0]], np.float32)
    for cnt in ([1] * 8, [1, 2, 3, 4, 5, 6, 7, 8], [3, 3, 1, 2, 2, 2, 9, 9], [5, 1, 1, 5, 2, 2, 2, 2]):
        for r in (1, 3, 6):
            cfg = det.make_config(1, 16, 50, r)
            d = do.detect(lib, cfg, cam, img, det.DetItem(0, pts, cnt, 0))
            kept, mask = model_set_mask(lib, pts, cnt, 40, 30, r)
            assert d.arrays.kept_index.tolist() == kept and np.array_equal(d.mask, mask), (cnt, r)
            assert d.r.n_kept == len(kept) and d.counters["dropped"] == 8 - len(kept) and d.r.n_new == 0 and d.eig is None
    # half to even: 6.5 -> 6, 5.5 -> 6, 25.5 -> 26
    d = do.detect(lib, det.make_config(1, 16, 50, 1), cam, img, det.DetItem(0, [[6.5, 5.5], [5.5, 25.5]], [1, 1], 0))
    assert d.mask[6, 6] == 0 and d.mask[26, 6] == 0 and (d.mask == 0).sum() == 10


def brute_candidates(eig, mask, quality):
    """(max_val, [(v, raster index)] sorted by descending v, then descending index)"""
    h, w = eig.shape
    sel = eig[mask != 0]
    max_val = np.float32(sel.max()) if sel.size else np.float32(0)
    t = np.float32(np.float64(max_val) * quality)
    v = np.where(eig > t, eig, np.float32(0)).astype(np.float32)
    if h < 3 or w < 3:
        return max_val, []
    dil = np.max([v[j:j + h - 2, i:i + w - 2] for j in range(3) for i in range(3)], axis=0)
    c = v[1:-1, 1:-1]
    ys, xs = np.nonzero((c != 0) & (c == dil) & (mask[1:-1, 1:-1] != 0))
    cand = [(float(c[y, x]), int((y + 1) * w + x + 1)) for y, x in zip(ys, xs)]
    return max_val, sorted(cand, key=lambda q: (-q[0], -q[1]))


def _good(ref):
    cfg, cam, scen, items, res = ref
    return [(s, it, d) for s, it, d in zip(scen, items, res) if d.r.status == det.ISV_DET_OK]


@pytest.mark.parametrize("min_dist", det_cases.MIN_DISTS)
def test_scenarios_candidates_and_selection_properties(lib, min_dist):
    ref = do.reference(min_dist)
    cfg, cam, scen, items, res = ref
    for s, d in zip(scen, res):
        assert d.r.status == s["want"], s["name"]
        if d.r.status != det.ISV_DET_OK:
            assert (d.r.n_kept, d.r.n_new, d.r.n_candidates, d.r.max_val) == (0, 0, 0, 0.0) and d.r.n_points == s["item"].c.n_points
    for s, it, d in _good(ref):
        name, w = s["name"], s["width"]
        kept, mask = model_set_mask(lib, it.points, it.track_cnt, w, s["image"].shape[0], min_dist)
        assert d.arrays.kept_index.tolist() == kept and np.array_equal(d.mask, mask), name
        if it.c.max_new == 0:
            assert d.eig is None and d.r.n_candidates == 0 and d.r.n_new == 0
            continue
        max_val, cand = brute_candidates(d.eig, d.mask, cfg.quality_level)
        assert np.float32(d.r.max_val).tobytes() == max_val.tobytes() and d.r.n_candidates == len(cand), name
        acc = d.arrays.new_pts.astype(np.int64)
        assert np.array_equal(acc.astype(np.float32), d.arrays.new_pts)
        accepted = {(int(x), int(y)): k for k, (x, y) in enumerate(acc)}
        assert len(accepted) == len(acc) == d.r.n_new <= it.c.max_new
        # every accepted pair is at least min_dist apart; every accepted corner is a candidate outside the mask discs
        if len(acc) > 1:
            d2 = ((acc[:, None, :] - acc[None, :, :]) ** 2).sum(axis=2)
            assert d2[~np.eye(len(acc), dtype=bool)].min() >= min_dist * min_dist, name
        cand_at = {(i % w, i // w): k for k, (_, i) in enumerate(cand)}
        assert all(p in cand_at and d.mask[p[1], p[0]] != 0 for p in accepted), name
        # in priority order: accepted in that order; a rejected one lies within min_dist of an accepted one of higher priority,
        # unless the cap was reached first
        n_acc = 0
        for v, i in cand:
            p = (i % w, i // w)
            if p in accepted:
                assert accepted[p] == n_acc, name
                n_acc += 1
            elif n_acc < it.c.max_new:
                assert n_acc > 0 and (((acc[:n_acc] - p) ** 2).sum(axis=1) < min_dist * min_dist).any(), (name, p)
        assert n_acc == d.r.n_new and d.counters["cap_reached"] == (n_acc == it.c.max_new)
        # the capped result is a prefix of the uncapped one; the lift is the tracker restatement's
        if name != "big":
            u = do.uncapped(lib, cfg, cam, s["image"], it, w)
            assert u.arrays.new_pts[:d.r.n_new].tobytes() == d.arrays.new_pts.tobytes() and u.r.n_new >= d.r.n_new, name
            assert d.r.n_new == min(u.r.n_new, it.c.max_new), name
        assert trk_oracle.lift(trk_oracle.load(), cam, d.arrays.new_pts[:40]).tobytes() == d.arrays.new_un_pts[:40].tobytes(), name


def test_rectangles_physical_check(lib):
    cfg, cam, scen, items, res = do.reference(30)
    (s, it, d), = [(s, it, d) for s, it, d in zip(scen, items, res) if s["name"] == "rects"]
    corners = np.array(det_cases.rect_corners())
    got = d.arrays.new_pts.astype(np.int64)
    # Sobel 3 after box 3 has a support of 2 pixels: farther than that from a rectangle corner the window sees a straight edge or a
    # flat area, one of Dx, Dy vanishes throughout it and the smaller eigenvalue is exactly 0
    cheb = np.abs(got[:, None, :] - corners[None, :, :]).max(axis=2)
    assert (cheb.min(axis=1) <= 2).all()
    assert d.r.n_new == len(corners) and sorted(cheb.argmin(axis=1).tolist()) == list(range(len(corners)))
    far = np.ones(d.eig.shape, bool)
    for x, y in corners:
        far[y - 2:y + 3, x - 2:x + 3] = False
    assert (d.eig[far] == 0).all() and d.r.max_val > 0
    # with a cap below the number of corners: a prefix
    capped = do.detect(lib, cfg, cam, s["image"], det.DetItem(0, None, None, 5))
    assert capped.r.n_new == 5 and capped.arrays.new_pts.tobytes() == d.arrays.new_pts[:5].tobytes() and capped.counters["cap_reached"]


def test_condition_coverage(lib):
    by = {}
    for md in det_cases.MIN_DISTS:
        cfg, cam, scen, items, res = do.reference(md)
        by[md] = {s["name"]: (it, d) for s, it, d in zip(scen, items, res)}
    it, d = by[30]["const"]
    assert d.r.max_val == 0 and d.r.n_candidates == 0 and d.r.n_new == 0 and (d.eig == 0).all()         # a constant image
    it, d = by[30]["covered"]
    assert d.counters["masked"] == 24 * 23 and d.r.max_val == 0 and d.r.n_new == 0 and d.r.n_kept == 1   # a mask that covers everything
    assert by[1]["covered"][1].r.n_new > 0
    it, d = by[3]["checker"]
    assert d.counters["plateau"] > 0 and d.counters["tie_pairs"] > 0 and d.r.n_new > 1                   # tied maxima; the raster index decides
    first = d.arrays.new_pts[0]
    _, cand = brute_candidates(d.eig, d.mask, 0.01)
    top = [i for v, i in cand if v == cand[0][0]]
    assert len(top) > 1 and first.tolist() == [max(top) % 64, max(top) // 64]
    for md in det_cases.MIN_DISTS:                                                                        # the cap reached exactly, and not
        for name in ("s24", "s64_first"):
            if (md, name) == (30, "s24"):         # its five discs cover the image
                continue
            it, d = by[md][name]
            assert d.r.n_new == it.c.max_new > 1 and d.counters["cap_reached"] and d.counters["rejected"] + d.r.n_new <= d.r.n_candidates, (md, name)
    it, d = by[30]["s64_one"]
    assert 0 < d.r.n_new < it.c.max_new and not d.counters["cap_reached"] and d.counters["rejected"] > 0
    it, d = by[1]["big"]
    assert d.r.n_new == it.c.max_new == 120 and d.r.n_candidates > 120
    assert all(by[md]["checker_big"][1].r.n_candidates > 16384 for md in (1, 3)) and by[3]["checker_big"][1].r.n_new == 40
    it, d = by[30]["s97"]
    assert d.r.n_new == 1 and it.c.max_new == 1
    it, d = by[30]["s200"]
    assert it.c.max_new == 0 and d.r.n_kept > 0 and d.counters["dropped"] > 0 and d.counters["clipped"] > 0   # setMask only; dropped; clipped
    assert by[30]["s3x3"][0].c.n_points == 0 and by[30]["s3x3"][1].r.n_kept == 0                          # no points
    assert by[30]["s3x3"][1].r.n_candidates <= 1 and by[30]["s2x5"][1].r.n_candidates == 0               # one interior pixel; none
    assert by[3]["s2x5"][1].r.n_kept == 1 and by[3]["s2x5"][1].counters["clipped"] == 1
    wants = {d.r.status for it, d in by[30].values()}
    assert wants == {det.ISV_DET_OK, det.ISV_DET_CAPACITY, det.ISV_DET_INPUT}
    # null output arrays with a non-zero count
    cfg, cam = det_cases.det_config(30), det_cases.trk_config()
    img = det_cases.scenarios()[4]["image"]
    r = det.isv_det_result_t()
    import ctypes as C
    item = det.DetItem(0, None, None, 3)
    lib.isvo_det_detect(C.byref(cfg), C.byref(cam), img.ctypes.data_as(do._u8p), 64, 48, 64, C.byref(item.c), C.byref(r), None, None, None, None, None, None)
    assert r.status == det.ISV_DET_INPUT
