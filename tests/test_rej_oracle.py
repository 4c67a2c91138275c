"""CPU checks that pin the restatement of the outlier rejection (tests/native/isv_rej_oracle.c, include/isvins_reject.h): the gate and
the choice of method by point count, the lift against a numpy statement, the RNG, the subsets and the serial RANSAC loop against the
Python-integer reading of tests/relpose_highprec.py, the LMedS median and sigma against numpy on recorded error vectors, the planted
outliers of the scenes, the hooks that switch single quirks off, the item refusals, and the edges the case table has to cover (asserted
from the restatement's own counts: the guard against a seed that drifts)."""
import ctypes as C
import math

import numpy as np
import pytest

import rej_cases as rc
import rej_oracle as ro
import relpose_highprec as rph
from isvins_amd import reject as rej, tracker as trk


@pytest.fixture(scope="module")
def lib():
    return ro.load()


@pytest.fixture(scope="module")
def table(lib):
    """every table case through the restatement, once: name -> (Case, Rejected)"""
    tc, cfg = rc.tracker_config(), rc.rejector_config()
    out = {}
    for name in rc.TABLE:
        c = rc.case(name)
        out[name] = (c, ro.reject(lib, tc, cfg, c.item()))
    return out


def lmeds_niters():
    """max(RANSACUpdateNumIters(0.99, 0.45, 7, 1000), 3), computed"""
    return max(round(math.log(1 - 0.99) / math.log(1 - (1 - 0.45) ** 7)), 3)


def test_gate_and_method_by_point_count(lib, table):
    assert lib.isvo_rej_lmeds_niters() == lmeds_niters() == 300
    for name, n, method in (("n0", 0, rej.NONE), ("n7", 7, rej.NONE), ("lmeds8_exact", 8, rej.LMEDS), ("lmeds14_exact", 14, rej.LMEDS), ("ransac15_exact", 15, rej.RANSAC)):
        c, r = table[name]
        assert (c.n, r.res.status, r.res.n_points, r.res.method) == (n, 0, n, method), name
        if method == rej.NONE:
            assert r.status.tolist() == [1] * n and (r.res.n_kept, r.res.iters, r.res.best_inliers, r.res.min_median) == (n, 0, 0, -1.0)
        elif method == rej.LMEDS:
            assert r.res.iters == lmeds_niters() and r.res.min_median >= 0 and r.res.best_inliers == r.res.n_kept
        else:
            assert 1 <= r.res.iters <= 1000 and r.res.min_median == -1.0
    for name, (c, r) in table.items():
        assert r.res.n_kept == int(r.status.sum()) and set(r.status.tolist()) <= {0, 1}, name
        if r.res.method == rej.RANSAC:
            assert r.res.best_inliers == r.res.n_kept, name        # no refit: the mask is the kept model's inliers again


@pytest.mark.parametrize("cam", [dict(), dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0), dict(fx=500.0, fy=510.0, cx=370.0, cy=230.0, k1=-0.1, k2=0.02, p1=1e-3, p2=-2e-3)],
                         ids=["euroc", "no_distortion", "other"])
def test_lift_is_the_numpy_statement(lib, cam):
    tc = rc.tracker_config(**cam)
    rng = np.random.Generator(np.random.PCG64(77))
    px = (rng.random((500, 2)) * np.array([752.0, 480.0])).astype(np.float32)
    for focal, w, h in ((460.0, 752, 480), (460.0, 753, 481), (100.5, 1, 8192)):
        cfg = rc.rejector_config(focal_length=focal)
        got, want = ro.lift(lib, tc, cfg, w, h, px), rc.lift(tc, px, focal, w, h)
        assert got.tobytes() == want.tobytes(), (focal, w, h)
    # the formula itself on an undistorted camera: x = FOCAL_LENGTH * (u - cx) / fx + COL / 2.0
    tc = rc.tracker_config(k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    got = ro.lift(lib, tc, rc.rejector_config(), 752, 480, px).astype(np.float64)
    want = np.stack([460.0 * (px[:, 0] - tc.cx) / tc.fx + 376.0, 460.0 * (px[:, 1] - tc.cy) / tc.fy + 240.0], axis=1)
    assert np.abs(got - want).max() < 1e-4


def test_rng_and_subsets_are_the_python_integer_reading(lib):
    state, mine = rph._M64, C.c_uint64(rph._M64)
    for n in (8, 14, 15, 150, 4096, 7, 1000003) * 20:
        state, v = rph.rng_uniform(state, n)
        assert lib.isvo_rej_uniform(C.byref(mine), n) == v and mine.value == state
    for count in (8, 14, 15, 64, 150, 4096):
        got, end = ro.subsets(lib, count, 130)
        state = rph._M64
        for k in range(130):
            state, idx = rph.subset(state, count)
            assert got[k].tolist() == idx and len(set(idx)) == 7, (count, k)
        assert end == state


def test_serial_loop_is_the_python_integer_reading(lib):
    """the RANSAC of a scene in normalised coordinates (an identity camera, focal 1, relpose's threshold) against
    relpose_highprec.Ransac on the restatement's own lifted points"""
    tc = rc.tracker_config(fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    cfg = rc.rejector_config(focal_length=1.0, f_threshold=rph.THRESH)
    for seed, n, outliers in ((40, 40, 10), (41, 24, 3)):
        c = rc.scene(n, seed, outliers=outliers, noise=0.1 / 460, cam=tc)
        item = rej.RejItem(1, 1, c.prev, c.cur)
        r = ro.reject(lib, tc, cfg, item)
        P = np.concatenate([ro.lift(lib, tc, cfg, 1, 1, c.prev), ro.lift(lib, tc, cfg, 1, 1, c.cur)], axis=1).astype(np.float64)
        st = dict(min_band=1.0, min_band64=1.0, min_gate=1.0, min_cheir=1.0, min_disc=1.0, min_f33=1.0, null_resid=0.0, routes=[], multi_keep_equal=[])
        ref = rph.Ransac(P, rph._M64, st)
        assert st["min_band"] > rph.BAND and st["min_band64"] > rph.BAND and not st["routes"] and not st["multi_keep_equal"], st   # the scene, not the code
        assert (r.res.method, r.res.iters, r.res.best_inliers) == (rej.RANSAC, ref.iters, ref.inliers), seed
        assert r.status.astype(bool).tolist() == ref.mask.tolist(), seed
        assert r.keeps == [k[0] for k in ref.keeps], seed
        assert not r.status[c.planted].any()


def np_median(e):
    """LMeDSPointSetRegistrator::run's median: the float32 patterns sorted as signed integers"""
    s = np.sort(np.array(e, np.float32).view(np.int32)).view(np.float32)
    n = len(s)
    return float(s[n // 2]) if n % 2 else float(np.float32(s[n // 2 - 1] + s[n // 2])) * 0.5


@pytest.mark.parametrize("name", list(rc.ERROR_VECTORS))
def test_median_and_sigma_against_numpy(lib, name):
    e = rc.ERROR_VECTORS[name]
    got, want = ro.median(lib, e), np_median(e)
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
    if name == "nan_first":
        assert want == 4.0                          # the NaN sorts above everything: the median is that of the nine with NaN as the largest
    if name == "inf_and_nan":
        assert want == 2.5
    if name == "even_inexact_sum":
        assert want != (float(np.float32(0.7)) + float(np.float32(1.0000001))) * 0.5      # the sum is rounded to float32 first
    for count in (8, 9, 14):
        for med in (want if want == want else 1.0, 0.0, 1e-30, 0.09):
            sigma = max(2.5 * 1.4826 * (1 + 5.0 / (count - 7)) * math.sqrt(med), 0.001)
            assert lib.isvo_rej_sigma(count, med) == sigma
    assert lib.isvo_rej_sigma(8, 0.0) == 0.001


def test_planted_outliers(table):
    seen = {"exact": 0, "noise": 0}
    for name, (c, r) in table.items():
        if r.res.method == rej.NONE or not c.planted.size or name.startswith("ransac40_unrelated"):
            continue
        st = r.status.astype(bool)
        if name in rc.UNDECIDABLE:
            assert r.res.min_median < 1e-20 and r.res.n_kept >= 7, name      # every model passes through 7 of the 8 points
            continue
        assert not st[c.planted].any(), name
        if c.noise == 0.0:
            assert st[~c.planted].all(), name
            seen["exact"] += int(c.planted.sum())
        else:
            seen["noise"] += int(c.planted.sum())
    assert seen["exact"] > 100 and seen["noise"] > 400


def test_each_hook_changes_a_named_case(lib, table):
    tc, cfg = rc.tracker_config(), rc.rejector_config()

    def with_hook(mask, name):
        with ro.quirks_off(lib, mask):
            return ro.reject(lib, tc, cfg, table[name][0].item())

    for mask, name in ((ro.DOUBLE_POINTS, "lmeds14_noise"), (ro.DOUBLE_ERROR, "lmeds14_noise"), (ro.RANSAC_BELOW_15, "lmeds14_exact")):
        assert with_hook(mask, name).key() != table[name][1].key(), (mask, name)
        assert with_hook(0, name).key() == table[name][1].key()
    assert with_hook(ro.RANSAC_BELOW_15, "lmeds14_exact").res.method == rej.RANSAC
    e = rc.ERROR_VECTORS["nan_first"]
    with ro.quirks_off(lib, ro.FLOAT_SORT):
        as_floats = ro.median(lib, e)
    assert as_floats == 3.0 and ro.median(lib, e) == 4.0       # by `<` the NaN stays in front and shifts the middle
    # a hook leaves what it does not concern alone
    assert with_hook(ro.RANSAC_BELOW_15 | ro.FLOAT_SORT, "ransac65_exact").key() == table["ransac65_exact"][1].key()


def test_refusals(lib):
    cfg = rc.rejector_config(max_points=20)
    c = rc.scene(20, 50, outliers=2)

    def status(width=752, height=480, n=None, prev=True, cur=True, has_out=1, poison=None):
        it = rej.RejItem(width, height, c.prev.copy(), c.cur.copy())
        if poison is not None:
            (it.prev_pts if poison[0] == 0 else it.cur_pts)[poison[1], poison[2]] = poison[3]
        if n is not None:
            it.c.n_points = n
        if not prev:
            it.c.prev_pts = None
        if not cur:
            it.c.cur_pts = None
        return lib.isvo_rej_check(C.byref(cfg), C.byref(it.c), has_out)

    assert status() == trk.ISV_TRK_OK and status(width=1, height=8192) == trk.ISV_TRK_OK
    for bad in (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(n=-1), dict(prev=False), dict(cur=False), dict(has_out=0),
                dict(poison=(0, 3, 1, float("nan"))), dict(poison=(1, 19, 0, float("inf"))), dict(poison=(1, 0, 1, float("-inf")))):
        assert status(**bad) == trk.ISV_TRK_INPUT, bad
    big = rej.RejItem(752, 480, np.zeros((21, 2)), np.zeros((21, 2)))
    assert lib.isvo_rej_check(C.byref(cfg), C.byref(big.c), 1) == trk.ISV_TRK_CAPACITY
    big.c.prev_pts = None                              # the capacity comes before the arrays are looked at
    assert lib.isvo_rej_check(C.byref(cfg), C.byref(big.c), 0) == trk.ISV_TRK_CAPACITY
    assert status(n=0, prev=False, cur=False, has_out=0) == trk.ISV_TRK_OK
    # a refused item writes nothing
    r = ro.reject(lib, rc.tracker_config(), cfg, big)
    assert (r.res.status, r.res.n_points, r.res.n_kept, r.res.method, r.res.min_median) == (trk.ISV_TRK_CAPACITY, 21, 0, rej.NONE, -1.0) and not len(r.status)
    # the configuration
    for bad in (dict(max_items=0), dict(max_items=65536), dict(max_points=0), dict(max_points=4097), dict(focal_length=0.0), dict(focal_length=float("nan")),
                dict(focal_length=float("inf")), dict(f_threshold=0.0), dict(f_threshold=-1.0), dict(f_threshold=float("nan")), dict(f_threshold=float("inf"))):
        assert lib.isvo_rej_check_config(C.byref(rej.make_config(**bad)), 65535) == 0, bad
    assert lib.isvo_rej_check_config(C.byref(rej.make_config(max_points=4096)), 65535) == 1
    assert lib.isvo_rej_check_config(C.byref(rej.make_config(max_points=300)), 299) == 0


def test_table_covers_the_edges(table):
    ransac = {n: r for n, (c, r) in table.items() if r.res.method == rej.RANSAC}
    iters = {n: r.res.iters for n, r in ransac.items()}
    assert any(i < 64 for i in iters.values())
    assert any(64 < i <= 128 for i in iters.values()), iters
    assert any(128 < i < 1000 for i in iters.values()), iters
    assert iters["ransac40_unrelated"] == 1000
    assert any(any(64 <= k < 128 for k in r.keeps) for r in ransac.values())                    # a keep in the second chunk
    assert any(r.keeps and r.keeps[-1] % 64 not in (0, 63) and r.res.iters > 128 and r.keeps[-1] == r.res.iters - 1 for r in ransac.values())   # ... that ends the loop mid-chunk
    c, r = table["ransac100_all_inliers"]
    assert r.res.iters == 1 and r.res.best_inliers == c.n == r.res.n_kept and r.keeps[0] == 0   # niters fell to 0 at the first keep
    assert {c.n for c, _ in table.values()} >= set(rc.COUNTS) and rc.MAX_POINTS == rej.MAX_POINTS == 4096
    assert {c.n for n, (c, r) in table.items() if r.res.method == rej.LMEDS} >= {8, 14}
    assert all(r.res.status == 0 for _, r in table.values())
    deg = rc.degenerate()
    assert {c.n for c in deg.values()} == {8, 14, 20} and len(deg) == 10
