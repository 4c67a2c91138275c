"""GPU parity of the batched outlier rejection (k_rej_f, include/isvins_reject.h) against the serial CPU restatement
tests/native/isv_rej_oracle.c over the case table of tests/rej_cases.py: every case alone, the cases in one shuffled batch and in a
batch padded to 130 items, refused items between good ones, the degenerate inputs, the timing contract, and one chain of tracking,
rejection and detection at 160 x 120 against the same chain through the three restatements.

Compared with the restatement with no tolerance: status, n_points, n_kept, method, iters, best_inliers, the bits of min_median and the
status array.  Both sides run one text (isv_init_common.h, isv_pinhole.h, isv_reject.h) with contraction off; they can differ only
where the device's and the host's pow / acos / cos / log round apart in a hypothesis' cubic."""
import numpy as np
import pytest

import det_oracle as do
import rej_cases as rc
import rej_oracle as ro
import trk_oracle as to
from isvins_amd import backend, detect as det, reject as rej, tracker as trk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    """the table's tracker (only its camera, device and stream matter) and rejector"""
    c = rc.tracker_config()
    tr = trk.Tracker(1, 1, 64, 48, max_points=c.max_points)
    rj = rej.Rejector(tr, max_items=130, **rc.R_CFG)
    yield tr, rj
    rj.close()
    tr.close()


@pytest.fixture(scope="module")
def want():
    """every table case and every degenerate input through the restatement, once: name -> (Case, Rejected)"""
    lib, tc, cfg = ro.load(), rc.tracker_config(), rc.rejector_config()
    cases = {n: rc.case(n) for n in rc.TABLE}
    cases.update(rc.degenerate())
    return {n: (c, ro.reject(lib, tc, cfg, c.item())) for n, c in cases.items()}


def _describe(res):
    return {f: getattr(res, f) for f in ro.FIELDS + ("min_median",)}


@pytest.mark.parametrize("name", list(rc.TABLE))
def test_case_against_restatement(gpu, want, name):
    c, ref = want[name]
    (r,), (st,) = gpu[1].reject_batch([c.item()])
    print(name, _describe(r), _describe(ref.res), "status arrays differ at", np.flatnonzero(st != ref.status)[:8])
    assert ro.key_of(r, st) == ref.key(), (name, _describe(r), _describe(ref.res))
    assert r.n_kept == int(st.sum())


def test_batch_independence(gpu, want):
    names = list(rc.TABLE)
    alone = {n: ro.key_of(*[x[0] for x in gpu[1].reject_batch([want[n][0].item()])]) for n in names}
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(names))
    rs, sts = gpu[1].reject_batch([want[names[i]][0].item() for i in order])
    for i, r, st in zip(order, rs, sts):
        assert ro.key_of(r, st) == alone[names[i]], ("shuffled", names[i])
    small = [n for n in names if want[n][0].n <= 150]
    padded = [small[k % len(small)] for k in range(130)]
    rs, sts = gpu[1].reject_batch([want[n][0].item() for n in padded])
    for n, r, st in zip(padded, rs, sts):
        assert ro.key_of(r, st) == alone[n], ("padded", n)
    assert gpu[1].reject_batch([]) == ([], [])


def test_refusals_between_good_items(gpu, want):
    tr, _ = gpu
    rj = rej.Rejector(tr, max_items=6, max_points=150)
    good = [want[n] for n in ("ransac150_noise", "lmeds14_noise", "ransac65_exact")]
    big = want["ransac_max_points"][0].item()                     # beyond this rejector's max_points
    bad_size = rej.RejItem(0, 480, good[0][0].prev, good[0][0].cur)
    nan = good[2][0].cur.copy(); nan[64, 1] = np.nan
    bad_point = rej.RejItem(752, 480, good[2][0].prev, nan)
    items = [good[0][0].item(), big, good[1][0].item(), bad_size, bad_point, good[2][0].item()]
    rs, sts = rj.reject_batch(items)                              # (reject_batch asserts that a refused item's array is untouched)
    assert [r.status for r in rs] == [0, trk.ISV_TRK_CAPACITY, 0, trk.ISV_TRK_INPUT, trk.ISV_TRK_INPUT, 0]
    for k, g in zip((0, 2, 5), good):
        assert ro.key_of(rs[k], sts[k]) == g[1].key(), k
    for k in (1, 3, 4):
        assert (rs[k].n_points, rs[k].n_kept, rs[k].method, rs[k].iters, rs[k].best_inliers, rs[k].min_median) == (items[k].c.n_points, 0, rej.NONE, 0, 0, -1.0)
        assert len(sts[k]) == 0
    null = good[0][0].item()
    null.c.cur_pts = None
    (r,), _ = rj.reject_batch([null])
    assert r.status == trk.ISV_TRK_INPUT
    rs, _ = rj.reject_batch([bad_size, big])                      # a call without a good item launches nothing
    assert [r.status for r in rs] == [trk.ISV_TRK_INPUT, trk.ISV_TRK_CAPACITY]
    rj.reject_batch([good[0][0].item()])
    ms = rj.last_ms()
    with pytest.raises(backend.BackendError, match="ISV_ERR_CAPACITY"):
        rj.reject_batch([good[1][0].item()] * 7)                  # more items than max_items: nothing is enqueued
    assert rj.last_ms() == ms
    rj.close()


def test_degenerate_inputs(gpu):
    deg = rc.degenerate()
    names = list(deg)
    rs, sts = gpu[1].reject_batch([deg[n].item() for n in names])
    for n, r, st in zip(names, rs, sts):
        c = deg[n]
        assert r.status == 0 and r.n_points == c.n == len(st) and set(st.tolist()) <= {0, 1} and r.n_kept == int(st.sum()), n
        assert r.method == (rej.LMEDS if c.n < 15 else rej.RANSAC) and 1 <= r.iters <= 1000, n
        (r1,), (s1,) = gpu[1].reject_batch([c.item()])
        assert ro.key_of(r1, s1) == ro.key_of(r, st), n


def test_timing_contract(gpu, want):
    rj = gpu[1]
    rj.reject_batch([want["ransac150_noise"][0].item()] * 16)
    ms = rj.last_ms()
    assert len(ms) == 4 and all(np.isfinite(m) and 0 <= m < 10000 for m in ms), ms
    assert ms[0] > 0 and ms[1] > 0 and ms[0] >= ms[1] + ms[2] + ms[3], ms


def test_chain_track_reject_detect_against_the_restatements():
    """two sequences at 160 x 120: track, reduceVector by both flag bits, rejectWithF, reduceVector by its status, setMask and
    goodFeaturesToTrack, against the same chain through the three restatements.  Every array goes from stage to stage as it is."""
    tlib, rlib, dlib = to.load(), ro.load(), do.load()
    w, h, MAX_CNT = 160, 120, 40
    tcfg = trk.make_config(2, 2, w, h, max_points=64)
    dcfg = det.make_config(2, 64, MAX_CNT, 10, det.QUALITY)
    tr = trk.Tracker(2, 2, w, h, max_points=64)
    dt = det.Detector(tr, 2, max_points=64, max_corners=MAX_CNT, min_dist=10)
    rj = rej.Rejector(tr)
    assert (rj.cfg.max_items, rj.cfg.max_points) == (2, 64)
    frames = [[trk.analytic_image(w, h, s, seed) for s in ((0, 0), shift)] for seed, shift in ((60, (2.25, -1.5)), (61, (-1.75, 2.5)))]
    # frame 0: the slots take the images, the first corners are born; the second sequence keeps 12 of them (LMedS)
    rs, _ = tr.track_batch([trk.TrkItem(s, frames[s][0], frames[s][0]) for s in (0, 1)])
    assert all(r.status == trk.ISV_TRK_OK for r in rs)
    _, born = dt.detect_batch([det.DetItem(s, None, None, MAX_CNT) for s in (0, 1)])
    pts = [born[0].new_pts.copy(), born[1].new_pts[:12].copy()]
    cnt = [np.ones(len(p), np.int32) for p in pts]
    assert len(pts[0]) >= 20 and len(pts[1]) == 12
    # frame 1 on the GPU
    g_t = tr.track_batch([trk.TrkItem(s, frames[s][1], None, pts[s]) for s in (0, 1)])
    g_red = [a.kept(pts[s], cnt[s]) for s, a in enumerate(g_t[1])]               # (cur_pts, cur_un_pts, prev_pts, track_cnt)
    g_r = rj.reject_batch([rej.RejItem(w, h, red[2], red[0]) for red in g_red])
    g_red2 = [rej.reduce_vector(st, red[2], red[0], red[3] + 1) for st, red in zip(g_r[1], g_red)]
    g_d = dt.detect_batch([det.DetItem(s, red[1], red[2], MAX_CNT - len(red[1])) for s, red in enumerate(g_red2)])
    # the same chain through the restatements
    for s in (0, 1):
        t = to.track(tlib, tcfg, trk.TrkItem(s, frames[s][1], frames[s][0], pts[s]))
        assert bytes(g_t[0][s]) == bytes(t.r) and all(getattr(g_t[1][s], f).tobytes() == getattr(t.arrays, f).tobytes() for f in ("cur_pts", "flags", "err", "cur_un_pts"))
        red = t.arrays.kept(pts[s], cnt[s])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(red, g_red[s]))
        r = ro.reject(rlib, tcfg, rj.cfg, rej.RejItem(w, h, red[2], red[0]))
        assert ro.key_of(g_r[0][s], g_r[1][s]) == r.key(), (s, _describe(g_r[0][s]), _describe(r.res))
        assert r.res.method == (rej.RANSAC, rej.LMEDS)[s] and r.res.n_points == len(red[0]) >= (15, 8)[s]
        red2 = rej.reduce_vector(r.status, red[2], red[0], red[3] + 1)
        assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(red2, g_red2[s]))
        d = do.detect(dlib, dcfg, tcfg, frames[s][1], det.DetItem(s, red2[1], red2[2], MAX_CNT - len(red2[1])))
        assert bytes(g_d[0][s]) == bytes(d.r) and all(getattr(g_d[1][s], f).tobytes() == getattr(d.arrays, f).tobytes() for f in ("kept_index", "new_pts", "new_un_pts"))
        assert d.r.status == det.ISV_DET_OK and d.r.n_kept + d.r.n_new <= MAX_CNT
    rj.close(); dt.close(); tr.close()
