"""GPU parity of the batched loop-closure verification (k_loop_match / k_loop_pnp, include/isvins_loop.h) against the CPU
restatement tests/native/isv_loop_oracle.c over the case list of tests/loop_cases.py, batch against single, kept buffers and
times, and the way into the pose graph.

Identical, with no exceptions: match_index, match_dist, n_matched, status, ransac_iters, ransac_inliers, n_final,
pnp_iterations, has_loop, loop_index and the inlier masks (the case list passes the knife-edge check of
tests/test_loop_oracle.py).  PnP_R_old / PnP_T_old / loop_info: |a - b| <= 1e-8 max(1, |b|), the SfM stage's figure for the same
CvLevMarq.  res / loop_weight are compared on the noisy cases only (on exact data the residual is float32 rounding noise, and a
1e-9 pose difference moves loop_weight by percents).
Measured on the MI355X over the seven noisy cases: worst relative difference of res 5.72e-15, of loop_weight 1.14e-14 (the worst
absolute pose difference over all cases was 2.84e-14).  Asserted: 100 x the larger figure, rounded up to a power of ten, 1e-11.
"""
import ctypes as C

import numpy as np
import pytest

import loop_cases
import loop_oracle
from isvins_amd import loop, posegraph as pg, synth

pytestmark = pytest.mark.gpu

RES_TOL = 1e-11
NOISY = ("noise2", "noise3", "out30_noise", "out60_noise", "m17", "m64", "m200")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return loop_oracle.build(tmp_path_factory.mktemp("loop_oracle"))


@pytest.fixture(scope="module")
def lv():
    v = loop.LoopVerifier(1024, loop_cases.MAX_POINTS, loop_cases.MAX_KEYPOINTS)
    yield v
    v.close()


@pytest.fixture(scope="module")
def reference(lib):
    """the restatement's answers for the case list, computed once"""
    return [loop_oracle.verify(lib, loop_cases.config(), p) for _, p, _ in loop_cases.all_pairs()]


INTS = ("status", "n_matched", "ransac_iters", "ransac_inliers", "pnp_iterations", "n_final", "has_loop", "loop_index")


def test_against_restatement(lv, reference):
    cases = loop_cases.all_pairs()
    rs, mis, mds, inls = lv.verify_batch([p for _, p, _ in cases], per_point=True)
    seen = set()
    worst = dict(pose=0.0, res=0.0, weight=0.0)
    for (name, pair, _), rg, mi, md, inl, (ro, omi, omd, oinl) in zip(cases, rs, mis, mds, inls, reference):
        seen.add(ro.status)
        assert [getattr(rg, f) for f in INTS] == [getattr(ro, f) for f in INTS], name
        if ro.status in (loop.ISV_LOOP_CAPACITY, loop.ISV_LOOP_INPUT):
            assert (mi == -2).all() and (md == -2).all() and (inl == -2).all(), name        # a refused pair's outputs stay untouched
            continue
        assert np.array_equal(mi, omi) and np.array_equal(md, omd) and np.array_equal(inl, oinl), name
        for f in ("PnP_R_old", "PnP_T_old", "loop_info"):
            a, b = rg.arr(f), ro.arr(f)
            worst["pose"] = max(worst["pose"], np.abs(a - b).max())
            assert (np.abs(a - b) <= 1e-8 * np.maximum(1.0, np.abs(b))).all(), (name, f)
        if name in NOISY:
            assert ro.res > 0 and ro.loop_weight > 0, name
            dr, dw = abs(rg.res - ro.res) / ro.res, abs(rg.loop_weight - ro.loop_weight) / ro.loop_weight
            worst["res"], worst["weight"] = max(worst["res"], dr), max(worst["weight"], dw)
            print(f"{name}: res {ro.res:.6e} rel diff {dr:.2e}; loop_weight {ro.loop_weight:.6e} rel diff {dw:.2e}")
    print(f"worst: pose {worst['pose']:.2e} res {worst['res']:.2e} loop_weight {worst['weight']:.2e}")
    assert seen == set(range(8)), seen
    assert worst["res"] <= RES_TOL and worst["weight"] <= RES_TOL, worst


def test_match_edges(lv):
    cases = loop_cases.match_cases()
    rs, mis, mds, inls = lv.verify_batch([p for _, p, _ in cases], per_point=True)
    for (name, pair, exp), r, mi, md in zip(cases, rs, mis, mds):
        assert (mi[0], md[0], r.n_matched == 1) == exp, name
        bi, bd, ba = loop_cases.brute_force(pair)
        assert np.array_equal(mi, bi) and np.array_equal(md, bd), name


def _usable():
    return [p for _, p, _ in loop_cases.all_pairs()]


@pytest.mark.parametrize("S", [1, 64, 1024])
def test_batch_bitwise(lv, S):
    ps = _usable()
    single = []
    for p in ps:
        r, mi, md, inl = lv.verify_batch([p], per_point=True)
        single.append((bytes(r[0]), mi[0].copy(), md[0].copy(), inl[0].copy()))
    idx = [(7 * i + 3) % len(ps) for i in range(S)]
    rs, mis, mds, inls = lv.verify_batch([ps[k] for k in idx], per_point=True)
    for i, (r, mi, md, inl) in enumerate(zip(rs, mis, mds, inls)):
        s = single[idx[i]]
        assert bytes(r) == s[0], i
        assert np.array_equal(mi, s[1]) and np.array_equal(md, s[2]) and np.array_equal(inl, s[3]), i


def test_buffers_kept_and_timed(lv):
    ps = [p for _, p, _ in loop_cases.all_pairs()]
    big = lv.verify_batch(ps * 16)
    call_ms, match_ms, pnp_ms = lv.last_ms()
    assert 0 < match_ms <= call_ms and 0 < pnp_ms <= call_ms and match_ms + pnp_ms <= call_ms
    small = lv.verify_batch(ps[:3])
    assert all(bytes(a) == bytes(b) for a, b in zip(small, big[:3]))
    assert lv.verify_batch([]) == []


def test_into_the_pose_graph(lv, lib):
    """a 20-keyframe chain without loops; its last keyframe verified against its first; isv_loop_apply fills the keyframe and
    isv_pgo_optimize closes the loop.  optimizeCS adds no factor of cur_index itself (pose_graph.cpp:314), so the list carries
    one more keyframe, the newest, as cur_index."""
    K = 20
    kf20, P, _ = pg.make_pose_graph(3, K, 0, drift=0.01)
    Rt = pg.pose_graph_truth(K)[1]
    kf = (pg.isv_pg_keyframe_t * (K + 1))()
    C.memmove(kf, kf20, C.sizeof(kf20))
    last, new = kf[K - 1], kf[K]
    C.memmove(C.byref(new), C.byref(last), C.sizeof(last))
    vR, vT = np.array(last.vio_R_w_i).reshape(3, 3), np.array(last.vio_T_w_i)
    step_R, step_t = synth._rot_zyx(0.05, 0.0, 0.0), np.array([0.3, 0.05, 0.0])
    new.index = K; new.time_stamp = 0.25 * K
    new.vio_T_w_i[:] = vT + vR @ step_t; new.vio_R_w_i[:] = (vR @ step_R).ravel()
    new.T_w_i[:] = new.vio_T_w_i[:]; new.R_w_i[:] = new.vio_R_w_i[:]
    last.relative_pose = kf[K - 2].relative_pose
    last.relative_pose.delta_t[:] = step_t; last.relative_pose.delta_R[:] = step_R.ravel()
    truth_last, truth_new = P[K - 1], P[K - 1] + Rt[K - 1] @ step_t
    # the old keyframe as the current (drifted) VIO frame sees it from the last keyframe
    old_R, old_T = vR @ Rt[K - 1].T @ Rt[0], vT + vR @ Rt[K - 1].T @ (P[0] - P[K - 1])
    pair, tr = loop.make_loop_scene(50, pixel_noise=loop_cases.NOISE, old_pose=(old_R, old_T), cur_pose=(vR, vT), old_index=0)
    rg = lv.verify_batch([pair])[0]
    ro = loop_oracle.verify(lib, loop_cases.config(), pair)[0]
    assert rg.status == ro.status == loop.ISV_LOOP_OK and rg.loop_index == 0
    by_hand = pg.clone_keyframes(kf)
    lv.apply(rg, kf[K - 1])
    assert kf[K - 1].has_loop == 1 and kf[K - 1].loop_index == 0
    h = by_hand[K - 1]
    h.has_loop, h.loop_index, h.loop_weight = 1, 0, ro.loop_weight
    h.loop_info[:] = list(ro.loop_info)
    opt = pg.PoseGraphOptimizer(64)
    before = (np.linalg.norm(np.array(kf[K - 1].T_w_i) - truth_last), np.linalg.norm(np.array(kf[K].T_w_i) - truth_new))
    r1 = opt.optimize(kf, 0, K)
    r2 = opt.optimize(by_hand, 0, K)
    opt.close()
    assert r1.status == 0 and r1.n_loop_edges == 1 and r2.n_loop_edges == 1
    after = (np.linalg.norm(np.array(kf[K - 1].T_w_i) - truth_last), np.linalg.norm(np.array(kf[K].T_w_i) - truth_new))
    print(f"last keyframe: {before[0]:.4f} m -> {after[0]:.4f} m from the truth; newest: {before[1]:.4f} -> {after[1]:.4f}")
    assert after[0] < before[0] and after[1] < before[1]
    same = bytes(rg.loop_info) == bytes(ro.loop_info) and rg.loop_weight == ro.loop_weight
    for k in range(K + 1):
        if same:
            assert bytes(kf[k]) == bytes(by_hand[k]), k
        else:
            assert np.abs(np.array(kf[k].T_w_i) - np.array(by_hand[k].T_w_i)).max() < 1e-8 and np.abs(np.array(kf[k].R_w_i) - np.array(by_hand[k].R_w_i)).max() < 1e-8, k
