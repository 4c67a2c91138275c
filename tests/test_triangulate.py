"""FeatureManager::triangulate (src/feature_tracker/feature_manager.cpp:206-258): the oracle restatement against
exact geometry (CPU), and the HIP kernel against the oracle through the C ABI (GPU)."""
import ctypes as C

import numpy as np
import pytest

from isvins_amd import abi, synth


def _exact_window(seed=3, n_lm=40):
    """a window whose observations are the exact projections of known landmarks (no noise, true poses)"""
    w = synth.make_window(seed, n_landmarks=n_lm)
    rng = np.random.default_rng(seed)
    N = w.N
    Ps, Rs = np.array(w.Ps).reshape(N, 3), np.array(w.Rs).reshape(N, 3, 3)
    tic, ric = np.array(w.tic).reshape(3), np.array(w.ric).reshape(3, 3)
    true_depth = np.zeros(w.L)
    pts = w.obs_point.reshape(-1, 3)
    for l in range(w.L):
        h, o0, o1 = int(w.lm_start_frame[l]), int(w.lm_obs_ptr[l]), int(w.lm_obs_ptr[l + 1])
        dep = rng.uniform(1.0, 7.0)
        true_depth[l] = dep
        pc = pts[o0] / pts[o0][2] * dep                         # point in the host camera frame (z = depth)
        pw = Rs[h] @ (ric @ pc + tic) + Ps[h]
        for o in range(o0 + 1, o1):
            j = h + (o - o0)
            pcj = ric.T @ (Rs[j].T @ (pw - Ps[j]) - tic)
            pts[o] = pcj / pcj[2]
    w.obs_point[...] = pts.reshape(w.obs_point.shape)
    return w, true_depth


def test_oracle_triangulate_recovers_exact_depths(oracle):
    w, true_depth = _exact_window()
    cfg = abi.make_config(w.N, w.Nvo, max_landmarks=w.L, max_obs=w.n_obs, max_batch=1)
    keep = np.array(w.lm_depth[: w.L]).copy()
    w.lm_depth[: w.L : 2] = -1.0                                # every other landmark has no depth yet
    assert oracle.isvo_triangulate(C.byref(cfg), C.byref(w.c())) == 0
    got = np.array(w.lm_depth[: w.L])
    assert np.array_equal(got[1::2], keep[1::2])                # landmarks with a depth are left alone
    assert np.abs(got[::2] / true_depth[::2] - 1).max() < 1e-8


def test_oracle_triangulate_clamps_to_init_depth(oracle):
    w, _ = _exact_window(seed=4)
    cfg = abi.make_config(w.N, w.Nvo, max_landmarks=w.L, max_obs=w.n_obs, max_batch=1)
    pts = w.obs_point.reshape(-1, 3)
    l = 0
    o0, o1 = int(w.lm_obs_ptr[l]), int(w.lm_obs_ptr[l + 1])
    pts[o0 + 1 : o1] = pts[o0]                                  # no parallax at all -> depth far outside [0.1, 8]
    w.obs_point[...] = pts.reshape(w.obs_point.shape)
    w.lm_depth[l] = 0.0
    assert oracle.isvo_triangulate(C.byref(cfg), C.byref(w.c())) == 0
    d0 = float(w.lm_depth[l])
    assert d0 == cfg.init_depth or 0.1 <= d0 <= 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,n_vo", [(11, 5), (18, 8)])
def test_gpu_triangulate_matches_oracle(oracle, n_frames, n_vo):
    from isvins_amd import backend
    backend.build()
    ws = synth.make_windows([60, 61, 62], n_frames=n_frames, n_vo=n_vo, n_landmarks=120)
    b = backend.Backend(n_frames, n_vo, max_landmarks=120, max_obs=120 * n_frames, max_batch=4)
    try:
        for w in ws:
            w.lm_depth[: w.L : 3] = -1.0
            w.lm_depth[1 : w.L : 7] = 0.0
        ref = [w.clone() for w in ws]
        for o in ref:
            assert oracle.isvo_triangulate(C.byref(b.cfg), C.byref(o.c())) == 0
        b.triangulate(ws)
        for w, o in zip(ws, ref):
            a, e = np.array(w.lm_depth[: w.L]), np.array(o.lm_depth[: o.L])
            # QR + one-sided Jacobi on the GPU vs one-sided Jacobi SVD in the oracle (against 40 digits: tests/test_gpu_prep_highprec.py)
            assert np.abs(a / e - 1).max() < 1e-7, np.abs(a / e - 1).max()
    finally:
        b.close()


@pytest.mark.gpu
def test_gpu_solve_odometry_is_triangulate_then_optimize(oracle):
    """isv_backend_solve_odometry_batch (one hand-over) against isv_backend_triangulate followed by
    isv_backend_optimize_batch: the same bits; and against the oracle doing the two steps (src/estimator.cpp:461-472)"""
    from isvins_amd import backend
    backend.build()
    ws = synth.make_windows(range(60, 66), n_landmarks=200)
    for w in ws:
        w.lm_depth[: w.L : 3] = -1.0                            # a third of the landmarks has no depth yet
    be = backend.Backend(11, 5, max_landmarks=200, max_obs=max(w.n_obs for w in ws), max_batch=len(ws))
    a = [w.clone() for w in ws]; b = [w.clone() for w in ws]
    sa, ma = be.solve_odometry_batch(a)
    be.triangulate(b); sb, mb = be.optimize_batch(b)
    for x, y, s1, s2 in zip(a, b, sa, sb):
        assert np.array_equal(x.state_vector(), y.state_vector()) and s1.final_cost == s2.final_cost and s1.iterations == s2.iterations
        assert np.array_equal(x.lm_solve_flag[: x.L], y.lm_solve_flag[: y.L])
    for i in (0, 5):
        o = ws[i].clone(); s = abi.isv_summary_t(); mg = abi.isv_marg_result_t()
        assert oracle.isvo_triangulate(C.byref(be.cfg), C.byref(o.c())) == 0
        assert oracle.isvo_optimize(C.byref(be.cfg), C.byref(o.c()), C.byref(s), C.byref(mg)) == 0
        assert sa[i].iterations == s.iterations and abs(sa[i].final_cost - s.final_cost) < 1e-8 * s.final_cost
        assert np.abs(a[i].Ps - o.Ps).max() < 1e-7 and np.abs(a[i].Rs - o.Rs).max() < 1e-7
    be.close()
