"""The landmark back-substitution inside k_build_solve_st (isv_build_solve_st.hip: all four wavefronts run backsub_landmark over the
window's landmarks before the kernel's outputs, from z_p and u_p staged over the dead pose blocks; chosen per upload,
UploadPlan::bsub_in_solve) against the same routine at the top of k_dogleg (ISV_BSUB_IN_DOGLEG=1, read when a handle is created): the same
routine on the same inputs in the same order per landmark, so every figure is BITWISE equal -- the Gauss-Newton step of the landmarks, the
steps, candidate cost and model cost change of the last iteration, and everything a caller downloads.

Two handles per case in one process, both forced onto k_build_solve_st (ISV_SOLVE_ST=1), the same windows, a full optimize.  A batch holds
three windows of different landmark counts: 1, 127, 128, 129, 257 and 300 are the trip edges of a 128-lane and a 256-lane loop; 384, 385 and
641 add a second and a third trip of the 256-lane loop.  The synthetic tracks are 2 + a geometric length, cut at the
window's end: every batch holds tracks of two frames (the minimum) and longer odd and even ones (asserted), the two trip forms of
backsub_landmark's pairwise loop."""
import ctypes

import numpy as np
import pytest

from isvins_amd import backend, synth
from test_gpu_solve import check_marg, check_window, oracle_run

pytestmark = pytest.mark.gpu

BATCHES = {"l1_128_257": (1, 128, 257), "l127_129_300": (127, 129, 300), "l384_385_641": (384, 385, 641)}


def _raw(x):
    return bytes(ctypes.string_at(ctypes.addressof(x), ctypes.sizeof(x)))


def _windows(N, Nvo, Ls, wid0):
    return [synth.make_window(wid0 + k, n_frames=N, n_vo=Nvo, n_landmarks=L) for k, L in enumerate(Ls)]


def _run(b, ws):
    """a full optimize of clones of ws on handle b -> every figure the two paths must share, as a dict of arrays / bytes"""
    gs = [w.clone() for w in ws]
    sums, margs = b.optimize_batch(gs)
    assert b.last_counts()[6] == 1                    # k_build_solve_st ran
    Ltot, B, npose = sum(w.L for w in ws), len(ws), 15 * (b.cfg.n_frames + b.cfg.estimate_extrinsic)      # (device frames: the extrinsic rides as a pseudo-frame)
    out = dict(gn_l=b.debug_read(11, Ltot), delta_p=b.debug_read(17, B * npose), delta_l=b.debug_read(18, Ltot),
               cost_c=b.debug_read(19, B), model=b.debug_read(20, B))
    for k, g in enumerate(gs):
        out[f"state{k}"] = g.state_vector(); out[f"depth{k}"] = g.lm_depth[: g.L].copy(); out[f"priors{k}"] = g.priors_vector()
    out["summaries"] = np.frombuffer(b"".join(_raw(s) for s in sums), np.uint8)          # (cost, radius, step and accept traces included)
    out["margs"] = np.frombuffer(b"".join(_raw(m) for m in margs), np.uint8)
    return out, gs, sums, margs


def _pair(monkeypatch, N, Nvo, ws, env=None, **kw):
    """(in k_dogleg, in k_build_solve_st): the same handle twice, the first created under ISV_BSUB_IN_DOGLEG=1"""
    cap = dict(max_landmarks=max(w.L for w in ws), max_obs=max(w.n_obs for w in ws), max_batch=len(ws), **kw)
    env = dict(env or {}, ISV_SOLVE_ST="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ISV_BSUB_IN_DOGLEG", "1")
    old = backend.Backend(N, Nvo, **cap)
    monkeypatch.delenv("ISV_BSUB_IN_DOGLEG")
    new = backend.Backend(N, Nvo, **cap)
    for k in env:
        monkeypatch.delenv(k)
    return old, new


def _assert_same(a, c):
    assert list(a) == list(c)
    for name in a:
        assert np.array_equal(a[name], c[name]), name
    assert np.isfinite(a["gn_l"]).all() and np.abs(a["gn_l"]).max() > 0


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("N,Nvo,generic", [(6, 3, False), (9, 4, False), (11, 5, False), (11, 5, True)])
def test_backsub_in_solve_is_bitwise_the_one_in_k_dogleg(monkeypatch, N, Nvo, generic, batch):
    """N = 6 and 9 run k_build_solve_st<false, 0>, N = 11 runs <false, 11> and, under ISV_GENERIC_N, <false, 0>"""
    ws = _windows(N, Nvo, BATCHES[batch], 500 + 10 * N)
    tracks = np.concatenate([np.diff(w.lm_obs_ptr[: w.L + 1]) for w in ws])
    assert tracks.min() == 2 and ((tracks > 2) & (tracks % 2 == 1)).any() and ((tracks > 2) & (tracks % 2 == 0)).any()
    old, new = _pair(monkeypatch, N, Nvo, ws, env=dict(ISV_GENERIC_N="1") if generic else None)
    try:
        a, _, sa, _ = _run(old, ws)
        c, _, _, _ = _run(new, ws)
        assert all(s.status == 0 and s.iterations >= 2 for s in sa)
        _assert_same(a, c)
    finally:
        old.close(); new.close()


def test_backsub_in_solve_behind_a_mu_retry(monkeypatch):
    """ISV_DEBUG_FORCE_RETRY=2 (the hook of test_gpu_branches.py; it is the handle's, so EVERY window of the batch retries): the first two
    factorisations of every iteration count as failed, mu goes up by 100, and the back-substitution runs with the kernel's FINAL mu"""
    ws = _windows(11, 5, (129, 40, 300), 640)
    old, new = _pair(monkeypatch, 11, 5, ws, env=dict(ISV_DEBUG_FORCE_RETRY="2"))
    monkeypatch.setenv("ISV_SOLVE_ST", "1")
    plain = backend.Backend(11, 5, max_landmarks=300, max_obs=max(w.n_obs for w in ws), max_batch=3)
    monkeypatch.delenv("ISV_SOLVE_ST")
    try:
        a, _, _, _ = _run(old, ws)
        c, _, _, _ = _run(new, ws)
        _assert_same(a, c)
        p, _, _, _ = _run(plain, ws)
        assert not np.array_equal(a["gn_l"], p["gn_l"])          # the retry changed the step: the hook did reach the kernel
    finally:
        old.close(); new.close(); plain.close()


def test_estimated_extrinsic_keeps_the_back_substitution_in_k_dogleg(oracle, monkeypatch):
    """ten real frames + the extrinsic's pseudo-frame: 11 device frames, so the 256-thread k_build_solve_st that holds the new routine, but
    the extrinsic block couples to every landmark (backsub_landmark<true>): the flag is off (tests/test_solve_plan_backsub.py), k_dogleg
    back-substitutes as before, and the solve agrees with the oracle; with and without the hook it is the same launch sequence, same bits"""
    ws = _windows(10, 5, (129, 40, 257), 660)
    old, new = _pair(monkeypatch, 10, 5, ws, estimate_extrinsic=1)
    try:
        a, _, _, _ = _run(old, ws)
        c, gs, sums, margs = _run(new, ws)
        _assert_same(a, c)
        for w, g, s, m in zip(ws, gs, sums, margs):
            o, so, mo = oracle_run(oracle, new.cfg, w)
            check_window(o, so, g, s); check_marg(mo, m, 5)
    finally:
        old.close(); new.close()
