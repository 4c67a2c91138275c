"""GPU parity of the batched visual-inertial alignment (k_visual_imu_align, is-vins_amd/csrc/isv_initial.h) against the CPU
restatement tests/native/isv_init_oracle.c, and batch against single.  Tolerances: status identical; repropagated deltas
1e-12; window states 1e-6 relative; g and s 1e-8 relative; a problem's result in a batch of 1 / 64 / 1024 bitwise equal to
the same problem solved alone.

The tolerances are round numbers, not derived ones.  What float64 allows on each field, per case, and how far the kernel is from the exact
answer of its own equations is tests/test_gpu_align_highprec.py (model and limits: tests/align_highprec.py; figures: DESIGN.md section 11).
Its limits lie 100 to 1e5 times below the tolerances here, and it asserts that the fields before the first atan2 are bytewise the
restatement's; the tolerances here stay as the coarse guard on every case, the singular and refused ones included."""
import ctypes as C

import numpy as np
import pytest

import align_oracle
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

CASES = [dict(), dict(seed=1, acc_noise=0.01, gyr_noise=0.001), dict(n_frames=20, cam_dt=0.05), dict(radius=3.0, speed=0.5),
         dict(bg=(0.01, -0.02, 0.005), Bgs0=np.full((11, 3), 0.002)), dict(hover=True),
         dict(n_frames=16, window_frame=[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 15]),
         dict(n_frames=initial.ISV_ALIGN_MAX_FRAMES, window_frame=list(range(0, 40, 2)), cam_dt=0.05, imu_per_frame=5),
         dict(sfm_scale=-0.37), dict(n_frames=initial.ISV_ALIGN_MAX_FRAMES + 1, window_frame=list(range(11))),
         dict(seed=14, speed=0.02, acc_noise=0.05, gyr_noise=0.002), dict(discrete=True),
         dict(discrete=True, R_w_c0=np.diag([1.0, -1.0, -1.0]))]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


@pytest.fixture(scope="module")
def be():
    b = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    yield b
    b.close()


def _problems():
    ps = [initial.make_problem(**kw) for kw in CASES]
    g = initial.make_problem()
    g.imu[:, 1:4] *= 1.2
    for f in g.frames:
        f.linearized_acc[:] = [1.2 * a for a in f.linearized_acc]
    ps.append(g)
    bad = initial.make_problem()
    bad.c.window_frame[3] = bad.c.window_frame[2]
    ps.append(bad)
    return ps


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def test_against_restatement(lib, be):
    ps = _problems()
    rs = initial.align_batch(be, ps)
    seen = set()
    for p, rg in zip(ps, rs):
        ro = align_oracle.solve(lib, p)
        assert rg.status == ro.status, (rg.status, ro.status)
        seen.add(ro.status)
        if ro.status == 4:
            continue
        nf, nw = p.c.n_frames, p.c.n_window
        assert _rel(rg.arr("delta_bg"), ro.arr("delta_bg")) < 1e-10
        assert _rel(rg.arr("rp_delta_p")[:nf], ro.arr("rp_delta_p")[:nf]) < 1e-12
        assert _rel(rg.arr("rp_delta_v")[:nf], ro.arr("rp_delta_v")[:nf]) < 1e-12
        assert _rel(rg.arr("rp_delta_q")[:nf], ro.arr("rp_delta_q")[:nf]) < 1e-12
        assert rg.n_state == ro.n_state
        assert _rel(rg.arr("g_linear"), ro.arr("g_linear")) < 1e-8
        assert abs(rg.s_linear - ro.s_linear) <= 1e-8 * max(1.0, abs(ro.s_linear))
        if ro.status != 0:
            continue
        assert _rel(rg.arr("g"), ro.arr("g")) < 1e-8 and _rel(rg.arr("g_c0"), ro.arr("g_c0")) < 1e-8
        assert abs(rg.s - ro.s) <= 1e-8 * max(1.0, abs(ro.s))
        for name in ("Ps", "Rs", "Vs", "Bgs"):
            assert _rel(rg.arr(name)[:nw], ro.arr(name)[:nw]) < 1e-6, name
        assert _rel(rg.arr("x")[:3 * nf + 3], ro.arr("x")[:3 * nf + 3]) < 1e-6
    assert seen == {0, 1, 2, 3, 4, 5, 6}, seen


def test_recovers_truth_on_device(be):
    p = initial.make_problem()
    r = initial.align_batch(be, [p])[0]
    assert r.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, p.c.n_window)
    assert ep < 3.4e-4 and ev < 3.2e-4 and es < 3.8e-4, (ep, ev, es)


@pytest.mark.parametrize("S", [1, 64, 1024])
def test_batch_bitwise(be, S):
    ps = _problems()
    single = [initial.align_batch(be, [p])[0] for p in ps]
    batch = [ps[(7 * i + 3) % len(ps)] for i in range(S)]
    rs = initial.align_batch(be, batch)
    for i, r in enumerate(rs):
        ref = single[(7 * i + 3) % len(ps)]
        assert bytes(r) == bytes(ref), i


def test_buffers_kept_and_timed(be):
    # the device block is kept on the handle between calls: a smaller batch after a larger one reuses it and gives the same bits
    ps = _problems()
    big = initial.align_batch(be, ps * 8)
    call_ms, kernel_ms = initial.last_ms(be)
    assert 0 < kernel_ms <= call_ms
    small = initial.align_batch(be, ps[:3])
    assert all(bytes(a) == bytes(b) for a, b in zip(small, big[:3]))


def test_empty_and_null(be):
    assert initial.align_batch(be, []) == []
    initial._bind(be.lib)
    assert be.lib.isv_internal_visual_imu_align_batch(be.h, 1, None, None) == -1
