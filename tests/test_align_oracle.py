"""CPU checks of the visual-inertial alignment restatement (tests/native/isv_init_oracle.c, is-vins_amd/csrc/isv_initial.h) on
synthetic all_image_frames with exact SfM poses at scale 0.37 (isvins_amd.initial.make_problem).

Measured with the restatement before the bounds were set (noise-free IMU, 11 frames 0.1 s apart, 10 samples per frame,
a 1 m circle at 1 m/s): position / velocity errors 3.4e-5 / 3.2e-5 after the 4-DoF alignment, relative scale error 3.8e-5,
|g - (0, 0, G)| ~ 1e-16 (gravity is exact by construction of g2R), rotation error 3e-16.  At 20 frames 0.05 s apart the
errors fall to 6e-6 (midpoint-rule discretisation).  Bounds below are 10x the measured errors."""
import numpy as np
import pytest

import align_oracle
from isvins_amd import initial, synth


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


def test_recovers_truth(lib):
    p = initial.make_problem()
    r = align_oracle.solve(lib, p)
    assert r.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, p.c.n_window)
    assert ep < 3.4e-4 and ev < 3.2e-4 and es < 3.8e-4 and er < 1e-12 and eg < 1e-12, (ep, ev, es, er, eg)
    assert abs(np.linalg.norm(list(r.g_linear)) - synth.G_NORM) < 1e-2


def test_recovers_truth_finer_sampling(lib):
    p = initial.make_problem(n_frames=20, cam_dt=0.05)
    r = align_oracle.solve(lib, p)
    assert r.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, p.c.n_window)
    assert ep < 6e-5 and ev < 6e-5 and es < 7e-5, (ep, ev, es)


def test_noisy_imu_lands_near_truth(lib):
    # measured: 2.2e-3 m / 2.6e-3 m/s / 2.4e-3 relative scale at 0.01 m/s^2 / 0.001 rad/s white noise per sample
    p = initial.make_problem(acc_noise=0.01, gyr_noise=0.001, seed=3)
    r = align_oracle.solve(lib, p)
    assert r.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, p.c.n_window)
    assert ep < 3e-2 and ev < 3e-2 and es < 3e-2, (ep, ev, es)


def test_repropagation_matches_preintegration(lib):
    # repropagate(0, Bgs[0] + delta_bg) of every frame == the numpy producer-side pre-integration with that bias
    p = initial.make_problem(bg=(0.01, -0.02, 0.005), Bgs0=np.full((11, 3), 0.003))
    r = align_oracle.solve(lib, p)
    bg0 = np.array(r.Bgs[0])
    assert np.allclose(bg0, 0.003 + np.array(r.delta_bg), rtol=0, atol=0)
    for j in range(1, p.c.n_frames):
        f = p.frames[j]
        rows = p.imu[f.imu_begin:f.imu_begin + f.imu_count]
        acc = np.vstack([list(f.linearized_acc), rows[:, 1:4]])[None]
        gyr = np.vstack([list(f.linearized_gyr), rows[:, 4:7]])[None]
        pre = synth.preintegrate(rows[0, 0], acc, gyr, np.zeros((1, 3)), bg0[None])
        assert np.abs(np.array(r.rp_delta_p[j]) - pre["delta_p"][0]).max() < 1e-13
        assert np.abs(np.array(r.rp_delta_v[j]) - pre["delta_v"][0]).max() < 1e-13
        q = pre["delta_q"][0]
        assert np.abs(np.array(r.rp_delta_q[j]) - [q[1], q[2], q[3], q[0]]).max() < 1e-13
        assert abs(r.rp_sum_dt[j] - pre["sum_dt"]) < 1e-15


def test_gyro_bias_quirk(lib):
    # quirk Q1: the bias Jacobian is jacobian.block<3,3>(3,3) (~ I), so the increment is the mean rotation error per frame
    # (about -bg * cam_dt here), not bg
    bg = np.array([0.01, -0.02, 0.005])
    r = align_oracle.solve(lib, initial.make_problem(bg=tuple(bg)))
    assert r.status == 0
    assert np.allclose(np.array(r.delta_bg), -0.1 * bg, rtol=0.2, atol=0)


def test_velocity_index_quirk(lib):
    # quirk Q3: with frames of all_image_frame outside the window (MARGIN_NEW), Vs[kv] takes x.segment<3>(3 kv), the
    # velocity of all_image_frame entry kv, rotated by keyframe kv's R
    wf = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 15]
    p = initial.make_problem(n_frames=16, window_frame=wf)
    r = align_oracle.solve(lib, p)
    assert r.status == 0
    R0 = np.array(r.R0).reshape(3, 3)
    x = np.array(r.x)
    for kv, f in enumerate(wf):
        R = np.array(p.frames[f].R).reshape(3, 3)
        assert np.allclose(np.array(r.Vs[kv]), R0 @ R @ x[3 * kv:3 * kv + 3], rtol=0, atol=1e-12)
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, len(wf))
    assert ep < 3.4e-4 and es < 3.8e-4      # positions and scale are unaffected
    assert ev > 1e-2                         # the velocities of the later keyframes are those of earlier frames


def test_hover_has_no_scale(lib):
    # a body at rest: the SfM translations vanish, the scale column of A is zero, LDLT's pseudo-inverse of D gives s = 0 -- not
    # refused by LinearAlignment (s < 0 is), exactly as the reference would
    r = align_oracle.solve(lib, initial.make_problem(hover=True))
    assert r.status == 0 and r.s == 0.0


def test_wrong_gravity_refused(lib):
    # |g| off by more than 1 m/s^2 (the IMU is scaled by 1.2): LinearAlignment refuses
    p = initial.make_problem()
    p.imu[:, 1:4] *= 1.2
    for f in p.frames:
        f.linearized_acc[:] = [1.2 * a for a in f.linearized_acc]
    r = align_oracle.solve(lib, p)
    assert r.status == 1, initial.STAGES[r.status]


def test_negative_scale_refused(lib):
    # SfM translations with the wrong sign: LinearAlignment's scale comes out negative
    p = initial.make_problem(sfm_scale=-0.37)
    r = align_oracle.solve(lib, p)
    assert r.status == 2 and r.s_linear < 0, initial.STAGES[r.status]


def test_refined_scale_refused(lib):
    # a slow (2 cm/s), noisy start: LinearAlignment accepts s = 5.88, RefineGravity's |g| = |G| constraint drives it to -2.64
    # (found by a search over seeds; both values are far from 0, so the sign does not hinge on rounding)
    p = initial.make_problem(seed=14, speed=0.02, acc_noise=0.05, gyr_noise=0.002)
    r = align_oracle.solve(lib, p)
    assert r.status == 3, initial.STAGES[r.status]
    assert r.s_linear > 1.0 and r.x[3 * p.c.n_frames + 2] < -1.0


def test_discrete_truth_exact(lib):
    # SfM poses that follow the pre-integration exactly: the alignment equations hold to rounding, so the state comes back to
    # rounding (measured 1.2e-11 m, 1.5e-11 m/s, 1.4e-11 relative scale)
    p = initial.make_problem(discrete=True)
    r = align_oracle.solve(lib, p)
    assert r.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(r, p.truth, p.c.n_window)
    assert ep < 1e-9 and ev < 1e-9 and es < 1e-9 and er < 1e-12, (ep, ev, es, er)
    assert np.abs(np.array(r.delta_bg)).max() < 1e-12


def test_antiparallel_refused(lib):
    # the SfM frame upside down (R_w_c0 = diag(1, -1, -1)) with exact data: g in that frame points along -z to rounding, the case
    # where Eigen's FromTwoVectors takes its SVD branch, which is not restated
    p = initial.make_problem(discrete=True, R_w_c0=np.diag([1.0, -1.0, -1.0]))
    r = align_oracle.solve(lib, p)
    assert r.status == 6, initial.STAGES[r.status]
    g = np.array(r.g_c0)
    assert g[2] / np.linalg.norm(g) < -1.0 + 1e-12


def test_capacity_and_input_refused(lib):
    r = align_oracle.solve(lib, initial.make_problem(n_frames=initial.ISV_ALIGN_MAX_FRAMES + 1, window_frame=list(range(11))))
    assert r.status == 4
    p = initial.make_problem()
    p.c.window_frame[3] = p.c.window_frame[2]
    assert align_oracle.solve(lib, p).status == 5
    p = initial.make_problem()
    p.frames[5].imu_count = 10 ** 6
    assert align_oracle.solve(lib, p).status == 5
