"""The solve's input kernels of TODAY -- k_triangulate, k_imu_prep, k_vector2double (is-vins_amd/csrc/isv_linearize.hip, isv_device_math.h)
-- against the 40-digit statements of tests/prep_highprec.py, live on the MI355X, through the C ABI (Backend.triangulate,
Backend.linearize, Backend.debug_read).  Cases, rules and margins: tests/prep_cases.py; the CPU oracle's side of the same comparison and
the checks of the table itself: tests/test_prep_highprec.py.

Triangulation, per rung: the decision rule (init_depth exactly iff the 40-digit depth is outside [0.1, 8]; positive depths come back with
their bits), and max e_gpu <= TRI_MARGIN * max e_ref, e = |d / d* - 1|, e_ref from the oracle and numpy.linalg.svd.
IMU weights, per covariance: an upper-triangular factor with exact zeros and a positive diagonal; U^T U and U against the 40-digit
cov^-1 and its Cholesky factor within IMU_MARGIN_* x the two float64 routes; and the bits of the oracle, as before.
vector2double, per window: the pose block's quaternion against quat_mp, component by component and signs included, within QUAT_ATOL (9
rounding units, derived at prep_highprec.QUAT_ATOL); the projection strips against the oracle at tests/test_gpu_linearize.py's tolerance.
The turned windows keep gravity where it was, so their IMU residuals are large: a linearisation is taken at whatever state it is given.

Measured on one MI355X (documentation; the margins come from the CPU routes alone).  The Gram kernel is the one this file replaced:

  rung                    sigma1/sigma3  e_ref (CPU)   Gram kernel (x e_ref)   QR kernel (x e_ref)
  ladder_s1_exact           1.1e+02     2.8e-14       4.3e-14 (   1.5)       2.4e-14 (0.88)
  ladder_s1_noisy           9.8e+01     3.6e-14       5.0e-14 (   1.4)       1.4e-14 (0.38)
  ladder_s0.1_exact         6.1e+02     1.5e-13       1.9e-11 ( 133.3)       1.5e-13 (1.05)
  ladder_s0.1_noisy         3.0e+02     5.6e-14       2.1e-12 (  37.7)       7.0e-14 (1.24)
  ladder_s0.01_exact        7.4e+03     1.1e-12       7.1e-10 ( 648.3)       2.6e-13 (0.24)
  ladder_s0.01_noisy        1.3e+03     2.6e-13       1.1e-11 (  44.1)       2.4e-13 (0.93)
  ladder_s0.001_exact       3.1e+03     7.2e-13       1.5e-10 ( 203.8)       5.9e-13 (0.82)
  ladder_s0.001_noisy       1.2e+03     1.4e-13       7.7e-11 ( 564.6)       9.1e-14 (0.66)
  ladder_s0.0002_exact      3.1e+03     6.9e-13       2.2e-10 ( 310.4)       2.8e-13 (0.41)
  ladder_s0.0002_noisy      1.4e+03     8.2e-13       7.9e-11 (  96.5)       5.9e-13 (0.72)
  tracks                    5.4e+01     1.4e-14       7.9e-14 (   5.5)       7.5e-15 (0.52)
  clamp                     9.3e+01     3.9e-14       2.3e-13 (   9.8)*      3.3e-14 (0.84)
  entry                     4.0e+01     2.0e-14       3.5e-14 (   1.8)       1.2e-14 (0.59)
  norm_plain                4.5e+01     4.1e-14       3.4e-14 (   0.8)       9.8e-15 (0.24)
  norm_x2p5                 4.5e+01     3.3e-14       6.4e-14 (   1.9)       9.6e-15 (0.29)
  norm_unit                 4.5e+01     4.5e-14       3.5e-14 (   0.8)       6.8e-15 (0.15)
  norm_varied               4.5e+01     3.3e-14       3.6e-14 (   1.1)       9.4e-15 (0.29)
  batch                     1.6e+02     2.1e-14       5.1e-13 (  24.6)       1.6e-14 (0.75)
  n18                       3.4e+02     7.2e-14       6.5e-13 (   9.0)       9.8e-14 (1.35)
  degenerate                3.1e+02     3.0e-13       1.5e-12 (   4.9)       7.7e-14 (0.26)
  * the Gram kernel's clamp row was taken before the rung gained its 4e-9 cases (e_ref 2.3e-14 then)

IMU weights: U^T U 1.8e-16 .. 3.4e-16, U's rows 3.6e-16 .. 3.6e-14, at most 1.83 x / 1.28 x the worse float64 route.  Quaternions: 0.50 ..
1.05 rounding units.  Single faults that fail this file (each built and run once): window 0's ric / tic for every window (batch); the f
normalisation dropped (all noisy rungs but the unit-vector one); dep > 8.0 turned into >= 8.0 - 1e-7 (clamp, the 4e-9 cases); the Gram
route (nine rungs); >= turned into > in q_from_R's x arm (tie_xy); k_imu_prep's last Cholesky column times 1 + 1e-9 (all six)."""
import ctypes as C

import numpy as np
import pytest

import prep_cases as pc
import prep_highprec as ph
from isvins_amd import abi, backend

pytestmark = pytest.mark.gpu
dp = C.POINTER(C.c_double)
TOL = 1e-9                   # tests/test_gpu_linearize.py's, on the projection strips


def P(a):
    return a.ctypes.data_as(dp)


def make_backend(shape=(11, 5), **kw):
    backend.build()
    return backend.Backend(*shape, max_landmarks=130, max_obs=130 * shape[0], max_batch=4, **kw)


@pytest.fixture(scope="module")
def be():
    b = make_backend()
    yield b
    b.close()


@pytest.fixture(scope="module")
def be18():
    b = make_backend((18, 8))
    yield b
    b.close()


def triangulated(b, windows):
    ws = [w.clone() for w in windows]
    b.triangulate(ws)
    return [np.array(w.lm_depth[: w.L]) for w in ws]


# ---- k_triangulate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.rungs()))
def test_gpu_triangulate_against_40_digits(oracle, be, be18, name):
    rung = pc.rungs()[name]
    b = be18 if rung.shape == (18, 8) else be
    got = triangulated(b, rung.windows)
    bad, e, e_ref, cond = pc.judge(oracle, name, got)
    assert not bad, bad
    assert e <= pc.TRI_MARGIN * e_ref, (name, cond, e, e_ref, e / e_ref)
    if len(rung.windows) > 1:
        # every window alone: the same bits as inside the batch (per-window ric / tic, the search over lm_off, and -- degenerate rung --
        # lanes beside an undetermined landmark)
        for i, w in enumerate(rung.windows):
            assert triangulated(b, [w])[0].tobytes() == got[i].tobytes(), (name, i)


# ---- k_imu_prep -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def imu_sqrt(be):
    w, idx = pc.imu_window()
    be.linearize(w)
    return be.debug_read(2, (w.N - 1) * 225).reshape(w.N - 1, 15, 15)


@pytest.mark.parametrize("name", list(pc.IMU_CASES))
def test_gpu_imu_weight_against_40_digits(oracle, imu_sqrt, name):
    w, idx = pc.imu_window()
    U = imu_sqrt[idx[name]]
    faults, ei, ef, yi, yf = pc.judge_imu(name, U)
    assert not faults, faults
    assert ei <= pc.IMU_MARGIN_INFO * yi, (name, ei, yi)
    assert ef <= pc.IMU_MARGIN_FACTOR * yf, (name, ef, yf)
    so = np.zeros(225); r = np.zeros(15)
    G = np.array([0, 0, 9.81007]); p7 = np.array([0, 0, 0, 0, 0, 0, 1.0]); z9 = np.zeros(9)
    oracle.isvo_x_imu(C.byref(w.imu[idx[name]]), P(G), P(p7), P(z9), P(p7), P(z9), 1, P(r), None, None, None, None, P(so))
    assert np.array_equal(U.ravel(), so), f"imu sqrt_info {name} not bitwise the oracle's (max diff {np.abs(U.ravel() - so).max()})"


# ---- k_vector2double ------------------------------------------------------------------------------------------------------------------------
def check_quaternions(tag, pose, mats):
    worst = 0.0
    for i, R in enumerate(mats):
        q = ph.quat_mp(R)
        d = max(abs(float(ph.mp.mpf(float(pose[i, 3 + c])) - q[c])) for c in range(4))
        worst = max(worst, d)
        assert d <= ph.QUAT_ATOL, (tag, i, ph.quat_arm(R), pose[i, 3:], [float(c) for c in q], d / 2.0 ** -53)
    print(f"QUAT {tag:10s} arms {sorted({ph.quat_arm(R)[0] for R in mats})} worst {worst / 2.0 ** -53:.2f} u (bound {ph.QUAT_ATOL / 2.0 ** -53:.0f} u)")


def check_strips(oracle, cfg, w, ps, cols=28):
    ps_o = np.zeros((w.n_factors, 28)); im_o = np.zeros((w.N - 1, 465)); c_o = np.zeros(1)
    assert oracle.isvo_linearize(C.byref(cfg), C.byref(w.c()), P(ps_o), P(im_o), None, P(c_o)) == 0
    sc = np.maximum(1.0, np.abs(ps_o).max(axis=1, keepdims=True))
    assert (np.abs(ps - ps_o)[:, :cols] / sc).max() < TOL, (np.abs(ps - ps_o)[:, :cols] / sc).max()


@pytest.mark.parametrize("name", list(pc.QUAT_CASES))
def test_gpu_vector2double_in_every_arm(oracle, be, name):
    w = pc.quat_window(name)
    ps, im, cost = be.linearize(w)
    pose = be.debug_read(5, w.N * 7).reshape(w.N, 7)
    assert np.array_equal(pose[:, :3], w.Ps)
    check_quaternions(name, pose, list(w.Rs))
    lam = be.debug_read(6, w.L)
    assert np.array_equal(lam, 1.0 / np.array(w.lm_depth[: w.L]))                  # para_Feature = 1 / estimated_depth
    check_strips(oracle, be.cfg, w, ps)


def test_gpu_vector2double_extrinsic_in_the_x_arm(oracle, be):
    """The extrinsic's quaternion is not readable on a handle with a fixed extrinsic; with estimate_extrinsic = 1 the extrinsic is the
    pose block after the last frame's and is read like any other.  On both handles it enters every projection strip: the fixed
    handle's strips are compared whole; the free handle's without the landmark column, which the oracle's strip does not carry then
    (its third Jacobian block is the extrinsic's; tests/test_gpu_extrinsic.py compares that block)."""
    w = pc.quat_window("ric_x_arm")
    ps, im, cost = be.linearize(w)
    check_strips(oracle, be.cfg, w, ps)
    b = make_backend(estimate_extrinsic=1)
    try:
        ps, im, cost = b.linearize(w)
        pose = b.debug_read(5, (w.N + 1) * 7).reshape(w.N + 1, 7)
        assert np.array_equal(pose[w.N, :3], w.tic)
        check_quaternions("ric_x_arm", pose, list(w.Rs) + [w.ric])
        check_strips(oracle, b.cfg, w, ps, cols=26)
    finally:
        b.close()
