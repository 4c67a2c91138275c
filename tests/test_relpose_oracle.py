"""CPU checks of the relative-pose stage's restatement (tests/native/isv_relpose_oracle.c, the checker of k_relpose in
is-vins_amd/csrc/isv_relpose.h): the serial pieces (solveCubic, run7Point, RANSACUpdateNumIters), ground truth on exact,
noisy and outlier scenes, every refusal, the quirks R1 / R2 / R4 / R5, the chain into the SfM and alignment restatements, and
the ctypes layouts.  Bounds are set from measured errors (noted beside each)."""
import ctypes as C
import math

import numpy as np
import pytest

import align_oracle
import relpose_oracle
import sfm_oracle
from isvins_amd import initial

NOISE = 0.5 / 460


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return relpose_oracle.build(tmp_path_factory.mktemp("relpose_oracle"))


def test_struct_sizes(lib):
    assert [lib.isvo_relpose_sizeof(i) for i in range(2)] == [C.sizeof(initial.isv_sfm_problem_t), C.sizeof(initial.isv_relpose_result_t)]


@pytest.mark.parametrize("c", [[2.0, -3.0, -11.0, 6.0],       # three real roots: 3, -2, 0.5
                               [1.0, 0.5, 2.0, -1.3],         # one real root
                               [0.0, 2.0, -3.0, -5.0],        # leading 0: the quadratic
                               [0.0, 0.0, 4.0, -2.0]])        # and the linear one
def test_solve_cubic(lib, c):
    n, r = relpose_oracle.solve_cubic(lib, c)
    want = np.sort(np.real([x for x in np.roots(c) if abs(np.imag(x)) < 1e-9]))
    assert n == len(want)
    assert np.allclose(np.sort(r[:n]), want, rtol=1e-12, atol=1e-12), (r[:n], want)


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def test_run7point_exact(lib):
    rng = np.random.default_rng(3)
    R = initial._rotvec(np.array([0.1, -0.2, 0.05]))
    t = np.array([0.8, 0.1, 0.3])
    X = np.c_[rng.uniform(-1, 1, (7, 2)), rng.uniform(4, 8, 7)]
    x0 = X[:, :2] / X[:, 2:]
    Xc = X @ R.T + t
    x1 = Xc[:, :2] / Xc[:, 2:]
    n, Fs = relpose_oracle.run7point(lib, np.c_[x0, x1])
    assert 1 <= n <= 3
    Ft = _skew(t) @ R   # x1^T F x0 = 0
    Ft = Ft / Ft[2, 2]
    h0, h1 = np.c_[x0, np.ones(7)], np.c_[x1, np.ones(7)]
    for F in Fs:
        assert np.abs(np.einsum("ij,jk,ik->i", h1, F, h0)).max() < 1e-12
        assert abs(np.linalg.det(F)) < 1e-10 * np.abs(F).max() ** 3
    assert min(np.abs(F - Ft).max() for F in Fs) < 1e-8


@pytest.mark.parametrize("ep,it", [(0.0, 1000), (0.3, 1000), (0.3, 40), (0.6, 1000), (0.95, 1000), (1.0, 500)])
def test_update_num_iters(lib, ep, it):
    denom = 1 - (1 - ep) ** 7
    if denom < 2.2250738585072014e-308:
        want = 0
    else:
        num, den = math.log(0.01), math.log(denom)
        want = it if den >= 0 or -num >= it * -den else int(round(num / den))   # (Python's round is half-even, as cvRound)
    assert lib.isvo_rp_update_num_iters(0.99, ep, 7, it) == want


def _rel_errors(r, kw):
    """relative_R against the truth, and the angle between relative_T and the true direction, for the l the stage found"""
    st, _ = initial.make_relpose_scene(**dict(kw, l=r.l))
    R = np.array(r.relative_R).reshape(3, 3)
    T = np.array(r.relative_T)
    Tt = st.truth["T"][-1]
    eR = np.linalg.norm(R - st.truth["Q"][-1])
    eT = math.acos(min(1.0, T @ Tt / np.linalg.norm(T) / np.linalg.norm(Tt)))
    return eR, eT, np.linalg.norm(T)


def _first_qualifying(r):
    """the candidates before l all failed a test, and l passed every one"""
    for i in range(r.l):
        assert r.n_corres[i] <= 20 or r.parallax[i] * 460 <= 30 or r.recover_inliers[i] <= 12, i
    assert r.n_corres[r.l] > 20 and r.parallax[r.l] * 460 > 30 and r.recover_inliers[r.l] > 12
    assert r.n_candidates == r.l + 1 and all(x == -1 for x in r.n_corres[r.l + 1:])


# exact data: measured (seeds 0-3) rotation 1.1e-6 (Frobenius), direction 1e-5 rad: the float32 rounding of the points (R1)
# sets the floor.  0.5 px: measured rotation 3.9e-2 and direction 9.2e-2 rad (seed 0), 2.4e-2 / 1.5e-2 (seed 1): the
# reference's 0.3 px threshold keeps only about half the points and no refit follows the 7-point model.
@pytest.mark.parametrize("kw,bR,bT", [(dict(seed=0), 1e-5, 1e-4), (dict(seed=1), 1e-5, 1e-4), (dict(seed=2), 1e-5, 1e-4),
                                      (dict(seed=3), 1e-5, 1e-4), (dict(seed=0, pixel_noise=NOISE), 0.1, 0.2),
                                      (dict(seed=1, pixel_noise=NOISE), 0.1, 0.2)])
def test_scene_recovers_truth(lib, kw, bR, bT):
    sp, _ = initial.make_relpose_scene(**kw)
    r, m = relpose_oracle.solve(lib, sp)
    assert r.status == 0 and r.l >= 0
    _first_qualifying(r)
    eR, eT, nT = _rel_errors(r, kw)
    assert eR < bR and eT < bT and abs(nT - 1) < 1e-12, (eR, eT)
    assert (m == 1).sum() == r.recover_inliers[r.l] and ((m == 0) | (m == 1)).sum() == r.n_corres[r.l]


def test_outliers_rejected(lib):
    # 30 % of the last-frame observations mismatched: measured rotation 6.7e-7, direction 2.8e-6 rad, 280 iterations
    kw = dict(seed=0, outliers=0.3)
    sp, _ = initial.make_relpose_scene(**kw)
    r, m = relpose_oracle.solve(lib, sp)
    assert r.status == 0 and len(sp.truth["outliers"]) > 0
    _first_qualifying(r)
    eR, eT, _ = _rel_errors(r, kw)
    assert eR < 1e-5 and eT < 1e-4, (eR, eT)
    assert not (m[sp.truth["outliers"]] == 1).any()
    assert 64 < r.ransac_iters[r.l] < 1000            # past one speculative chunk of the kernel


def test_ransac_runs_to_the_cap(lib):
    # outliers and 0.5 px noise: no model reaches the inlier share that would cut 1000 iterations short; the first two
    # RANSAC candidates fail recoverPose (<= 12), so l moves on
    sp, _ = initial.make_relpose_scene(seed=5, outliers=0.3, pixel_noise=NOISE)
    r, _ = relpose_oracle.solve(lib, sp)
    assert r.status == 0
    _first_qualifying(r)
    assert r.ransac_iters[r.l] == 1000
    assert sum(1 for i in range(r.l) if r.ransac_iters[i] > 0) >= 1


def test_failed_ransac_candidate_moves_l_on(lib):
    # seed 1 at 0.5 px: candidate 3 has 21 correspondences and 274 px of parallax, but recoverPose keeps 12 points only
    sp, _ = initial.make_relpose_scene(seed=1, pixel_noise=NOISE)
    r, _ = relpose_oracle.solve(lib, sp)
    assert r.status == 0 and r.l == 4
    assert r.n_corres[3] > 20 and r.parallax[3] * 460 > 30 and r.ransac_iters[3] > 0 and r.recover_inliers[3] <= 12


def low_parallax_scene():
    """every observation pulled 95 % of the way to its track's first one: the image barely moves, the IMU still does"""
    sp, _ = initial.make_relpose_scene(seed=0)
    for j in range(sp.c.n_tracks):
        T = sp.tracks[j]
        a, b = T.obs_off, T.obs_off + T.n_obs
        sp.obs[a:b] = sp.obs[a] + 0.05 * (sp.obs[a:b] - sp.obs[a])
    return sp


def refusal_cases():
    """(name, problem, expected status); shared with the GPU test"""
    out = []
    sp, _ = initial.make_relpose_scene(seed=8, hover=True)
    out.append(("excitation", sp, 1))
    sp, _ = initial.make_relpose_scene(seed=0, per_frame=12)
    out.append(("few_correspondences", sp, 2))
    out.append(("low_parallax", low_parallax_scene(), 2))
    sp, _ = initial.make_relpose_scene(seed=0, depth=(60.0, 120.0))
    out.append(("recover_pose_inliers", sp, 2))
    sp, _ = initial.make_relpose_scene(seed=0)
    sp.c.n_tracks = initial.ISV_SFM_MAX_TRACKS + 1
    out.append(("capacity", sp, 3))
    sp, _ = initial.make_relpose_scene(seed=0)
    sp.pt_id[sp.pt_off[3]] = sp.pt_id[sp.pt_off[3] + 1]
    out.append(("input_csr", sp, 4))
    sp, _ = initial.make_relpose_scene(seed=0)
    sp.c.window_frame[4] = sp.c.window_frame[3]
    out.append(("input_window", sp, 4))
    return out


@pytest.mark.parametrize("case", range(7))
def test_refusals(lib, case):
    name, sp, want = refusal_cases()[case]
    r, _ = relpose_oracle.solve(lib, sp)
    assert r.status == want, (name, r.status)
    assert r.l == -1
    ev = range(r.n_candidates)
    if name == "excitation":
        assert r.excitation_var < 0.25 and r.n_candidates == 0
    if name == "few_correspondences":
        assert r.excitation_var >= 0.25 and r.n_candidates == sp.c.n_window - 2 and all(r.n_corres[i] <= 20 for i in ev)
        assert all(x == -1 for x in r.ransac_iters)
    if name == "low_parallax":
        assert r.excitation_var >= 0.25 and any(r.n_corres[i] > 20 for i in ev)
        assert all(r.parallax[i] * 460 <= 30 for i in ev if r.n_corres[i] > 20) and all(x == -1 for x in r.ransac_iters)
    if name == "recover_pose_inliers":   # the points lie beyond recoverPose's dist = 50 baselines
        ran = [i for i in ev if r.ransac_iters[i] > 0]
        assert ran and all(0 <= r.recover_inliers[i] <= 12 for i in ran)


def test_r1_float_points_matter(lib):
    sp, _ = initial.make_relpose_scene(seed=0, pixel_noise=NOISE)
    r, _ = relpose_oracle.solve(lib, sp)
    r1, _ = relpose_oracle.solve(lib, sp, quirks_off=1)
    assert r.status == r1.status == 0 and r.parallax[r.l] == r1.parallax[r1.l]   # the parallax test reads the doubles
    assert bytes(r.relative_R) != bytes(r1.relative_R)


def test_r2_float_error_matters(lib):
    # F of a pure x translation: the error of (x0, y0, x1, y1) is (y0 - y1)^2.  Just above thresh^2 in double, it rounds to
    # (float)(thresh^2) in float32
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], dtype=np.float64)
    t2 = (0.3 / 460) ** 2
    q = np.array([0.1, 0.0, 0.2, -math.sqrt(t2 * (1 + 1e-9))])
    dp = C.POINTER(C.c_double)
    assert (q[3] - q[1]) ** 2 > t2
    assert lib.isvo_rp_is_inlier(F.ctypes.data_as(dp), q.ctypes.data_as(dp)) == 1
    assert relpose_oracle.with_quirks_off(lib, 2, lib.isvo_rp_is_inlier, F.ctypes.data_as(dp), q.ctypes.data_as(dp)) == 0


def test_r4_fresh_rng_per_candidate(lib):
    # candidate 3 runs a RANSAC before l = 4: with one RNG continued across candidates, candidate 4 draws other subsets
    sp, _ = initial.make_relpose_scene(seed=1, pixel_noise=NOISE)
    r, _ = relpose_oracle.solve(lib, sp)
    r4, _ = relpose_oracle.solve(lib, sp, quirks_off=4)
    assert r.ransac_iters[3] == r4.ransac_iters[3] and r.ransac_iters[3] > 0
    assert (r.ransac_iters[4], bytes(r.relative_R)) != (r4.ransac_iters[4], bytes(r4.relative_R))


def r5_scene():
    return initial.make_relpose_scene(seed=1, n_window=4, extra=6, per_frame=40)[0]


def test_r5_last_but_one_never_tried(lib):
    sp = r5_scene()
    r, _ = relpose_oracle.solve(lib, sp)
    assert r.status == 2 and r.n_candidates == sp.c.n_window - 2
    r5, _ = relpose_oracle.solve(lib, sp, quirks_off=8)
    assert r5.status == 0 and r5.l == sp.c.n_window - 2


@pytest.fixture(scope="module")
def slib(tmp_path_factory):
    return sfm_oracle.build(tmp_path_factory.mktemp("sfm_oracle"))


@pytest.fixture(scope="module")
def alib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


@pytest.mark.parametrize("seed", [0, 3])
def test_chain_from_tracks(lib, slib, alib, seed):
    # relpose -> SfM -> alignment, all restatements, on an exact 18-frame scene: §12's bounds of the chain with the true
    # relative pose (measured here, seeds 0 and 3: P 2.9e-5 m, R 4.0e-8, V 2.0e-5 m/s, scale 2.5e-5 relative)
    sp, _ = initial.make_relpose_scene(seed=seed)
    r, _ = relpose_oracle.solve(lib, sp)
    assert r.status == 0
    initial.apply_relpose(r, sp)
    _, ap = initial.make_relpose_scene(seed=seed, l=r.l)   # the alignment's truth scale is the baseline of l
    rs, _, _ = sfm_oracle.solve(slib, sp)
    assert rs.status == 0
    initial.copy_sfm_to_align(rs, ap)
    ra = align_oracle.solve(alib, ap)
    assert ra.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(ra, ap.truth, ap.c.n_window)
    assert ep < 1e-4 and ev < 1e-4 and es < 1e-4 and er < 1e-7, (ep, er, ev, es)
