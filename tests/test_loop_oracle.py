"""The CPU restatement of the loop-closure verification (tests/native/isv_loop_oracle.c; contract: include/isvins_loop.h) on its
own: its matching against a numpy brute force, its EPnP and DLT + LM routines and the whole pair against the scene's truth, every
status, the quirk hooks L1 / L3 / L5 / L6, and the knife-edge check of the GPU case list (tests/loop_cases.py).

Accuracy of the restatement against the truth on EXACT data (float32 inputs, the committed seeds of tests/loop_cases.py and
seeds 40..59 here; 16 to 150 inliers), measured: worst rotation error 1.40e-8 rad, worst translation error 6.33e-8 m -- float32
rounding of the points, 6e-8 relative, at a few metres.  Asserted: 10 x the figures rounded up to a power of ten, 1e-6 rad and
1e-6 m.  The ceilings that must hold regardless (1e-4 rad, 1e-3 m with at least 30 well-spread inliers) hold with room."""
import ctypes as C

import numpy as np
import pytest

import loop_cases
import loop_oracle
from isvins_amd import loop

ROT_TOL, TRANS_TOL = 1e-6, 1e-6


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return loop_oracle.build(tmp_path_factory.mktemp("loop_oracle"))


@pytest.fixture(scope="module")
def lib_o0(tmp_path_factory):
    return loop_oracle.build(tmp_path_factory.mktemp("loop_oracle_o0"), "-O0")


CFG = loop_cases.config()


def rot_err(R, Rt):
    return np.linalg.norm(R - Rt) / np.sqrt(2.0)            # the angle, to first order


def pose_err(r, tr):
    return rot_err(r.arr("PnP_R_old").reshape(3, 3), tr["R_old"]), np.linalg.norm(r.arr("PnP_T_old") - tr["T_old"])


# ---------------------------------------------------------------- matching
def test_match_against_brute_force(lib):
    for name, pair, _ in loop_cases.all_pairs():
        if pair.c.n_points < 0 or pair.c.n_keypoints < 0 or not pair.c.window_brief:
            continue
        mi, md, src = loop_oracle.match(lib, CFG, pair)
        bi, bd, ba = loop_cases.brute_force(pair)
        assert np.array_equal(mi, bi) and np.array_equal(md, bd), name
        assert np.array_equal(src, np.nonzero(ba)[0]), name


def test_match_edges(lib):
    for name, pair, exp in loop_cases.match_cases():
        mi, md, src = loop_oracle.match(lib, CFG, pair)
        assert (mi[0], md[0], len(src) == 1) == exp, name
    for name in ("p0", "k0", "k1"):
        pair = [p for n, p, _ in loop_cases.all_pairs() if n == name][0]
        mi, md, src = loop_oracle.match(lib, CFG, pair)
        assert len(mi) == pair.c.n_points
        if name == "k0":
            assert (mi == -1).all() and (md == 128).all() and len(src) == 0
        if name == "k1":
            assert mi[0] == 0 and md[0] == 20 and set(mi[1:]) <= {-1, 0} and list(src) == [0]


# ---------------------------------------------------------------- the solvers alone
def _points(seed, n):
    rng = np.random.Generator(np.random.PCG64(0xE9_0000 + seed))
    R = loop.synth._rot_zyx(0.4 - 0.1 * seed, 0.2, -0.3)
    t = np.array([0.3, -0.2, 0.5])
    z = rng.uniform(2, 8, n)
    pc = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.45, 0.45, n) * z, z], 1)
    X = (pc - t) @ R                                        # pc = R X + t
    return X, pc[:, :2] / pc[:, 2:3], R, t


@pytest.mark.parametrize("n", [5, 6, 16, 60])
def test_epnp_alone(lib, n):
    """exact non-planar points in doubles.  Measured over the 16 cases: rotation 8.4e-15 rad, translation 1.8e-14 m and
    reprojection 7.2e-15 at worst (five points included: M^T M's two-dimensional null space does not keep the Gauss-Newton
    refinement of the betas from the pose); asserted 10 x that, rounded up to a power of ten."""
    for seed in range(4):
        X, uv, R, t = _points(seed, n)
        Re, te = loop_oracle.epnp(lib, X, uv)
        assert abs(np.linalg.det(Re) - 1) < 1e-9 and np.abs(Re @ Re.T - np.eye(3)).max() < 1e-9
        pc = X @ Re.T + te
        reproj = np.abs(pc[:, :2] / pc[:, 2:3] - uv).max()
        print(f"epnp n={n} seed={seed}: reprojection {reproj:.2e} rotation {rot_err(Re, R):.2e} translation {np.linalg.norm(te - t):.2e}")
        assert (pc[:, 2] > 0).all() and reproj < 1e-13, (n, seed)
        assert rot_err(Re, R) < 1e-13 and np.linalg.norm(te - t) < 1e-12, (n, seed)


@pytest.mark.parametrize("n", [6, 16, 60])
def test_iterative_alone(lib, n):
    """the DLT + CvLevMarq on exact non-planar points in doubles.  Five points are left out: they give the DLT ten equations
    for twelve unknowns, so its initialisation is not determined, and behind findConnection's gates it sees at least ten."""
    for seed in range(4):
        X, uv, R, t = _points(seed, n)
        planar, Ri, ti, iters = loop_oracle.iterative(lib, X, uv)
        assert planar == 0 and 1 <= iters <= 20
        assert rot_err(Ri, R) < 1e-8 and np.linalg.norm(ti - t) < 1e-8, (n, seed, rot_err(Ri, R), np.linalg.norm(ti - t))


def test_iterative_refuses_planar(lib):
    X, uv, R, t = _points(0, 30)
    X[:, 2] = 1.0
    assert loop_oracle.iterative(lib, X, uv)[0] == 1


def test_eig_jacobi_sym(lib):
    rng = np.random.Generator(np.random.PCG64(5))
    for n in (3, 12):
        B = rng.standard_normal((n - 2 if n > 3 else n, n))
        A = B.T @ B                                          # n = 12: a two-dimensional null space, as EPnP's M^T M on five points
        w, V = loop_oracle.eig_sym(lib, A)
        assert np.all(np.diff(w) <= 0) and np.abs(V.T @ V - np.eye(n)).max() < 1e-12
        assert np.abs(A @ V - V * w).max() < 1e-12 * max(1.0, w[0])
        assert np.abs(w - np.linalg.eigvalsh(A)[::-1]).max() < 1e-12 * max(1.0, w[0])


# ---------------------------------------------------------------- the whole pair
def test_exact_scenes_recover_the_truth(lib):
    worst_r = worst_t = 0.0
    kws = [kw for n, kw in loop_cases.scene_cases() if n in ("exact0", "exact1", "out30", "m16", "m65")] + [dict(seed=s) for s in range(40, 60)]
    for kw in kws:
        pair, tr = loop.make_loop_scene(**kw)
        r, mi, md, inl = loop_oracle.verify(lib, CFG, pair)
        assert r.status == loop.ISV_LOOP_OK and r.has_loop == 1 and r.loop_index == pair.c.old_index, kw
        assert r.n_final == r.ransac_inliers == int((~tr["is_outlier"]).sum()), kw
        assert (inl[tr["is_outlier"]] == 0).all() and (inl[~tr["is_outlier"]] == 1).all(), kw
        er, et = pose_err(r, tr)
        worst_r, worst_t = max(worst_r, er), max(worst_t, et)
        assert er < ROT_TOL and et < TRANS_TOL, (kw, er, et)
        assert np.abs(r.arr("loop_info")[:3] - tr["relative_t"]).max() < 10 * TRANS_TOL and abs(r.loop_info[7] - tr["yaw_deg"]) < np.degrees(ROT_TOL)
    print(f"exact scenes: worst rotation error {worst_r:.2e} rad, worst translation error {worst_t:.2e} m")


def test_noise_and_outliers(lib):
    for kw in [dict(seed=2, pixel_noise=loop_cases.NOISE), dict(seed=5, outliers=0.3, pixel_noise=loop_cases.NOISE), dict(seed=41, outliers=0.3),
               dict(seed=42, outliers=0.3, pixel_noise=loop_cases.NOISE)]:
        pair, tr = loop.make_loop_scene(**kw)
        r, mi, md, inl = loop_oracle.verify(lib, CFG, pair)
        assert r.status == loop.ISV_LOOP_OK, kw
        assert (inl[tr["is_outlier"]] == 0).all(), kw               # every outlier outside the final mask
        assert r.n_final >= 0.9 * (~tr["is_outlier"]).sum(), kw
        er, et = pose_err(r, tr)
        # 0.5 px on >= 100 points a few metres away: well inside a centimetre and a milliradian
        assert er < 2e-3 and et < 1e-2, (kw, er, et)
        assert r.loop_weight > 0 and r.res > 0


def test_every_status(lib):
    seen = {}
    for name, pair, _ in loop_cases.all_pairs():
        r = loop_oracle.verify(lib, CFG, pair)[0]
        seen.setdefault(r.status, []).append(name)
        if r.status != loop.ISV_LOOP_OK:
            assert r.has_loop == 0 and r.loop_index == -1, name
    assert set(seen) == set(range(8)), seen
    by = {n: s for s, ns in seen.items() for n in ns}
    assert by["l1_12"] == by["l1_10"] == by["l1_15"] == loop.ISV_LOOP_UNDEFINED_POSE and by["few9"] == loop.ISV_LOOP_FEW_MATCHES
    assert by["yaw40"] == by["far25"] == loop.ISV_LOOP_GATE and by["planar"] == loop.ISV_LOOP_PLANAR and by["all_outliers"] == loop.ISV_LOOP_PNP_FAILED
    for name, pair, st in loop_cases.refusal_cases():
        assert by[name] == st, name


def test_ransac_shapes_of_the_case_list(lib):
    """the GPU list holds a RANSAC that stops inside its first 64-hypothesis chunk, one that runs all 100 iterations (two chunks),
    one that keeps no model, 16 / 17 / 64 / 65 / 200 matches, and the chunk edges below"""
    rs = {n: loop_oracle.verify(lib, CFG, p)[0] for n, p, _ in loop_cases.all_pairs()}
    assert rs["exact0"].ransac_iters < 64 and rs["out60_noise"].ransac_iters == 100
    assert rs["all_outliers"].ransac_iters == 100 and rs["all_outliers"].ransac_inliers == 0 and rs["all_outliers"].n_final == 0
    assert [rs[n].n_matched for n in ("m16", "m17", "m64", "m65", "m200")] == [16, 17, 64, 65, 200]
    assert 10 <= rs["l1_10"].n_matched and rs["l1_15"].n_matched == 15 and rs["few9"].n_matched == 9
    # the chunk edges (tests/loop_highprec_cases.py has the table): a stop at hypothesis 64, the last of the first chunk; at 65, where
    # the second chunk is drawn with one hypothesis; the cap with the final model kept in the second chunk; no model with four inliers
    # at the keep rule's floor; 63 / 64 / 65 / 129 final inliers with the unmatchable window points interleaved
    assert (rs["stop64"].n_matched, rs["stop64"].ransac_inliers, rs["stop64"].ransac_iters) == (29, 17, 64)
    assert (rs["stop65"].n_matched, rs["stop65"].ransac_inliers, rs["stop65"].ransac_iters) == (41, 24, 65)
    assert (rs["keep2_f63"].n_matched, rs["keep2_f63"].ransac_iters, rs["keep2_f63"].n_final) == (158, 100, 63)
    assert (rs["floor4"].n_matched, rs["floor4"].ransac_iters, rs["floor4"].ransac_inliers) == (16, 100, 0)
    assert [rs[n].n_final for n in ("f64", "f65", "f129")] == [64, 65, 129] and [rs[n].n_matched for n in ("f64", "f65", "f129")] == [70, 72, 142]
    assert rs["late129"].n_matched == 48 and rs["late129"].ransac_iters == 100        # (its event needs ransac_iterations = 129)


# ---------------------------------------------------------------- quirks
def test_quirk_l1(lib):
    pair, tr = loop.make_loop_scene(seed=8, n_matchable=12, n_keypoints=loop_cases.T - 1)
    assert loop_oracle.verify(lib, CFG, pair)[0].status == loop.ISV_LOOP_UNDEFINED_POSE
    r = loop_oracle.verify(lib, CFG, pair, loop_oracle.L1)[0]
    assert r.status == loop.ISV_LOOP_OK and r.n_final == 12 and pose_err(r, tr)[1] < 1e-4


def test_quirk_l3(lib):
    pair, tr = loop.make_loop_scene(seed=2, pixel_noise=loop_cases.NOISE)
    a = loop_oracle.verify(lib, CFG, pair)[0]
    b = loop_oracle.verify(lib, CFG, pair, loop_oracle.L3)[0]
    assert a.status == b.status == 0 and bytes(a.PnP_R_old) == bytes(b.PnP_R_old)
    assert a.res != b.res and a.loop_weight != b.loop_weight
    # off: the mean normalised reprojection residual of 0.5 px noise, about 0.5 / 460 * sqrt(pi / 2)
    assert 0.5 * loop_cases.NOISE < b.res / b.n_final < 2.5 * loop_cases.NOISE
    # on: the same residual divided by FOCAL_LENGTH once more (the two forms of the point round apart, no more)
    assert abs(a.res * 460.0 / b.res - 1) < 1e-6
    assert abs(a.loop_weight / (b.loop_weight * 460.0 ** 2) - 1) < 1e-5


def test_quirk_l5(lib):
    """the RANSAC's reprojection error is a float32 number formed from the float32 projection"""
    X, uv, R, t = _points(1, 8)
    rvec = np.array([0.1, -0.2, 0.3]); tvec = np.array([0.05, 0.02, -0.1])
    Rm = np.zeros(9); lib.isvo_rodrigues_v2m(rvec.ctypes.data_as(C.POINTER(C.c_double)), Rm.ctypes.data_as(C.POINTER(C.c_double)))
    changed = 0
    for k in range(8):
        Xf, uvf = X[k].astype(np.float32), uv[k].astype(np.float32)
        on = loop_oracle.point_error(lib, rvec, tvec, Xf, uvf)
        off = loop_oracle.point_error(lib, rvec, tvec, Xf, uvf, loop_oracle.L5)
        pc = Rm.reshape(3, 3) @ Xf.astype(np.float64) + tvec
        pf = (pc[:2] / pc[2]).astype(np.float32)
        d = uvf - pf
        assert on == float(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) and np.float32(on) == on
        assert abs(off - on) <= 1e-5 * on
        changed += off != on
    assert changed >= 6


def test_quirk_l5_changes_a_pair(lib):
    """one matched corner is moved by about 0.02 so that its error sits at the RANSAC threshold: at the largest threshold (to the
    last bit) at which the comparison in doubles still calls the point an outlier, the float32 error against the float32
    threshold calls it an inlier, and the pair's inlier count and mask differ"""
    pair, tr = loop.make_loop_scene(seed=60, n_points=40, n_keypoints=100)
    j = 7
    pair.keypoints_norm[int(tr["counterpart"][j]), 0] += np.float32(0.02)

    def run(thr, off):
        cfg = loop_cases.config(); cfg.ransac_threshold = thr
        r, mi, md, inl = loop_oracle.verify(lib, cfg, pair, off)
        assert r.status == loop.ISV_LOOP_OK
        return r.ransac_inliers, inl

    lo, hi = 0.015, 0.025
    assert run(lo, loop_oracle.L5)[1][j] == 0 and run(hi, loop_oracle.L5)[1][j] == 1
    while True:                                                   # bisect the doubles' threshold down to two neighbouring numbers
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if run(mid, loop_oracle.L5)[1][j] == 1:
            hi = mid
        else:
            lo = mid
    (g_on, inl_on), (g_off, inl_off) = run(lo, 0), run(lo, loop_oracle.L5)
    assert (g_on, inl_on[j]) == (40, 1) and (g_off, inl_off[j]) == (39, 0)
    assert np.array_equal(np.delete(inl_on, j), np.delete(inl_off, j))


def test_quirk_l6(lib):
    pair, tr = loop.make_loop_scene(seed=3, n_points=40, n_keypoints=200)
    k = int(tr["counterpart"][0])
    pair.window_brief[1] = loop.flip_bits(pair.brief[k], range(25))           # point 1 claims point 0's corner too, at 25 bits
    a = loop_oracle.verify(lib, CFG, pair)
    b = loop_oracle.verify(lib, CFG, pair, loop_oracle.L6)
    assert a[1][0] == a[1][1] == k and a[0].n_matched == 40 and a[3][1] == 0      # both matched; the false claim is a RANSAC outlier
    assert b[0].n_matched == 39 and b[3][1] == -1 and b[3][0] == 1                # off: only the closer claimant reaches the PnP


# ---------------------------------------------------------------- knife edge
def test_case_list_is_off_the_rounding_edges(lib, lib_o0):
    """every integer output of every GPU case is the same at -O0 and -O2 (both -ffp-contract=off): a case that fails this sits
    on a rounding edge and must be replaced in tests/loop_cases.py, because the GPU test compares these outputs exactly"""
    for name, pair, _ in loop_cases.all_pairs():
        a, b = loop_oracle.verify(lib, CFG, pair), loop_oracle.verify(lib_o0, CFG, pair)
        ints = lambda r: (r.status, r.n_matched, r.ransac_iters, r.ransac_inliers, r.pnp_iterations, r.n_final, r.has_loop, r.loop_index)
        assert ints(a[0]) == ints(b[0]), name
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y), name
