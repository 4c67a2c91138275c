"""CPU checks of the SfM stage's restatement (tests/native/isv_sfm_oracle.c, the checker of k_sfm in
is-vins_amd/csrc/isv_sfm.h): ground truth on exact data, the chain into the alignment restatement, every refusal, the quirks
S1 / S2 / S4 / S5, and the ctypes layouts.  Bounds are set from measured errors (noted beside each)."""
import ctypes as C

import numpy as np
import pytest

import align_oracle
import sfm_oracle
from isvins_amd import initial


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sfm_oracle.build(tmp_path_factory.mktemp("sfm_oracle"))


@pytest.fixture(scope="module")
def alib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


def test_struct_sizes(lib):
    assert [lib.isvo_sfm_sizeof(i) for i in range(3)] == [C.sizeof(initial.isv_sfm_track_t), C.sizeof(initial.isv_sfm_problem_t),
                                                         C.sizeof(initial.isv_sfm_result_t)]


# exact data, exact relative pose: the SfM frame is fixed by camera l and the unit baseline, so Q / T / points are compared
# with the truth directly.  Measured (seeds 0, 1, 4, 6): Q 6.4e-9, T 1.9e-7, points 4.0e-5, all-frame R 2.0e-8, T 1.9e-7;
# the float32 rounding of the PnP points (S2) sets the floor.
@pytest.mark.parametrize("kw", [dict(seed=0), dict(seed=1, n_window=18), dict(seed=4, extra=6), dict(seed=6, l=9)])
def test_exact_scene_recovers_truth(lib, kw):
    sp, _ = initial.make_scene(**kw)
    r, _, _ = sfm_oracle.solve(lib, sp)
    assert r.status == 0 and r.fail_frame == -1
    assert r.ba_termination in (1, 2, 3, 5) and r.ba_final_cost < 1e-12
    eq, et, ep, eR, eT = initial.sfm_errors(r, sp)
    assert eq < 1e-7 and et < 1e-6 and ep < 2e-4 and eR < 1e-7 and eT < 1e-6, (eq, et, ep, eR, eT)
    nf = sp.c.n_frames
    assert list(r.is_key_frame[:nf]) == [int(f in list(sp.c.window_frame[:sp.c.n_window])) for f in range(nf)]


def test_chain_into_alignment(lib, alib):
    # the all-frame R / T of the SfM, copied into the alignment problem of the same seed, recover the window states
    # (measured: P 3.4e-5 m, R 1.8e-9, V 3.2e-5 m/s, scale 3.7e-5 relative; window-only: with non-keyframes the alignment's
    # own quirk Q3 picks the wrong velocities, as the reference does)
    sp, ap = initial.make_scene(seed=0)
    r, _, _ = sfm_oracle.solve(lib, sp)
    assert r.status == 0
    initial.copy_sfm_to_align(r, ap)
    ra = align_oracle.solve(alib, ap)
    assert ra.status == 0
    ep, er, ev, eg, es = initial.ate_4dof(ra, ap.truth, ap.c.n_window)
    assert ep < 1e-4 and ev < 1e-4 and es < 1e-4 and er < 1e-7, (ep, er, ev, es)


def refusal_cases():
    """(name, problem, expected status); shared with the GPU test"""
    out = []
    sp, _ = initial.make_scene(seed=8, hover=True)
    out.append(("excitation", sp, 1))
    sp, _ = initial.make_scene(seed=9, per_frame=12)
    out.append(("sfm_pnp_points", sp, 2))
    sp, _ = initial.make_scene(seed=10, rel_rot_err=0.6, rel_dir_err=0.6, pixel_noise=0.02)
    out.append(("ba_not_converged", sp, 3))
    sp, _ = initial.make_scene(seed=4, extra=6)
    f = next(f for f in range(sp.c.n_frames) if f not in list(sp.c.window_frame[:sp.c.n_window]))
    a, b = sp.pt_off[f], sp.pt_off[f + 1]
    sp.pt_id[a + 5:b] = sp.pt_id[a + 5:b] + 1000000   # ids no track has: five points left (S3: < 6)
    out.append(("all_pnp_points", sp, 4))
    sp, _ = initial.make_scene(seed=0)
    sp.c.n_tracks = initial.ISV_SFM_MAX_TRACKS + 1
    out.append(("capacity", sp, 5))
    sp, _ = initial.make_scene(seed=0)
    sp.c.l = sp.c.n_window - 1
    out.append(("input_l", sp, 6))
    sp, _ = initial.make_scene(seed=0)
    sp.pt_id[sp.pt_off[3]] = sp.pt_id[sp.pt_off[3] + 1]
    out.append(("input_csr", sp, 6))
    sp, _ = initial.make_scene(seed=0)
    sp.c.window_frame[4] = sp.c.window_frame[3]
    out.append(("input_window", sp, 6))
    return out


@pytest.mark.parametrize("case", range(8))
def test_refusals(lib, case):
    name, sp, want = refusal_cases()[case]
    r, _, _ = sfm_oracle.solve(lib, sp)
    assert r.status == want, (name, r.status)
    if want in (2, 4):
        assert r.fail_frame >= 0
    if want == 4:
        assert r.pnp_points[r.fail_frame] == 5


def test_s1_sum_g_starts_at_zero(lib):
    sp, _ = initial.make_scene(seed=3)
    r, _, _ = sfm_oracle.solve(lib, sp)
    nf = sp.c.n_frames
    g = sp.delta_v[1:nf] / sp.sum_dt[1:nf, None]
    var = np.sqrt(((g - g.sum(0) / (nf - 1)) ** 2).sum() / (nf - 1))
    assert abs(r.excitation_var - var) < 1e-12 * var
    r1, _, _ = sfm_oracle.solve(lib, sp, quirks_off=1)
    assert r1.excitation_var != r.excitation_var


def test_s2_float_rounding_matters(lib):
    sp, _ = initial.make_scene(seed=0, extra=4)
    r, _, _ = sfm_oracle.solve(lib, sp)
    r2, _, _ = sfm_oracle.solve(lib, sp, quirks_off=2)
    assert r.status == r2.status == 0
    assert bytes(r.R) != bytes(r2.R) and bytes(r.Q) != bytes(r2.Q)


def test_s4_next_keyframe_guess_matters(lib):
    sp, _ = initial.make_scene(seed=4, extra=6)
    r, _, _ = sfm_oracle.solve(lib, sp)
    r4, _, _ = sfm_oracle.solve(lib, sp, quirks_off=4)
    assert r.status == r4.status == 0
    assert bytes(r.Q) == bytes(r4.Q)            # the window is untouched
    assert bytes(r.R) != bytes(r4.R)            # the non-keyframes start from another guess


def test_s5_point_behind_cameras_enters_ba(lib):
    sp, _ = initial.make_scene(seed=0, behind=3)
    r, pos, st = sfm_oracle.solve(lib, sp)
    n = sp.c.n_tracks
    assert r.status == 0 and st[n - 3:n].all()
    assert np.abs(pos[n - 3:n] - sp.truth["points"][n - 3:n]).max() < 1e-4   # the points behind, where they are
    r5, _, st5 = sfm_oracle.solve(lib, sp, quirks_off=8)
    assert not st5[n - 3:n].any() and r5.n_triangulated == r.n_triangulated - 3
