"""GPU parity of the batched SfM stage (k_sfm, is-vins_amd/csrc/isv_sfm.h) against the CPU restatement
tests/native/isv_sfm_oracle.c, batch against single, the handle's grow-only buffers, and initial_structure_batch.
Identical: status, refusing frame, BA iterations / termination, PnP iterations and point counts, track states.
Q / T, points and the all-frame R / T agree to 1e-8 relative, the BA's costs to 1e-10 relative above a 1e-18 floor (the two
differ only where the device and host libm round sin / cos / acos / exp apart)."""
import numpy as np
import pytest

import sfm_oracle
import test_sfm_oracle
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

CASES = [dict(seed=0), dict(seed=1, n_window=18), dict(seed=2, pixel_noise=1.0 / 460), dict(seed=3, rel_rot_err=0.01, rel_dir_err=0.02),
         dict(seed=4, extra=6), dict(seed=5, l=0), dict(seed=6, l=9), dict(seed=12, l=0, n_window=5),
         dict(seed=7, n_window=20, extra=20, cam_dt=0.05, imu_per_frame=5, per_frame=400), dict(seed=11, n_window=18, pixel_noise=0.5 / 460, extra=3),
         dict(seed=0, behind=3)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sfm_oracle.build(tmp_path_factory.mktemp("sfm_oracle"))


@pytest.fixture(scope="module")
def be():
    b = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    yield b
    b.close()


def _problems():
    return [initial.make_scene(**kw)[0] for kw in CASES] + [c[1] for c in test_sfm_oracle.refusal_cases()]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max()) if a.size else 0.0


def test_against_restatement(lib, be):
    ps = _problems()
    rs = initial.sfm_batch(be, ps)
    got = [(p.position.copy(), p.state.copy()) for p in ps]
    seen = set()
    for p, rg, (pg, sg) in zip(ps, rs, got):
        ro, po, so = sfm_oracle.solve(lib, p)
        seen.add(ro.status)
        assert (rg.status, rg.fail_frame) == (ro.status, ro.fail_frame)
        assert rg.excitation_var == pytest.approx(ro.excitation_var, rel=1e-14, abs=0)
        nw, nf, nt = p.c.n_window, p.c.n_frames, p.c.n_tracks
        assert list(rg.sfm_pnp_points[:nw]) == list(ro.sfm_pnp_points[:nw])
        assert list(rg.sfm_pnp_iterations[:nw]) == list(ro.sfm_pnp_iterations[:nw])
        if ro.status in (0, 3, 4):
            assert (rg.ba_iterations, rg.ba_termination, rg.ba_residuals, rg.n_triangulated) == \
                (ro.ba_iterations, ro.ba_termination, ro.ba_residuals, ro.n_triangulated)
        if ro.status in (0, 4):
            # (status 3 is a BA that runs to the 50-iteration cap on a relative pose 0.6 rad off: there the ulp differences
            # grow along the path, measured 33 against 34 accepted steps, so only status / iterations / termination are pinned)
            assert rg.ba_successful == ro.ba_successful
            # on exact data the costs sit at the rounding floor (1e-17 final, 1e-14 initial): poses 1e-16 apart (sin / cos in
            # Rodrigues) move a cost of n_res residuals of ~1e-7 by ~n_res * 1e-7 * 1e-16 = 3e-20 (measured 4.6e-20): 1e-18 absolute
            assert abs(rg.ba_final_cost - ro.ba_final_cost) <= 1e-10 * abs(ro.ba_final_cost) + 1e-18
            assert abs(rg.ba_initial_cost - ro.ba_initial_cost) <= 1e-10 * abs(ro.ba_initial_cost) + 1e-18
            assert np.array_equal(sg[:nt], so[:nt])
            assert _rel(pg[:nt], po[:nt]) < 1e-8
        if ro.status in (0, 4):
            assert _rel(rg.arr("Q")[:nw], ro.arr("Q")[:nw]) < 1e-8 and _rel(rg.arr("T")[:nw], ro.arr("T")[:nw]) < 1e-8
            k = ro.fail_frame if ro.status == 4 else nf
            assert list(rg.pnp_points[:k]) == list(ro.pnp_points[:k]) and list(rg.pnp_iterations[:k]) == list(ro.pnp_iterations[:k])
            assert list(rg.is_key_frame[:k]) == list(ro.is_key_frame[:k])
            assert _rel(rg.arr("R")[:k], ro.arr("R")[:k]) < 1e-8 and _rel(rg.arr("Tf")[:k], ro.arr("Tf")[:k]) < 1e-8
    assert seen == {0, 1, 2, 3, 4, 5, 6}, seen


@pytest.mark.parametrize("S", [1, 64, 1024])
def test_batch_bitwise(be, S):
    ps = _problems()
    single = []
    for p in ps:
        r = initial.sfm_batch(be, [p])[0]
        single.append((bytes(r), p.position.copy(), p.state.copy()))
    idx = [(7 * i + 3) % len(ps) for i in range(S)]
    batch = [initial.make_scene(**CASES[k])[0] if k < len(CASES) else ps[k] for k in idx]
    rs = initial.sfm_batch(be, batch)
    for i, (r, p) in enumerate(zip(rs, batch)):
        ref = single[idx[i]]
        assert bytes(r) == ref[0], i
        if r.status in (0, 3, 4):
            assert np.array_equal(p.position, ref[1]) and np.array_equal(p.state, ref[2]), i


def test_buffers_kept_and_timed(be):
    ps = [initial.make_scene(**kw)[0] for kw in CASES]
    big = initial.sfm_batch(be, ps * 16)
    call_ms, kernel_ms = initial.sfm_last_ms(be)
    assert 0 < kernel_ms <= call_ms
    small = initial.sfm_batch(be, ps[:3])
    assert all(bytes(a) == bytes(b) for a, b in zip(small, big[:3]))


def test_initial_structure_batch_recovers_truth(be):
    # the restatement chain's bound (tests/test_sfm_oracle.py::test_chain_into_alignment)
    scenes = [initial.make_scene(seed=0), initial.make_scene(seed=1, n_window=18), initial.make_scene(seed=8, hover=True)]
    sr, ar = initial.initial_structure_batch(be, [s[0] for s in scenes], [s[1] for s in scenes])
    assert [r.status for r in sr] == [0, 0, 1] and ar[2] is None
    for (sp, ap), ra in zip(scenes[:2], ar[:2]):
        assert ra.status == 0
        ep, er, ev, eg, es = initial.ate_4dof(ra, ap.truth, ap.c.n_window)
        assert ep < 1e-4 and ev < 1e-4 and es < 1e-4 and er < 1e-7, (ep, er, ev, es)


def test_empty_and_null(be):
    assert initial.sfm_batch(be, []) == []
    initial._bind_sfm(be.lib)
    assert be.lib.isv_internal_sfm_batch(be.h, 1, None, None) == -1
