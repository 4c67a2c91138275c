"""GPU parity of the batched relative-pose stage (k_relpose, is-vins_amd/csrc/isv_relpose.h) against the CPU restatement
tests/native/isv_relpose_oracle.c, batch against single, and initial_structure_from_tracks_batch against relpose_batch
followed by initial_structure_batch.  Identical: status, l, per-candidate correspondence counts, RANSAC iterations and
inliers, recoverPose counts and chosen solutions, the per-track masks; the parallax bitwise (the same sums in the same
order).  relative_R / relative_T agree to 1e-9: the two run the same operations, and only the device and host libm can round
solveCubic's acos / cos / pow apart by an ulp, which moves a model by about that much.

The restatement is the same text as the kernel's serial pieces; tests/test_gpu_relpose_highprec.py holds the kernel to an independent 40-digit
reference instead, at 21 to 129 correspondences (every case here has 21 to 41) and at the chunk edges of the speculative RANSAC."""
import numpy as np
import pytest

import relpose_oracle
import test_relpose_oracle
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

NOISE = 0.5 / 460
CASES = [dict(seed=0), dict(seed=1), dict(seed=2), dict(seed=3), dict(seed=0, pixel_noise=NOISE), dict(seed=1, pixel_noise=NOISE),
         dict(seed=0, outliers=0.3), dict(seed=5, outliers=0.3, pixel_noise=NOISE), dict(seed=6, outliers=0.2, pixel_noise=0.2 / 460),
         dict(seed=0, n_window=5, per_frame=30), dict(seed=0, n_window=4, extra=4, per_frame=60), dict(seed=4, extra=6, n_window=18),
         dict(seed=7, n_window=20, extra=20, cam_dt=0.05, imu_per_frame=5, per_frame=400)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return relpose_oracle.build(tmp_path_factory.mktemp("relpose_oracle"))


@pytest.fixture(scope="module")
def be():
    b = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    yield b
    b.close()


def _problems():
    return ([initial.make_relpose_scene(**kw)[0] for kw in CASES] + [test_relpose_oracle.r5_scene()]
            + [c[1] for c in test_relpose_oracle.refusal_cases()])


def test_against_restatement(lib, be):
    ps = _problems()
    rs, ms = initial.relpose_batch(be, ps, masks=True)
    seen = set()
    for k, (p, rg, mg) in enumerate(zip(ps, rs, ms)):
        ro, mo = relpose_oracle.solve(lib, p)
        seen.add(ro.status)
        assert (rg.status, rg.l, rg.n_candidates) == (ro.status, ro.l, ro.n_candidates), k
        if ro.status in (3, 4):
            continue
        assert rg.excitation_var == ro.excitation_var, k
        for f in ("n_corres", "ransac_iters", "ransac_inliers", "recover_inliers", "solution", "parallax"):
            assert list(getattr(rg, f)) == list(getattr(ro, f)), (k, f)
        assert np.array_equal(mg, mo), k
        if ro.status == 0:
            assert np.abs(rg.arr("relative_R") - ro.arr("relative_R")).max() < 1e-9, k
            assert np.abs(rg.arr("relative_T") - ro.arr("relative_T")).max() < 1e-9, k
    assert seen == {0, 1, 2, 3, 4}, seen


@pytest.mark.parametrize("S", [1, 64, 1024])
def test_batch_bitwise(be, S):
    ps = _problems()
    single = []
    for p in ps:
        r, m = initial.relpose_batch(be, [p], masks=True)
        single.append((bytes(r[0]), m[0].copy()))
    idx = [(7 * i + 3) % len(ps) for i in range(S)]
    batch = [ps[k] for k in idx]
    rs, ms = initial.relpose_batch(be, batch, masks=True)
    for i, (r, m) in enumerate(zip(rs, ms)):
        assert bytes(r) == single[idx[i]][0], i
        if r.status not in (3, 4):
            assert np.array_equal(m, single[idx[i]][1]), i


def test_buffers_kept_and_timed(be):
    ps = [initial.make_relpose_scene(**kw)[0] for kw in CASES]
    big = initial.relpose_batch(be, ps * 16)
    call_ms, kernel_ms = initial.relpose_last_ms(be)
    assert 0 < kernel_ms <= call_ms
    small = initial.relpose_batch(be, ps[:3])
    assert all(bytes(a) == bytes(b) for a, b in zip(small, big[:3]))


def _scenes():
    kws = [dict(seed=0), dict(seed=3), dict(seed=1, pixel_noise=NOISE), dict(seed=8, hover=True), dict(seed=0, per_frame=12)]
    return kws, [initial.make_relpose_scene(**kw) for kw in kws]


def test_chain_equals_stages(be):
    kws, sc = _scenes()
    rr, sr, ar = initial.initial_structure_from_tracks_batch(be, [s[0] for s in sc], [s[1] for s in sc])
    assert [r.status for r in rr] == [0, 0, 0, 1, 2] and sr[3] is None and ar[4] is None
    _, sc2 = _scenes()
    rr2 = initial.relpose_batch(be, [s[0] for s in sc2], write=True)
    ok = [i for i, r in enumerate(rr2) if r.status == 0]
    sr2, ar2 = initial.initial_structure_batch(be, [sc2[i][0] for i in ok], [sc2[i][1] for i in ok])
    assert [bytes(r) for r in rr] == [bytes(r) for r in rr2]
    for j, i in enumerate(ok):
        assert bytes(sr[i]) == bytes(sr2[j]) and (ar[i] is None) == (ar2[j] is None)
        if ar[i] is not None:
            assert bytes(ar[i]) == bytes(ar2[j])
        assert np.array_equal(sc[i][0].position, sc2[i][0].position)


def test_chain_recovers_truth(be):
    # the restatement chain's bound (tests/test_relpose_oracle.py::test_chain_from_tracks)
    kws, sc = _scenes()
    rr, sr, ar = initial.initial_structure_from_tracks_batch(be, [s[0] for s in sc[:2]], [s[1] for s in sc[:2]])
    for kw, r, s, a in zip(kws, rr, sr, ar):
        assert r.status == 0 and s.status == 0 and a.status == 0
        _, ap = initial.make_relpose_scene(**dict(kw, l=r.l))
        ep, er, ev, eg, es = initial.ate_4dof(a, ap.truth, ap.c.n_window)
        assert ep < 1e-4 and ev < 1e-4 and es < 1e-4 and er < 1e-7, (ep, er, ev, es)


def test_empty_and_null(be):
    assert initial.relpose_batch(be, []) == []
    initial._bind_relpose(be.lib)
    assert be.lib.isv_internal_relpose_batch(be.h, 1, None, None, None) == -1
