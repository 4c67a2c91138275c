"""The CPU restatement of the relative-pose stage (tests/native/isv_relpose_oracle.c, the same text as k_relpose's serial pieces) against the
40-digit reference of tests/relpose_highprec.py, an independent reading of the same definitions, on the cases of tests/relpose_cases.py.

Identical on every case: status, l, n_candidates, n_corres, ransac_iters, ransac_inliers, recover_inliers and the per-track mask (`solution`
is a label of OpenCV's root order and SVD signs and is not compared: the pose is matched to the nearest of the reference's four cameras,
whose count must be recover_inliers and the strict maximum).  Within their limits: parallax, excitation_var, relative_R, relative_T
(relpose_cases: MARGIN * max(e64, n 2^-53), and MARGIN_CV * max(e64, ecv, n 2^-53) for a one-root model; the measured ratios are in
DESIGN.md section 13).  Also asserted here: the reference's conditions on every case, that every edge the case list names is really taken,
and that every negative control has power where it is used (it changes an integer output or moves a vector by at least POWER limits) and
none where the stage cannot see it.

The references are computed once per process and shared by the tests (relpose_cases.reference; nothing is cached in a file).  Measured
here, the module takes 44 s: 8 s for the 28 problems and the restatement's records, 25 s for the 28 references (old_7, three candidates
that run to the 1000 cap, 4.3 s; no other above 1.5 s; c29_cap, the new case at the cap, 0.8 s), 9 s for the 10 corrupted references that
need a RANSAC of their own."""
import numpy as np
import pytest

import relpose_cases as rc
import relpose_highprec as rh
import relpose_oracle

NAMES = rc.names()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return relpose_oracle.build(tmp_path_factory.mktemp("relpose_oracle"))


@pytest.fixture(scope="module")
def records(lib):
    """{case: (result, mask)} of the restatement"""
    return {n: relpose_oracle.solve(lib, rc.problem(n)) for n in NAMES}


def test_rng_is_opencvs():
    # RNG(2^64 - 1): the first states by hand, state = (unsigned)state * 4164903690 + (state >> 32)
    s = (1 << 64) - 1
    s1 = 0xFFFFFFFF * 4164903690 + 0xFFFFFFFF
    assert rh.rng_uniform(s, 1000)[0] == s1 and rh.rng_uniform(s, 1000)[1] == (s1 & 0xFFFFFFFF) % 1000
    state, idx = rh.subset(s, 8)
    assert len(set(idx)) == 7 and all(0 <= v < 8 for v in idx)


def test_bound_is_the_float32_decision():
    # float32(err) <= TF exactly when err < BOUND: one float64 ulp either side of BOUND
    lo, hi = np.nextafter(rh.BOUND, 0.0), np.nextafter(rh.BOUND, 1.0)
    assert np.float32(lo) <= rh.TF < np.float32(hi)
    assert rh.TF == np.float32((0.3 / 460) * (0.3 / 460))


@pytest.mark.parametrize("name", NAMES)
def test_reference_conditions(name):
    rc.reference(name).conditions()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_40_digits(records, name):
    res, mask = records[name]
    ref = rc.reference(name)
    bad, ratios = rc.measure(ref, res, mask)
    print(f"RATIO cpu {name:15s} " + " ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    assert not bad, (name, bad)
    for k, r in ratios.items():
        assert r <= rc.margin_of(k, rc.MARGIN), (name, k, r)


def test_edges_are_taken():
    """the events that relpose_cases' table names, read from the reference's own record of its loop"""
    ran = {n: [c for c in rc.reference(n).cands if c.ransac is not None] for n in rc.NEW}
    first = {n: ran[n][0] for n in rc.NEW}
    assert {n: first[n].count for n in ("c21_exact", "c63_stop64", "c64_noise", "c65_noise", "c65_exact", "c129_stop65", "c129_mixed")} == \
        dict(c21_exact=21, c63_stop64=63, c64_noise=64, c65_noise=65, c65_exact=65, c129_stop65=129, c129_mixed=129)
    assert first["c21_exact"].ransac.iters == 1 and first["c21_exact"].ransac.inliers == 21
    assert first["c65_exact"].ransac.iters == 1 and abs(1 - rc.reference("c65_exact").stats["sv_ratio"]) < 1e-6
    assert (first["c63_stop64"].ransac.iters, first["c63_stop64"].ransac.inliers) == (64, 43)
    assert (first["c129_stop65"].ransac.iters, first["c129_stop65"].ransac.inliers) == (65, 88)
    r = first["c30_stop_early"].ransac
    assert 1 < r.iters < 64 and 0 < r.keeps[-1][0] < r.iters - 1
    r = first["c40_late"].ransac
    assert r.keeps[-1][0] >= 64 and r.iters > r.keeps[-1][0] + 1
    assert first["c29_cap"].ransac.iters == 1000 and first["c29_cap"].count == 29 and first["c29_cap"].recover == 13
    assert first["c129_mixed"].ransac.keeps[-1][0] >= 128          # a keep in the third chunk or later
    # spanning tracks beyond index 128 of the track list, others between them
    trk = first["c129_mixed"].trk
    assert trk[-1] > 128 and len(trk) == 129 and all(b - a > 1 for a, b in zip(trk, trk[1:]))
    # a subset with three real roots, one with a single one, one whose models all lose; a kept model of either kind
    for n in rc.NEW:
        if first[n].ransac.iters > 1:
            r = first[n].ransac
            assert r.roots[3] > 0 and r.roots[1] > 0 and r.all_lose > 0, (n, r.roots, r.all_lose)
    assert {first[n].ransac.kept[3] for n in rc.NEW} == {1, 3}
    # a RANSAC that keeps a model and fails recoverPose, so that l moves on; the second candidate restarts the RNG
    ref = rc.reference("far0_then1")
    c0, c1 = ref.cands
    assert ref.l == 1 and c0.ransac.inliers > 12 and c0.ransac.iters > 1 and c0.recover <= 12 and c1.recover > 12 and c1.ransac.iters > 1
    assert (c0.count, c1.count) == (30, 42)
    # every status the stage can give from a valid input is in the list
    assert {rc.reference(n).status for n in NAMES} == {0, 1, 2}


@pytest.mark.parametrize("control,name", [(c, n) for c, names in rc.CONTROL_CASES.items() for n in names])
def test_control_has_power(records, control, name):
    res, mask = records[name]
    assert not rc.failures(rc.reference(name), res, mask, rc.MARGIN)
    pw = rc.power(rc.reference(name, control), res, mask, rc.MARGIN)
    print(f"CONTROL {control:18s} {name:15s} restatement / corrupted reference {pw:.3g} limits")
    assert pw >= rc.POWER, (control, name, pw)


def test_rng_control_needs_an_earlier_ransac(records):
    # where no candidate before l runs a RANSAC the carried RNG is the fresh one: the control must change nothing there
    res, mask = records["c30_stop_early"]
    assert not rc.failures(rc.reference("c30_stop_early", "rng_carried"), res, mask, rc.MARGIN)
