"""CPU checks of the serial restatement of the rotation calibration (tests/native/isv_exr_oracle.c, which pins k_exr_calibrate): its
pieces against independent numpy / Python-integer statements of include/isvins_exrot.h (the method by count, the RNG and the subsets
against tests/relpose_highprec.py, the quaternion conversions, the L and R blocks, the huber rule, the cofactor inverse, the success
rule at its two thresholds), each hook changing a named case, every item and configuration refusal, a refused item leaving its slot
untouched, and the case table reaching the edge each case is named for."""
import ctypes as C

import numpy as np
import pytest

import exr_cases as xc
import exr_oracle as xo
import relpose_highprec as rhp
from isvins_amd import exrot as exr

OK, CAPACITY, INPUT, NO_MODEL = exr.ISV_EXR_OK, exr.ISV_EXR_CAPACITY, exr.ISV_EXR_INPUT, exr.ISV_EXR_NO_MODEL


@pytest.fixture(scope="module")
def lib():
    return xo.load()


@pytest.fixture(scope="module")
def table(lib):
    """every case on a fresh slot: name -> (result, what the restatement left, the slot)"""
    out = {}
    for n, fr in xc.CASES.items():
        S = xo.Slots(exr.make_config(**xc.CFG))
        r = xo.calibrate_batch(lib, S, [fr.item(0)])[0]
        out[n] = (r, xo.last(lib) if len(fr.corres) >= 9 else None, S.read_slot(0))
    return out


@pytest.fixture(scope="module")
def sequences(lib):
    out = {}
    for n, sq in xc.SEQUENCES.items():
        S = xo.Slots(exr.make_config(**sq.cfg))
        out[n] = [xo.calibrate_batch(lib, S, [fr.item(1)])[0] for fr in sq.frames]
    return out


def test_method_by_count(lib):
    for n in range(0, 40):
        assert lib.isvo_exr_method(n) == (exr.NONE if n < 9 else exr.LMEDS if n < 15 else exr.RANSAC)


def test_rng_and_subsets_against_the_integer_reading(lib):
    state, s = (1 << 64) - 1, C.c_uint64((1 << 64) - 1)
    for n in (9, 14, 15, 150, 4096) * 20:
        state, want = rhp.rng_uniform(state, n)
        assert lib.isvo_exr_uniform(C.byref(s), n) == want and s.value == state
    for count in (9, 10, 14, 15, 65, 150):
        got, end = xo.subsets(lib, count, 40)
        st = (1 << 64) - 1
        for k in range(40):
            st, idx = rhp.subset(st, count)
            assert list(got[k]) == list(idx)
        assert end == st


def np_q_from_R(m):
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0); q[0] = 0.5 * t; t = 0.5 / t
        q[1:] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0); q[1 + i] = 0.5 * t; t = 0.5 / t
        q[0] = (m[k, j] - m[j, k]) * t; q[1 + j] = (m[j, i] + m[i, j]) * t; q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def test_quaternion_conversions(lib):
    rng = np.random.default_rng(0)
    branches = set()
    for k in range(200):
        axis, deg = rng.normal(size=3), rng.uniform(0, 180) if k % 2 else rng.uniform(170, 180)
        R = xc.rot(axis, deg)
        q = xo.q_from_R(lib, R)
        assert np.array_equal(q, np_q_from_R(R))
        branches.add(0 if np.trace(R) > 0 else 1 + int(np.argmax(np.abs(q[1:]))))
        assert abs(np.linalg.norm(q) - 1) < 1e-12 and np.abs(xo.q_to_R(lib, q) - R).max() < 1e-12
        want = xc.quat(axis, deg)
        assert min(np.abs(q - want).max(), np.abs(q + want).max()) < 1e-9
    assert branches == {0, 1, 2, 3}
    # toRotationMatrix does not normalise
    assert np.abs(xo.q_to_R(lib, [2.0, 0, 0, 0]) - np.diag([1.0, 1.0, 1.0])).max() == 0 and xo.q_to_R(lib, [0, 2.0, 0, 0])[1, 1] == -7.0


def test_cofactor_inverse(lib):
    rng = np.random.default_rng(1)
    for _ in range(50):
        m = rng.normal(size=(3, 3))
        inv = xo.inv3(lib, m)
        assert np.abs(inv @ m - np.eye(3)).max() < 1e-9 * np.linalg.cond(m)
        cof = lambda i, j: m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3]
        det = cof(0, 0) * m[0, 0] + cof(1, 0) * m[1, 0] + cof(2, 0) * m[2, 0]
        want = np.array([[cof(c, r) * (1.0 / det) for c in range(3)] for r in range(3)])
        assert np.array_equal(inv, want)
    assert np.array_equal(xo.inv3(lib, np.eye(3)), np.eye(3))


def np_blocks(q1, q2):
    def skew(q):
        return np.array([[0, -q[3], q[2]], [q[3], 0, -q[1]], [-q[2], q[1], 0]])
    L, R = np.zeros((4, 4)), np.zeros((4, 4))
    L[:3, :3] = q1[0] * np.eye(3) + skew(q1); L[:3, 3] = q1[1:]; L[3, :3] = -q1[1:]; L[3, 3] = q1[0]
    R[:3, :3] = q2[0] * np.eye(3) - skew(q2); R[:3, 3] = q2[1:]; R[3, :3] = -q2[1:]; R[3, 3] = q2[0]
    return L, R


def test_blocks_angle_and_the_huber_rule(lib):
    rng = np.random.default_rng(2)
    seen = set()
    for k in range(120):
        Rc, Rimu = xc.rot(rng.normal(size=3), rng.uniform(0, 40)), xc.rot(rng.normal(size=3), rng.uniform(0, 40))
        Rg = Rc @ xc.rot(rng.normal(size=3), rng.uniform(0, 10) if k % 2 else rng.uniform(4.9, 5.1))
        ang, hub, blk = xo.row(lib, Rc, Rimu, Rg)
        true = np.degrees(np.arccos(np.clip((np.trace(Rc.T @ Rg) - 1) / 2, -1, 1)))
        assert abs(ang - true) < 1e-6
        assert hub == (5.0 / ang if ang > 5.0 else 1.0)
        seen.add(ang > 5.0)
        L, R = np_blocks(np_q_from_R(Rc), np_q_from_R(Rimu))
        assert np.array_equal(blk, hub * (L - R))
    assert seen == {True, False}
    # A x = 0 for the inverse of the true extrinsic quaternion (q_c x = x q_imu; ric is toRotationMatrix(x).inverse()): Rc = ric^T Rimu ric
    ric, Rimu = xc.RIC_TRUE, xc.rot((0.3, 1, -0.2), 25.0)
    _, _, blk = xo.row(lib, ric.T @ Rimu @ ric, Rimu, ric.T @ Rimu @ ric)
    q = np_q_from_R(ric)
    assert np.abs(blk @ np.array([-q[1], -q[2], -q[3], q[0]])).max() < 1e-12
    # angularDistance takes |w|: q and -q are the same rotation
    assert xo.row(lib, np.eye(3), np.eye(3), np.eye(3))[0] == 0.0


def test_rc_g_uses_the_inverse_and_delta_q_as_given(lib):
    ric, dq = xc.rot((1, 2, 3), 20.0), xc.quat((0.2, -1, 0.4), 15.0)
    Rimu, Rg = xo.imu_rows(lib, ric, dq)
    assert np.abs(Rimu - xc.rot((0.2, -1, 0.4), 15.0)).max() < 1e-15
    assert np.abs(Rg - ric.T @ Rimu @ ric).max() < 1e-15
    Rimu2, _ = xo.imu_rows(lib, ric, 2 * dq)                   # not normalised
    assert np.array_equal(Rimu2, xo.q_to_R(lib, 2 * dq)) and abs(Rimu2[0, 0] - Rimu[0, 0]) > 0.05
    skewed = ric + 0.1 * np.arange(9).reshape(3, 3)            # a ric that is no rotation: the inverse, not the transpose
    assert np.abs(xo.imu_rows(lib, skewed, dq)[1] - np.linalg.inv(skewed) @ Rimu @ skewed).max() < 1e-9


def test_success_rule_at_its_two_thresholds(lib):
    cal = lambda fc, vo, s2: lib.isvo_exr_calibrated(fc, vo, np.array([1.0, 0.5, s2, 0.0]).ctypes.data_as(xo._f64p))
    above = float(np.nextafter(0.25, 1))
    assert cal(8, 8, above) == 1 and cal(8, 8, 0.25) == 0 and cal(7, 8, above) == 0 and cal(9, 8, above) == 1
    assert cal(2, 2, above) == 1 and cal(1, 2, above) == 0 and cal(8, 8, float("nan")) == 0


def test_solve_against_numpy(lib):
    rng = np.random.default_rng(3)
    for rows in (4, 8, 32, 48):
        A = rng.normal(size=(rows, 4))
        s, ric = xo.solve(lib, A)
        U, S, Vt = np.linalg.svd(A)
        assert np.abs(s - S).max() < 1e-12
        x = Vt[3]
        want = np.linalg.inv(xo.q_to_R(lib, [x[3], x[0], x[1], x[2]]))
        assert np.abs(ric - want).max() < 1e-9 / (S[2] - S[3])


def test_tie_rule(lib):
    ch = lambda f, n: lib.isvo_exr_choose(np.array(f, np.int32).ctypes.data_as(xo._i32p), n)
    assert ch([5, 0, 0, 5], 10) == 2 and ch([5, 0, 4, 0], 10) == 1 and ch([0, 5, 4, 4], 10) == 1 and ch([0, 0, 0, 0], 10) == 2 and ch([3, 4, 0, 5], 9) == 2


def test_the_table_reaches_its_edges(lib, table, sequences):
    r = {n: v[0] for n, v in table.items()}
    assert all(x.status == OK and x.frame_count == 1 for x in r.values())
    assert [r[n].method for n in ("n0", "n8_identity", "n9_lmeds", "n14_lmeds", "n15_ransac", "n150")] == [0, 0, 1, 1, 2, 2]
    for n in ("n0", "n8_identity"):                            # X5: identity, the frame counts
        assert np.array_equal(np.array(r[n].Rc).reshape(3, 3), np.eye(3)) and r[n].choice == 0 and r[n].iters == 0
    assert r["n9_lmeds"].iters == r["n14_lmeds"].iters == 300 > 3
    for n in ("n15_ransac", "n63", "n64", "n65", "n129", "n150", "n150_mismatch"):
        # X2: at a threshold of 3.0 the first model keeps every point and niters falls to 0
        assert r[n].iters == 1 and r[n].best_inliers == len(xc.CASES[n].corres) and table[n][1].keep_iter == 0
    assert r["negated"].negated == 1 and table["negated"][1].det_first + 1.0 < 1e-9
    assert r["not_negated"].negated == 0 and table["not_negated"][1].det_first > 0
    f = r["tie"].front
    assert max(f[0], f[1]) == max(f[2], f[3]) > 0 and r["tie"].choice == 2
    assert any(x.choice == 1 for x in r.values()) and any(x.choice == 2 for x in r.values())
    pt = r["pure_translation"]
    assert np.abs(np.array(pt.Rc).reshape(3, 3) - np.eye(3)).max() < 1e-6 and pt.calibrated == 0 and pt.singular[0] < 1e-6
    assert r["huber_over"].angle_deg > 5 and r["huber_over"].huber == 5.0 / r["huber_over"].angle_deg < 1
    assert 4.5 < r["huber_under"].angle_deg < 5 and r["huber_under"].huber == 1.0
    assert sum(x.front[k] for x in r.values() for k in range(4)) > 500
    e = sequences["excited"]
    assert [x.calibrated for x in e[:7]] == [0] * 7 and e[6].singular[2] > 0.25 and e[7].calibrated == 1 and e[7].frame_count == 8
    o = sequences["one_axis"]
    assert all(x.calibrated == 0 and x.status == OK for x in o) and all(x.singular[2] < 0.25 for x in o[7:]) and o[9].frame_count == 10
    v = sequences["vo2"]
    assert [x.calibrated for x in v] == [0, 1, 1]
    fl = sequences["fill"]
    assert [x.status for x in fl] == [OK] * 8 + [CAPACITY] and fl[8].frame_count == 8


def test_front_counts_do_not_depend_on_the_float32_reading(lib, table, sequences):
    """X4's exact rounding sequence is restated, not checked: no scene here has a depth near zero, so the counts are the same with the
    triangulation test kept in doubles"""
    frames = list(xc.CASES.items()) + [(f"{n}[{k}]", fr) for n, sq in xc.SEQUENCES.items() for k, fr in enumerate(sq.frames)]
    for n, fr in frames:
        a = xo.calibrate_batch(lib, xo.Slots(exr.make_config(**xc.CFG)), [fr.item(0)])[0]
        with xo.quirks_off(lib, xo.DOUBLE_TRIANGULATION):
            b = xo.calibrate_batch(lib, xo.Slots(exr.make_config(**xc.CFG)), [fr.item(0)])[0]
        assert list(a.front) == list(b.front) and a.choice == b.choice, n


def test_each_hook_changes_a_named_case(lib, table):
    def run(name, mask):
        with xo.quirks_off(lib, mask):
            r = xo.calibrate_batch(lib, xo.Slots(exr.make_config(**xc.CFG)), [xc.CASES[name].item(0)])[0]
            return r, xo.last(lib)
    # X1: the estimator sees the double correspondences: another F, another Rc
    r, L = run("n150", xo.DOUBLE_POINTS)
    assert not np.array_equal(L.F, table["n150"][1].F) and xo.key_of(r) != xo.key_of(table["n150"][0])
    assert np.abs(np.array(r.Rc).reshape(3, 3) - xc.CASES["n150"].Rc_true).max() < np.abs(np.array(table["n150"][0].Rc).reshape(3, 3) - xc.CASES["n150"].Rc_true).max()
    # X4: the triangulation test stays double.  The issue asks for a named case that the hook changes, and it also rules that no
    # scene may depend on the float32 reading; both cannot hold for a table case, so the counts of the table are shown NOT to move
    # (above and below) and the hook is shown on points at infinity of n150's kept R1: there the depth's sign is rounding's, and
    # the float32 camera and point round it differently.  The points are searched for, not stored (R1 depends on the host's libm to an
    # ulp, so a stored point could stop being one): about one in ten moves, and 4000 are tried.
    L0 = table["n150"][1]
    pts = xc.CASES["n150"].corres.astype(np.float32).astype(np.float64)
    P = lambda R, t: (np.ascontiguousarray(R).ctypes.data_as(xo._f64p), np.ascontiguousarray(t).ctypes.data_as(xo._f64p))

    def counts(mask, q, n):
        with xo.quirks_off(lib, mask):
            return tuple(lib.isvo_exr_front_count(*P(R, L0.t), sg, n, q.ctypes.data_as(xo._f64p)) for R in (L0.R1, L0.R2) for sg in (1.0, -1.0))
    assert counts(0, pts, 150) == counts(xo.DOUBLE_TRIANGULATION, pts, 150) == tuple(table["n150"][0].front)
    rng = np.random.default_rng(0)
    moved = 0
    for _ in range(4000):
        x, y = rng.uniform(-0.5, 0.5), rng.uniform(-0.35, 0.35)
        v = L0.R1 @ np.array([x, y, 1.0])
        far = np.array([[x, y, v[0] / v[2], v[1] / v[2]]]).astype(np.float32).astype(np.float64)
        moved += counts(0, far, 1) != counts(xo.DOUBLE_TRIANGULATION, far, 1)
    print(f"X4: {moved} of 4000 points at infinity change a front count with the triangulation kept in doubles")
    assert moved >= 20


def test_configuration_refusals(lib):
    ok = lambda **kw: lib.isvo_exr_check_config(C.byref(exr.make_config(**dict(xc.CFG, **kw))))
    assert ok() == 1 and ok(max_slots=1, max_frames=8, max_corres=9, vo_size=2) == 1 and ok(max_slots=65535, max_frames=1024, max_corres=4096) == 1
    for bad in (dict(max_slots=0), dict(max_slots=65536), dict(max_frames=7), dict(max_frames=1025), dict(max_corres=8), dict(max_corres=4097),
                dict(vo_size=1), dict(vo_size=0), dict(max_slots=-1)):
        assert ok(**bad) == 0, bad
    assert lib.isvo_exr_check_config(None) == 0


def test_item_refusals_leave_the_slot_untouched(lib):
    cfg = exr.make_config(**dict(xc.CFG, max_frames=8, max_slots=6))
    S = xo.Slots(cfg)
    fr, frames = xc.CASES["n15_ransac"], xc.SEQUENCES["fill"].frames
    for f in frames[:8]:
        xo.calibrate_batch(lib, S, [f.item(5)])
    xo.calibrate_batch(lib, S, [frames[0].item(s) for s in (1, 2, 3)])
    before = [S.state_bytes(s) for s in range(6)]
    bad = lambda **kw: exr.ExrItem(kw.get("slot", 1), kw.get("corres", fr.corres), kw.get("dq", fr.dq))
    nan, inf = fr.corres.copy(), fr.corres.copy()
    nan[14, 3] = np.nan; inf[0, 0] = -np.inf
    neg = bad(); neg.c.n_corres = -1
    null = bad(); null.c.corres = None
    items = [bad(corres=nan), bad(slot=2, corres=inf), bad(slot=3, dq=(0, 0, 0, 0)), bad(slot=3), bad(slot=-1), bad(slot=6),
             bad(slot=4, corres=np.zeros((161, 4))), frames[8].item(5), bad(slot=0, dq=(np.nan, 0, 0, 1))]
    res = xo.calibrate_batch(lib, S, items)
    assert [r.status for r in res] == [INPUT, INPUT, INPUT, INPUT, INPUT, INPUT, CAPACITY, CAPACITY, INPUT]
    assert [r.frame_count for r in res] == [1, 1, 1, 1, -1, -1, 0, 8, 0]
    assert all(not xo.doubles_of(r).any() and r.method == 0 and r.calibrated == 0 for r in res)
    assert [S.state_bytes(s) for s in range(6)] == before
    for it in (neg, null):
        assert xo.calibrate_batch(lib, S, [it])[0].status == INPUT
    # a refused item does not stop the batch, and a good item's result does not depend on its neighbours
    solo = xo.calibrate_batch(lib, xo.Slots(cfg), [fr.item(0)])[0]
    mixed = xo.calibrate_batch(lib, S, [bad(corres=nan), fr.item(0), fr.item(0), bad(slot=9)])
    assert [r.status for r in mixed] == [INPUT, OK, INPUT, INPUT] and xo.key_of(mixed[1]) == xo.key_of(solo)
    assert mixed[2].frame_count == 1                           # the duplicate reports the slot's count after the call
    # no correspondences and a null pointer: a good item (X5)
    empty = exr.ExrItem(4, np.zeros((0, 4)), fr.dq); empty.c.corres = None
    assert xo.calibrate_batch(lib, S, [empty])[0].status == OK


def test_no_model_leaves_the_slot_untouched(lib):
    """ISV_EXR_NO_MODEL needs an estimator that keeps nothing: all-zero correspondences give a 7-point system without a model in
    every subset, under RANSAC (>= 15) and under LMedS (9 .. 14).  The slot holds two frames before: nothing of it moves, the result is
    zero apart from status and frame_count, the batch goes on, and the next good frame is the slot's third."""
    S = xo.Slots(exr.make_config(**xc.CFG))
    frames = xc.SEQUENCES["excited"].frames
    for fr in frames[:2]:
        assert xo.calibrate_batch(lib, S, [fr.item(3)])[0].status == OK
    before = S.state_bytes(3)
    for n in (9, 12, 14, 15, 20, 65, 160):
        res = xo.calibrate_batch(lib, S, [xc.CASES["n63"].item(0), exr.ExrItem(3, np.zeros((n, 4)), frames[2].dq), xc.CASES["n63"].item(1)])
        S.reset([0, 1])
        r = res[1]
        assert [x.status for x in res] == [OK, NO_MODEL, OK], n
        assert r.frame_count == 2 and not xo.doubles_of(r).any() and not any(r.front), n
        assert (r.method, r.iters, r.best_inliers, r.negated, r.choice, r.calibrated) == (0, 0, 0, 0, 0, 0), n
        assert S.state_bytes(3) == before, n
        assert xo.key_of(res[0]) == xo.key_of(res[2])
    third = xo.calibrate_batch(lib, S, [frames[2].item(3)])[0]
    assert third.status == OK and third.frame_count == 3
