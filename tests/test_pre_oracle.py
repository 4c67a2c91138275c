"""CPU checks of the pre-integration's serial restatement (tests/native/isv_pre_oracle.c, which runs the shared text
is-vins_amd/csrc/isv_preint.h): bit for bit against the window manager's host code (PreIntegration::push_back and processIMU's
propagation in isv_estimator.cpp) over 400 random samples, at 1e-12 against the oracle's dense restatement on the same stream, the
slot semantics (split pushes, repropagate, merge, dt = 0) and every refusal of the status list with the store's bytes unchanged."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import pre_cases as pc
import pre_oracle as po
import sequence_harness as sh
from isvins_amd import abi, backend, preint as pre

OK, CAPACITY, INPUT, UNSET = pre.ISV_PRE_OK, pre.ISV_PRE_CAPACITY, pre.ISV_PRE_INPUT, pre.ISV_PRE_UNSET
RECORD_FIELDS = ("delta_p", "delta_q", "delta_v", "linearized_ba", "linearized_bg", "sum_dt", "jacobian", "covariance")


@pytest.fixture(scope="module")
def lib():
    return po.load()


@pytest.fixture(scope="module")
def stream():
    """the 400 samples of tests/test_sequence.py::test_native_preintegration_matches_the_oracle through the window manager, once:
    frame 1's pre-integration and nav state as the host code leaves them, and what they started from"""
    backend.build()
    from isvins_amd import estimator as E
    oracle = oracle_lib.load()
    cfg = abi.make_config(11, 5, max_landmarks=100, max_obs=1100, max_batch=1)
    params = sh.estimator_params(cfg)
    est = E.SequenceEstimator(params, 1, solver=sh.oracle_vtbl(oracle, cfg))
    rng = np.random.default_rng(5)
    acc0, gyr0 = np.array([0.1, -0.2, 9.7]), np.array([0.01, 0.02, -0.01])
    est.process_imu(0, 0.005, acc0, gyr0)
    est.push_image(0, 0.0, np.arange(30, dtype=np.int32), np.tile([0.1, 0.2, 1.0], (30, 1))); est.step()
    w0 = est.window(0)
    dt = rng.uniform(0.002, 0.01, 400); acc = rng.normal(0, 2.0, (400, 3)) + [0, 0, 9.8]; gyr = rng.normal(0, 0.5, (400, 3))
    ref = sh.PreInt(oracle, acc0, gyr0, np.zeros(3), np.zeros(3))
    for i in range(400):
        est.process_imu(0, dt[i], acc[i], gyr[i]); ref.push_back(dt[i], acc[i], gyr[i])
    out = dict(got=est.preintegration(0, 1), w0=w0, w1=est.window(0), dt=dt, acc=acc, gyr=gyr, acc0=acc0, gyr0=gyr0, dense=ref.pod,
               cfg=pre.make_config(2, max_samples=400, max_items=4, acc_n=params.acc_n, gyr_n=params.gyr_n, acc_w=params.acc_w, gyr_w=params.gyr_w,
                                   gravity=list(params.cfg.gravity)))
    est.close()
    return out


@pytest.fixture(scope="module")
def restated(lib, stream):
    """the same stream through the restatement: one reset PUSH with the nav state"""
    s = stream
    assert not s["w0"]["Bas"][1].any() and not s["w0"]["Bgs"][1].any()
    st = po.Store(lib, s["cfg"])
    nav = (s["w0"]["Rs"][1], s["w0"]["Ps"][1], s["w0"]["Vs"][1], s["w0"]["Bas"][1], s["w0"]["Bgs"][1])
    (res,), (rec,) = st.run_batch([pre.push(1, s["dt"], s["acc"], s["gyr"], reset=True, acc_0=s["acc0"], gyr_0=s["gyr0"], nav=nav, want_record=True)])
    assert res.status == OK and res.n_buffered == 400
    return res, rec, st


def test_restatement_matches_the_window_manager_bitwise(stream, restated):
    res, rec, _ = restated
    got = stream["got"]
    for f in RECORD_FIELDS:
        a, b = np.array(getattr(got, f)), np.array(getattr(rec, f))
        assert a.tobytes() == b.tobytes(), (f, np.abs(a - b).max())
    w1 = stream["w1"]
    for name, a, b in (("Ps", w1["Ps"][1], res.P), ("Rs", w1["Rs"][1], res.R), ("Vs", w1["Vs"][1], res.V)):
        assert np.ascontiguousarray(a).tobytes() == np.array(b).tobytes(), name
    assert np.array(res.delta_p).tobytes() == np.array(got.delta_p).tobytes() and res.sum_dt == got.sum_dt
    assert np.abs(w1["Ps"][1] - stream["w0"]["Ps"][1]).max() > 0.1           # (the nav state moved)


def test_restatement_matches_the_oracles_dense_restatement(stream, restated):
    _, rec, _ = restated
    for f in RECORD_FIELDS:
        a, b = np.atleast_1d(np.array(getattr(rec, f))), np.atleast_1d(np.array(getattr(stream["dense"], f)))
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), f


def test_the_store_keeps_the_samples_and_the_first_sample(stream, restated):
    _, _, st = restated
    acc_0, gyr_0, lin_acc, lin_gyr, constructed, n = st.head(1)
    assert constructed == 1 and n == 400 and st.head(0)[4:] == (0, 0)
    assert np.array_equal(lin_acc, stream["acc0"]) and np.array_equal(lin_gyr, stream["gyr0"])
    assert np.array_equal(acc_0, stream["acc"][-1]) and np.array_equal(gyr_0, stream["gyr"][-1])
    assert np.array_equal(st.buffer(1), np.column_stack([stream["dt"], stream["acc"], stream["gyr"]]))


@pytest.fixture(scope="module")
def played(lib):
    """every scenario of the table on a store of its own: name -> the last call's (result, record) key"""
    out = {}
    for name in pc.SCENARIOS:
        st = po.Store(lib, pre.make_config(4, **pc.CFG))
        calls = pc.play(st, name, 1)
        assert all(r.status == OK for res, _ in calls for r in res), name
        out[name] = po.key_of(calls[-1][0][0], calls[-1][1][0])
        assert out[name][1] is not None
        st.close()
    return out


@pytest.mark.parametrize("a,b", pc.EQUAL)
def test_scenarios_that_give_the_same_bits(played, a, b):
    assert played[a] == played[b]


def test_scenarios_that_differ(played):
    assert played["repropagate_changed"] != played["whole"] and played["merge"] != played["whole"] and played["fresh_empty"] != played["whole"]


def test_the_constructor_record(lib):
    st = po.Store(lib, pre.make_config(2, **pc.CFG))
    (res,), (rec,) = st.run_batch([pre.push(0, reset=True, acc_0=(1, 2, 3), gyr_0=(4, 5, 6), ba=(0.1, 0.2, 0.3), bg=(0.4, 0.5, 0.6), want_record=True)])
    assert (res.status, res.n_buffered, res.sum_dt) == (OK, 0, 0.0)
    assert list(rec.delta_p) == [0, 0, 0] and list(rec.delta_q) == [0, 0, 0, 1] and list(rec.delta_v) == [0, 0, 0] and rec.sum_dt == 0
    assert list(rec.linearized_ba) == [0.1, 0.2, 0.3] and list(rec.linearized_bg) == [0.4, 0.5, 0.6]
    assert np.array_equal(np.array(rec.jacobian).reshape(15, 15), np.eye(15)) and not np.array(rec.covariance).any()
    assert not np.array(res.R).any()                                          # no nav state: zero
    h = st.head(0)
    assert list(h[0]) == list(h[2]) == [1, 2, 3] and list(h[1]) == list(h[3]) == [4, 5, 6] and h[4:] == (1, 0)


def test_a_sample_with_dt_zero(lib):
    c = pc.CASES["dt0"]
    st = po.Store(lib, pre.make_config(1, **pc.CFG))
    k = c.n // 3
    (before,), _ = st.run_batch([c.item(0, 0, k)])
    (after,), (rec,) = st.run_batch([c.item(0, k, k + 1, reset=False)])
    assert c.dt[k] == 0.0 and after.status == OK and after.n_buffered == k + 1
    assert after.sum_dt == before.sum_dt
    assert np.array_equal(np.array(after.delta_p), np.array(before.delta_p)) and np.array_equal(np.array(after.delta_v), np.array(before.delta_v))
    assert all(np.isfinite(np.array(getattr(rec, f))).all() for f in RECORD_FIELDS) and np.isfinite(np.array(after.R)).all()
    (whole,), (rec,) = st.run_batch([c.item(0)])
    assert whole.status == OK and all(np.isfinite(np.array(getattr(rec, f))).all() for f in RECORD_FIELDS)


def test_every_refusal_leaves_every_slot_untouched(lib):
    S = 8
    st = po.Store(lib, pre.make_config(S, **pc.CFG))
    pc.prepare(st)
    before = st.raw()
    for label, item, status in pc.refusals(S):
        (r,), (rec,) = st.run_batch([item])
        assert r.status == status, label
        want = pc.PREPARED.get(item.c.slot, -1)
        assert po.key_of(r)[0] == po.key_of(pre.isv_pre_result_t(status=status, n_buffered=want))[0], label   # zero apart from the two
        assert rec is None and st.raw() == before, label
    # the rules between the items of one call: a slot named twice (the second refused, also behind a refused first), a MERGE whose
    # source is another item's slot, before or behind it
    B = pc.B
    twice = [B.item(4, reset=True), B.item(4, reset=True)]
    res, _ = st.run_batch(twice)
    assert [r.status for r in res] == [OK, INPUT] and [r.n_buffered for r in res] == [4, 4]
    before = st.raw()
    res, _ = st.run_batch([pre.push(6, B.dt, B.acc, B.gyr), pre.push(6, reset=True)])
    assert [r.status for r in res] == [UNSET, INPUT] and [r.n_buffered for r in res] == [-1, -1] and st.raw() == before
    res, _ = st.run_batch([pre.merge(0, 1), pre.repropagate(1, (0, 0, 0), (0, 0, 0))])
    assert [r.status for r in res] == [INPUT, OK]
    res, _ = st.run_batch([pre.repropagate(1, B.ba, B.bg), pre.merge(0, 1)])
    assert [r.status for r in res] == [OK, INPUT]
    res, _ = st.run_batch([pre.merge(0, 1), pre.push(1, [np.nan], np.zeros((1, 3)), np.zeros((1, 3)))])      # a refused item names its slot too
    assert [r.status for r in res] == [INPUT, INPUT]
    assert st.head(0)[5] == 10 and np.array_equal(st.buffer(0), np.column_stack([pc.A.dt, pc.A.acc, pc.A.gyr]))
    # two MERGEs may share a source: it is only read
    res, _ = st.run_batch([pre.merge(0, 1), pre.merge(2, 1)])
    assert [(r.status, r.n_buffered) for r in res] == [(OK, 14), (OK, 4)]
    # the entry point's own refusals
    assert pre.run_on(lib.isvo_pre_run_batch, st.h, [pre.push(7, reset=True)] * (pc.CFG["max_items"] + 1))[0] == -1
    assert st.run_batch([]) == ([], [])
    st.close()


def test_config_checks(lib):
    assert lib.isvo_pre_check_config(C.byref(pre.make_config())) == 1
    for bad in po.BAD_CONFIGS:
        assert lib.isvo_pre_check_config(C.byref(pre.make_config(**bad))) == 0, bad
    for good in (dict(max_slots=pre.MAX_SLOTS), dict(max_samples=pre.MAX_SAMPLES), dict(max_items=pre.MAX_ITEMS), dict(acc_n=0.0, gyr_w=0.0)):
        assert lib.isvo_pre_check_config(C.byref(pre.make_config(**good))) == 1, good
