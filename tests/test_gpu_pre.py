"""The batched IMU pre-integration on the MI355X (include/isvins_preint.h, k_pre_integrate) against its serial restatement
(tests/native/isv_pre_oracle.c), bit for bit: status, n_buffered, every double of the result and the full record of every table case
(tests/pre_cases.py) alone; GPU against GPU, the cases in one shuffled batch, in a batch padded to 130 items and in batches of 1 and 5;
the scenarios that carry state across calls (split pushes, repropagate, merge, a reset on a used slot), call by call against the
restatement; every refusal between two good items with the refused slots read back untouched; an empty call and the timing contract."""
import numpy as np
import pytest

import pre_cases as pc
import pre_oracle as po
from isvins_amd import preint as pre

pytestmark = pytest.mark.gpu
OK, CAPACITY, INPUT, UNSET = pc.OK, pc.CAPACITY, pc.INPUT, pc.UNSET
NAMES = list(pc.CASES)


@pytest.fixture(scope="module")
def lib():
    return po.load()


@pytest.fixture(scope="module")
def gpu():
    g = pre.PreIntegrator(140, **pc.CFG)
    yield g
    g.close()


def keys(out):
    res, recs = out
    return [po.key_of(r, c) for r, c in zip(res, recs)]


@pytest.fixture(scope="module")
def alone(lib, gpu):
    """every case in a call of its own: name -> its key on the GPU, equal to the restatement's"""
    st = po.Store(lib, gpu.cfg)
    out = {}
    for i, n in enumerate(NAMES):
        (got,), (ref,) = keys(gpu.run_batch([pc.CASES[n].item(i)])), keys(st.run_batch([pc.CASES[n].item(i)]))
        assert got == ref, n
        out[n] = got
    st.close()
    return out


def test_every_case_alone_matches_the_restatement(alone):
    for n, (res, rec) in alone.items():
        c = pc.CASES[n]
        r = pre.isv_pre_result_t.from_buffer_copy(res)
        assert (r.status, r.n_buffered) == (OK, c.n), n
        assert (rec is not None) == c.want_record and bool(np.array(r.R).any()) == c.nav, n
        assert np.isfinite(np.frombuffer(res[8:], np.float64)).all() and (rec is None or np.isfinite(np.frombuffer(rec, np.float64)).all()), n
    assert alone["n10"][1] == alone["n10_record_only"][1] and alone["n10"][0] == alone["n10_nav_only"][0]
    assert alone["big_rotation"] != alone["n10"] and alone["zero_gyro"] != alone["n10"]


def test_batches_shuffled_padded_and_small_are_bitwise(gpu, alone):
    rng = np.random.default_rng(11)
    order = [NAMES[k] for k in rng.permutation(len(NAMES))]
    assert keys(gpu.run_batch([pc.CASES[n].item(20 + i) for i, n in enumerate(order)])) == [alone[n] for n in order]
    padded = [NAMES[k % len(NAMES)] for k in rng.permutation(130)]
    assert keys(gpu.run_batch([pc.CASES[n].item(i) for i, n in enumerate(padded)])) == [alone[n] for n in padded]
    for size in (1, 5):
        some = order[:size]
        assert keys(gpu.run_batch([pc.CASES[n].item(60 + i) for i, n in enumerate(some)])) == [alone[n] for n in some]
    assert gpu.run_batch([]) == ([], [])


def test_state_across_calls_matches_the_restatement(lib, gpu):
    st = po.Store(lib, gpu.cfg)
    last = {}
    for k, name in enumerate(pc.SCENARIOS):
        got, ref = pc.play(gpu, name, 100 + 2 * k), pc.play(st, name, 100 + 2 * k)
        assert [keys(c) for c in got] == [keys(c) for c in ref], name
        assert all(r.status == OK for res, _ in got for r in res), name
        last[name] = keys(got[-1])[0]
    for a, b in pc.EQUAL:
        assert last[a] == last[b], (a, b)
    # all scenarios again in one batch per call, on other slots, interleaved at their different call numbers
    names = list(pc.SCENARIOS)
    for call in range(2):
        batch = [(n, pc.SCENARIOS[n][call](100 + 2 * ((k + 5) % len(names)))) for k, n in enumerate(names) if call < len(pc.SCENARIOS[n])]
        out = keys(gpu.run_batch([it for _, items in batch for it in items]))
        at = 0
        for n, items in batch:
            if call == len(pc.SCENARIOS[n]) - 1:
                assert out[at] == last[n], n
            at += len(items)
    st.close()


def read_back(runner, slots):
    """each slot through a no-op PUSH (n_samples = 0, no reset) with want_record"""
    return keys(runner.run_batch([pre.push(s, want_record=True) for s in slots]))


def test_refused_items_between_good_ones(lib, alone):
    S = 12
    g = pre.PreIntegrator(S, **pc.CFG)
    st = po.Store(lib, g.cfg)
    pc.prepare(g); pc.prepare(st)
    before = read_back(g, range(6))
    assert before == read_back(st, range(6)) and [pre.isv_pre_result_t.from_buffer_copy(k[0]).status for k in before] == [OK] * 4 + [UNSET] * 2
    good = lambda slot: pc.CASES["n10"].item(slot)
    for label, item, status in pc.refusals(S):
        got = g.run_batch([good(8), item, good(9)])
        assert [r.status for r in got[0]] == [OK, status, OK], label
        assert got[0][1].n_buffered == pc.PREPARED.get(item.c.slot, -1) and got[1][1] is None, label
        k = keys(got)
        assert k[0] == k[2] == alone["n10"], label
        assert k[1] == keys(st.run_batch([item]))[0], label
    assert read_back(g, range(6)) == before
    # the buffers behind the records are untouched too: repropagate rebuilds each record from its slot's buffer
    same = [pre.repropagate(0, pc.A.ba, pc.A.bg, want_record=True), pre.repropagate(1, pc.B.ba, pc.B.bg, want_record=True)]
    assert keys(g.run_batch(same)) == before[:2]
    # the rules between the items of one call, against the restatement
    B = pc.B
    for call in ([B.item(4), good(8), B.item(4)], [pre.push(6, B.dt, B.acc, B.gyr), good(8), pre.push(6, reset=True)],
                 [pre.merge(0, 1), good(8), pre.repropagate(1, B.ba, B.bg)], [pre.repropagate(1, B.ba, B.bg), pre.merge(0, 1), good(8)],
                 [pre.merge(0, 1), pre.push(1, [np.nan], np.zeros((1, 3)), np.zeros((1, 3))), good(8)], [pre.merge(0, 1, want_record=True), pre.merge(2, 1, want_record=True)]):
        a, b = g.run_batch(call), st.run_batch(call)
        assert keys(a) == keys(b), [r.status for r in a[0]]
    assert [r.status for r in a[0]] == [OK, OK] and [r.n_buffered for r in a[0]] == [14, 4]
    assert read_back(g, range(8)) == read_back(st, range(8))
    with pytest.raises(Exception):
        g.run_batch([pre.push(7, reset=True)] * (pc.CFG["max_items"] + 1))
    g.close(); st.close()


def test_empty_calls_and_the_timing_contract():
    g = pre.PreIntegrator(2, **pc.CFG)
    assert g.last_ms() == (0.0, 0.0, 0.0)
    assert g.run_batch([]) == ([], []) and g.last_ms() == (0.0, 0.0, 0.0)
    res, recs = g.run_batch([pre.push(-1, reset=True)])                    # no good item: nothing is launched
    assert res[0].status == INPUT and recs == [None] and g.last_ms() == (0.0, 0.0, 0.0)
    assert g.run_batch([pc.CASES["n65"].item(0)])[0][0].status == OK
    whole, kernel, upload = g.last_ms()
    assert whole >= kernel > 0.0 and whole >= upload >= 0.0
    g.run_batch([pre.push(1)])                                             # UNSET
    assert g.last_ms() == (whole, kernel, upload)                          # a call that launched nothing leaves the last call's times
    g.close()
