"""The batched rotation calibration on the MI355X (include/isvins_exrot.h, k_exr_calibrate) against its serial restatement
(tests/native/isv_exr_oracle.c): every table case and every sequence frame by frame, the restatement starting each frame from the
slot state the GPU holds; the discrete fields and front[] exactly; the doubles and the slot history bitwise where the host's and the
device's libm agree (atan2 in a frame's angle, and through its weight in A; acos / cos / pow / log in the estimator), otherwise within
twice the case's high-precision bound (tests/exr_highprec.py, exr_cases.K), and which cases needed that is printed.  Then GPU against
GPU, bitwise: the sequences interleaved in one batch at different frame counts, shuffled, and padded to 130 items; a reset slot
replaying its sequence; refused items (INPUT, CAPACITY, a duplicate slot, NO_MODEL) between good ones with untouched slots; an empty call and the timing contract."""
import numpy as np
import pytest

import exr_cases as xc
import exr_highprec as hp
import exr_oracle as xo
from isvins_amd import exrot as exr
from test_exr_highprec import kept_model

pytestmark = pytest.mark.gpu
OK, CAPACITY, INPUT, NO_MODEL = exr.ISV_EXR_OK, exr.ISV_EXR_CAPACITY, exr.ISV_EXR_INPUT, exr.ISV_EXR_NO_MODEL
BIG = dict(xc.CFG, max_slots=170)


@pytest.fixture(scope="module")
def lib():
    return xo.load()


@pytest.fixture(scope="module")
def cal():
    c = exr.Calibrator(**BIG)
    yield c
    c.close()


def state_key(state):
    fc, ric, hist = state
    return fc, ric.tobytes(), hist.tobytes()


def compare(lib, where, frame, ref, got, ref_state, got_state, loose):
    """one frame's result and slot against the restatement's; notes in `loose` where the bits differed"""
    for f in xo.INT_FIELDS:
        assert getattr(ref, f) == getattr(got, f), (where, f, getattr(ref, f), getattr(got, f))
    assert list(ref.front) == list(got.front), where
    assert ref_state[0] == got_state[0], where
    if xo.key_of(ref) == xo.key_of(got) and state_key(ref_state) == state_key(got_state):
        return
    loose.append(where)
    assert ref.status == OK
    F = ref.frame_count
    # twice the high-precision bounds of this frame
    km = kept_model(lib, frame)
    tol_Rc = 2 * xc.K["Rc"] * hp.check_Rc(np.array(ref.Rc).reshape(3, 3), km[0])[1] if km is not None else 0.0
    tol_ang = 2 * xc.K["row"] * hp.EPS * max(ref.angle_deg, 180 / np.pi)
    sv = hp.check_svd(xo.build_A(lib, ref_state[2]), ref.singular, ref.ric)
    tol_sig, tol_ric = 2 * xc.K["sigma"] * sv["sigma"][1], 2 * xc.K["ric"] * sv["ric"][1]
    assert np.abs(np.array(ref.Rc) - np.array(got.Rc)).max() <= tol_Rc, where
    assert abs(ref.angle_deg - got.angle_deg) <= tol_ang and abs(ref.huber - got.huber) <= tol_ang / 5, where
    assert np.abs(np.array(ref.singular) - np.array(got.singular)).max() <= tol_sig, where
    assert np.abs(np.array(ref.ric) - np.array(got.ric)).max() <= tol_ric, where       # (inf for an undetermined vector)
    assert np.array_equal(np.array(got.ric).reshape(3, 3), got_state[1]), where
    # the history: earlier frames untouched, this frame's Rimu and Rc_g (no libm in them) bitwise, its Rc as the result's
    assert ref_state[2][:F - 1].tobytes() == got_state[2][:F - 1].tobytes(), where
    assert ref_state[2][F - 1, 1:].tobytes() == got_state[2][F - 1, 1:].tobytes(), where
    assert np.array_equal(got_state[2][F - 1, 0], np.array(got.Rc).reshape(3, 3)), where


def test_every_case_matches_the_restatement(lib, cal):
    names = list(xc.CASES)
    cal.reset(range(len(names)))
    S = xo.Slots(cal.cfg)
    items = [xc.CASES[n].item(i) for i, n in enumerate(names)]
    ref, got = xo.calibrate_batch(lib, S, items), cal.calibrate_batch(items)
    loose = []
    for i, n in enumerate(names):
        compare(lib, n, xc.CASES[n], ref[i], got[i], S.read_slot(i), cal.read_slot(i), loose)
    print(f"cases compared within twice the high-precision bound, not bitwise: {loose}")


@pytest.mark.parametrize("name", list(xc.SEQUENCES))
def test_every_sequence_matches_the_restatement_frame_by_frame(lib, name):
    sq = xc.SEQUENCES[name]
    g = exr.Calibrator(**sq.cfg)
    S = xo.Slots(g.cfg)
    loose, flags = [], []
    for f, fr in enumerate(sq.frames):
        before = g.read_slot(1)
        S.load_slot(1, before)                         # the restatement starts the frame from the GPU's slot
        ref, got = xo.calibrate_batch(lib, S, [fr.item(1)])[0], g.calibrate_batch([fr.item(1)])[0]
        after = g.read_slot(1)
        if ref.status != OK:
            assert state_key(before) == state_key(after)
        compare(lib, f"{name}[{f + 1}]", fr, ref, got, S.read_slot(1), after, loose)
        flags.append((got.status, got.calibrated))
    g.close()
    print(f"{name}: frames compared within twice the high-precision bound, not bitwise: {loose}")
    if name == "excited":
        assert flags[6] == (OK, 0) and flags[7] == (OK, 1)
    if name == "one_axis":
        assert all(fl == (OK, 0) for fl in flags)
    if name == "vo2":
        assert flags[0] == (OK, 0) and flags[1] == (OK, 1)
    if name == "fill":
        assert flags[7][0] == OK and flags[8] == (CAPACITY, 0)


def run_alone(cal, slot, frames):
    cal.reset([slot])
    return [xo.key_of(cal.calibrate_batch([fr.item(slot)])[0]) for fr in frames], state_key(cal.read_slot(slot))


def test_batching_interleaved_shuffled_and_padded_is_bitwise(cal):
    seqs = {20: xc.SEQUENCES["excited"].frames, 21: xc.SEQUENCES["one_axis"].frames, 22: list(xc.CASES.values())[:12]}
    start = {20: 0, 21: 2, 22: 1}                      # the call at which a sequence begins: different frame counts in one batch
    alone = {s: run_alone(cal, s, fr) for s, fr in seqs.items()}
    pad_frames = list(xc.CASES.values())
    rng = np.random.default_rng(7)
    for way in ("interleaved", "shuffled", "padded"):
        cal.reset(list(seqs))
        keys = {s: [] for s in seqs}
        for call in range(max(start[s] + len(seqs[s]) for s in seqs)):
            batch = [(s, seqs[s][call - start[s]]) for s in seqs if 0 <= call - start[s] < len(seqs[s])]
            if way == "padded":
                pads = list(range(30, 30 + 130 - len(batch)))
                cal.reset(pads)
                batch += [(p, pad_frames[(p + call) % len(pad_frames)]) for p in pads]
                assert len(batch) == 130
            if way != "interleaved":
                batch = [batch[k] for k in rng.permutation(len(batch))]
            res = cal.calibrate_batch([fr.item(s) for s, fr in batch])
            for (s, _), r in zip(batch, res):
                if s in keys:
                    keys[s].append(xo.key_of(r))
        for s in seqs:
            assert keys[s] == alone[s][0], (way, s)
            assert state_key(cal.read_slot(s)) == alone[s][1], (way, s)


def test_a_reset_slot_replays_its_sequence_to_the_same_bits(cal):
    frames = xc.SEQUENCES["excited"].frames
    first = run_alone(cal, 5, frames)
    assert cal.read_slot(5)[0] == len(frames)
    cal.reset([5])
    fc, ric, hist = cal.read_slot(5)
    assert fc == 0 and np.array_equal(ric, np.eye(3)) and len(hist) == 0
    assert run_alone(cal, 5, frames) == first
    assert run_alone(cal, 6, frames) == first          # and another slot gives the same bits


def test_refused_items_between_good_ones(lib, cal):
    fr = xc.CASES["n15_ransac"]
    good = lambda slot: xc.CASES["n63"].item(slot)
    nan = fr.corres.copy(); nan[3, 2] = np.nan
    full = exr.Calibrator(**dict(xc.CFG, max_frames=8, max_slots=3))
    for f in xc.SEQUENCES["fill"].frames[:8]:
        assert full.calibrate_batch([f.item(2)])[0].status == OK
    before_full = state_key(full.read_slot(2))
    r = full.calibrate_batch([good(0), xc.SEQUENCES["fill"].frames[8].item(2), good(1)])
    assert [x.status for x in r] == [OK, CAPACITY, OK] and r[1].frame_count == 8 and state_key(full.read_slot(2)) == before_full
    full.close()
    cal.reset(range(12))
    cal.calibrate_batch([xc.CASES["n9_lmeds"].item(s) for s in (2, 4, 6, 7, 8, 9)])      # slots with something to leave untouched
    items = [good(0), exr.ExrItem(2, nan, fr.dq), good(1), exr.ExrItem(4, np.zeros((161, 4)), fr.dq), good(3), good(3), exr.ExrItem(-1, fr.corres, fr.dq),
             exr.ExrItem(170, fr.corres, fr.dq), exr.ExrItem(6, fr.corres, (0, 0, 0, 0)), exr.ExrItem(7, fr.corres, (1, np.inf, 0, 0)), good(5),
             exr.ExrItem(8, np.zeros((20, 4)), fr.dq), good(10), exr.ExrItem(9, np.zeros((12, 4)), fr.dq), good(11)]      # no model: RANSAC, LMedS
    S = xo.Slots(cal.cfg)
    for s in range(12):
        S.load_slot(s, cal.read_slot(s))
    before = [state_key(cal.read_slot(s)) for s in range(12)]
    ref, got = xo.calibrate_batch(lib, S, items), cal.calibrate_batch(items)
    assert [r.status for r in got] == [OK, INPUT, OK, CAPACITY, OK, INPUT, INPUT, INPUT, INPUT, INPUT, OK, NO_MODEL, OK, NO_MODEL, OK]
    assert [r.frame_count for r in got] == [1, 1, 1, 1, 1, 1, -1, -1, 1, 1, 1, 1, 1, 1, 1]
    for a, b in zip(ref, got):
        assert [getattr(a, f) for f in xo.INT_FIELDS] == [getattr(b, f) for f in xo.INT_FIELDS]
        if b.status != OK:
            assert xo.key_of(a) == xo.key_of(b) and not xo.doubles_of(b).any()
    for s in (2, 4, 6, 7, 8, 9):
        assert state_key(cal.read_slot(s)) == before[s], s
    # the kernel's exit without a model left the host's mirror of the counts alone too: the next good frame is the slot's second
    assert [r.frame_count for r in cal.calibrate_batch([good(8), good(9)])] == [2, 2]
    solo = exr.Calibrator(**xc.CFG)                    # the good items are what they are alone
    assert xo.key_of(solo.calibrate_batch([good(0)])[0]) == xo.key_of(got[0]) == xo.key_of(got[2]) == xo.key_of(got[10]) == xo.key_of(got[12]) == xo.key_of(got[14])
    solo.close()


def test_empty_calls_and_the_timing_contract(cal):
    c = exr.Calibrator(**xc.CFG)
    assert c.last_ms() == (0.0, 0.0)
    assert c.calibrate_batch([]) == [] and c.last_ms() == (0.0, 0.0)
    r = c.calibrate_batch([exr.ExrItem(-1, np.zeros((0, 4)), (1, 0, 0, 0))])      # no good item: nothing is launched
    assert r[0].status == INPUT and c.last_ms() == (0.0, 0.0)
    c.reset([])
    assert c.calibrate_batch([xc.CASES["n150"].item(0)])[0].status == OK
    whole, kernel = c.last_ms()
    assert whole >= kernel > 0.0
    c.calibrate_batch([exr.ExrItem(-1, np.zeros((0, 4)), (1, 0, 0, 0))])
    assert c.last_ms() == (whole, kernel)              # a call that launched nothing leaves the last call's times
    with pytest.raises(Exception):
        c.reset([40])
    with pytest.raises(Exception):
        c.read_slot(-1)
    c.close()
