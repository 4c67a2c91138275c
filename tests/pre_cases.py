"""The case table of the batched IMU pre-integration (include/isvins_preint.h), deterministic, fixed seeds: CASES are single reset
PUSH items at the smallest shapes at which k_pre_integrate can still go wrong (sample counts 0, 1, 2, 10, 64, 65 = one past a
wavefront's lanes, max_samples exactly; zero gyro, a rotation of about 1 rad per step, dt = 0; with and without the nav state and the
record copy); SCENARIOS are the operations that carry state from one call to the next, each a list of calls on slots counted from a
base slot.  Used by tests/test_pre_oracle.py on the restatement alone and by tests/test_gpu_pre.py on the GPU against it."""
import numpy as np

from isvins_amd import preint as pre

MAX_SAMPLES = 96
CFG = dict(max_samples=MAX_SAMPLES, max_items=256)         # max_slots is the test's


def samples(n, seed, motion="normal"):
    """dt [n], acc [n][3], gyr [n][3]; the first sample acc_0, gyr_0; the biases ba, bg"""
    rng = np.random.default_rng(seed)
    dt = rng.uniform(0.002, 0.01, n)
    acc = rng.normal(0, 2.0, (n, 3)) + [0, 0, 9.8]
    gyr = rng.normal(0, 0.5, (n, 3))
    acc_0, gyr_0 = rng.normal(0, 2.0, 3) + [0, 0, 9.8], rng.normal(0, 0.5, 3)
    ba, bg = rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)
    if motion == "zero_gyro":
        gyr[:] = 0.0; gyr_0[:] = 0.0; bg[:] = 0.0
    if motion == "big_rotation":                           # |w| dt about 1
        dt[:] = 0.01
        gyr = 100.0 * gyr / np.linalg.norm(gyr, axis=1, keepdims=True)
    if motion == "dt0":                                    # the EuRoC boundary sample, inside and at the end
        dt[n // 3] = 0.0; dt[-1] = 0.0
    return dt, acc, gyr, acc_0, gyr_0, ba, bg


def nav_state(seed):
    rng = np.random.default_rng(1000 + seed)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.linalg.det(Q)), rng.normal(0, 3.0, 3), rng.normal(0, 1.0, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)


class Case:
    def __init__(self, n, seed, motion="normal", nav=True, want_record=True):
        self.n, self.seed, self.motion, self.nav, self.want_record = n, seed, motion, nav, want_record
        self.dt, self.acc, self.gyr, self.acc_0, self.gyr_0, self.ba, self.bg = samples(n, seed, motion)

    def item(self, slot, lo=0, hi=None, reset=True, want_record=None, bg=None):
        """the reset PUSH of the case on `slot`; or of its samples [lo, hi) only, without the constructor where reset is False"""
        hi = self.n if hi is None else hi
        return pre.push(slot, self.dt[lo:hi], self.acc[lo:hi], self.gyr[lo:hi], reset=reset, acc_0=self.acc_0, gyr_0=self.gyr_0, ba=self.ba,
                        bg=self.bg if bg is None else bg, nav=nav_state(self.seed) if self.nav else None,
                        want_record=self.want_record if want_record is None else want_record)


CASES = {
    "n0": Case(0, 1), "n1": Case(1, 2), "n2": Case(2, 3), "n10": Case(10, 4), "n64": Case(64, 5), "n65": Case(65, 6), "n_max": Case(MAX_SAMPLES, 7),
    "zero_gyro": Case(10, 8, "zero_gyro"), "big_rotation": Case(10, 9, "big_rotation"), "dt0": Case(10, 10, "dt0"),
    "n10_plain": Case(10, 4, nav=False, want_record=False), "n10_nav_only": Case(10, 4, want_record=False), "n10_record_only": Case(10, 4, nav=False),
    "n0_plain": Case(0, 1, nav=False, want_record=False), "n65_plain": Case(65, 6, nav=False, want_record=False),
}

A, B = Case(10, 21, nav=False), Case(4, 22, nav=False)
BG2 = A.bg + [0.003, -0.002, 0.001]                        # repropagate's new gyroscope bias
BA2 = A.ba + [0.01, 0.02, -0.03]

# name -> calls; a call is a function of the base slot that gives the call's items
SCENARIOS = {
    "whole": [lambda s: [A.item(s)]],
    "split": [lambda s: [A.item(s, 0, 5)], lambda s: [A.item(s, 5, 10, reset=False)]],
    "repropagate_same": [lambda s: [A.item(s)], lambda s: [pre.repropagate(s, A.ba, A.bg, want_record=True)]],
    "repropagate_changed": [lambda s: [A.item(s)], lambda s: [pre.repropagate(s, BA2, BG2, want_record=True)]],
    "fresh_changed": [lambda s: [pre.push(s, A.dt, A.acc, A.gyr, reset=True, acc_0=A.acc_0, gyr_0=A.gyr_0, ba=BA2, bg=BG2, want_record=True)]],
    "repropagate_empty": [lambda s: [A.item(s, 0, 0)], lambda s: [pre.repropagate(s, BA2, BG2, want_record=True)]],
    "fresh_empty": [lambda s: [pre.push(s, reset=True, acc_0=A.acc_0, gyr_0=A.gyr_0, ba=BA2, bg=BG2, want_record=True)]],
    "merge": [lambda s: [A.item(s), B.item(s + 1)], lambda s: [pre.merge(s, s + 1, want_record=True)]],
    "pushed": [lambda s: [A.item(s)], lambda s: [pre.push(s, B.dt, B.acc, B.gyr, want_record=True)]],
    "merge_empty": [lambda s: [A.item(s), B.item(s + 1, 0, 0)], lambda s: [pre.merge(s, s + 1, want_record=True)]],
    "reset_used": [lambda s: [A.item(s)], lambda s: [B.item(s)]],
    "fresh_b": [lambda s: [B.item(s)]],
}
# scenarios whose last result and record are the same bits
EQUAL = [("whole", "split"), ("whole", "repropagate_same"), ("repropagate_changed", "fresh_changed"), ("repropagate_empty", "fresh_empty"),
         ("merge", "pushed"), ("whole", "merge_empty"), ("reset_used", "fresh_b")]


OK, CAPACITY, INPUT, UNSET = pre.ISV_PRE_OK, pre.ISV_PRE_CAPACITY, pre.ISV_PRE_INPUT, pre.ISV_PRE_UNSET
PREPARED = {0: 10, 1: 4, 2: 0, 3: MAX_SAMPLES}         # slot -> buffered samples after prepare()


def refusals(max_slots):
    """(label, the item on a store / handle set up by `prepare`, the status it gets): slots 0 and 1 hold 10 and 4 samples, slot 2 is
    constructed and empty, slot 3 is full, the others were never constructed"""
    nan = A.acc.copy(); nan[3, 1] = np.nan
    inf = A.dt.copy(); inf[0] = np.inf
    big = MAX_SAMPLES + 1
    null = A.item(4); null.c.gyr = None
    norec = A.item(4, want_record=True); norec.c.record = None
    badop = A.item(4); badop.c.op = 3
    neg = A.item(4); neg.c.n_samples = -1
    return [
        ("max_samples + 1", pre.push(4, np.full(big, 0.005), np.zeros((big, 3)), np.zeros((big, 3)), reset=True), CAPACITY),
        ("push over the cap", pre.push(3, [0.005], np.zeros((1, 3)), np.zeros((1, 3))), CAPACITY),
        ("merge over the cap", pre.merge(3, 1), CAPACITY),
        ("NaN sample", pre.push(0, A.dt, nan, A.gyr), INPUT),
        ("infinite dt", pre.push(4, inf, A.acc, A.gyr, reset=True), INPUT),
        ("NaN bias", pre.repropagate(0, (0, np.nan, 0), (0, 0, 0)), INPUT),
        ("NaN first sample", pre.push(4, reset=True, acc_0=(np.nan, 0, 0)), INPUT),
        ("infinite nav", pre.push(0, B.dt, B.acc, B.gyr, nav=(np.eye(3), (0, 0, np.inf), (0, 0, 0), (0, 0, 0), (0, 0, 0))), INPUT),
        ("n_samples < 0", neg, INPUT),
        ("null array", null, INPUT),
        ("want_record without a record", norec, INPUT),
        ("unknown op", badop, INPUT),
        ("slot -1", A.item(-1), INPUT),
        ("slot max_slots", A.item(max_slots), INPUT),
        ("merge from itself", pre.merge(0, 0), INPUT),
        ("merge from no such slot", pre.merge(0, max_slots), INPUT),
        ("push on an unconstructed slot", pre.push(5, B.dt, B.acc, B.gyr), UNSET),
        ("repropagate an unconstructed slot", pre.repropagate(5, (0, 0, 0), (0, 0, 0)), UNSET),
        ("merge into an unconstructed slot", pre.merge(5, 0), UNSET),
        ("merge from an unconstructed slot", pre.merge(0, 5), UNSET),
    ]


def prepare(runner):
    full = Case(MAX_SAMPLES, 31, nav=False, want_record=False)
    res, _ = runner.run_batch([A.item(0), B.item(1), A.item(2, 0, 0), full.item(3)])
    assert [(r.status, r.n_buffered) for r in res] == [(OK, 10), (OK, 4), (OK, 0), (OK, MAX_SAMPLES)]


def play(runner, name, base):
    """the scenario's calls on runner.run_batch -> the (results, records) of every call"""
    return [runner.run_batch(call(base)) for call in SCENARIOS[name]]
