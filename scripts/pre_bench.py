"""Throughput of the batched IMU pre-integration (include/isvins_preint.h): 512 and 2048 reset PUSH items of 10 samples with the nav
state in one call, without and with the record copied back (want_record), one such item alone, 2048 REPROPAGATE items over 10
buffered samples, the last_ms split of each, and as the CPU figure the window manager's PreIntegration::push_back per sample on one
host core, through isv_estimator_process_imu_n on an estimator created with the oracle solver seam.  The median of --repeats calls
after two warm-ups; the first 8 items of every batch are compared bit for bit with the restatement (tests/native/isv_pre_oracle.c).
Prints one JSON line per run.

    python scripts/pre_bench.py [--repeats 7] [--samples 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isvins_loader  # noqa: E402

isvins_loader.load()
from isvins_amd import abi, preint as pre  # noqa: E402


def median_run(call, last_ms, repeats):
    """two warm-ups, then the run with the median call time: (python wall ms,) + last_ms()"""
    runs = []
    for r in range(repeats + 2):
        t0 = time.perf_counter()
        call()
        if r >= 2:
            runs.append(((time.perf_counter() - t0) * 1e3,) + last_ms())
    runs.sort(key=lambda x: x[1])
    return runs[len(runs) // 2]


def host_push_back_us(n_samples=20000):
    """microseconds per sample of the window manager's push_back with processIMU's propagation, one core"""
    import oracle_lib
    import sequence_harness as sh
    from isvins_amd import estimator as E
    oracle = oracle_lib.load()
    cfg = abi.make_config(11, 5, max_landmarks=100, max_obs=1100, max_batch=1)
    est = E.SequenceEstimator(sh.estimator_params(cfg), 1, solver=sh.oracle_vtbl(oracle, cfg))
    est.process_imu(0, 0.005, [0.1, -0.2, 9.7], [0.01, 0.02, -0.01])      # frame 0 takes no IMU; one image moves on to frame 1
    est.push_image(0, 0.0, np.arange(30, dtype=np.int32), np.tile([0.1, 0.2, 1.0], (30, 1))); est.step()
    rng = np.random.default_rng(5)
    dt, acc, gyr = rng.uniform(0.002, 0.01, n_samples), rng.normal(0, 2.0, (n_samples, 3)) + [0, 0, 9.8], rng.normal(0, 0.5, (n_samples, 3))
    est.process_imu_n(0, dt[:100], acc[:100], gyr[:100])
    t0 = time.perf_counter()
    est.process_imu_n(0, dt, acc, gyr)
    us = (time.perf_counter() - t0) * 1e6 / n_samples
    est.close()
    return us


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=10)
    args = ap.parse_args()
    import pre_cases
    import pre_oracle
    lib = pre_oracle.load()
    n_max, K = 2048, args.samples
    g = pre.PreIntegrator(n_max, max_samples=max(K, 16), max_items=n_max)
    st = pre_oracle.Store(lib, g.cfg)
    cases = [pre_cases.Case(K, 500 + s, want_record=False) for s in range(32)]
    host_us = host_push_back_us()
    runs = [("push", 512, False), ("push", 2048, False), ("push_want_record", 512, True), ("push_want_record", 2048, True), ("push_one", 1, False),
            ("repropagate", 2048, False)]
    for label, n, rec in runs:
        if label == "repropagate":                 # over the samples the last PUSH run left in the slots
            items = [pre.repropagate(i, cases[i % 32].ba + 0.01, cases[i % 32].bg - 0.001, want_record=rec) for i in range(n)]
        else:
            items = [cases[i % 32].item(i, want_record=rec) for i in range(n)]
        got, ref = g.run_batch(items), st.run_batch(items[:8])
        for i in range(min(n, 8)):
            assert pre_oracle.key_of(got[0][i], got[1][i]) == pre_oracle.key_of(ref[0][i], ref[1][i]), (label, i)
        wall, call, kernel, upload = median_run(lambda: g.run_batch(items), g.last_ms, args.repeats)
        print(json.dumps(dict(
            run=label, items=n, samples_per_item=K, call_ms=round(call, 3), k_pre_integrate_ms=round(kernel, 4), upload_ms=round(upload, 3),
            python_wall_ms=round(wall, 3), kernel_ns_per_sample=round(1e6 * kernel / (n * K), 1), call_us_per_sample=round(1e3 * call / (n * K), 3),
            items_per_s=round(1e3 * n / call, 1), host_push_back_us_per_sample=round(host_us, 3),
            host_one_core_ms_for_the_batch=round(host_us * n * K / 1e3, 3))), flush=True)
    st.close()
    g.close()
