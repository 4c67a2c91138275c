"""Throughput of the batched camera-IMU rotation calibration (include/isvins_exrot.h): 512 sequences of 150 correspondences with 10 %
mismatches in one call, at frame counts 1, 8 and 32, and one sequence alone at the same frame counts.  Before every timed call the
slots are reset and brought to the frame count before it by calls that are not timed.  The serial restatement
(tests/native/isv_exr_oracle.c) per item on one host core is the CPU figure.  The median of --repeats calls after two warm-ups.
Prints one JSON line per run.

    python scripts/exr_bench.py [--sequences 512] [--repeats 5]
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
from isvins_amd import exrot as exr  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--corres", type=int, default=150)
    ap.add_argument("--scenes", type=int, default=32, help="different scenes per frame; the batch cycles through them")
    args = ap.parse_args()
    import exr_cases as xc
    import exr_oracle as xo
    lib = xo.load()
    max_frames = 32
    cfg = dict(max_slots=args.sequences, max_frames=max_frames, max_corres=args.corres, vo_size=8)
    cal = exr.Calibrator(**cfg)
    # scene[f][s]: frame f of scene s
    frames = [[xc.scene(1000 * f + s, args.corres, xc.AXES[(f + s) % len(xc.AXES)], 10.0, (0.2, -0.05, 0.08), mismatch=0.10)[:2] for s in range(args.scenes)]
              for f in range(max_frames)]

    def items_of(f, n):
        return [exr.ExrItem(i, *frames[f][i % args.scenes]) for i in range(n)]

    for label, n, at in (("batch", args.sequences, 1), ("batch", args.sequences, 8), ("batch", args.sequences, 32), ("one", 1, 1), ("one", 1, 8), ("one", 1, 32)):
        prefix = [items_of(f, n) for f in range(at - 1)]
        timed = items_of(at - 1, n)
        runs = []
        for r in range(args.repeats + 2):
            cal.reset(range(n))
            for it in prefix:
                cal.calibrate_batch(it)
            t0 = time.perf_counter()
            res = cal.calibrate_batch(timed)
            wall = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                runs.append((wall,) + cal.last_ms())
        assert all(x.status == exr.ISV_EXR_OK and x.frame_count == at for x in res)
        runs.sort(key=lambda x: x[1])
        wall, call, kernel = runs[len(runs) // 2]
        # the restatement on one core: the same frame count, the first scenes
        m = min(n, 8)
        S = xo.Slots(exr.make_config(**cfg))
        for it in prefix:
            xo.calibrate_batch(lib, S, it[:m])
        t0 = time.perf_counter()
        cpu = xo.calibrate_batch(lib, S, timed[:m])
        cpu_ms = (time.perf_counter() - t0) * 1e3 / m
        assert [x.frame_count for x in cpu] == [at] * m
        print(json.dumps(dict(
            run=label, sequences=n, frame_count=at, corres_per_item=args.corres, method=("none", "lmeds", "ransac")[res[0].method],
            mean_iters=round(float(np.mean([x.iters for x in res])), 1), calibrated=int(sum(x.calibrated for x in res)),
            call_ms=round(call, 3), k_exr_calibrate_ms=round(kernel, 4), python_wall_ms=round(wall, 3), items_per_s=round(1e3 * n / call, 1),
            front_counts_equal_to_cpu=f"{sum(list(a.front) == list(b.front) for a, b in zip(cpu, res[:m]))}/{m}",
            cpu_restatement_ms_per_item=round(cpu_ms, 3), cpu_items_per_s=round(1e3 / cpu_ms, 1))), flush=True)
    cal.close()
