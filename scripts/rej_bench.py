"""Throughput of the batched outlier rejection (include/isvins_reject.h): 512 items of 150 points at 752 x 480 with about 10 % planted
outliers and 0.3 px noise in one call, one such item alone, one 14-point item alone (LMedS), the last_ms split of each, and the
serial restatement (tests/native/isv_rej_oracle.c) per item on one host core as the CPU figure.  The items of a batch are scenes of
different seeds, so their RANSAC iteration counts differ as they do between sequences.  The median of --repeats calls after two
warm-ups; the first 8 items of every batch are compared bit for bit with the restatement.  Prints one JSON line per batch.

    python scripts/rej_bench.py [--items 512] [--repeats 5]
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
from isvins_amd import reject as rej, tracker as trk  # noqa: E402


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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=150)
    ap.add_argument("--scenes", type=int, default=32, help="different scenes; the batch cycles through them")
    args = ap.parse_args()
    import rej_cases
    import rej_oracle
    lib = rej_oracle.load()
    W, H = rej_cases.WIDTH, rej_cases.HEIGHT
    tcfg = trk.make_config(1, 1, 64, 48, max_points=args.points)
    tr = trk.Tracker(1, 1, 64, 48, max_points=args.points)
    rj = rej.Rejector(tr, max_items=args.items)
    scenes = [rej_cases.scene(args.points, 300 + s, outliers=args.points // 10, noise=0.3) for s in range(args.scenes)]
    small = [rej_cases.scene(14, 400 + s, outliers=2, noise=0.3) for s in range(args.scenes)]
    for label, cases, n in (("batch", scenes, args.items), ("one", scenes, 1), ("one_lmeds", small, 1)):
        t0 = time.perf_counter()
        cpu = [rej_oracle.reject(lib, tcfg, rj.cfg, c.item()) for c in cases]
        cpu_ms = (time.perf_counter() - t0) * 1e3 / len(cases)
        items = [cases[i % len(cases)].item() for i in range(n)]
        rs, sts = rj.reject_batch(items)
        for i in range(min(n, 8)):
            assert rej_oracle.key_of(rs[i], sts[i]) == cpu[i].key(), (label, i)
        wall, call, kernel, upload, pack = median_run(lambda: rj.reject_batch(items), rj.last_ms, args.repeats)
        print(json.dumps(dict(
            run=label, items=n, points_per_item=len(cases[0].prev), method=("none", "lmeds", "ransac")[rs[0].method],
            mean_iters=round(float(np.mean([r.iters for r in rs])), 1), max_iters=int(max(r.iters for r in rs)),
            kept_per_item=round(float(np.mean([r.n_kept for r in rs])), 1), planted_outliers_kept=int(sum(int(st[c.planted].sum()) for st, c in zip(sts, cases))),
            call_ms=round(call, 3), k_rej_f_ms=round(kernel, 4), upload_ms=round(upload, 3), host_pack_ms=round(pack, 3), python_wall_ms=round(wall, 3),
            items_per_s=round(1e3 * n / call, 1), cpu_restatement_ms_per_item=round(cpu_ms, 3), cpu_items_per_s=round(1e3 / cpu_ms, 1))), flush=True)
    rj.close()
    tr.close()
