"""Throughput of the batched feature detection (include/isvins_detect.h) at 752 x 480 for 1, 64 and 512 slots per call, in two
cases: the steady state (about 100 surviving points, max_new = 50) and the first frame (no points, max_new = 150).  The images are
resident in the tracker's slots, so a call uploads the points only.  Per case and batch size: the median of 5 calls after two
warm-ups, the per-kernel split from isv_det_last_ms, the candidate counts per image, and the serial restatement
(tests/native/isv_det_oracle.c) on one host core as the CPU figure; the first 8 items are compared byte for byte with it.  Prints
one JSON line per case and batch size.

    python scripts/det_bench.py [--slots 1,64,512] [--repeats 5]
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
from isvins_amd import detect as det, tracker as trk  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,512")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    W, H, K = 752, 480, 8
    images = [trk.analytic_image(W, H, (0.0, 0.0), 300 + i) for i in range(K)]
    rng = np.random.Generator(np.random.PCG64(2))
    # about 100 surviving points: 100 drawn, those inside an earlier one's disc are dropped by setMask as in the reference
    points = [np.column_stack([rng.uniform(1, W - 2, 100), rng.uniform(1, H - 2, 100)]).astype(np.float32) for _ in range(K)]
    counts = [rng.integers(1, 30, 100).astype(np.int32) for _ in range(K)]
    cases = {"steady": lambda s, i: det.DetItem(s, points[i], counts[i], 50), "first_frame": lambda s, i: det.DetItem(s, None, None, det.MAX_CNT)}
    import det_oracle
    lib = det_oracle.load()
    tcfg, dcfg = trk.make_config(1, 1, W, H), det.make_config(1, 128, det.MAX_CNT, det.MIN_DIST, det.QUALITY)
    cpu, cpu_ms = {}, {}
    for name, make in cases.items():
        t0 = time.perf_counter()
        cpu[name] = [det_oracle.detect(lib, dcfg, tcfg, images[i], make(0, i)) for i in range(K)]
        cpu_ms[name] = (time.perf_counter() - t0) * 1e3 / K
    for n in [int(x) for x in args.slots.split(",")]:
        tr = trk.Tracker(n, n, W, H)
        tr.track_batch([trk.TrkItem(s, images[s % K], images[s % K]) for s in range(n)])      # the slots take their images
        dt = det.Detector(tr, n, max_points=128)
        for name, make in cases.items():
            items = [make(s, s % K) for s in range(n)]
            for _ in range(args.warmup):
                rs, arrs = dt.detect_batch(items)
            for i in range(min(n, K)):
                want = cpu[name][i]
                assert bytes(rs[i]) == bytes(want.r), (name, i, det_oracle.describe(rs[i]), det_oracle.describe(want.r))
                for f in ("kept_index", "new_pts", "new_un_pts"):
                    assert getattr(arrs[i], f).tobytes() == getattr(want.arrays, f).tobytes(), (name, i, f)
            runs = []
            for r in range(args.repeats):
                t0 = time.perf_counter()
                dt.detect_batch(items)
                runs.append(((time.perf_counter() - t0) * 1e3,) + dt.last_ms())
            runs.sort(key=lambda x: x[1])
            wall, call, eig, mask, select, transfer = runs[len(runs) // 2]
            print(json.dumps(dict(case=name, slots=n, python_call_ms=round(wall, 3), call_ms=round(call, 3), images_per_s=round(1e3 * n / call, 1),
                                  k_det_eig_ms=round(eig, 4), k_det_mask_ms=round(mask, 4), cand_select_ms=round(select, 4), transfers_ms=round(transfer, 4),
                                  kept_per_image=round(float(np.mean([r.n_kept for r in rs])), 1), new_per_image=round(float(np.mean([r.n_new for r in rs])), 1),
                                  candidates_per_image=round(float(np.mean([r.n_candidates for r in rs])), 1),
                                  cpu_restatement_ms_per_image=round(cpu_ms[name], 2), cpu_images_per_s=round(1e3 / cpu_ms[name], 1))), flush=True)
        dt.close()
        tr.close()
