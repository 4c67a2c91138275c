"""Throughput of the batched keyframe extraction (include/isvins_keyframe.h) at 752 x 480 for 1, 64 and 512 images per call:
keyframes per second, each kernel's milliseconds, the share of the call that is the upload, and the serial restatement
(tests/native/isv_kf_oracle.c) on one host core as the CPU figure.  Prints one JSON line per batch size.

    python scripts/kf_bench.py [--batches 1,64,512] [--repeats 5]
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
from isvins_amd import keyframe as kf  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,512")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=150)
    args = ap.parse_args()
    W, H = 752, 480
    images = [kf.make_image(100 + i, W, H, contrast=35) for i in range(8)]
    rng = np.random.Generator(np.random.PCG64(1))
    points = [np.column_stack([rng.uniform(0, W, args.points), rng.uniform(0, H, args.points)]).astype(np.float32) for _ in images]
    import kf_oracle
    lib = kf_oracle.load()
    cfg = kf.make_config(1, W, H, max_points=args.points)
    t0 = time.perf_counter()
    cpu = [kf_oracle.extract(lib, cfg, kf.KfItem(im, p))[0].n_keypoints for im, p in zip(images, points)]
    cpu_ms = (time.perf_counter() - t0) * 1e3 / len(images)
    for n in [int(x) for x in args.batches.split(",")]:
        ext = kf.KeyframeExtractor(n, W, H, max_points=args.points)
        items = [kf.KfItem(images[i % len(images)], points[i % len(images)]) for i in range(n)]
        rs, _ = ext.extract_batch(items)          # warm-up: the block's allocation
        assert [r.n_keypoints for r in rs[:len(images)]] == cpu[:n]
        runs = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ext.extract_batch(items)
            runs.append(((time.perf_counter() - t0) * 1e3,) + ext.last_ms())
        runs.sort()
        wall, call, blur, fast, select, brief, upload, pack = runs[len(runs) // 2]
        print(json.dumps(dict(images=n, corners_per_image=round(float(np.mean([r.n_keypoints for r in rs])), 1), python_call_ms=round(wall, 3),
                              call_ms=round(call, 3), keyframes_per_s=round(1e3 * n / call, 1), k_kf_blur_ms=round(blur, 4), k_kf_fast_ms=round(fast, 4),
                              k_kf_select_ms=round(select, 4), k_kf_brief_ms=round(brief, 4), upload_ms=round(upload, 3),
                              upload_share=round(upload / call, 3), host_pack_ms=round(pack, 3), host_pack_share=round(pack / call, 3), cpu_restatement_ms_per_image=round(cpu_ms, 2),
                              cpu_keyframes_per_s=round(1e3 / cpu_ms, 1))), flush=True)
        ext.close()
