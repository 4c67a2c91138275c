"""Throughput of the batched feature tracking (include/isvins_tracker.h) at 752 x 480 with 150 points per image for 1, 64 and 512
sequences per call, in the steady state (prev resident in the slot: one image uploaded and one pyramid built per frame): frames
per second, the pyramid kernels' and the tracking kernel's milliseconds, the upload and the host's packing, and the serial
restatement (tests/native/isv_trk_oracle.c) on one host core as the CPU figure.  Prints one JSON line per batch size.

    python scripts/trk_bench.py [--slots 1,64,512] [--repeats 5]
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
from isvins_amd import tracker as trk  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,512")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=150)
    args = ap.parse_args()
    W, H = 752, 480
    # eight sequences of three frames: a texture moving by a few pixels per frame
    shifts = [(0.0, 0.0), (3.3, -1.9), (7.1, -4.2)]
    seqs = [[trk.analytic_image(W, H, s, 200 + i) for s in shifts] for i in range(8)]
    rng = np.random.Generator(np.random.PCG64(1))
    points = [np.column_stack([rng.uniform(12, W - 12, args.points), rng.uniform(12, H - 12, args.points)]).astype(np.float32) for _ in seqs]
    import trk_oracle
    lib = trk_oracle.load()
    cfg = trk.make_config(1, 1, W, H, max_points=args.points)
    t0 = time.perf_counter()
    cpu = [trk_oracle.track(lib, cfg, trk.TrkItem(0, f[2], f[1], p)) for f, p in zip(seqs, points)]
    cpu_ms = (time.perf_counter() - t0) * 1e3 / len(seqs)
    for n in [int(x) for x in args.slots.split(",")]:
        tr = trk.Tracker(n, n, W, H, max_points=args.points)
        k = len(seqs)
        seed = [trk.TrkItem(i, seqs[i % k][0], seqs[i % k][0]) for i in range(n)]
        steady = [[trk.TrkItem(i, seqs[i % k][f], None, points[i % k]) for i in range(n)] for f in (1, 2)]
        tr.track_batch(seed)                      # the slots take frame 0; the block's allocation
        tr.track_batch(steady[0])
        rs, arrs = tr.track_batch(steady[1])
        for i in range(min(n, k)):                # frame 1 -> frame 2, prev resident: the restatement's bytes
            assert arrs[i].cur_pts.tobytes() == cpu[i].arrays.cur_pts.tobytes() and arrs[i].flags.tobytes() == cpu[i].arrays.flags.tobytes()
        runs = []
        for r in range(args.repeats):             # alternate the two frames: every call is a steady-state frame
            t0 = time.perf_counter()
            tr.track_batch(steady[r % 2])
            runs.append(((time.perf_counter() - t0) * 1e3,) + tr.last_ms())
        runs.sort(key=lambda x: x[1])
        wall, call, pyramid, track, upload, pack = runs[len(runs) // 2]
        print(json.dumps(dict(slots=n, points_per_image=args.points, kept_per_image=round(float(np.mean([r.n_kept for r in rs])), 1),
                              python_call_ms=round(wall, 3), call_ms=round(call, 3), frames_per_s=round(1e3 * n / call, 1), pyramid_ms=round(pyramid, 4),
                              k_trk_track_ms=round(track, 4), upload_ms=round(upload, 3), upload_share=round(upload / call, 3), host_pack_ms=round(pack, 3),
                              host_pack_share=round(pack / call, 3), cpu_restatement_ms_per_image=round(cpu_ms, 2), cpu_frames_per_s=round(1e3 / cpu_ms, 1))),
              flush=True)
        tr.close()
