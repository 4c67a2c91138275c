"""Throughput of the batched CLAHE (include/isvins_equalize.h) at 752 x 480 with 150 points per image for 1, 64 and 512 sequences per
call, in the steady state (prev resident in the slot: one raw image uploaded, equalised and one pyramid built per frame):
isv_eq_track_batch beside isv_trk_track_batch on the same handle and images, the CLAHE kernels' milliseconds, isv_eq_apply_batch,
and the serial restatement (tests/native/isv_eq_oracle.c) on one host core as the CPU figure.  The median of --repeats calls after two warm-ups; the first 8 items are compared byte for byte with the
restatements.  Prints one JSON line per batch size.

    python scripts/eq_bench.py [--slots 1,64,512] [--repeats 5]
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
from isvins_amd import equalize as eq, tracker as trk  # noqa: E402


def median_run(call, last_ms, repeats):
    """two warm-ups, then the run with the median call time: (python wall ms,) + last_ms()"""
    runs = []
    for r in range(repeats + 2):
        t0 = time.perf_counter()
        call(r)
        if r >= 2:
            runs.append(((time.perf_counter() - t0) * 1e3,) + last_ms())
    runs.sort(key=lambda x: x[1])
    return runs[len(runs) // 2]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,64,512")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=150)
    args = ap.parse_args()
    W, H = 752, 480
    # eight sequences of three frames: a dark, low-contrast texture moving by a few pixels per frame
    shifts = [(0.0, 0.0), (3.3, -1.9), (7.1, -4.2)]
    seqs = [[(trk.analytic_image(W, H, s, 200 + i).astype(np.int32) // 3 + 12).astype(np.uint8) for s in shifts] for i in range(8)]
    rng = np.random.Generator(np.random.PCG64(1))
    points = [np.column_stack([rng.uniform(12, W - 12, args.points), rng.uniform(12, H - 12, args.points)]).astype(np.float32) for _ in seqs]
    import eq_oracle
    import trk_oracle
    elib, tlib = eq_oracle.load(), trk_oracle.load()
    cfg, ecfg = trk.make_config(1, 1, W, H, max_points=args.points), eq.make_config()
    t0 = time.perf_counter()
    restated = [[eq_oracle.apply(elib, ecfg, f) for f in fs] for fs in seqs]
    cpu_ms = (time.perf_counter() - t0) * 1e3 / (3 * len(seqs))
    clipped = np.mean([r.counters["clipped"] for rs in restated for r in rs])
    cpu = [trk_oracle.track(tlib, cfg, trk.TrkItem(0, r[2].out, r[1].out, p)) for r, p in zip(restated, points)]
    k = len(seqs)
    for n in [int(x) for x in args.slots.split(",")]:
        tr = trk.Tracker(n, n, W, H, max_points=args.points)
        e = eq.Equalizer(tr)
        seed = [trk.TrkItem(i, seqs[i % k][0], seqs[i % k][0]) for i in range(n)]
        steady = [[trk.TrkItem(i, seqs[i % k][f], None, points[i % k]) for i in range(n)] for f in (1, 2)]
        out = dict(slots=n, points_per_image=args.points, clipped_tiles_per_image=round(float(clipped), 1))
        # the tracker's own call on the raw images: every call is a steady-state frame, the two frames alternate
        tr.track_batch(seed)
        wall, call, pyramid, track, upload, pack = median_run(lambda r: tr.track_batch(steady[r % 2]), tr.last_ms, args.repeats)
        out.update(trk_call_ms=round(call, 3), trk_pyramid_ms=round(pyramid, 4), trk_k_trk_track_ms=round(track, 4), trk_upload_ms=round(upload, 3),
                   trk_host_pack_ms=round(pack, 3))
        # the equaliser's call on the same handle, slots and images
        e.track_batch(seed)
        e.track_batch(steady[0])
        rs, arrs = e.track_batch(steady[1])
        for i in range(min(n, k)):                # frame 1 -> frame 2, prev resident: level 0 and the restatements' bytes
            assert np.array_equal(tr.read_level(i, 0), restated[i][2].out) and np.array_equal(tr.read_level(i, 0, 1), restated[i][1].out)
            assert arrs[i].cur_pts.tobytes() == cpu[i].arrays.cur_pts.tobytes() and arrs[i].flags.tobytes() == cpu[i].arrays.flags.tobytes()
            assert arrs[i].err.tobytes() == cpu[i].arrays.err.tobytes() and arrs[i].cur_un_pts.tobytes() == cpu[i].arrays.cur_un_pts.tobytes()
        wall, call, clahe, pyramid, track, upload, pack = median_run(lambda r: e.track_batch(steady[r % 2]), e.last_ms, args.repeats)
        out.update(eq_call_ms=round(call, 3), eq_clahe_ms=round(clahe, 4), eq_pyramid_ms=round(pyramid, 4), eq_k_trk_track_ms=round(track, 4),
                   eq_upload_ms=round(upload, 3), eq_host_pack_ms=round(pack, 3), eq_frames_per_s=round(1e3 * n / call, 1),
                   kept_per_image=round(float(np.mean([r.n_kept for r in rs])), 1))
        e.close()
        # the stand-alone apply: n images in, n equalised images out
        ea = eq.Equalizer(tr, n)
        imgs = [eq.EqImage(seqs[i % k][2]) for i in range(n)]
        st, got = ea.apply_batch(imgs)
        for i in range(min(n, k)):
            assert st[i] == 0 and got[i].tobytes() == restated[i][2].out.tobytes()
        wall, call, clahe, _, _, upload, pack = median_run(lambda r: ea.apply_batch(imgs), ea.last_ms, args.repeats)
        out.update(apply_call_ms=round(call, 3), apply_clahe_ms=round(clahe, 4), apply_upload_ms=round(upload, 3), apply_images_per_s=round(1e3 * n / call, 1))
        ea.close()
        out.update(cpu_restatement_ms_per_image=round(cpu_ms, 2), cpu_images_per_s=round(1e3 / cpu_ms, 1))
        print(json.dumps(out), flush=True)
        tr.close()
