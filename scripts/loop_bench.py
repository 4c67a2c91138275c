"""Times isv_loop_verify_batch (include/isvins_loop.h) for S = 1, 256, 1024, 4096 keyframe pairs of 150 window points x 1000 old
corners: the whole call (host packing, one upload, k_loop_match, k_loop_pnp, one download; device buffers kept on the handle
after the warm-up call) and each kernel alone (HIP events, isv_loop_last_ms); then the CPU restatement
tests/native/isv_loop_oracle.c per pair on one core (built here with gcc -O2 -ffp-contract=off).  The pairs cycle through 8
synthetic scenes (isvins_amd.loop.make_loop_scene, pixel noise 0.5 px at f = 460, 20 % outliers).  Prints one JSON line per
measurement; median of 5 calls after one warm-up call."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isvins_loader  # noqa: E402

isvins_loader.load()
from isvins_amd import loop  # noqa: E402
import loop_oracle  # noqa: E402

KW = [dict(seed=s, n_points=150, n_keypoints=1000, pixel_noise=0.5 / 460, outliers=0.2) for s in range(8)]


def main():
    base = [loop.make_loop_scene(**kw)[0] for kw in KW]
    lv = loop.LoopVerifier(4096, 150, 1000)
    for S in (1, 256, 1024, 4096):
        ps = [base[i % len(base)] for i in range(S)]
        lv.verify_batch(ps)
        ts, ms_match, ms_pnp = [], [], []
        for _ in range(5):
            t = time.perf_counter()
            rs = lv.verify_batch(ps)
            ts.append(time.perf_counter() - t)
            _, a, b = lv.last_ms()
            ms_match.append(a); ms_pnp.append(b)
        ms = statistics.median(ts) * 1e3
        print(json.dumps({"what": "gpu_loop_verify_batch", "S": S, "ms": round(ms, 3), "match_kernel_ms": round(statistics.median(ms_match), 3),
                          "pnp_kernel_ms": round(statistics.median(ms_pnp), 3), "us_per_pair": round(ms * 1e3 / S, 2),
                          "ok": sum(r.status == 0 for r in rs), "ransac_iters_per_pair": round(sum(r.ransac_iters for r in rs) / S, 1)}), flush=True)
    lv.close()
    lib = loop_oracle.build(tempfile.mkdtemp())
    cfg = loop.make_config(1, 150, 1000)
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        for p in base:
            loop_oracle.verify(lib, cfg, p)
        ts.append((time.perf_counter() - t) / len(base))
    print(json.dumps({"what": "cpu_restatement", "us_per_pair": round(statistics.median(ts) * 1e6, 2)}))


if __name__ == "__main__":
    main()
