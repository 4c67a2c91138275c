"""Times isv_internal_sfm_batch (is-vins_amd/csrc/isv_sfm.h) for S = 1, 256, 1024, 4096 18-frame scenes: the whole call
(host packing, one upload, the kernel, one download; device buffers kept on the handle after the warm-up call) and the kernel
alone (HIP events, isv_internal_sfm_last_ms), and the CPU restatement tests/native/isv_sfm_oracle.c per problem on one core
(built here with gcc -O2 -ffp-contract=off).  The problems cycle through 8 synthetic scenes (isvins_amd.initial.make_scene,
pixel noise 0.5 px at f = 460).  Prints one JSON line per measurement; median of 5 calls after one warm-up call."""
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
from isvins_amd import backend, initial  # noqa: E402
import sfm_oracle  # noqa: E402


def main():
    base = [initial.make_scene(seed=s, n_window=18, pixel_noise=0.5 / 460)[0] for s in range(8)]
    be = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    for S in (1, 256, 1024, 4096):
        ps = [base[i % len(base)] for i in range(S)]
        initial.sfm_batch(be, ps)
        ts, ks = [], []
        for _ in range(5):
            t = time.perf_counter()
            rs = initial.sfm_batch(be, ps)
            ts.append(time.perf_counter() - t)
            ks.append(initial.sfm_last_ms(be)[1])
        ok = sum(r.status == 0 for r in rs)
        ms, kms = statistics.median(ts) * 1e3, statistics.median(ks)
        print(json.dumps({"what": "gpu_sfm_batch", "S": S, "ms": round(ms, 3), "kernel_ms": round(kms, 3), "us_per_problem": round(ms * 1e3 / S, 2),
                          "ok": ok}), flush=True)
    be.close()
    lib = sfm_oracle.build(tempfile.mkdtemp())
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        for p in base:
            sfm_oracle.solve(lib, p)
        ts.append((time.perf_counter() - t) / len(base))
    print(json.dumps({"what": "cpu_restatement", "us_per_problem": round(statistics.median(ts) * 1e6, 2)}))


if __name__ == "__main__":
    main()
