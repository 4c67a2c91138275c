"""Times isv_internal_relpose_batch (is-vins_amd/csrc/isv_relpose.h) for S = 1, 256, 1024, 4096 18-frame scenes: the whole call
(host packing, one upload, the kernel, one download; device buffers kept on the handle after the warm-up call) and the kernel
alone (HIP events, isv_internal_relpose_last_ms); then the whole chain from tracks (initial_structure_from_tracks_batch:
relpose, SfM, alignment) at the same sizes; and the CPU restatement tests/native/isv_relpose_oracle.c per problem on one core
(built here with gcc -O2 -ffp-contract=off).  The problems cycle through 8 synthetic scenes (isvins_amd.initial
.make_relpose_scene, pixel noise 0.5 px at f = 460; every other one with 20 % mismatched last-frame observations).  Prints one
JSON line per measurement; median of 5 calls after one warm-up call (3 for the chain)."""
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
import relpose_oracle  # noqa: E402

KW = [dict(seed=s, pixel_noise=0.5 / 460, outliers=0.2 if s % 2 else 0.0) for s in range(8)]


def main():
    base = [initial.make_relpose_scene(**kw)[0] for kw in KW]
    be = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    for S in (1, 256, 1024, 4096):
        ps = [base[i % len(base)] for i in range(S)]
        initial.relpose_batch(be, ps)
        ts, ks = [], []
        for _ in range(5):
            t = time.perf_counter()
            rs = initial.relpose_batch(be, ps)
            ts.append(time.perf_counter() - t)
            ks.append(initial.relpose_last_ms(be)[1])
        ok = sum(r.status == 0 for r in rs)
        iters = sum(sum(x for x in r.ransac_iters if x > 0) for r in rs) / S
        ms, kms = statistics.median(ts) * 1e3, statistics.median(ks)
        print(json.dumps({"what": "gpu_relpose_batch", "S": S, "ms": round(ms, 3), "kernel_ms": round(kms, 3), "us_per_problem": round(ms * 1e3 / S, 2),
                          "ok": ok, "ransac_iters_per_problem": round(iters, 1)}), flush=True)
    for S in (1, 256, 1024, 4096):
        sc = [initial.make_relpose_scene(**KW[i % len(KW)]) for i in range(min(S, len(KW)))]
        sps = [sc[i % len(sc)][0] for i in range(S)]
        aps = [sc[i % len(sc)][1] for i in range(S)]
        initial.initial_structure_from_tracks_batch(be, sps, aps)
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            rr, sr, ar = initial.initial_structure_from_tracks_batch(be, sps, aps)
            ts.append(time.perf_counter() - t)
        ms = statistics.median(ts) * 1e3
        print(json.dumps({"what": "gpu_chain_from_tracks", "S": S, "ms": round(ms, 3), "us_per_problem": round(ms * 1e3 / S, 2),
                          "relpose_ok": sum(r.status == 0 for r in rr), "sfm_ok": sum(s is not None and s.status == 0 for s in sr),
                          "align_ok": sum(a is not None and a.status == 0 for a in ar)}), flush=True)
    be.close()
    lib = relpose_oracle.build(tempfile.mkdtemp())
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        for p in base:
            relpose_oracle.solve(lib, p)
        ts.append((time.perf_counter() - t) / len(base))
    print(json.dumps({"what": "cpu_restatement", "us_per_problem": round(statistics.median(ts) * 1e6, 2)}))


if __name__ == "__main__":
    main()
