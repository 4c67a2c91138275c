"""Times isv_bow_detect_batch (include/isvins_bow.h) for S = 1, 256, 1024 databases of 500 entries, 500 features per keyframe, with
a synthetic k10 / L4 and a k10 / L6 vocabulary (isvins_amd.bow.make_vocabulary): the whole call (host packing, one upload, the four
kernels, one download; device buffers kept on the handle) and each kernel alone (HIP events, isv_bow_last_ms); then the CPU
restatement tests/native/isv_bow_oracle.c per keyframe on one core (built here with gcc -O2 -ffp-contract=off) on a database of
the same size.  Keyframes are drawn from a pool of 32 descriptor arrays whose descriptors come from a pool of 4000, so that
entries share words.  Prints one JSON line per measurement; median of 5 DETECT calls after one warm-up call.
Usage: bow_bench.py [S ...] (default 1 256 1024)."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import isvins_loader  # noqa: E402

isvins_loader.load()
from isvins_amd import bow  # noqa: E402
import bow_oracle  # noqa: E402

ENTRIES, FEATURES, POOL = 500, 500, 32


def keyframes():
    rng = np.random.Generator(np.random.PCG64(0xBE7C))
    base = rng.integers(0, 2 ** 64, size=(4000, 4), dtype=np.uint64)
    return [base[rng.integers(0, len(base), size=FEATURES)] for _ in range(POOL)]


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1, 256, 1024]
    pool = keyframes()
    lib = bow_oracle.build(tempfile.mkdtemp())
    for L in (4, 6):
        vb = bow.make_vocabulary(30 + L, 10, L)
        for S in sizes:
            det = bow.LoopDetector(vb, S, S, FEATURES, initial_entry_capacity=512)
            items = [[bow.BowItem(d, 0, pool[(p + d) % POOL], bow.ISV_BOW_ADD) for d in range(S)] for p in range(POOL)]
            t_fill = time.perf_counter()
            for e in range(ENTRIES):
                det.detect_batch(items[(7 * e) % POOL])
            t_fill = time.perf_counter() - t_fill
            probe = [bow.BowItem(d, 600, pool[(5 + d) % POOL]) for d in range(S)]
            det.detect_batch(probe)
            ts, parts = [], []
            for _ in range(5):
                t = time.perf_counter()
                rs = det.detect_batch(probe)
                ts.append(time.perf_counter() - t)
                parts.append(det.last_ms())
            ms = statistics.median(ts) * 1e3
            med = [statistics.median(p[i] for p in parts) for i in range(5)]
            print(json.dumps({"what": "gpu_bow_detect_batch", "vocabulary": f"k10L{L}", "S": S, "ms": round(ms, 3), "call_ms_inside": round(med[0], 3),
                              "transform_ms": round(med[1], 3), "score_ms": round(med[2], 3), "select_ms": round(med[3], 3),
                              "append_ms": round(med[4], 3), "us_per_keyframe": round(ms * 1e3 / S, 2), "fill_s": round(t_fill, 2),
                              "loops": sum(r.loop_index >= 0 for r in rs), "n_scored": rs[0].n_scored}), flush=True)
            det.close()
        o = bow_oracle.Oracle(lib, vb, bow.make_config(1, 1, FEATURES))
        for e in range(ENTRIES):
            o.detect(bow.BowItem(0, 0, pool[(7 * e) % POOL], bow.ISV_BOW_ADD))
        ts = []
        for k in range(6):
            it = bow.BowItem(0, 600, pool[5])
            t = time.perf_counter()
            o.detect(it)
            ts.append(time.perf_counter() - t)
        us = statistics.median(ts[1:]) * 1e6
        print(json.dumps({"what": "cpu_restatement", "vocabulary": f"k10L{L}", "us_per_keyframe_one_core": round(us, 2),
                          "us_per_keyframe_16_cores_ideal": round(us / 16, 2)}), flush=True)
        o.close()


if __name__ == "__main__":
    main()
