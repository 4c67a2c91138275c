"""Bit-level A/B of two builds of the library for the batched initialisation stages, which scripts/ab_bits.py does not reach:
one sha256 per case over the SfM stage's result record and position array (the cases of tests/test_gpu_sfm.py), the
relative-pose stage's result record and inlier mask (the cases of tests/test_gpu_relpose.py) and the three records of its chains
from tracks, with the library named by ISVINS_LIB (default: the in-tree one).  Run it once per library and diff."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import isvins_loader; isvins_loader.load()
import numpy as np
from isvins_amd import backend, initial
import test_gpu_sfm, test_gpu_relpose

be = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
ps = [initial.make_scene(**kw)[0] for kw in test_gpu_sfm.CASES]
rs = initial.sfm_batch(be, ps)
for kw, p, r in zip(test_gpu_sfm.CASES, ps, rs):
    print("sfm", kw, hashlib.sha256(bytes(r) + np.ascontiguousarray(p.position).tobytes()).hexdigest()[:16], flush=True)
ps = [initial.make_relpose_scene(**kw)[0] for kw in test_gpu_relpose.CASES]
rs, ms = initial.relpose_batch(be, ps, masks=True)
for kw, r, m in zip(test_gpu_relpose.CASES, rs, ms):
    print("relpose", kw, hashlib.sha256(bytes(r) + np.ascontiguousarray(m).tobytes()).hexdigest()[:16], flush=True)
kws, sc = test_gpu_relpose._scenes()
rr, sr, ar = initial.initial_structure_from_tracks_batch(be, [s[0] for s in sc], [s[1] for s in sc])
for kw, a, b, c in zip(kws, rr, sr, ar):
    print("chain", kw, hashlib.sha256(bytes(a) + (bytes(b) if b is not None else b"") + (bytes(c) if c is not None else b"")).hexdigest()[:16], flush=True)
be.close()
