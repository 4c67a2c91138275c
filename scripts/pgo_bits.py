"""Bit-level A/B of two builds of the library for the pose-graph call (isv_pgo_optimize / isv_pgo_optimize_batch), which
scripts/ab_bits.py and scripts/init_bits.py do not reach: one sha256 per case over the keyframe bytes and the result record.  The
cases are the single graphs of tests/test_gpu_pgo.py (also with ISV_PGO_WAVES 1 / 4 and ISV_PGO_IDX_GLOBAL=1), its 70-graph batch
cold and cached at ISV_PGO_CHUNKS default / 1 / 3 / 4 and with the same three hooks, and a batch with one refused graph (the error
is part of the digest): 54 lines.  The
library is named by ISVINS_LIB (default: the in-tree one).  Run it once per library and diff."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import isvins_loader; isvins_loader.load()
from isvins_amd import backend, posegraph as pg


def digest(kfs, res, extra=b""):
    return hashlib.sha256(b"".join(bytes(k) for k in kfs) + b"".join(bytes(r) for r in res) + extra).hexdigest()[:16]


def env(**kw):
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


# ---- single graphs -----------------------------------------------------------------------------------------------------
opt = pg.PoseGraphOptimizer(1024, max_graphs=8)
singles = [((s, K, L), {}, K - 1) for (s, K, L) in [(0, 120, 3), (1, 200, 6), (2, 60, 0), (4, 400, 10), (5, 12, 1), (11, 300, 8), (3, 200, 5), (7, 40, 1), (9, 64, 0)]]
for spec, kw, cur in singles:
    kf, _, first = pg.make_pose_graph(*spec, **kw)
    for name, hook in (("default", {}), ("waves1", {"ISV_PGO_WAVES": "1"}), ("waves4", {"ISV_PGO_WAVES": "4"}), ("idx_global", {"ISV_PGO_IDX_GLOBAL": "1"})):
        env(**hook)
        g = pg.clone_keyframes(kf); r = opt.optimize(g, first, cur)
        env(**{k: None for k in hook})
        print("single", spec, name, digest([g], [r]), flush=True)
# cur in the middle (the tail gets the drift correction); sequence 0 constant with loop closures far outside the Huber radius
kf, _, first = pg.make_pose_graph(9, 150, 4)
cur = [k for k in range(150) if kf[k].has_loop][-1]
g = pg.clone_keyframes(kf); r = opt.optimize(g, first, cur)
print("single cur_in_the_middle", digest([g], [r]), flush=True)
kf, _, first = pg.make_pose_graph(13, 90, 5, drift=0.01)
for k in range(30):
    kf[k].sequence = 0
for k in range(90):
    if kf[k].has_loop:
        kf[k].loop_weight = 5e3
g = pg.clone_keyframes(kf); r = opt.optimize(g, first, 89)
print("single sequence_zero_huber", digest([g], [r]), flush=True)
opt.close()

# ---- the 70-graph batch of five shapes, cold and cached, per chunk count --------------------------------------------------
specs = [(30, 90, 3), (31, 40, 1), (32, 150, 5), (33, 25, 0), (34, 120, 2)]
graphs = [pg.make_pose_graph(*s) for s in specs]
n = 70
firsts = [graphs[i % 5][2] for i in range(n)]; curs = [specs[i % 5][1] - 1 for i in range(n)]
for name, hook in (("chunks default", {}), ("chunks 1", {"ISV_PGO_CHUNKS": "1"}), ("chunks 3", {"ISV_PGO_CHUNKS": "3"}), ("chunks 4", {"ISV_PGO_CHUNKS": "4"}),
                   ("waves1", {"ISV_PGO_WAVES": "1"}), ("waves4", {"ISV_PGO_WAVES": "4"}), ("idx_global", {"ISV_PGO_IDX_GLOBAL": "1"})):
    opt = pg.PoseGraphOptimizer(160, max_graphs=n, max_loop_blocks=8 * 160)
    env(**hook)
    for rep in ("cold", "cached"):
        b = [pg.clone_keyframes(graphs[i % 5][0]) for i in range(n)]
        r = opt.optimize_batch(b, firsts, curs)
        print("batch70", name, rep, digest(b, r), "hits", opt.structure_cache_hits(), flush=True)
    env(**{k: None for k in hook})
    opt.close()

# ---- a batch with one refused graph (a non-finite pose): nothing is written, the first refusal in index order reports ------
opt = pg.PoseGraphOptimizer(160, max_graphs=5, max_loop_blocks=8 * 160)
for rep in ("cold", "warm"):
    b = [pg.clone_keyframes(kf) for (kf, _, _) in graphs]
    if rep == "warm":
        opt.optimize_batch(b, firsts[:5], curs[:5])
        b = [pg.clone_keyframes(kf) for (kf, _, _) in graphs]
    b[3][7].vio_R_w_i[4] = float("nan")
    try:
        opt.optimize_batch(b, firsts[:5], curs[:5]); msg = "accepted"
    except backend.BackendError as e:
        msg = str(e)
    print("batch5 one_refused", rep, digest(b, [], msg.encode()), msg, "hits", opt.structure_cache_hits(), flush=True)
opt.close()
