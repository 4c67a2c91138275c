"""The loop-verification case list shared by tests/test_loop_oracle.py (restatement against numpy, the knife-edge check) and
tests/test_gpu_loop.py (k_loop_match / k_loop_pnp against the restatement).  Shapes follow the kernels: k_loop_match stages the
old descriptors through tiles of T = 512 with four wavefronts of 64 lanes per workgroup, k_loop_pnp runs 64 hypotheses per chunk."""
import numpy as np

from isvins_amd import loop, synth

T = 512                      # k_loop_match's tile (kTile in is-vins_amd/csrc/isv_loop.hip)
WAVES = 4                    # its wavefronts per workgroup
MAX_POINTS, MAX_KEYPOINTS = 200, 1100
NOISE = 0.5 / 460


def config(max_pairs=1):
    return loop.make_config(max_pairs, MAX_POINTS, MAX_KEYPOINTS)


def far_corners(rng, w, n):
    """n descriptors at Hamming distance >= 216 from w (its complement with at most 40 bits flipped back)"""
    out = np.empty((n, 4), np.uint64)
    for k in range(n):
        out[k] = loop.flip_bits(~np.asarray(w, np.uint64), rng.permutation(256)[:int(rng.integers(0, 41))])
    return out


def single_point_pair(seed, n_keypoints, placed):
    """one window point; old corner k at exactly placed[k] bits from it, every other corner far (>= 216)"""
    rng = np.random.Generator(np.random.PCG64(0x7E57_0000 + seed))
    w = rng.integers(0, 2 ** 64, size=4, dtype=np.uint64)
    kb = far_corners(rng, w, n_keypoints)
    for k, d in placed.items():
        kb[k] = loop.flip_bits(w, rng.permutation(256)[:d])
    kpn = rng.uniform(-0.5, 0.5, (n_keypoints, 2))
    return loop.LoopPair(w[None], rng.uniform(1, 5, (1, 3)), np.zeros((1, 2)), kb, kpn, np.zeros(3), np.eye(3), old_index=3)


def match_cases():
    """(name, pair, expected (index, dist, accepted) of point 0 or None)"""
    out = []
    for d, exp in [(79, (7, 79, True)), (80, (7, 80, False)), (127, (7, 127, False)), (128, (-1, 128, False))]:
        out.append((f"min{d}", single_point_pair(d, 65, {7: d}), exp))
    out.append(("ties_lanes", single_point_pair(1, 2 * T + 1, {70: 40, 5: 40, 300: 40, 2: 41}), (5, 40, True)))
    out.append(("ties_tiles", single_point_pair(2, 2 * T + 1, {2 * T: 40, T + 88: 40, 100: 40, 3: 41}), (100, 40, True)))
    out.append(("later_tile_wins", single_point_pair(3, 2 * T + 1, {900: 30, 3: 31, 2 * T: 31}), (900, 30, True)))
    out.append(("first_of_tile_edge", single_point_pair(4, T + 1, {T - 1: 50, T: 50}), (T - 1, 50, True)))
    return out


def scene_cases():
    """(name, make_loop_scene keywords)"""
    c = [("exact0", dict(seed=0)), ("exact1", dict(seed=1)), ("noise2", dict(seed=2, pixel_noise=NOISE)), ("noise3", dict(seed=3, pixel_noise=NOISE)),
         ("out30", dict(seed=4, outliers=0.3)), ("out30_noise", dict(seed=5, outliers=0.3, pixel_noise=NOISE)),
         ("out60_noise", dict(seed=6, outliers=0.6, pixel_noise=NOISE)), ("all_outliers", dict(seed=7, n_points=24, n_keypoints=T, outliers=1.0)),
         ("l1_12", dict(seed=8, n_matchable=12, n_keypoints=T - 1)), ("l1_10", dict(seed=9, n_matchable=10, n_keypoints=63)),
         ("l1_15", dict(seed=10, n_matchable=15, n_keypoints=64)), ("few9", dict(seed=11, n_matchable=9, n_keypoints=65)),
         ("yaw40", dict(seed=12, yaw=0.7)), ("far25", dict(seed=13, offset=(25.0, 0.0, 0.0))), ("planar", dict(seed=14, planar=True)),
         ("m16", dict(seed=15, n_points=16, n_keypoints=T)), ("m17", dict(seed=16, n_points=17, n_keypoints=T + 1, pixel_noise=NOISE)),
         ("m64", dict(seed=17, n_points=64, n_keypoints=2 * T + 1, pixel_noise=NOISE)), ("m65", dict(seed=18, n_points=65, n_keypoints=100, outliers=0.2)),
         ("m200", dict(seed=19, n_points=200, n_keypoints=MAX_KEYPOINTS, pixel_noise=NOISE, outliers=0.1)),
         ("p5", dict(seed=20, n_points=WAVES + 1, n_keypoints=70)), ("p1", dict(seed=21, n_points=1, n_keypoints=1)),
         ("p0", dict(seed=22, n_points=0, n_keypoints=40)), ("k0", dict(seed=23, n_points=30, n_keypoints=0, n_matchable=0)),
         ("k1", dict(seed=24, n_points=30, n_keypoints=1, n_matchable=1))]
    return c + CHUNK_EDGES


# k_loop_pnp's chunk edges and lane loops (64 hypotheses a chunk, 64 lanes), found by a seed search with the CPU restatement; the
# unmatchable window points stand between the matchable ones (make_scene).  tests/loop_highprec_cases.py has the table.  The old
# keyframe stands at seed 0's pose: make_loop_scene moves it by 0.1 m and 0.1 rad per seed, which at seed 1000 puts float32 points
# 150 m from the origin and makes the DLT's 12 x 12 system needlessly ill-conditioned.
OLD_POSE = (synth._rot_zyx(0.3, 0.05, -0.04), np.array([1.0, -2.0, 0.5]))
CHUNK_EDGES = [
    ("stop64", dict(seed=1006, n_points=43, n_matchable=29, n_keypoints=70, outliers=0.41, interleave=True, old_pose=OLD_POSE)),
    ("stop65", dict(seed=1017, n_points=60, n_matchable=41, n_keypoints=129, outliers=0.41, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
    ("keep2_f63", dict(seed=1087, n_points=190, n_matchable=158, n_keypoints=400, outliers=0.6, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
    ("late129", dict(seed=1644, n_points=60, n_matchable=48, n_keypoints=150, outliers=0.62, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
    ("f64", dict(seed=1005, n_points=93, n_matchable=70, n_keypoints=300, outliers=0.08, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
    ("f65", dict(seed=1005, n_points=96, n_matchable=72, n_keypoints=300, outliers=0.08, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
    ("floor4", dict(seed=171, n_points=24, n_matchable=16, n_keypoints=80, outliers=0.75, interleave=True, old_pose=OLD_POSE)),
    ("f129", dict(seed=1013, n_points=189, n_matchable=142, n_keypoints=300, outliers=0.08, pixel_noise=NOISE, interleave=True, old_pose=OLD_POSE)),
]


def make_scene(kw):
    """loop.make_loop_scene(**kw); with interleave=True the window points are reordered so that the unmatchable ones stand between
    the matchable ones (make_loop_scene puts the matchable first): a matched point's window index `src` then differs from its
    position in the match list, which is what the inlier mask and the compaction are indexed by"""
    kw = dict(kw)
    if not kw.pop("interleave", False):
        return loop.make_loop_scene(**kw)
    pair, tr = loop.make_loop_scene(**kw)
    n, nm = pair.c.n_points, kw["n_matchable"]
    keys = [(j + 0.5) / nm for j in range(nm)] + [(u + 0.25) / (n - nm) for u in range(n - nm)]
    order = np.argsort(keys, kind="stable")
    out = loop.LoopPair(pair.window_brief[order], pair.point_3d[order], pair.point_2d_norm[order], pair.brief, pair.keypoints_norm,
                        pair.origin_vio_T, pair.origin_vio_R, pair.c.old_index)
    tr = dict(tr, is_outlier=tr["is_outlier"][order], counterpart=tr["counterpart"][order])
    return out, tr


def refusal_cases():
    """(name, pair, status)"""
    big = loop.make_loop_scene(30, n_points=MAX_POINTS + 1)[0]
    bigk = loop.make_loop_scene(31, n_points=20, n_keypoints=MAX_KEYPOINTS + 1)[0]
    nan = loop.make_loop_scene(32, n_points=40, n_keypoints=80)[0]
    nan.point_3d[17, 1] = np.nan
    inf = loop.make_loop_scene(33, n_points=40, n_keypoints=80)[0]
    inf.keypoints_norm[5, 0] = np.inf
    neg = loop.make_loop_scene(34, n_points=40, n_keypoints=80)[0]
    neg.c.n_keypoints = -1
    null = loop.make_loop_scene(35, n_points=40, n_keypoints=80)[0]
    null.c.window_brief = None
    return [("cap_points", big, loop.ISV_LOOP_CAPACITY), ("cap_keypoints", bigk, loop.ISV_LOOP_CAPACITY), ("nan_point", nan, loop.ISV_LOOP_INPUT),
            ("inf_corner", inf, loop.ISV_LOOP_INPUT), ("negative_count", neg, loop.ISV_LOOP_INPUT), ("null_array", null, loop.ISV_LOOP_INPUT)]


_cache = None


def all_pairs():
    """every case as (name, pair, truth or None), built once"""
    global _cache
    if _cache is None:
        out = [(n, p, None) for n, p, _ in match_cases()]
        for n, kw in scene_cases():
            p, tr = make_scene(kw)
            out.append((n, p, tr))
        out += [(n, p, None) for n, p, _ in refusal_cases()]
        _cache = out
    return _cache


def brute_force(pair):
    """numpy: Hamming distances by unpackbits, the reference's decision rule -> (index, dist, accepted) per window point"""
    n, K = pair.c.n_points, pair.c.n_keypoints
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z.astype(bool)
    if K == 0:
        return np.full(n, -1), np.full(n, 128), np.zeros(n, bool)
    a = pair.window_brief.view(np.uint8).reshape(n, 1, 32)
    b = pair.brief.view(np.uint8).reshape(1, K, 32)
    d = np.unpackbits(a ^ b, axis=2).sum(axis=2).astype(np.int64)
    idx = d.argmin(axis=1)                                  # the first of equal minima
    dist = d[np.arange(n), idx]
    found = dist < 128
    return np.where(found, idx, -1), np.where(found, dist, 128), found & (dist < 80)
