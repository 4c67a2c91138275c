"""The problem PoseGraph::optimizeCS states (include/isvins_posegraph.h:10-17) recomputed at 40 digits in mpmath, on small pose graphs
whose LOOP TOPOLOGY is chosen so that k_pgo (csrc/isv_posegraph.hip) takes each of its hand-scheduled branches.  Test infrastructure:
tests/test_pgo_highprec.py pins this file to the CPU oracle, tests/test_gpu_pgo_highprec.py compares the kernel with it.

Topologies (`make_topology`).  Every graph starts from posegraph.make_pose_graph(seed, K, 0) -- a chain without loops -- and gets its
loops here: keyframe j re-observes keyframe i (has_loop / loop_index / loop_info / loop_weight), the measurement being the relative
pose of the two VIO poses composed with a fixed, seeded perturbation [dt, dtheta].  At x0 (the VIO poses) the loop's residual IS
that perturbation, so its whitened norm sqrt(loop_weight) |[dt, dtheta]| is chosen directly: 0.35 of the Huber radius 0.1 ("in")
or 3.5 times it ("out").  Every graph with loops also lets `cur` itself close a loop onto keyframe 0: that is the loop closure that
triggers the solve in the reference, it makes first_looped_index = 0 the smallest matched index, and it is NOT part of the solve
(the edge loop stops before cur).  So all K keyframes are parameter blocks, keyframe 0 is the constant one and the free index of
keyframe k is k - 1 (unless keyframes of sequence 0 are constant too).  Because cur's own loop is left out, the LAST free row
(cur's) can be a loop row only through a forward loop -- a keyframe whose loop_index names cur: ring_pos0 and forward use one; the
oracle and the library both accept it (the matched keyframe only has to lie inside the optimised range).
`structure()` restates the skyline rule of the library's structure analysis (start[hi] = min(start[hi], lo) over the edges with
both ends free) and `make_topology` asserts with it every property a topology is named after; spans are counted in free-pose
indices, r - start[r].

Reference (`reference`).  Residuals: relpose_res / rollpitch_res of tests/test_highprec_jacobians.py; Jacobians: central
differences through plus_mp (1e-18 step at 40 digits), both factors' analytic Jacobians being exact derivatives; loop edges under
HuberLoss(0.1) with Ceres 2.0.0's Corrector (rho'' <= 0 beyond the radius: residual and Jacobian scale by sqrt(rho')).  J^T J is
formed block by block, factorised by a scalar Cholesky that skips leading zeros of a row (exact arithmetic does not care), and
inverted column by column; all of it in mpmath (6 nf <= 140).  Beside every quantity the same quantity by a plain float64 route --
the Jacobians rounded to float64, J.T @ J by numpy, the solve and the inverse by LAPACK through scipy, the cost by the same
residual code at 53 bits: its error against the 40-digit one is the yardstick e64 of the tests.
"""
import functools

import mpmath as mp
import numpy as np

from isvins_amd import abi, posegraph as pg, synth
from marg_highprec import jac_pose_mp, q_to_R
from test_highprec_jacobians import mpv, plus_mp, q_from_pose, q_from_R, relpose_res, rollpitch_res

mp.mp.dps = 40
ZERO, ONE = mp.mpf(0), mp.mpf(1)
HUBER = 0.1
LOOP_WEIGHT = 1e4                  # information of a loop edge comparable to the chain's (sqrt_info 200 / 500): the fill of a loop row matters
IN, OUT = 0.35, 3.5                # whitened loop residual at x0 in units of the Huber radius
PD = PS = 8                        # the ring depths of factor() and solve() (csrc/isv_posegraph.hip)


# ---- topologies -------------------------------------------------------------------------------------------------------------
# name -> dict(K, seed, loops = [(keyframe, matched keyframe, IN | OUT)], cur (default K - 1), seq0 (keyframes of sequence 0),
#              rollpitch_every, weight (loop_weight of every loop), chain_noise (perturbation of the chain's measurements))
def _t(K, seed, loops=(), **kw):
    return dict(K=K, seed=seed, loops=list(loops), **kw)


SPECS = {
    # chain only: one free pose; two; nf = 8 and 9 either side of one full PS ring
    # (at x0 a chain's own edges have zero residuals: their measurements get a seeded perturbation, or x0 would be the optimum)
    "chain_k2": _t(2, 101, chain_noise=0.01), "chain_k3": _t(3, 102, chain_noise=0.01), "chain_k9": _t(9, 103, chain_noise=0.01),
    "chain_k10": _t(10, 104, chain_noise=0.01),
    # one loop by span: a single interior column; two; 8 and 9 interior columns around one PD ring; two rings and a remainder
    "span2": _t(6, 111, [(4, 2, IN)]), "span3": _t(7, 112, [(5, 2, OUT)], weight=50.0), "span9": _t(13, 113, [(11, 2, IN)]),
    "span10": _t(14, 114, [(12, 2, OUT)]), "span18": _t(22, 115, [(20, 2, OUT)], weight=400.0),
    # the loop row on the constant first pose (no off-diagonal block) and on the first free pose (start[r] = 0)
    "onto_constant_first": _t(8, 121, [(5, 0, OUT)]), "onto_first_free": _t(8, 122, [(5, 1, IN)]),
    # two loops: free rows (r1, r2) and starts (i1, i2)
    "nested": _t(14, 123, [(8, 4, IN), (11, 2, OUT)]),              # i2 < i1 < r1 < r2
    "crossing": _t(14, 124, [(8, 2, OUT), (11, 5, IN)]),            # i1 < i2 < r1 < r2
    "back_to_back": _t(14, 125, [(7, 3, IN), (11, 7, OUT)]),        # r1 = i2
    "adjacent_rows": _t(14, 126, [(9, 3, OUT), (10, 5, IN)]),       # rows r and r + 1
    "shared_match": _t(14, 127, [(7, 3, OUT), (10, 3, IN)]),        # both onto keyframe 3
    # cur in the middle of the list, the loop closed by the last optimised keyframe before it; a drift-corrected tail follows
    "cur_in_the_middle": _t(16, 128, [(9, 4, OUT)], cur=10, weight=50.0),
    # the first third of sequence 0 (constant), one loop into the prefix and one among the free poses
    "seq0_prefix": _t(12, 129, [(8, 2, OUT), (10, 5, IN)], seq0=range(4)),
    "sparse_rollpitch": _t(10, 130, [(7, 3, OUT)], rollpitch_every=3, weight=50.0),
    # keyframe 6 names the LATER keyframe 11, which closes a loop of its own onto 3: row 10 has an interior H(10, 5) != 0
    "forward": _t(14, 131, [(11, 3, IN), (6, 11, OUT)]),
}
# one loop of span 4 in K = 20 (nf = 19), the loop row at nf - 1 - p: one graph per position of solve()'s backward ring and the wrap
RING = [f"ring_pos{p}" for p in range(PS + 1)]
SPECS["ring_pos0"] = _t(20, 140, [(15, 19, OUT)])                   # cur's row: only a forward loop makes it a loop row
for _p in range(1, PS + 1):
    SPECS[f"ring_pos{_p}"] = _t(20, 140 + _p, [(19 - _p, 15 - _p, OUT if _p % 2 else IN)])
TOPOLOGIES = list(SPECS)


def _loop_measurement(kf, own, matched, size, weight, rng):
    """loop_info of keyframe `own` re-observing `matched`: T_matched^-1 T_own of the VIO poses, perturbed by [dt, dtheta] of norm
    size * HUBER / sqrt(weight) in a seeded direction"""
    d = rng.normal(6)
    d = d / np.linalg.norm(d) * size * HUBER / np.sqrt(weight)
    Ri, Rj = abi.arr(kf[matched].vio_R_w_i, (3, 3)), abi.arr(kf[own].vio_R_w_i, (3, 3))
    rel_t = Ri.T @ (abi.arr(kf[own].vio_T_w_i) - abi.arr(kf[matched].vio_T_w_i)) + d[:3]
    rel_R = Ri.T @ Rj @ synth._exp_so3(d[3:])
    q = pg._quat_wxyz(rel_R)
    return [rel_t[0], rel_t[1], rel_t[2], q[0], q[1], q[2], q[3], 0.0]


def structure(kf, first, cur):
    """the parameter blocks and the skyline as the library's structure analysis derives them: dict(local = list positions of the
    parameter blocks, free = free index per block or -1, nf, start[nf], edges = [(kind, a, b)] in local indices, kind 0 roll/pitch,
    1 chain, 2 loop with a = the matched keyframe, loops = [(free row or -1, free column or -1, keyframe)])"""
    local = [k for k in range(len(kf)) if first <= kf[k].index <= cur]
    pos = {kf[k].index: li for li, k in enumerate(local)}
    free, nf = [], 0
    for k in local:
        const = kf[k].index == first or kf[k].sequence == 0
        free.append(-1 if const else nf)
        nf += 0 if const else 1
    edges, loops = [], []
    for li, k in enumerate(local[:-1]):                              # the factors of cur itself are left out
        if kf[k].has_rollpitch:
            edges.append((0, li, li))
        edges.append((1, li, li + 1))
        if kf[k].has_loop:
            edges.append((2, pos[kf[k].loop_index], li))
            loops.append((free[li], free[pos[kf[k].loop_index]], k))
    start = list(range(nf))
    for kind, a, b in edges:
        if kind and free[a] >= 0 and free[b] >= 0:
            lo, hi = sorted((free[a], free[b]))
            start[hi] = min(start[hi], lo)
    return dict(local=local, free=free, nf=nf, start=start, edges=edges, loops=loops)


def loop_regions(kf, first, cur):
    """{keyframe: whitened residual norm of its loop edge at x0 over the Huber radius}, the loops inside the solve, in float64"""
    from scipy.spatial.transform import Rotation as Rot
    out = {}
    for k in structure(kf, first, cur)["loops"]:
        k = k[2]
        i = kf[k].loop_index
        Ri, Rj = abi.arr(kf[i].vio_R_w_i, (3, 3)), abi.arr(kf[k].vio_R_w_i, (3, 3))
        li = list(kf[k].loop_info)
        dR = Rot.from_quat([li[4], li[5], li[6], li[3]]).as_matrix()
        r = np.concatenate([np.array(li[:3]) - Ri.T @ (abi.arr(kf[k].vio_T_w_i) - abi.arr(kf[i].vio_T_w_i)), Rot.from_matrix(dR @ Rj.T @ Ri).as_rotvec()])
        out[k] = float(np.sqrt(kf[k].loop_weight) * np.linalg.norm(r) / HUBER)
    return out


def make_topology(name):
    """-> (keyframe array, first_looped_index, cur_index); asserts what the topology is named after"""
    spec = SPECS[name]
    K, cur = spec["K"], spec.get("cur", spec["K"] - 1)
    kf, _, _ = pg.make_pose_graph(spec["seed"], K, 0, rollpitch_every=spec.get("rollpitch_every", 1))
    for k in spec.get("seq0", ()):
        kf[k].sequence = 0
    rng = synth.SplitMix64(0x70_0000 + spec["seed"])
    weight = spec.get("weight", LOOP_WEIGHT)
    if spec.get("chain_noise"):
        for k in range(K - 1):
            d = spec["chain_noise"] * rng.normal(6)
            rp = kf[k].relative_pose
            rp.delta_t[:] = list(abi.arr(rp.delta_t) + d[:3])
            rp.delta_R[:] = list((abi.arr(rp.delta_R, (3, 3)) @ synth._exp_so3(d[3:])).ravel())
    loops = list(spec["loops"])
    if loops:
        loops.append((cur, 0, IN))                                   # cur's own loop closure: sets first, stays out of the solve
    for own, matched, size in loops:
        assert not kf[own].has_loop and own != matched
        kf[own].has_loop, kf[own].loop_index, kf[own].loop_weight = 1, matched, weight
        kf[own].loop_info[:] = _loop_measurement(kf, own, matched, size, weight, rng)
    first = min([m for _, m, _ in loops] + [o for o, _, _ in loops]) if loops else 0
    assert first == (min(m for _, m, _ in loops) if loops else 0) == 0          # the smallest matched index
    s = structure(kf, first, cur)
    nf, start = s["nf"], s["start"]
    rows = sorted(r for r in range(nf) if start[r] < r - 1)          # the loop rows
    span = {r: r - start[r] for r in rows}
    reg = loop_regions(kf, first, cur)
    for own, matched, size in spec["loops"]:
        assert abs(reg[own] - size) < 1e-6 * size, (name, own, reg[own])          # inside (0.35) or outside (3.5) the Huber radius
    assert len(reg) == len(spec["loops"])                            # cur's own loop is not in the solve
    if not spec.get("seq0"):
        assert nf == cur and s["free"] == [-1] + list(range(nf))
    # ---- the claims ----
    if name.startswith("chain_k"):
        assert rows == [] and nf == K - 1 and start == [0] + list(range(nf - 1))
        assert {"chain_k2": nf == 1, "chain_k3": nf == 2, "chain_k9": nf == PS, "chain_k10": nf == PS + 1}[name]
    elif name.startswith("span"):
        want = int(name[4:])
        assert len(rows) == 1 and span[rows[0]] == want and start[rows[0]] > 0
        interior = want - 1                                          # columns start + 1 .. r - 1
        assert {2: interior == 1, 3: interior == 2, 9: interior == PD, 10: interior == PD + 1, 18: interior == 2 * PD + 1}[want]
    elif name.startswith("ring_pos"):
        p = int(name[8:])
        assert nf == 19 and rows == [nf - 1 - p] and span[rows[0]] == 4
        assert (p // PS, p % PS) == ((0, p) if p < PS else (1, 0))   # (ring round, slot u) of the backward pass
    elif name == "onto_constant_first":
        assert rows == [] and s["loops"] == [(4, -1, 5)] and start == [0] + list(range(nf - 1))
    elif name == "onto_first_free":
        assert rows == [4] and start[4] == 0
    elif name in ("nested", "crossing", "back_to_back", "adjacent_rows", "shared_match"):
        (r1, r2), (i1, i2) = rows, (start[rows[0]], start[rows[1]])
        assert {"nested": i2 < i1 < r1 < r2, "crossing": i1 < i2 < r1 < r2, "back_to_back": r1 == i2, "adjacent_rows": r2 == r1 + 1 and i2 < r1,
                "shared_match": i1 == i2 and r1 < r2}[name], (rows, start)
    elif name == "cur_in_the_middle":
        assert cur < K - 1 and rows == [nf - 2] and s["loops"][0][2] == cur - 1 and len(s["local"]) == cur + 1
    elif name == "seq0_prefix":
        n0 = len(spec["seq0"])
        assert 3 * n0 == K and s["free"][:n0] == [-1] * n0 and nf == K - n0
        assert sorted(c for _, c, _ in s["loops"]) == [-1, 5 - n0] and rows == [10 - n0]
    elif name == "sparse_rollpitch":
        assert [kf[k].has_rollpitch for k in range(K)] == [int(k % 3 == 0) for k in range(K)] and len(rows) == 1
    elif name == "forward":
        assert rows == [10] and start[10] == 2 and (5, 10, 6) in s["loops"]       # keyframe 6 (free 5) matched with the later free 10
        assert start[10] < 5 < 10 - 1 and start[5] == 4              # H(10, 5) != 0 at an interior column that is a chain row
    else:
        raise KeyError(name)
    return kf, first, cur


# ---- poses ------------------------------------------------------------------------------------------------------------------
def poses_of(kf, first, cur, which="vio"):
    """the parameter blocks [p, qx qy qz qw] (mpmath) from the keyframes' VIO poses ("vio": x0, tmp_q = tmp_r normalised) or from
    their optimised ones ("opt")"""
    out = []
    for k in range(len(kf)):
        if not first <= kf[k].index <= cur:
            continue
        t, R = (kf[k].vio_T_w_i, kf[k].vio_R_w_i) if which == "vio" else (kf[k].T_w_i, kf[k].R_w_i)
        q = q_from_R(mpv(R))
        out.append(mpv(t) + [q[1], q[2], q[3], q[0]])
    return out


def pose_TR(x):
    """[T (3) | R row-major (9)] of one parameter block, mpmath"""
    R = q_to_R(q_from_pose(x))
    return list(x[:3]) + [R[a, b] for a in range(3) for b in range(3)]


def _plus64(x, d):
    q = np.array([x[6], x[3], x[4], x[5]])
    w, v = 1.0, 0.5 * d[3:]
    r = np.array([q[0] * w - q[1:] @ v, *(q[0] * v + w * q[1:] + np.cross(q[1:], v))])
    r = r / np.linalg.norm(r)
    return np.concatenate([x[:3] + d[:3], r[1:], r[:1]])


def _TR64(x):
    from scipy.spatial.transform import Rotation as Rot
    return np.concatenate([x[:3], Rot.from_quat(x[3:]).as_matrix().ravel()])


# ---- exact linear algebra on lists of mpf -----------------------------------------------------------------------------------
def _first_nonzero(A):
    return [next(c for c in range(i + 1) if A[i][c] != 0) for i in range(len(A))]


def cholesky_mp(A):
    """(L, first): lower Cholesky factor of the symmetric positive definite A, rows from their first non-zero column on"""
    n = len(A)
    first = _first_nonzero(A)
    L = [[ZERO] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(first[i], i):
            Lj = L[j]
            s = A[i][j]
            for k in range(max(first[i], first[j]), j):
                s -= Li[k] * Lj[k]
            Li[j] = s / Lj[j]
        s = A[i][i]
        for k in range(first[i], i):
            s -= Li[k] * Li[k]
        assert s > 0
        Li[i] = mp.sqrt(s)
    return L, first


def cholesky_solve_mp(L, first, b):
    n = len(b)
    y = list(b)
    for i in range(n):
        s = y[i]
        for k in range(first[i], i):
            s -= L[i][k] * y[k]
        y[i] = s / L[i][i]
    for i in range(n - 1, -1, -1):
        y[i] = y[i] / L[i][i]
        for k in range(first[i], i):
            y[k] -= L[i][k] * y[i]
    return y


def inverse_diagonal_blocks_mp(L, first, nf):
    """the 6 x 6 diagonal blocks of (L L^T)^-1: block f = Y^T Y with Y = L^-1 [e_6f .. e_6f+5]"""
    n = len(L)
    out = []
    for f in range(nf):
        Y = []
        for c in range(6 * f, 6 * f + 6):
            y = [ZERO] * n
            for i in range(c, n):
                s = ONE if i == c else ZERO
                for k in range(max(first[i], c), i):
                    s -= L[i][k] * y[k]
                y[i] = s / L[i][i]
            Y.append(y)
        out.append([[mp.fsum(Y[a][i] * Y[b][i] for i in range(6 * f, n)) for b in range(6)] for a in range(6)])
    return out


def readout(S):
    """the reference's 7x7-as-6x6 read-out of a tangent covariance block (pose_graph.cpp:346-350, test_oracle_pgo.py::
    test_covariance_is_the_inverse_gauss_newton_hessian_with_the_reference_readout): the first 36 numbers of the row-major 7 x 7
    [Sigma 0; 0 0] re-read as a column-major 6 x 6, stored row-major.  Rows 0 .. 4 of Sigma survive (and Sigma(5, 0)); the rest of
    its sixth row is not in the stored block at all"""
    c7 = [S[a][b] if a < 6 and b < 6 else 0 for a in range(7) for b in range(7)]
    return [c7[a + 6 * b] for a in range(6) for b in range(6)]


# ---- the reference ----------------------------------------------------------------------------------------------------------
class Linearisation:
    """the corrected residuals and Jacobian blocks at x: blocks = [(r [dim], [(free index, J dim x 6 as lists)], kind, edge number)]"""

    def __init__(self, ref, x, rho_scale=None):
        self.blocks, self.cost, self.regions = [], ZERO, {}
        for e, (kind, a, b, f) in enumerate(ref.edges):
            r = f(x[a], x[b])
            s = mp.fsum(v * v for v in r)
            sc = ONE
            if kind == 2:
                if s > ref.huber ** 2:
                    self.cost += (2 * ref.huber * mp.sqrt(s) - ref.huber ** 2) / 2
                    sc = mp.sqrt(ref.huber / mp.sqrt(s))
                else:
                    self.cost += s / 2
                self.regions[e] = float(mp.sqrt(s) / ref.huber)
                if rho_scale and e in rho_scale:
                    sc = sc * rho_scale[e]
            else:
                self.cost += s / 2
            cols = []
            if ref.free[a] >= 0:
                J = jac_pose_mp(lambda q: f(q, x[b]), x[a], len(r))
                cols.append((ref.free[a], [[J[i, c] * sc for c in range(6)] for i in range(len(r))]))
            if kind and ref.free[b] >= 0:
                J = jac_pose_mp(lambda q: f(x[a], q), x[b], len(r))
                cols.append((ref.free[b], [[J[i, c] * sc for c in range(6)] for i in range(len(r))]))
            self.blocks.append(([v * sc for v in r], cols, kind, e))
        self.n = 6 * ref.nf
        self.nres = sum(len(b[0]) for b in self.blocks)

    def normal_equations(self, scale=None):
        """(J^T J, J^T r) of J diag(scale), block by block"""
        n = self.n
        H = [[ZERO] * n for _ in range(n)]
        g = [ZERO] * n
        sc = scale or [ONE] * n
        for r, cols, _, _ in self.blocks:
            for fa, Ja in cols:
                for a in range(6):
                    ca = 6 * fa + a
                    g[ca] += mp.fsum(Ja[i][a] * r[i] for i in range(len(r))) * sc[ca]
                    for fb, Jb in cols:
                        for b in range(6):
                            cb = 6 * fb + b
                            H[ca][cb] += mp.fsum(Ja[i][a] * Jb[i][b] for i in range(len(r))) * sc[ca] * sc[cb]
        return H, g

    def dense64(self):
        J = np.zeros((self.nres, self.n))
        r = np.zeros(self.nres)
        o = 0
        for rb, cols, _, _ in self.blocks:
            d = len(rb)
            r[o:o + d] = [float(v) for v in rb]
            for f, Jb in cols:
                J[o:o + d, 6 * f:6 * f + 6] = [[float(v) for v in row] for row in Jb]
            o += d
        return J, r


class Reference:
    """the problem of one optimizeCS pass over kf[first .. cur]; x: list of parameter blocks [p, qx qy qz qw] in mpmath"""

    def __init__(self, kf, first, cur, x, huber=HUBER):
        s = structure(kf, first, cur)
        self.kf, self.first, self.cur, self.x = kf, first, cur, [list(p) for p in x]
        self.local, self.free, self.nf, self.start, self.huber = s["local"], s["free"], s["nf"], s["start"], mp.mpf(huber)
        assert len(self.x) == len(self.local)
        self.edges = []
        for kind, a, b in s["edges"]:
            k = self.local[b if kind == 2 else a]                    # the keyframe whose factor this is
            if kind == 0:
                R, S = mpv(kf[k].rollpitch.R), mpv(kf[k].rollpitch.sqrt_info)
                f = lambda xa, xb, R=R, S=S: rollpitch_res(xa, R, S)
            elif kind == 1:
                rp = kf[k].relative_pose
                dt, dR, S = mpv(rp.delta_t), mpv(rp.delta_R), mpv(rp.sqrt_info)
                f = lambda xa, xb, dt=dt, dR=dR, S=S: relpose_res(xa, xb, dt, dR, S)
            else:
                li = mpv(kf[k].loop_info)
                qn = mp.sqrt(mp.fsum(c * c for c in li[3:7]))        # (Eigen's toRotationMatrix of a unit quaternion; loop_info's is unit to rounding)
                Rm = q_to_R(tuple(c / qn for c in li[3:7]))
                dR = [Rm[u, v] for u in range(3) for v in range(3)]
                w = mp.sqrt(mp.mpf(float(kf[k].loop_weight)))
                S = [w if u == v else ZERO for u in range(6) for v in range(6)]
                f = lambda xa, xb, dt=li[:3], dR=dR, S=S: relpose_res(xa, xb, dt, dR, S)
            self.edges.append((kind, a, b, f))
        self.loop_edges = [e for e, ed in enumerate(self.edges) if ed[0] == 2]
        self.drop, self.rho_scale, self.drop_fill = set(), {}, None   # corruptions (the negative controls of the GPU test)
        self._lin0 = None

    # -- evaluation --
    def _active(self):
        if not self.drop:
            return self
        c = object.__new__(Reference)
        c.__dict__.update(self.__dict__)
        c.edges = [ed for e, ed in enumerate(self.edges) if e not in self.drop]
        return c

    def linearise(self, x):
        act = self._active()
        shift = {e: e - sum(1 for d in self.drop if d < e) for e in self.rho_scale}
        return Linearisation(act, x, {shift[e]: v for e, v in self.rho_scale.items()})

    def cost(self, x, prec=None):
        """sum rho / 2 at x (prec = 53: the same arithmetic in float64, the yardstick's)"""
        def run():
            c = ZERO
            for kind, a, b, f in self._active().edges:
                s = mp.fsum(v * v for v in f(x[a], x[b]))
                c += (2 * self.huber * mp.sqrt(s) - self.huber ** 2) / 2 if kind == 2 and s > self.huber ** 2 else s / 2
            return c
        if prec is None:
            return run()
        with mp.workprec(prec):
            x = [[+v for v in p] for p in x]
            return run()

    def lm_step(self, x0, radius=1e4):
        """the first LevenbergMarquardtStrategy step at x0 -> dict(delta = step * scale [6 nf], x1 = Plus(x0, delta), TR = [T | R] per
        parameter block, model = the model cost change, norm = |delta|_2, and delta64 / TR64: the float64 route)"""
        lin = self.linearise(x0)
        n = lin.n
        cn = [ZERO] * n
        for r, cols, _, _ in lin.blocks:
            for f, J in cols:
                for c in range(6):
                    cn[6 * f + c] += mp.fsum(J[i][c] ** 2 for i in range(len(r)))
        scale = [1 / (1 + mp.sqrt(v)) for v in cn]
        H, g = lin.normal_equations(scale)
        rad = mp.mpf(radius)
        for i in range(n):
            H[i][i] += min(max(cn[i] * scale[i] ** 2, mp.mpf("1e-6")), mp.mpf("1e32")) / rad
        L, first = cholesky_mp(H)
        step = [-v for v in cholesky_solve_mp(L, first, g)]
        delta = [step[i] * scale[i] for i in range(n)]
        model = ZERO                                                  # -(J_s step)^T (r + J_s step / 2)
        for r, cols, _, _ in lin.blocks:
            for i in range(len(r)):
                m = mp.fsum(J[i][c] * delta[6 * f + c] for f, J in cols for c in range(6))
                model -= m * (r[i] + m / 2)
        x1 = [plus_mp(p, delta[6 * f:6 * f + 6]) if f >= 0 else list(p) for p, f in zip(x0, self.free)]
        out = dict(delta=delta, x1=x1, model=model, TR=[pose_TR(p) for p in x1], norm=mp.sqrt(mp.fsum(v * v for v in delta)), lin=lin)
        # the float64 route
        import scipy.linalg
        J, r = lin.dense64()
        sc = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
        Js = J * sc
        A = Js.T @ Js + np.diag(np.clip((Js * Js).sum(0), 1e-6, 1e32) / radius)
        d64 = -scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), Js.T @ r) * sc
        x64 = [np.array([float(v) for v in p]) for p in x0]
        out["delta64"] = d64
        out["TR64"] = [_TR64(_plus64(p, d64[6 * f:6 * f + 6]) if f >= 0 else p) for p, f in zip(x64, self.free)]
        return out

    def covariance(self, x):
        """-> (cov, cov64): per parameter block BEFORE cur the stored 36 numbers (row-major 6 x 6 after the reference's read-out) of the
        block's tangent-space marginal covariance, the diagonal block of (J^T J)^-1 at x; zero for constant blocks.  cov in mpmath
        rounded to float64 at the end, cov64 by the float64 route"""
        lin = self.linearise(x)
        H, _ = lin.normal_equations()
        L, first = cholesky_mp(H)
        if self.drop_fill is not None:                                # (corruption: a block of the factor's fill is left out)
            r, c = self.drop_fill
            for a in range(6):
                for b in range(6):
                    L[6 * r + a][6 * c + b] = ZERO
        blocks = inverse_diagonal_blocks_mp(L, first, self.nf)
        import scipy.linalg
        J, _ = lin.dense64()
        L64 = np.linalg.cholesky(J.T @ J)
        if self.drop_fill is not None:                                # (the yardstick is the float64 route of the SAME system)
            L64[6 * r:6 * r + 6, 6 * c:6 * c + 6] = 0.0
        S64 = scipy.linalg.cho_solve((L64, True), np.eye(lin.n))
        cov, cov64 = [], []
        for f in self.free[:-1]:
            if f < 0:
                cov.append(np.zeros(36)); cov64.append(np.zeros(36))
            else:
                cov.append(np.array([float(v) for v in readout(blocks[f])]))
                cov64.append(np.array(readout(S64[6 * f:6 * f + 6, 6 * f:6 * f + 6].tolist()), float))
        return cov, cov64


def reference(kf, first, cur, x):
    return Reference(kf, first, cur, x)


@functools.lru_cache(maxsize=None)
def first_step(name):
    """(Reference at x0, its lm_step) of a topology: shared by every test that needs it, never modified"""
    kf, first, cur = make_topology(name)
    x0 = poses_of(kf, first, cur, "vio")
    ref = Reference(kf, first, cur, x0)
    return ref, ref.lm_step(x0)


# ---- the norms of the comparisons -------------------------------------------------------------------------------------------
def keyframe_TR(kf, first, cur):
    """[T | R] of the parameter blocks as the keyframes store them after a solve (float64)"""
    return [np.concatenate([abi.arr(kf[k].T_w_i), abi.arr(kf[k].R_w_i)]) for k in range(len(kf)) if first <= kf[k].index <= cur]


def step_errors(ref, st, got_TR):
    """(err, e64, floor) of the poses after the first step: max-norm of the pose difference [T | R] over the 2-norm of the reference
    step; floor = 2^-53 max(n, |x0|_inf / |step|_2), the rounding of storing a pose (the step is read back through the pose)"""
    norm = float(st["norm"])
    want = [np.array([float(v) for v in p]) for p in st["TR"]]
    exact = lambda TR: max(float(max(abs(mp.mpf(float(g)) - w) for g, w in zip(G, W))) for G, W in zip(TR, st["TR"]))
    x_inf = max(float(np.abs(w).max()) for w in want)
    return exact(got_TR) / norm, exact(st["TR64"]) / norm, 2.0 ** -53 * max(6 * ref.nf, x_inf / norm)


def cost_errors(ref, x0, got):
    """(err, e64, floor) of the cost at x0, relative; floor = (number of residuals) 2^-53"""
    c = ref.cost(x0)
    nres = sum(2 if ed[0] == 0 else 6 for ed in ref.edges)
    return float(abs(mp.mpf(float(got)) - c) / c), float(abs(ref.cost(x0, 53) - c) / c), nres * 2.0 ** -53


def cov_errors(cov, cov64, got):
    """[(block, err, e64)]: per block with a non-zero reference, max-abs over the block's largest reference entry; zero blocks
    (constant poses) must be zero"""
    out = []
    for k, (c, c64, g) in enumerate(zip(cov, cov64, got)):
        m = np.abs(c).max()
        if m == 0:
            assert not np.any(g), k
            continue
        out.append((k, float(np.abs(g - c).max() / m), float(np.abs(c64 - c).max() / m)))
    return out
