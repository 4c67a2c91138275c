"""The windows on which MargForward / MargBackward are compared LIVE with the 40-digit recomputation of tests/marg_highprec.py
(tests/test_marg_highprec.py: the CPU oracle; tests/test_gpu_marg_highprec.py: the HIP kernels), and the comparison both share.

A case is a synthetic window solved by the oracle (num_iterations = 10); MargForward / MargBackward then run at exactly that state
(num_iterations = 0: vector2double, update() with old == new, double2vector, the two routines), and marg_highprec recomputes them from
the para_* arrays and the post-update priors of the side under test.

Yardstick.  Errors are max-norm distances of an information matrix (sqrt_info^T sqrt_info) from the 40-digit one, relative to its
largest entry.  A value passes when  err <= MARGIN * max(e64, float64_limit, floor):
  e64            the same algebra in numpy float64 from the 40-digit intermediates rounded to double (marg_highprec.e64_*),
  float64_limit  2^-52 max|Lam| / min(kept eigenvalue): on these windows Lam reaches 2e11 (the IMU bias information), the smallest kept
                 eigenvalue of the 21 x 21 marginal is about 80, so NO double-precision MargBackward is closer than ~5e-7,
  floor          n 2^-53 with n the length of the sums behind one entry (21 backward, 12 forward).
All three come from the reference side alone."""
import ctypes as C

import mpmath as mp
import numpy as np

import marg_highprec as mh
from isvins_amd import abi, synth

# name: (window id, N, Nvo, landmarks, make_window extras, estimate_extrinsic, marginalised landmarks)
CASES = {
    "n6_l25": (560, 6, 3, 25, {}, 0, 7),
    "n11_l40": (610, 11, 5, 40, {}, 0, 7),
    "n18_l40": (680, 18, 8, 40, {}, 0, 4),
    "n11_l300": (620, 11, 5, 300, {}, 0, 60),                                        # a second, partly filled chunk of 256 lanes in k_marg_fwd
    "n11_host0_l33": (630, 11, 5, 33, dict(host_frames=(0, 1)), 0, 33),               # one row beyond k_marg_fwd's staging of 32
    "n11_host0_l65": (631, 11, 5, 65, dict(host_frames=(0, 1)), 0, 65),               # two stagings and one row
    "n11_none": (632, 11, 5, 40, dict(host_frames=(1, 5)), 0, 0),                     # nothing hosted in frame 0
    "n11_l40_ex": (633, 11, 5, 40, {}, 1, 7),
}
FWD = ("forward_pose_prior", "combined_relpose")
BWD = ("backward_relpose", "backward_vb", "backward_rollpitch")
DIMS = {"forward_pose_prior": 6, "combined_relpose": 6, "backward_relpose": 6, "backward_vb": 9, "backward_rollpitch": 2}
FLOOR_FWD, FLOOR_BWD = 12 * 2.0 ** -53, 21 * 2.0 ** -53


def oracle_run(oracle, cfg, w):
    o = w.clone(); s = abi.isv_summary_t(); m = abi.isv_marg_result_t()
    assert oracle.isvo_optimize(C.byref(cfg), C.byref(o.c()), C.byref(s), C.byref(m)) == 0
    return o, s, m


def solved_window(oracle, wid, N, Nvo, L, extra, ex, margin_old=1):
    """-> (the oracle's solved window, the num_iterations = 0 config of its shape)"""
    w = synth.make_window(wid, n_frames=N, n_vo=Nvo, n_landmarks=L, margin_old=margin_old, **extra)
    kw = dict(max_landmarks=L, max_obs=w.n_obs, estimate_extrinsic=ex)
    o, s, _ = oracle_run(oracle, abi.make_config(N, Nvo, num_iterations=10, **kw), w)
    assert s.iterations > 0
    return o, abi.make_config(N, Nvo, num_iterations=0, **kw)


_SOLVED = {}


def solved_case(oracle, name):
    if name not in _SOLVED:
        _SOLVED[name] = solved_window(oracle, *CASES[name][:6])
    return _SOLVED[name]


def info_of(m, name):
    f = m.combined.relative_pose if name == "combined_relpose" else getattr(m, name)
    U = abi.arr(f.sqrt_info, (DIMS[name], DIMS[name]))
    return U.T @ U


def measured_parts(m):
    return dict(combined_delta_t=m.combined.relative_pose.delta_t, combined_delta_R=m.combined.relative_pose.delta_R,
                backward_delta_t=m.backward_relpose.delta_t, backward_delta_R=m.backward_relpose.delta_R, VB=m.backward_vb.VB,
                rollpitch_R=m.backward_rollpitch.R, forward_t=m.forward_pose_prior.t, forward_R=m.forward_pose_prior.R)


class Reference:
    """marg_forward + marg_backward at 40 digits from `ins` (inputs_from_window), with the yardstick of each quantity"""

    def __init__(self, ins):
        alpha = mp.mpf(float(ins["alpha"]))
        self.f, self.b = mh.marg_forward(ins, "", alpha), mh.marg_backward(ins, "", alpha)
        self.e64 = dict(mh.e64_forward(self.f, alpha), **mh.e64_backward(self.b, alpha))
        self.limit_fwd = mh.float64_limit(mh.to_np(self.f["_fwd_S12"]), self.f["_fwd_eigs"])
        self.limit_bwd = mh.float64_limit(mh.to_np(self.b["_bwd_Lam"]), self.b["_bwd_kept"])
        self.alpha = float(alpha)

    def exact(self, name):
        return mh.to_np((self.b if name in BWD else self.f)[name])

    def yardstick(self, name):
        return max(self.e64[name], self.limit_bwd, FLOOR_BWD) if name in BWD else max(self.e64[name], self.limit_fwd, FLOOR_FWD)

    def check_conditions(self, n_marg):
        """what makes the comparison meaningful; the reference alone must meet it"""
        f, b = self.f, self.b
        assert f["_fwd_rank"] == 6 and min(f["_fwd_eigs"]) >= 100 * self.alpha, (f["_fwd_rank"], f["_fwd_eigs"])
        assert b["_bwd_rank"] == 15, b["_bwd_eigs"]
        kept = [e for e in b["_bwd_eigs"] if e > self.alpha]
        dropped = [e for e in b["_bwd_eigs"] if e <= self.alpha]
        assert len(kept) == 15 and min(kept) >= 100 * self.alpha, kept
        assert len(dropped) == 6 and max(abs(e) for e in dropped) <= 1e-6 * self.alpha, dropped
        assert f["_fwd_n_landmarks"] == n_marg

    def ratios(self, m, names=FWD + BWD):
        """{quantity: (err, e64, limit, err / yardstick)} of a marginalisation record"""
        out = {}
        for name in names:
            e = mh.rel(info_of(m, name), self.exact(name))
            out[name] = (e, self.e64[name], self.limit_bwd if name in BWD else self.limit_fwd, e / self.yardstick(name))
        return out

    def ratio_covrel(self, m):
        e = mh.rel(abi.arr(m.combined.covRel, (6, 6)), mh.to_np(self.f["covRel"]))
        return e, self.e64["covRel"], self.limit_fwd, e / max(self.e64["covRel"], self.limit_fwd, FLOOR_FWD)

    def measurements(self, ins):
        """the measurement parts of the recovered factors at 40 digits -- plain functions of the states"""
        f64 = lambda v: np.array([float(x) for x in v])
        out = {}
        for tag, i, j in (("combined", 0, 1), ("backward", 2, 3)):
            xi, xj = mh.mpv(ins["pose"][i]), mh.mpv(ins["pose"][j])
            Qi, Qj = mh.q_from_pose(xi), mh.q_from_pose(xj)
            out[tag + "_delta_t"] = f64(mh.qrot(mh.q_inv(Qi), [xj[k] - xi[k] for k in range(3)]))
            out[tag + "_delta_R"] = mh.to_np(mh.q_to_R(mh.qmul(mh.q_inv(Qi), Qj))).ravel()
        out["VB"] = np.asarray(ins["sb"][1], float).copy()
        out["rollpitch_R"] = mh.to_np(mh.q_to_R(mh.q_from_pose(mh.mpv(ins["pose"][2])))).ravel()
        out["forward_t"] = np.asarray(ins["pose"][1][:3], float).copy()
        out["forward_R"] = mh.to_np(mh.q_to_R(mh.q_from_pose(mh.mpv(ins["pose"][1])))).ravel()
        return out


def inputs_distance(a, b):
    """largest difference between two inputs_from_window dicts (the byte-recorded structures compared as their doubles)"""
    worst = 0.0
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if x.dtype == np.uint8:
            n = x.size - (0 if k == "imu" else 8)     # the priors end with two int32 (index / imu_i, imu_j / padding); isv_imu_t is all doubles
            assert x[n:].tobytes() == y[n:].tobytes(), k
            x, y = x[:n].view(np.float64), y[:n].view(np.float64)
        if x.size:
            worst = max(worst, float(np.abs(x - y).max()))
    return worst
