"""MargForward / MargBackward as the HIP kernels of TODAY compute them -- k_marg_fwd<256> / <64>, k_marg_bwd<3> (isv_marg.hip) -- against
the 40-digit recomputation of tests/marg_highprec.py, live on the MI355X.  tests/test_gpu_tail.py says the four-wavefront forms are
bytewise the one-wavefront ones, tests/test_gpu_solve.py::check_marg that the GPU is within 1e-6 of the CPU oracle, and
tests/test_marg_third_opinion.py reads device numbers recorded long ago: none says how far today's kernels are from the exact answer.

Cases, yardstick and conditions: tests/marg_cases.py (the CPU oracle's side of the same comparison: tests/test_marg_highprec.py).  The handle
has num_iterations = 0 and is fed the ORACLE's solved window; the reference is recomputed from the GPU's own downloaded para_* and
post-update priors (asserted equal to the oracle side's to 1e-15; measured <= 2.8e-16), so the comparison sees the marginalisation's
rounding alone.  max_batch = 2: k_marg_fwd<256> and k_marg_bwd<3>.  Why these shapes: k_marg_fwd compacts the landmarks hosted in frame 0
by ballot per chunk of MTF lanes and stages their rows 32 at a time -- 33 and 65 marginalised landmarks cross the staging once and twice,
300 landmarks (60 of them scattered hosts in frame 0) fill a second chunk partly, n11_none has no slot at all; N = 6 / 11 / 18 move Nvo
and with it the frame pair MargBackward reads; one case frees the extrinsic.  k_marg_fwd<64> (batches above 2 x CUs) has a test of its
own below (full_batch_w*: window ids 560, 562, 563 of the n6_l25 shape).

A value passes when err_gpu <= MARGIN * max(e64, float64_limit, floor); one margin forward (with covRel), one backward; each 4 x the
worst ratio measured on one MI355X, rounded up to a power of two.  Measured (documentation; the margins are derived from it by hand),
err_gpu and err_gpu / yardstick:

  case            forward_pose_prior combined_relpose   covRel             backward_relpose   backward_vb        backward_rollpitch
  n6_l25          9.2e-14  0.691     5.9e-13  4.392     4.9e-13  3.643     6.2e-07  1.098     4.1e-07  0.717     1.0e-08  0.018
  n11_l40         3.2e-13  1.919     6.2e-13  3.629     3.4e-13  2.026     2.2e-07  0.403     1.4e-07  0.255     2.7e-09  0.005
  n18_l40         5.1e-14  0.601     3.6e-13  4.205     1.3e-13  1.500     3.1e-07  0.561     2.1e-07  0.385     1.3e-08  0.025
  n11_l300        4.9e-13  0.596     5.8e-13  0.709     7.4e-13  0.908     3.5e-07  0.632     2.3e-07  0.414     1.2e-08  0.022
  n11_host0_l33   3.4e-13  0.654     6.0e-13  1.161     6.9e-13  1.342     1.0e-07  0.114     7.0e-08  0.114     2.7e-09  0.005
  n11_host0_l65   3.0e-13  0.352     6.1e-13  0.711     8.5e-13  0.999     2.7e-07  0.498     1.9e-07  0.343     5.3e-09  0.010
  n11_none        9.0e-16  0.020     1.0e-15  0.022     8.4e-16  0.018     2.2e-07  0.375     1.4e-07  0.245     4.9e-09  0.008
  n11_l40_ex      9.7e-15  0.051     6.5e-16  0.003     1.1e-15  0.006     5.6e-07  0.878     3.6e-07  0.631     3.0e-09  0.005
  full_batch_w0   9.2e-14  0.691     5.9e-13  4.392     4.9e-13  3.643     6.2e-07  1.098     4.1e-07  0.717     1.0e-08  0.018
  full_batch_w2   3.2e-13  1.994     5.5e-13  3.459     6.8e-13  4.237     4.2e-07  0.726     2.8e-07  0.476     1.0e-08  0.018
  full_batch_w3   3.4e-13  1.740     5.9e-13  3.042     4.5e-13  2.305     1.4e-07  0.259     9.5e-08  0.176     1.8e-09  0.003

Forward: worst 4.392 -> MARGIN_FWD = 32 (17.6); the closed-form landmark downdates keep the pose prior at 1e-13, where the oracle's
full-pivot LU is at 2e-11 (ratio 150, tests/test_marg_highprec.py).  Backward: worst 1.098 -> MARGIN_BWD = 8 (4.39): the kernels sit
AT the cancellation limit of double precision (5.5e-7 on these windows), like the oracle (0.88) and plain numpy (e64 up to 9e-7).  No
ratio comes near the 100 that would make it a finding: the Gauss-Jordan of the 9 x 9 speed/bias block, the Jacobi stopping rule and
the landmark downdates lose nothing beyond what the format does.  full_batch_w0 (k_marg_fwd<64>) repeats n6_l25 (k_marg_fwd<256>) digit
for digit.

The measurement parts (delta_t, delta_R, VB, R, forward t / R) are plain functions of the states: 1e-12 against the 40-digit values
(measured <= 1.7e-16)."""
import ctypes as C
import re

import numpy as np
import pytest

import marg_cases as mc
import marg_highprec as mh
from isvins_amd import abi, backend

pytestmark = pytest.mark.gpu

MARGIN_FWD = 32.0            # forward_pose_prior, combined_relpose, covRel: 4 x 4.392 = 17.6 -> 32
MARGIN_BWD = 8.0             # backward_relpose, backward_vb, backward_rollpitch: 4 x 1.098 = 4.39 -> 8


def raw(x):
    return bytes(C.string_at(C.addressof(x), C.sizeof(x)))


def compare(tag, ref, m):
    """{quantity: (err_gpu, e64, float64_limit, err_gpu / yardstick)} of the record `m`, printed"""
    res = ref.ratios(m)
    res["covRel"] = ref.ratio_covrel(m)
    for k, (e, e64, lim, r) in res.items():
        print(f"RATIO {tag} {k:20s} err_gpu {e:.2e} e64 {e64:.2e} limit {lim:.2e} ratio {r:.3f}")
    return res


def margin_of(k):
    return MARGIN_BWD if k in mc.BWD else MARGIN_FWD


def check_against_40_digits(tag, ins, m, n_marg):
    """the record `m` of one marginalised window against the reference recomputed from that window's own inputs"""
    ref = mc.Reference(ins)
    ref.check_conditions(n_marg)
    assert m.valid == 1 and m.n_marg_landmarks == n_marg
    for name in mc.FWD + mc.BWD:
        f = m.combined.relative_pose if name == "combined_relpose" else getattr(m, name)
        U = abi.arr(f.sqrt_info, (mc.DIMS[name], mc.DIMS[name]))
        assert not np.tril(U, -1).any() and np.isfinite(U).all(), (tag, name)
    res = compare(tag, ref, m)
    want = ref.measurements(ins)
    dev = {k: float(np.abs(abi.arr(v) - want[k]).max()) for k, v in mc.measured_parts(m).items()}
    print(f"MEAS  {tag} " + " ".join(f"{k} {d:.1e}" for k, d in dev.items()))
    for k, (e, e64, lim, r) in res.items():
        assert r <= margin_of(k), (tag, k, e, e64, lim, r)
    for k, d in dev.items():
        assert d < 1e-12, (tag, k, d)


_RUNS = {}


def gpu_run(oracle, name):
    """-> (inputs rebuilt from the GPU's downloaded window, its marginalisation record), once per case"""
    if name in _RUNS:
        return _RUNS[name]
    wid, N, Nvo, L, extra, ex, n_marg = mc.CASES[name]
    o, cfg0 = mc.solved_case(oracle, name)
    assert o.margin_old == 1
    o2, so, mo = mc.oracle_run(oracle, cfg0, o)
    backend.build()
    be = backend.Backend(N, Nvo, max_landmarks=L, max_obs=o.n_obs, max_batch=2, num_iterations=0, estimate_extrinsic=ex)
    try:
        g = o.clone()
        sg, mg = be.optimize(g)
    finally:
        be.close()
    assert sg.iterations == 0 and so.iterations == 0
    ins = mh.inputs_from_window(be.cfg, g)
    d_in = mc.inputs_distance(ins, mh.inputs_from_window(cfg0, o2))
    print(f"INPUT {name} GPU inputs against the oracle side's: {d_in:.1e}")
    assert d_in <= 1e-15
    _RUNS[name] = (ins, mg)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(mc.CASES))
def test_gpu_marginalisation_against_40_digits(oracle, name):
    ins, mg = gpu_run(oracle, name)
    check_against_40_digits(name, ins, mg, mc.CASES[name][6])


def test_gpu_marg_forward_one_wavefront_form_in_a_full_batch(oracle, capfd, monkeypatch):
    """k_marg_fwd<64> is launched for batches above twice the CU count only: 2 x CUs + 4 windows of (N, Nvo) = (6, 3), four distinct
    ones cycled (the second with margin_old = 0: the early return beside working workgroups).  Every copy's record is bytewise the
    first copy's, and the three marginalised originals pass the 40-digit comparison above."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus + 4
    wid, N, Nvo, L, extra, ex, n_marg = mc.CASES["n6_l25"]
    four = [mc.solved_window(oracle, wid + i, N, Nvo, L, extra, ex, margin_old=0 if i == 1 else 1)[0] for i in range(4)]
    backend.build()
    monkeypatch.setenv("ISV_DEBUG_PATH", "1")                     # (read when the handle is created)
    be = backend.Backend(N, Nvo, max_landmarks=L, max_obs=max(w.n_obs for w in four), max_batch=B, num_iterations=0)
    monkeypatch.delenv("ISV_DEBUG_PATH")
    try:
        batch = [four[i % 4].clone() for i in range(B)]
        capfd.readouterr()
        sums, margs = be.optimize_batch(batch)
        said = capfd.readouterr().err
    finally:
        be.close()
    assert int(re.search(r"isv: enqueue B=(\d+)", said).group(1)) == B > 2 * cus           # (isv_solver_enqueue: d.B > 2 n_cus -> k_marg_fwd<64>)
    recs = [raw(m) for m in margs]
    assert [m.valid for m in margs[:4]] == [1, 0, 1, 1] and recs[1] == bytes(len(recs[1]))
    assert len({recs[0], recs[2], recs[3]}) == 3
    for i in range(4, B):
        assert recs[i] == recs[i % 4], i
    for i in (0, 2, 3):
        assert sums[i].iterations == 0
        ins = mh.inputs_from_window(be.cfg, batch[i])
        check_against_40_digits(f"full_batch_w{i}", ins, margs[i], len(mh.selected_landmarks(four[i])))


# ---- the check must be able to fail ---------------------------------------------------------------------------------------
def _drop_the_row_beyond_the_staging(ins):
    """the 33rd marginalised landmark -- the one row of k_marg_fwd's second staging of 32 -- missing from the REFERENCE"""
    return dict(ins, lam=ins["lam"][:32], pts=ins["pts"][:32])


def _speed_bias_prior_off_by_1e_5(ins):
    """the speed/bias prior's sqrt_info scaled by 1 + 1e-5 in the REFERENCE: the recovered information moves by 2e-5, forty times the
    float64 limit -- what a MargBackward that lost two more digits would show, and what check_marg's 1e-6 against the oracle would
    see only as a 20-fold excess of a bound that its two sides already fill"""
    vb = mh.struct_of(abi.isv_linear9_t, ins["vb_prior"])
    for k in range(81):
        vb.sqrt_info[k] *= 1.0 + 1e-5
    return dict(ins, vb_prior=mh.raw(vb))


@pytest.mark.parametrize("corruption,hit", [(_drop_the_row_beyond_the_staging, mc.FWD + ("covRel",)), (_speed_bias_prior_off_by_1e_5, mc.BWD)],
                         ids=["drop_the_row_beyond_the_staging", "speed_bias_prior_off_by_1e_5"])
def test_corrupted_reference_is_rejected(oracle, corruption, hit):
    """negative control on n11_host0_l33: no fault goes into a kernel -- the reference is corrupted, and the comparison that passes
    above must reject every quantity the corruption reaches (measured on the CPU with the oracle's record: 7e9 / 7e10 / 9e10
    yardsticks forward, 17 / 25 / 37 backward) and no other"""
    ins, mg = gpu_run(oracle, "n11_host0_l33")
    res = compare(corruption.__name__[1:], mc.Reference(corruption(ins)), mg)
    for k, (e, e64, lim, r) in res.items():
        assert (r > margin_of(k)) == (k in hit), (k, e, e64, lim, r)
