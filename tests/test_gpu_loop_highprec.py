"""k_loop_match / k_loop_pnp (is-vins_amd/csrc/isv_loop.hip) against the 40-digit reference of tests/loop_highprec.py, live on the MI355X.
tests/test_gpu_loop.py holds the kernels to the CPU restatement, which compiles the same text (isv_loop_common.h, isv_pnp.h) and so is the
same reading of the same code; tests/test_loop_highprec.py holds the restatement to the reference.  This test holds the KERNEL to the
reference: status, n_matched, match_index, match_dist, ransac_iters, ransac_inliers, n_final, pnp_iterations, has_loop, loop_index and the
inlier mask identical; PnP_R_old, PnP_T_old, loop_info, res, loop_weight within MARGIN_GPU * max(e64, n 2^-53).  res / loop_weight are
compared on the noisy cases only: on exact data the residual is float32 rounding noise (as tests/test_gpu_loop.py says of its own check).

The cases of a configuration go through ONE verify_batch(per_point=True) on that configuration's handle (100 iterations, 129 iterations,
the L5 case's threshold).  What only the GPU exercises: the speculative chunks of 64 hypotheses (a stop at hypothesis 64, the last of the
first chunk; at 65, where the second chunk is drawn with cnt = 1; a keep inside the second chunk with Lbest surviving the overwrite of
Lmod / Lgood; a third chunk, of one hypothesis, with and without a keep in it) and the 64-lane mask / compaction / pnp_solve loops at 63,
64, 65 and 129 final inliers, with `src` different from the list position.  The new cases run again singly and in a batch of
2 x CUs + 4 pairs that cycles through them: records and per-point arrays must be bytewise the mixed batch's.  Every negative control of
tests/loop_highprec_cases.py (a corruption of the reference, never of the kernel; its power is shown on the CPU) must be rejected by the
GPU's record too.

Host time of the whole reference, measured on one x86-64 core: 19 references and the 6 second RANSACs of the controls take about 100 s
(keep2_f63 25 s, late129 17 s, out60_noise and floor4 10 s each, the two all-outlier runs under keep_no_floor 9 s and 12 s); they are
computed once per process (loop_highprec_cases.reference) and shared with tests/test_loop_highprec.py.  The GPU work of this file is
three mixed batches, the single reruns and three batches of 2 x CUs + 4 pairs: milliseconds.

Measured on one MI355X, error / max(e64, n 2^-53) per case; in brackets the restatement's figure on the host where it differs:
  case          ransac_iters  n_final  pnp_it  PnP_R_old  PnP_T_old     loop_info     res           loop_weight
  stop64        64            17       1       0.264      0.888         1.00          (exact data: not compared)
  stop65        65            24       3       0.156      0.889 (1.11)  1.69 (1.00)   0.806 (0.934) 0.814 (0.936)
  keep2_f63     100           63       3       0.137      2.51          1.14          1.05          1.06
  out60_noise   100           67       3       0.219      1.52          1.45 (0.963)  1.51 (0.617)  1.50 (0.617)
  all_outliers  100           0        -       no model: integers only
  floor4        100           0        -       no model: integers only
  f64           5             64       3       0.025      0.203         0.424         0.514         0.516
  f65           5             65       3       0.097      0.460 (0.233) 0.728         0.411 (1.21)  0.400 (1.19)
  f129          5             129      3       0.076      0.914         0.304         0.981         0.971
  noise2        1             150      3       0.245      1.27 (1.13)   0.102 (0.091) 2.84 (2.11)   3.01 (2.27)
  out30_noise   33            100      3       0.162      0.166         1.15 (0.237)  5.59          4.78
  m17           1             17       3       0.403      1.00          0.939         1.00          1.01
  m200          8             171      3       0.225      0.608 (0.478) 1.00          1.63 (1.10)   1.63 (1.10)
  yaw40         1             150      1       0.098      0.715         (no loop)     (exact data)
  far25         1             150      1       0.313      0.853         (no loop)     (exact data)
  planar        1             150      -       refused: integers only
  none129       129           0        -       no model: integers only
  late129       129           23       3       0.102      0.952         0.271         2.89          2.91
  l5            1             40       3       0.079      0.680         0.276         (exact data)
MARGIN_GPU = 32: 4 x 5.59 = 22.4, rounded up to a power of two; the restatement's MARGIN is the same (its worst is the same 5.59).  No
ratio comes near the 100 that would make it a finding: no kernel finding, nothing under csrc/ changed.  The recorded ransac_iters
include 64, 65, 100 with a last keep at hypothesis 81, and 129 on the second handle with a last keep at hypothesis 128; the recorded
n_final include 63, 64, 65 and 129 (test_recorded_edges).
"""
import pytest
import torch

import loop_cases
import loop_highprec_cases as lc
from isvins_amd import loop

pytestmark = pytest.mark.gpu

NAMES = lc.names()


@pytest.fixture(scope="module")
def handles():
    hs = {k: loop.LoopVerifier(1024, loop_cases.MAX_POINTS, loop_cases.MAX_KEYPOINTS, **kw) for k, kw in lc.CONFIGS.items()}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def batch(handles):
    """{case: (record, match_index, match_dist, inlier)}: one mixed batch per configuration"""
    out = {}
    for key, h in handles.items():
        ns = [n for n in NAMES if lc.CASES[n][1] == key]
        rs, mis, mds, inls = h.verify_batch([lc.pair(n) for n in ns], per_point=True)
        out.update({n: (r, mi, md, inl) for n, r, mi, md, inl in zip(ns, rs, mis, mds, inls)})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_gpu_loop_against_40_digits(batch, name):
    r, mi, md, inl = batch[name]
    ref = lc.reference(name)
    ref.conditions()
    bad, ratios = lc.measure(name, ref, r, mi, md, inl)
    print(f"RATIO gpu {name:13s} status {r.status} n_matched {r.n_matched} ransac_iters {r.ransac_iters} ransac_inliers {r.ransac_inliers} "
          f"n_final {r.n_final} pnp_iterations {r.pnp_iterations}; " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert not bad, (name, bad)
    for k, v in ratios.items():
        assert v <= lc.MARGIN_GPU, (name, k, v)


def test_recorded_edges(batch):
    iters = {n: batch[n][0].ransac_iters for n in NAMES}
    final = {n: batch[n][0].n_final for n in NAMES}
    assert (iters["stop64"], iters["stop65"], iters["out60_noise"], iters["keep2_f63"], iters["none129"], iters["late129"]) == (64, 65, 100, 100, 129, 129)
    assert [final[n] for n in ("keep2_f63", "f64", "f65", "f129")] == [63, 64, 65, 129]


def test_new_cases_bitwise_alone_and_cycled(handles, batch):
    S = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 4
    for key, h in handles.items():
        new = [n for n in lc.NEW if lc.CASES[n][1] == key]
        for n in new:
            r1, mi1, md1, inl1 = h.verify_batch([lc.pair(n)], per_point=True)
            r, mi, md, inl = batch[n]
            assert bytes(r1[0]) == bytes(r) and (mi1[0] == mi).all() and (md1[0] == md).all() and (inl1[0] == inl).all(), n
        idx = [(5 * i + 2) % len(new) for i in range(S)]
        assert set(idx) == set(range(len(new)))
        rs, mis, mds, inls = h.verify_batch([lc.pair(new[k]) for k in idx], per_point=True)
        for i, (r, mi, md, inl) in enumerate(zip(rs, mis, mds, inls)):
            r0, mi0, md0, inl0 = batch[new[idx[i]]]
            assert bytes(r) == bytes(r0) and (mi == mi0).all() and (md == md0).all() and (inl == inl0).all(), (i, new[idx[i]])


@pytest.mark.parametrize("control,name", [(c, n) for c, names in lc.CONTROL_CASES.items() for n in names])
def test_corrupted_reference_is_rejected(batch, control, name):
    r, mi, md, inl = batch[name]
    why = lc.failures(name, lc.reference(name, control), r, mi, md, inl, lc.MARGIN_GPU)
    print(f"CONTROL {control:15s} {name:13s} gpu: {why}")
    assert why, (control, name)
