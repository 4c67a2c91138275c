"""k_relpose (is-vins_amd/csrc/isv_relpose.hip) against the 40-digit reference of tests/relpose_highprec.py, live on the MI355X.
tests/test_gpu_relpose.py holds the kernel to the CPU restatement, which compiles the same text (isv_init_common.h) and so is the same reading
of the same code; tests/test_relpose_highprec.py holds the restatement to the reference.  This test holds the KERNEL to the reference: status,
l, n_candidates, n_corres, ransac_iters, ransac_inliers, recover_inliers and the per-track mask identical, the parallax within
(count + 4) 2^-53, excitation_var / relative_R / relative_T within MARGIN_GPU * max(e64, n 2^-53), or MARGIN_CV * max(e64, ecv, n 2^-53) where the
kept model comes from solveCubic's one-real-root branch (tests/relpose_cases.py).

All cases of tests/relpose_cases.py go through ONE relpose_batch.  What only the GPU exercises: the 64-track ballot compaction with a prefix
carried across passes (spanning tracks up to index 263 of the track list), the second and third pass of the kept model's mask loop and of the
four cheirality ballots (64, 65 and 129 correspondences), Lp / Lpar / Ltrk / Lm indexed past 63, the in-order parallax sum of 129 terms, and
the speculative chunks' edges (a stop at hypothesis 64, the last of the first chunk, and at 65, the first of the second; the last chunk cut
to niters - iter; a keep in a later chunk).  The new cases run again singly and in a batch of 2 x CUs + 4 problems that cycles through them:
records and masks must be bytewise the mixed batch's.  Every negative control of tests/relpose_cases.py (a corruption of the reference, never
of the kernel; its power is shown on the CPU) must be rejected by the GPU's record too.

Measured on one MI355X, error / yardstick per case (the restatement's figures on the host are the same to three digits; excitation_var is at
most 1.0 and the parallax at most 0.11 of its limit everywhere; cv: a one-root model, measured against the yardstick with ecv):
  case            relative_R  relative_T      case      relative_R  relative_T      case      relative_R  relative_T
  c21_exact  cv   0.008       0.011           old_0 cv  0.84        0.90            old_7     0.36        0.20
  c63_stop64      1.71        1.48            old_1 cv  0.15        0.089           old_8     0.80        4.65
  c64_noise       0.27        1.23            old_2     3.09        15.5            old_9     1.09        1.22
  c65_noise       1.08        12.5            old_3 cv  0.013       0.014           old_10    0.50        1.38
  c65_exact       3.83        3.58            old_4 cv  0.032       0.040           old_11    0.30        0.82
  c129_stop65     0.17        4.31            old_5 cv  0.51        0.52            old_12 cv 0.023       0.021
  c129_mixed      0.57        7.86            old_6     1.79        2.43
  c40_late        0.35        1.27            c29_cap   0.60        0.61
  c30_stop_early  1.79        0.21            far0_then1 1.75       4.10
MARGIN_GPU = 64: 4 x 15.5 = 62, rounded up to a power of two; MARGIN_CV = 4: 4 x 0.90 = 3.6.  No ratio reaches the 100 that would make it a
finding; the one finding of this comparison is in the definition, not in the kernel (solveCubic's 12-digit cube-root
exponent, which is what ecv measures)."""
import pytest
import torch

import relpose_cases as rc
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

NAMES = rc.names()


@pytest.fixture(scope="module")
def be():
    b = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    yield b
    b.close()


@pytest.fixture(scope="module")
def batch(be):
    """{case: (problem, record, mask)} from the one mixed batch"""
    ps = [rc.problem(n) for n in NAMES]
    rs, ms = initial.relpose_batch(be, ps, masks=True)
    return {n: (p, r, m) for n, p, r, m in zip(NAMES, ps, rs, ms)}


@pytest.mark.parametrize("name", NAMES)
def test_gpu_relpose_against_40_digits(batch, name):
    _, res, mask = batch[name]
    ref = rc.reference(name)
    ref.conditions()
    bad, ratios = rc.measure(ref, res, mask)
    print(f"RATIO gpu {name:15s} " + " ".join(f"{k} {r:.3g}" for k, r in ratios.items()))
    assert not bad, (name, bad)
    for k, r in ratios.items():
        assert r <= rc.margin_of(k, rc.MARGIN_GPU), (name, k, r)


def test_new_cases_bitwise_alone_and_cycled(be, batch):
    new = list(rc.NEW)
    for n in new:
        p, r, m = batch[n]
        r1, m1 = initial.relpose_batch(be, [p], masks=True)
        assert bytes(r1[0]) == bytes(r) and (m1[0] == m).all(), n
    S = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 4
    idx = [(5 * i + 2) % len(new) for i in range(S)]
    rs, ms = initial.relpose_batch(be, [batch[new[k]][0] for k in idx], masks=True)
    assert set(idx) == set(range(len(new)))
    for i, (r, m) in enumerate(zip(rs, ms)):
        _, r0, m0 = batch[new[idx[i]]]
        assert bytes(r) == bytes(r0) and (m == m0).all(), (i, new[idx[i]])


@pytest.mark.parametrize("control,name", [(c, n) for c, names in rc.CONTROL_CASES.items() for n in names])
def test_corrupted_reference_is_rejected(batch, control, name):
    _, res, mask = batch[name]
    why = rc.failures(rc.reference(name, control), res, mask, rc.MARGIN_GPU)
    print(f"CONTROL {control:18s} {name:15s} gpu: {why}")
    assert why, (control, name)
