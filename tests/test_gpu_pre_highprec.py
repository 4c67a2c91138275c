"""k_pre_integrate (is-vins_amd/csrc/isv_preint.hip) live on the MI355X against the 50-digit statement of tests/pre_highprec.py: every
case of tests/pre_highprec_cases.py in ONE run_batch on one handle (want_record, the nav state beside it), the state-carrying
sequences call by call on the same handle, no_walk on a second small handle of its configuration.  Each result and record is judged in
every measure (delta_p / delta_q / delta_v / sum_dt, the jacobian and the covariance per 3 x 3 block, R / P / V) within
PRE_MARGIN x max(route a, route b, 2^-53); blocks that are exactly zero at 50 digits must come back 0.0.  The restatement is not
consulted here: tests/test_gpu_pre.py holds the kernel to it bit for bit, tests/test_pre_highprec.py holds it to the same 50 digits.

Measured on one MI355X (documentation; the margin, 7.5, comes from the CPU routes alone): the kernel's error per case and measure in
units of u = 2^-53 and, in brackets, as a multiple of e_ref = max(route a, route b, u).  The worst multiple is 1.86 (n65, V).  The
record's columns often show 1.00 because the oracle's dense step forms the same products as the kernel and adding exact zeros changes
no sum; the numpy route is the independent one there.

  case                    delta_p      delta_q      delta_v      sum_dt       J            C            R            P            V
  n1                      0.7 (0.66)   0.9 (0.89)   1.0 (1.00)   0.0 (0.00)   0.9 (0.92)   1.8 (1.00)   1.2 (1.00)   0.7 (0.74)   0.5 (0.52)
  n2                      0.1 (0.15)   1.1 (1.00)   0.8 (0.75)   0.6 (0.59)   1.7 (1.00)   3.1 (1.00)   1.4 (1.00)   0.3 (0.33)   1.0 (1.00)
  n10                     0.8 (0.83)   0.1 (0.11)   1.7 (1.00)   0.3 (0.35)   3.7 (1.00)   5.3 (1.00)   4.9 (1.00)   2.6 (1.00)   2.6 (0.81)
  n64                     0.1 (0.06)   0.4 (0.29)   1.8 (1.00)   0.5 (0.53)   6.7 (0.83)   14.0 (1.00)  3.6 (0.47)   0.7 (0.20)   3.6 (1.00)
  n65                     1.1 (1.00)   0.5 (0.53)   2.0 (1.00)   2.2 (1.00)   9.4 (1.00)   16.4 (0.94)  6.8 (1.00)   0.8 (0.30)   6.1 (1.86)
  n_max                   3.9 (1.00)   0.8 (0.82)   2.8 (1.00)   3.1 (1.00)   8.3 (0.93)   17.1 (1.00)  6.7 (0.81)   6.6 (1.00)   4.1 (1.00)
  zero_gyro               1.0 (0.98)   0.0 (0.00)   1.9 (1.00)   1.9 (1.00)   1.9 (0.74)   5.4 (0.84)   1.8 (1.00)   3.6 (1.00)   1.6 (1.58)
  big_rotation            0.9 (0.45)   0.9 (0.76)   1.0 (1.00)   0.9 (0.94)   2.2 (0.77)   4.1 (0.73)   4.2 (1.29)   2.2 (1.00)   0.9 (0.91)
  dt0                     0.7 (0.70)   0.2 (0.21)   0.7 (0.73)   0.0 (0.00)   2.6 (1.00)   3.2 (0.67)   2.9 (1.00)   0.6 (0.55)   0.7 (0.72)
  tiny_dt                 1.0 (1.00)   0.3 (0.26)   0.6 (0.62)   1.7 (1.00)   2.2 (0.97)   3.6 (1.00)   4.3 (1.00)   0.3 (0.26)   0.2 (0.16)
  long_dt                 0.6 (0.59)   0.7 (0.69)   0.5 (0.47)   1.5 (1.00)   2.2 (1.00)   7.6 (0.92)   1.3 (0.43)   2.3 (0.94)   1.1 (1.00)
  saturated               1.2 (1.00)   0.9 (0.85)   1.9 (1.00)   0.9 (0.94)   5.3 (1.00)   9.8 (1.00)   4.8 (1.22)   3.2 (1.00)   1.8 (0.76)
  big_bias                0.4 (0.42)   0.5 (0.51)   0.3 (0.34)   0.7 (0.69)   2.1 (1.00)   5.1 (1.00)   1.8 (0.57)   1.9 (1.00)   3.0 (1.00)
  far_nav                 1.4 (1.00)   0.9 (0.88)   0.3 (0.26)   0.8 (0.76)   2.6 (1.00)   5.9 (1.00)   5.1 (1.00)   1.1 (1.00)   0.5 (0.46)
  no_walk                 0.5 (0.46)   0.0 (0.01)   0.6 (0.61)   0.5 (0.55)   3.0 (1.00)   2.0 (1.00)   2.8 (1.00)   1.8 (1.00)   0.4 (0.44)
  seq_split               0.8 (0.79)   0.1 (0.07)   0.2 (0.17)   0.1 (0.06)   3.3 (1.00)   7.1 (1.00)
  seq_merge               0.2 (0.21)   0.6 (0.59)   0.2 (0.23)   0.8 (0.82)   3.2 (1.00)   7.6 (1.00)
  seq_repropagate_changed 0.8 (0.82)   0.8 (0.77)   0.7 (0.69)   0.1 (0.06)   3.0 (1.00)   6.9 (1.00)
  seq_reset_used          0.6 (0.59)   0.9 (0.88)   1.3 (1.00)   0.6 (0.63)   1.1 (1.00)   2.5 (1.00)"""
import numpy as np
import pytest

import pre_cases as pc
import pre_highprec_cases as hc
from isvins_amd import preint as pre

pytestmark = pytest.mark.gpu
OK = pre.ISV_PRE_OK
BATCH = [n for n in hc.CASES if n != "no_walk"]


@pytest.fixture(scope="module")
def live():
    """name -> the dict pre_highprec.errors takes, from the GPU"""
    g = pre.PreIntegrator(hc.SLOTS, **pc.CFG)
    nw = pre.PreIntegrator(2, acc_w=0.0, gyr_w=0.0, **pc.CFG)
    out = {}
    try:
        res, recs = g.run_batch([hc.CASES[n].item(i) for i, n in enumerate(BATCH)])
        (r,), (c,) = nw.run_batch([hc.CASES["no_walk"].item(1)])
        for n, r, c in list(zip(BATCH, res, recs)) + [("no_walk", r, c)]:
            assert r.status == OK and r.n_buffered == hc.CASES[n].n and c is not None, n
            assert all(np.array_equal(np.array(getattr(r, f)), np.array(getattr(c, f))) for f in ("delta_p", "delta_q", "delta_v", "sum_dt")), n
            out[n] = hc.got_of(r, c, nav=True)
        for k, n in enumerate(hc.SEQUENCES):
            calls = pc.play(g, n, len(BATCH) + 2 * k)
            assert all(r.status == OK for res, _ in calls for r in res), n
            out["seq_" + n] = hc.got_of(calls[-1][0][0], calls[-1][1][0])
    finally:
        g.close(); nw.close()
    return out


@pytest.mark.parametrize("name", list(hc.ALL))
def test_gpu_pre_integration_against_50_digits(live, name):
    faults, over = hc.judge(name, live[name], "gpu")
    assert not faults, (name, faults)
    assert not over, (name, [(m, e / hc.U, b / hc.U) for m, e, b in over])


def test_gpu_record_structure(live):
    for name, got in live.items():
        assert np.array_equal(got["J"][9:], np.eye(15)[9:]), name              # the bias rows are the identity's
        assert not got["J"][3:6, 9:12].any(), name                             # the rotation does not depend on ba
    C = live["no_walk"]["C"]
    assert not C[9:, :].any() and not C[:, 9:].any() and C[:9, :9].any()       # no bias walk: exact zeros
