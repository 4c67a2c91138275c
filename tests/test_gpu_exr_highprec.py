"""The batched rotation calibration on the MI355X against the 40-digit reading of tests/exr_highprec.py: the walk of
tests/test_exr_highprec.py over the whole case table with a Calibrator in the restatement's place, held to the same exr_cases.K that
was measured on the CPU.  The kernel does not return the F it kept, so the F stage is not part of this walk (it would check the
restatement again); the rotation stage takes the restatement's F of the same frame (the two agree bitwise wherever libm does, and the
bound covers the rest)."""
import pytest

import exr_cases as xc
import exr_oracle as xo
from isvins_amd import exrot as exr
from test_exr_highprec import walk, worst

pytestmark = pytest.mark.gpu


def test_gpu_within_the_float64_limits():
    lib = xo.load()
    rows, results = walk(lib, lambda **cfg: exr.Calibrator(**cfg), f_stage=False)
    w = worst(rows)
    for stage, (ratio, where) in sorted(w.items()):
        print(f"stage {stage:6s} worst error / limit {ratio:10.3f} at {where}  (K {xc.K[stage]})")
    assert set(w) == set(xc.K) - {"F"}                 # (no F stage on the GPU: above)
    bad = [(where, stage, err, lim) for where, stage, err, lim in rows if err > xc.K[stage] * lim]
    assert not bad, bad[:5]
    assert results["excited[7]"].calibrated == 0 and results["excited[8]"].calibrated == 1
