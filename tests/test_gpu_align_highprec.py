"""k_visual_imu_align (is-vins_amd/csrc/isv_initial.hip) against the 40-digit model of tests/align_highprec.py, stage by stage, live on the
MI355X.  tests/test_gpu_align.py holds the kernel to the CPU restatement, which was written from the same reading of the reference;
tests/test_align_highprec.py holds the restatement to the model.  This test holds the KERNEL to the model, each stage recomputed from the
GPU result's own preceding outputs, with the float64 limit itself as the bound on the three solve stages (margin 1) and 16 yardsticks on
the closed-form rebuild.  The limits are 100 to 1e5 times tighter than test_gpu_align.py's round tolerances (tests/align_cases.py asserts
10 at least, and names the one exception).

All cases of tests/align_cases.py go through ONE align_batch: the batch's nf_max is 40, so every smaller case runs in the LDS carve-up of
the largest.  The 4-, 21- and 40-frame cases are also solved alone (nf_max = 4, 21, 40) and must come back bytewise.  What only the GPU
exercises: the 64-lane strides of the LDLT's column updates and of the entry-strided assembly (n = 64 fills one stride, n = 67 wraps),
the packed triangle's index arithmetic up to n = 124, and the carve-up.

Every negative control of tests/align_cases.py (a corruption of the model, never of the kernel; its power is shown on the CPU) must be
rejected by the GPU's record too.

The kernel's header says that its result matches the restatement operation by operation; up to g_c0 both sides use + - * / and sqrt only,
with contraction off, so the fields of align_cases.BYTEWISE_FIELDS must be bytewise equal between the two (the fields after the rebuild pass
through atan2 / sin / cos of two different math libraries).  test_bytewise_against_the_restatement asserts it.

Measured on one MI355X: the table in DESIGN.md section 11."""
import numpy as np
import pytest

import align_cases as ac
import align_highprec as ah
import align_oracle
from isvins_amd import backend, initial

pytestmark = pytest.mark.gpu

NAMES = list(ac.CASES)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return align_oracle.build(tmp_path_factory.mktemp("init_oracle"))


@pytest.fixture(scope="module")
def be():
    b = backend.Backend(11, 5, max_landmarks=64, max_obs=704, max_batch=1)
    yield b
    b.close()


@pytest.fixture(scope="module")
def batch(be):
    """{case: (problem, its record from the one mixed batch)} and the cache of 40-digit references built on those records"""
    ps = [ac.problem(n) for n in NAMES]
    assert max(p.c.n_frames for p in ps) == initial.ISV_ALIGN_MAX_FRAMES
    rs = initial.align_batch(be, ps)
    return {n: (p, r) for n, p, r in zip(NAMES, ps, rs)}, {}


def reference(batch, name):
    runs, refs = batch
    if name not in refs:
        p, r = runs[name]
        assert r.status == 0, (name, initial.STAGES[r.status])
        refs[name] = ac.Reference(name, p, r)
    return refs[name]


@pytest.mark.parametrize("name", ac.ALONE)
def test_alone_is_bytewise_the_mixed_batch(be, batch, name):
    p, r = batch[0][name]
    alone = initial.align_batch(be, [p])[0]
    assert bytes(alone) == bytes(r), name


@pytest.mark.parametrize("name", NAMES)
def test_gpu_alignment_against_40_digits(batch, name):
    ref = reference(batch, name)
    ref.check_conditions()
    ratios = ref.ratios()
    worst = ac.report("gpu", name, ratios)
    for s, r in worst.items():
        assert r <= 1.0, (name, s, ratios[s])


def test_worst_ratio_per_stage(batch):
    """over all cases, for the record: at most 1 on the solve stages, at most 16 yardsticks on the rebuild"""
    per_case = [reference(batch, n).ratios() for n in NAMES]
    worst = {s: max(max(r[s].values()) for r in per_case) for s in ah.STAGES}
    print("WORST gpu " + " ".join(f"{s} {w:.3f}" for s, w in worst.items()) + f" (rebuild: {16.0 * worst['rebuild']:.3f} yardsticks)")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("control,name", [(c, n) for c, names in ac.CONTROL_CASES.items() for n in names])
def test_corrupted_model_is_rejected(batch, control, name):
    rej = reference(batch, name).rejects(control)
    print(f"CONTROL {control:20s} {name:12s} gpu / corrupted model {rej:.3g}")
    assert rej > 1.0, (control, name, rej)


@pytest.mark.parametrize("name", NAMES)
def test_bytewise_against_the_restatement(lib, batch, name):
    p, rg = batch[0][name]
    ro = align_oracle.solve(lib, p)
    assert rg.status == ro.status == 0 and rg.n_state == ro.n_state
    inp = ah.Inputs(p)
    vg, vo = ah.result_values(inp, rg), ah.result_values(inp, ro)
    vg["rp_delta_q"], vo["rp_delta_q"] = rg.arr("rp_delta_q")[:inp.nf], ro.arr("rp_delta_q")[:inp.nf]
    bad = []
    for k in ac.BYTEWISE_FIELDS:
        a, b = np.ascontiguousarray(vg[k]).ravel(), np.ascontiguousarray(vo[k]).ravel()
        if a.tobytes() != b.tobytes():
            ulps = np.abs(a.view("i8") - b.view("i8"))
            bad.append(k)
            print(f"BYTEWISE {name} {k}: {int((ulps != 0).sum())} of {a.size} values differ, at most {int(ulps.max())} ulps")
    assert not bad, (name, bad)
