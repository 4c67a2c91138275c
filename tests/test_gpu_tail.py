"""The tail of the solve on four wavefronts per window -- k_finalize<256> (prior updates, double2vector, depths, the clear of
the marginalisation record) and k_marg_bwd<3> (MargBackward in one launch) -- against the one-wavefront forms it replaces
(ISV_TAIL_ONE_WAVE=1: k_finalize<64> + k_marg_clear, and k_marg_bwd<2> or build / k_marg_jacobi / project by the handle's
max_batch) and against the three-launch MargBackward (ISV_MARG_SPLIT=1).

The four-wavefront forms change no arithmetic, only which lanes run it and when: every comparison is BYTEWISE -- window
states, depths and solve flags, the Linear9 / SE3 / relative-pose / roll-pitch priors, the summaries, and the whole
isv_marg_result_t.  The hooks are read when a handle is created; each of the three modes runs all cases in one fresh child
process of its own, and the parent compares what the children recorded.

Shapes: 40 landmarks (nothing in the tail depends on their count beyond the depth loop: 40 is less than one pass of 64
lanes), three windows of which the middle one has margin_old = 0 (the marginalisation kernels' early return beside two
working workgroups), N = 11 / 18 / 6; a handle of max_batch = 1100 (more than 3 x CUs: the hook side takes k_marg_bwd<2>);
the free-extrinsic instantiation; and initFactorGraph, which runs k_finalize without the prior updates."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"default": {}, "one_wave": {"ISV_TAIL_ONE_WAVE": "1"}, "marg_split": {"ISV_MARG_SPLIT": "1"}}
HOOKS = ("ISV_TAIL_ONE_WAVE", "ISV_MARG_SPLIT", "ISV_MARG_ONE_KERNEL")
# name: (N, Nvo, max_batch, estimate_extrinsic, initFactorGraph)
CASES = {
    "n11": (11, 5, 3, 0, False),
    "n18": (18, 8, 3, 0, False),
    "n6": (6, 3, 3, 0, False),
    "n11_handle_of_1100": (11, 5, 1100, 0, False),
    "n11_free_extrinsic": (11, 5, 3, 1, False),
    "n11_init_factor_graph": (11, 5, 3, 0, True),
}
N_LM = 40


def _raw(x):
    return bytes(C.string_at(C.addressof(x), C.sizeof(x)))


def _window_record(w):
    rec = {name: getattr(w, name).tobytes() for name in ("Ps", "Rs", "Vs", "Bas", "Bgs", "tic", "ric", "lm_depth", "lm_solve_flag",
                                                         "para_Pose", "para_SpeedBias", "para_Ex_Pose", "para_Feature")}
    rec["pose_prior"] = _raw(w.pose_prior); rec["vb_prior"] = _raw(w.vb_prior)
    rec["relpose"] = _raw(w.relpose); rec["rollpitch"] = _raw(w.rollpitch)
    return rec


def _child(out_path):
    """all cases on this process's handles (the hooks are in the environment); the records go to out_path"""
    sys.path.insert(0, ROOT)
    import isvins_loader
    isvins_loader.load()
    from isvins_amd import backend, synth
    out = {}
    for name, (N, Nvo, max_batch, ex, init) in CASES.items():
        ws = [synth.make_window(500 + 10 * N + i, n_frames=N, n_vo=Nvo, n_landmarks=N_LM, margin_old=0 if i == 1 else 1) for i in range(3)]
        be = backend.Backend(N, Nvo, max_landmarks=N_LM, max_obs=max(w.n_obs for w in ws), max_batch=max_batch, estimate_extrinsic=ex)
        try:
            if init:
                sums, klds = be.init_factor_graph_batch(ws)
                out[name] = {"windows": [_window_record(w) for w in ws], "summaries": [_raw(s) for s in sums], "klds": klds.tobytes()}
            else:
                be.upload(ws); be.run_optimize(); sums, margs = be.download(ws)          # isv_batch_upload / _optimize / _download
                out[name] = {"windows": [_window_record(w) for w in ws], "summaries": [_raw(s) for s in sums], "margs": [_raw(m) for m in margs],
                             "valid": [int(m.valid) for m in margs], "iterations": [int(s.iterations) for s in sums]}
        finally:
            be.close()
    with open(out_path, "wb") as f:
        pickle.dump(out, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tail")
    res = {}
    for mode, hooks in MODES.items():
        env = {k: v for k, v in os.environ.items() if k not in HOOKS}
        env.update(hooks)
        path = str(d / (mode + ".pkl"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (mode, p.stdout[-2000:], p.stderr[-2000:])
        with open(path, "rb") as f:
            res[mode] = pickle.load(f)
    return res


def test_the_cases_do_the_work_they_are_meant_to(runs):
    """windows 0 and 2 were marginalised (the record is valid), window 1 took the early return and its record is the cleared
    one (all zero bytes: the clear folded into k_finalize<256> as k_marg_clear's); every window was solved"""
    for name, (N, Nvo, max_batch, ex, init) in CASES.items():
        r = runs["default"][name]
        if init:
            continue
        assert r["valid"] == [1, 0, 1], name
        assert r["margs"][1] == bytes(len(r["margs"][1])), name
        assert all(it > 0 for it in r["iterations"]), name


@pytest.mark.parametrize("other", ["one_wave", "marg_split"])
@pytest.mark.parametrize("case", list(CASES))
def test_four_wavefront_tail_is_bytewise_the_other_forms(runs, case, other):
    a, b = runs["default"][case], runs[other][case]
    assert a.keys() == b.keys()
    for i, (wa, wb) in enumerate(zip(a["windows"], b["windows"])):
        for field in wa:
            assert wa[field] == wb[field], (case, other, "window", i, field)
    for key in ("summaries", "margs", "klds"):
        if key in a:
            assert a[key] == b[key], (case, other, key)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2])
