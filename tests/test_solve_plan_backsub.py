"""Where the landmark back-substitution runs (UploadPlan::bsub_in_solve, is-vins_amd/csrc/isv_solve_plan.h), on the CPU through the
stand-alone program tests/native/solve_plan_backsub_print.cpp built under AddressSanitizer + UBSan (runtimes linked statically; nothing
is loaded into Python).  The field is on when the handle solves with k_build_solve_st, the upload takes the fused LDS path, the window
is short (the 256-thread instantiation), the extrinsic is constant and k_backsub_split does not run; ISV_BSUB_IN_DOGLEG turns it off.
The cases are shaped with test_solve_plan.words (a handle as isv_backend_create shapes it, 256 CUs)."""
import os
import re
import subprocess

import pytest

import test_solve_plan as tsp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = tmp_path_factory.mktemp("solve_plan_backsub") / "solve_plan_backsub_print"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "native", "solve_plan_backsub_print.cpp"), "-o", str(exe)])

    def run(cases):
        text = "".join(f"case={name} " + " ".join(f"{k}={v}" for k, v in words.items()) + "\n" for name, words in cases.items())
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        res = {}
        for line in out.stdout.splitlines():
            res[re.match(r"case (\S+) ", line).group(1)] = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}
        assert list(res) == list(cases)
        return res
    return run


def test_on_for_the_benchmarks_handle_and_upload(printer):
    """bench.py: 1024 windows of 11 frames / 5 visual-odometry frames / 300 landmarks on a handle of the same capacity: 1024 > 2 * 256, so
    k_build_solve_st<false, 11> (256 threads); 300 landmarks fit k_lin_gram (fused), lg_lcap = 320 <= 1024 (no k_backsub_split)"""
    got = printer({"bench": tsp.words(11, 5, 300, 1024, B=1024), "bench_hook": tsp.words(11, 5, 300, 1024, B=1024, env=dict(ISV_BSUB_IN_DOGLEG=1)),
                   "bench_generic": tsp.words(11, 5, 300, 1024, B=1024, env=dict(ISV_GENERIC_N=1)), "bench_of_4": tsp.words(11, 5, 300, 1024, B=4)})
    assert got["bench"] == dict(bsub_in_solve=1, solve_st=1, fused=1, threads=256, est_ex=0, bsub_split=0, hook=0, solve=6)       # 6: ST_N11
    assert got["bench_hook"] == dict(got["bench"], bsub_in_solve=0, hook=1)
    assert got["bench_generic"] == dict(got["bench"], solve=7)                     # 7: ST_RT, the run-time-N instantiation
    assert got["bench_of_4"] == got["bench"]                                       # the handle decides, not the uploaded batch size


def test_off_at_each_conditions_boundary(printer):
    """1. the handle's kernel: N = 11 solves with k_build_solve_st from max_batch = 513 (> 2 * 256 CUs), with k_build_solve_sb up to 512;
          ISV_SOLVE_ST = 1 | 0 force either.
       2. the fused path: a window of 8192 factors is the longest k_lin_gram takes (ISV_FUSED_MAX_FACTORS), 8193 goes to k_proj_linearize<0> +
          k_sweep_mfma; ISV_LEGACY_VISUAL does the same for every upload.
       3. the window length: 11 frames run the 256-thread instantiation, 12 the 512-thread one (k_build_solve_st from max_batch = 257 there).
       4. the extrinsic: 10 real frames + the pseudo-frame are 11 device frames, still the 256-thread kernel, but backsub_landmark<true>.
       5. k_backsub_split: a one-window handle splits the elimination from four 64-landmark passes on, and lg_lcap > 1024 moves the
          back-substitution to k_backsub_split: 1024 landmarks -> lg_lcap 1024, no; 1025 -> 1056, yes."""
    st = dict(ISV_SOLVE_ST=1)
    got = printer({
        "mb512": tsp.words(11, 5, 300, 512, B=512), "mb513": tsp.words(11, 5, 300, 513, B=513),
        "st_forced": tsp.words(11, 5, 100, 1, env=st), "st_off": tsp.words(11, 5, 300, 1024, B=1024, env=dict(ISV_SOLVE_ST=0)),
        "f8192": tsp.words(11, 5, 300, 1024, B=2, Fmax=8192), "f8193": tsp.words(11, 5, 300, 1024, B=2, Fmax=8193),
        "legacy": tsp.words(11, 5, 300, 1024, B=1024, env=dict(ISV_LEGACY_VISUAL=1)),
        "n3": tsp.words(3, 2, 25, 1024, B=3), "n6": tsp.words(6, 2, 60, 3, B=3, env=st), "n9": tsp.words(9, 5, 80, 3, B=3, env=st),
        "n12": tsp.words(12, 5, 300, 1024, B=1024), "n18": tsp.words(18, 8, 300, 1024, B=1024),
        "ex_nr10": tsp.words(10, 5, 100, 1024, ex=1, B=1024), "nr10": tsp.words(10, 5, 100, 1024, B=1024),
        "l1024": tsp.words(11, 5, 1024, 1, env=st), "l1025": tsp.words(11, 5, 1025, 1, env=st),
        "l1025_nosplit": tsp.words(11, 5, 1025, 1, env=dict(ISV_SOLVE_ST=1, ISV_NO_SPLIT=1)),
    })
    on = {k: v["bsub_in_solve"] for k, v in got.items()}
    assert on == dict(mb512=0, mb513=1, st_forced=1, st_off=0, f8192=1, f8193=0, legacy=0, n3=1, n6=1, n9=1, n12=0, n18=0, ex_nr10=0, nr10=1,
                      l1024=1, l1025=0, l1025_nosplit=1)
    # ... and each is off for the reason meant
    assert (got["mb512"]["solve_st"], got["mb513"]["solve_st"], got["st_off"]["solve_st"]) == (0, 1, 0)
    assert (got["f8192"]["fused"], got["f8193"]["fused"], got["legacy"]["fused"]) == (1, 0, 0) and got["f8193"]["solve_st"] == got["legacy"]["solve_st"] == 1
    assert [(got[k]["solve_st"], got[k]["threads"]) for k in ("n3", "n6", "n9", "n12", "n18")] == [(1, 256)] * 3 + [(1, 512)] * 2
    assert (got["ex_nr10"]["solve_st"], got["ex_nr10"]["threads"], got["ex_nr10"]["fused"], got["ex_nr10"]["est_ex"]) == (1, 256, 1, 1)
    assert (got["l1024"]["bsub_split"], got["l1025"]["bsub_split"], got["l1025_nosplit"]["bsub_split"]) == (0, 1, 0)
    assert got["l1025"]["solve_st"] == got["l1025"]["fused"] == 1 and got["l1025"]["threads"] == 256
