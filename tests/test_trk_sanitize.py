"""AddressSanitizer + UBSan run of the serial restatement of the feature tracking (tests/native/isv_trk_oracle.c) on the CPU,
through the stand-alone program tests/native/trk_oracle_sanitize.cpp: images from 1 x 1 up to 200 x 120, strides, points on, at and
beyond every edge and beyond the range of int, every quirk hook, every capacity and every malformed item, with exact-size heap
blocks throughout.  Nothing is loaded into python, and nothing of this touches a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include")]


def test_restatement_border_scenarios_under_asan_ubsan(tmp_path):
    obj, exe = tmp_path / "isv_trk_oracle.o", tmp_path / "trk_oracle_sanitize"
    subprocess.check_call(["gcc", "-std=gnu11", *SAN, "-c", os.path.join(ROOT, "tests", "native", "isv_trk_oracle.c"), "-o", str(obj)])
    subprocess.check_call(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "trk_oracle_sanitize.cpp"), str(obj), "-o", str(exe), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
