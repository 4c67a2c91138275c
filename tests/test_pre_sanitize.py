"""AddressSanitizer + UBSan run of the serial restatement of the IMU pre-integration (tests/native/isv_pre_oracle.c, and with it the
shared text is-vins_amd/csrc/isv_preint.h) on the CPU, through the stand-alone program tests/native/pre_oracle_sanitize.cpp: the
shapes of the case table, the operations that carry state across calls, a buffer filled to max_samples exactly and every refusal,
with exact-size heap blocks throughout.  The sanitizer runtimes are linked statically into the program; nothing is loaded into python,
the environment is passed through apart from ASAN_OPTIONS, and nothing of this touches a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", os.path.join(ROOT, "include")]


def test_restatement_under_asan_ubsan(tmp_path):
    obj, exe = tmp_path / "isv_pre_oracle.o", tmp_path / "pre_oracle_sanitize"
    subprocess.check_call(["gcc", "-std=gnu11", *SAN, "-c", os.path.join(ROOT, "tests", "native", "isv_pre_oracle.c"), "-o", str(obj)])
    subprocess.check_call(["g++", "-std=c++17", *SAN, "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "native", "pre_oracle_sanitize.cpp"),
                           str(obj), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
