"""AddressSanitizer + UBSan run of the host half of the whole-frame feature tracker (is-vins_amd/csrc/isv_fe_host.h: the item checks,
the refusal of slots named twice, the validation of a planted state, PubImageData's gate) on the CPU, through the stand-alone program
tests/native/fe_host_sanitize.cpp.  The sanitizer runtimes are linked statically; nothing is loaded into Python and nothing runs on
a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_front_end_host_half_under_asan_ubsan(tmp_path):
    exe = tmp_path / "fe_host_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "native", "fe_host_sanitize.cpp"), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:") and "FAILED" not in out.stdout
