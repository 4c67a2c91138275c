"""AddressSanitizer + UBSan run of the host half of the pose-graph call (is-vins_amd/csrc/isv_pgo_host.h: structure analysis, the
slot-resident structure and its key, the number fill, the layout, the assembly, the chunk pipeline's hand-over on a team of
threads, the write-back) on the CPU, through the stand-alone program tests/native/pgo_host_sanitize.cpp with a stand-in device.
The sanitizer runtimes are linked statically, so the child's environment is the parent's apart from the two settings below."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_graph_host_path_under_asan_ubsan(tmp_path):
    exe = tmp_path / "pgo_host_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                           "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "native", "pgo_host_sanitize.cpp"), "-o", str(exe)])
    for threads in ("1", "4"):
        env = dict(os.environ, ISV_HOST_THREADS=threads, ASAN_OPTIONS="detect_leaks=1")
        out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("ok:") and f"on {threads} host thread(s)" in out.stdout
