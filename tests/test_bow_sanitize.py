"""AddressSanitizer + UBSan run of the host-only vocabulary parser (is-vins_amd/csrc/isv_bow_vocab.h) on the CPU, through the
stand-alone program tests/native/bow_vocab_sanitize.cpp: the valid file, every truncation length, over-long files, every
malformed case and byte corruptions, each handed over as an exact-size heap block so that one byte read too many is seen."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vocabulary_parser_under_asan_ubsan(tmp_path):
    exe = tmp_path / "bow_vocab_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "native", "bow_vocab_sanitize.cpp"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok:")
