"""CPU: the host-only unit of the seeded ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule, the seeded encryptors, every argument
check of the seeded calls) compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C host
(tests/c/seeded_sanitize_main.c).  Nothing in it makes a HIP call, so no device is needed, and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("gcc") and shutil.which("g++")), reason="gcc/g++ not available")
def test_seeded_unit_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "rustfhe_amd", "csrc")
    exe = tmp_path / "seeded_sanitize"
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread"]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", csrc]
    unit, main = tmp_path / "seeded.o", tmp_path / "main.o"
    subprocess.check_call(["g++", "-std=c++17"] + san + inc + ["-c", os.path.join(csrc, "rtfhe_seeded.cpp"), "-o", str(unit)])
    subprocess.check_call(["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "tests", "c", "seeded_sanitize_main.c"), "-o", str(main)])
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-pthread", str(main), str(unit), "-lm", "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "seeded sanitizer walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
