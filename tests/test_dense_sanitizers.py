"""CPU: the host-only part of rtfhe_dense_create and rtfhe_tlwe_dense_batch[_dev] -- every argument check that needs no context, the
correction words and the launch rule (rustfhe_amd/csrc/rtfhe_dense_plan.cpp) -- compiled by g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and driven from a stand-alone C host (tests/c/dense_sanitize_main.c).  It runs before any HIP call, so no device
is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("gcc") and shutil.which("g++")), reason="gcc/g++ not available")
def test_dense_plan_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "rustfhe_amd", "csrc")
    exe = tmp_path / "dense_sanitize"
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", csrc]
    plan, main = tmp_path / "plan.o", tmp_path / "main.o"
    subprocess.check_call(["g++", "-std=c++17"] + san + inc + ["-c", os.path.join(csrc, "rtfhe_dense_plan.cpp"), "-o", str(plan)])
    subprocess.check_call(["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "tests", "c", "dense_sanitize_main.c"), "-o", str(main)])
    subprocess.check_call(["g++", "-fsanitize=address,undefined", str(main), str(plan), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "dense sanitizer walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
