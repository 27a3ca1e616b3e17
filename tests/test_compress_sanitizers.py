"""CPU: the host-only part of compressed results -- every argument check of rtfhe_tlwe_compress_batch_dev / rtfhe_trlwe_compress_batch_dev and
the CPU twins rtfhe_tlwe_compress / _expand and rtfhe_trlwe_compress / _expand (rustfhe_amd/csrc/rtfhe_compress_plan.cpp, with the coefficient
list of rtfhe_extract_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C host
(tests/c/compress_sanitize_main.c) at ragged shapes with buffers of exact size.  Nothing is loaded into Python, and no device is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("gcc") and shutil.which("g++")), reason="gcc/g++ not available")
def test_compress_plan_and_twins_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "rustfhe_amd", "csrc")
    exe = tmp_path / "compress_sanitize"
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", csrc]
    objs = []
    for unit in ("rtfhe_compress_plan.cpp", "rtfhe_extract_plan.cpp"):
        objs.append(str(tmp_path / (unit + ".o")))
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + ["-c", os.path.join(csrc, unit), "-o", objs[-1]])
    main = tmp_path / "main.o"
    subprocess.check_call(["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "tests", "c", "compress_sanitize_main.c"), "-o", str(main)])
    subprocess.check_call(["g++", "-fsanitize=address,undefined", str(main)] + objs + ["-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "compress sanitizer walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
