"""CPU: the host-only unit of the seeded lvl0 ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule for rows of length n, the
seeded lvl0 encryptors, the seeded key-switching key, every argument check of the seeded lvl0 calls) compiled by g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and driven from a stand-alone C host (tests/c/tlwe_seeded_sanitize_main.c), together with rtfhe_seeded.cpp, whose
rtfhe_mask_expand the walk ties the new rule to.  Nothing in them makes a HIP call, so no device is needed, and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not (shutil.which("gcc") and shutil.which("g++")), reason="gcc/g++ not available")
def test_tlwe_seeded_unit_under_asan_and_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "rustfhe_amd", "csrc")
    exe = tmp_path / "tlwe_seeded_sanitize"
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-pthread"]
    inc = ["-I", os.path.join(ROOT, "include"), "-I", csrc]
    units = []
    for name in ("rtfhe_seeded",):
        units.append(str(tmp_path / (name + ".o")))
        subprocess.check_call(["g++", "-std=c++17"] + san + inc + ["-c", os.path.join(csrc, name + ".cpp"), "-o", units[-1]])
    main = tmp_path / "main.o"
    subprocess.check_call(["gcc", "-std=gnu11"] + san + inc + ["-c", os.path.join(ROOT, "tests", "c", "tlwe_seeded_sanitize_main.c"), "-o", str(main)])
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-pthread", str(main)] + units + ["-lm", "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "tlwe seeded sanitizer walk ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
