"""The one build-and-walk recipe of the tests/test_*_sanitizers.py modules: host-only units of the product (or the oracle) and a stand-alone C
main from tests/c/ compiled under AddressSanitizer + UndefinedBehaviorSanitizer, linked into one program and run as a process of its own.
Nothing is loaded into Python and nothing is preloaded; no device is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra"]

needs_gcc = pytest.mark.skipif(not shutil.which("gcc"), reason="gcc not available")
needs_gcc_and_gxx = pytest.mark.skipif(not (shutil.which("gcc") and shutil.which("g++")), reason="gcc/g++ not available")


def walk(tmp_path, units, main, ok, flags=(), libs=(), args=(), timeout=300):
    """Compiles `units` (paths from the repository root: .cpp by g++, .c by gcc) and tests/c/`main` with SAN + flags, links them (+ libs), runs
    the program with `args` and asserts that it printed the line `ok`, returned 0 and that neither sanitizer spoke."""
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "rustfhe_amd", "csrc"), "-I", os.path.join(ROOT, "oracle")]
    objs = []
    for k, src in enumerate(list(units) + [os.path.join("tests", "c", main)]):
        objs.append(str(tmp_path / ("%d_%s.o" % (k, os.path.basename(src)))))
        cc = ["g++", "-std=c++17"] if src.endswith(".cpp") else ["gcc", "-std=gnu11"]
        subprocess.check_call(cc + SAN + list(flags) + inc + ["-c", os.path.join(ROOT, src), "-o", objs[-1]])
    exe = str(tmp_path / os.path.splitext(main)[0])
    subprocess.check_call(["g++", "-fsanitize=address,undefined"] + [f for f in flags if f == "-pthread"] + objs + list(libs) + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0 and ok in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
