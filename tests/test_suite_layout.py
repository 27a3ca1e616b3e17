"""CPU: how the suite itself is laid out.  No module under tests/ or scripts/ imports from a test module -- what two test modules share lives
in tests/kit.py, tests/gpu_kit.py, a *_kit.py or an *_oracle.py ("How the test suite is laid out") -- and the guard behind the
GPU suite's output buffers reports what it should, checked here on numpy arrays."""
import ast
import glob
import os

import numpy as np
import pytest

import gpu_kit as gk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_module_imports_from_a_test_module():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py")))
    assert len(paths) > 80, "the globs found the suite"
    bad = []
    for path in paths:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += ["%s:%d imports %s" % (os.path.relpath(path, ROOT), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, "\n".join(bad)


def test_check_guard_reports_a_changed_canary_word_and_nothing_else():
    n = 100
    img = gk.guarded(n)
    assert img.shape == (n + gk.CANARY,) and img.dtype == np.uint32 and (img == gk.FILL).all()
    assert np.array_equal(gk.check_guard(img, n), np.full(n, gk.FILL, np.uint32)), "an untouched image passes"
    init = np.arange(n, dtype=np.uint32)
    assert np.array_equal(gk.check_guard(gk.guarded(n, init=init), n), init), "the payload starts as init"
    for at in (n, n + gk.CANARY - 1):                # the first and the last canary word
        hit = gk.guarded(n)
        hit[at] ^= 1
        with pytest.raises(AssertionError, match="words behind d_out were written"):
            gk.check_guard(hit, n)
    payload = gk.guarded(n)
    payload[:n] = np.arange(n, dtype=np.uint32) * 7
    assert np.array_equal(gk.check_guard(payload, n), np.arange(n, dtype=np.uint32) * 7), "payload words may change"
    other = gk.guarded(n, fill=0x12345678, canary=3)
    assert other.shape == (n + 3,) and np.array_equal(gk.check_guard(other, n, 0x12345678), other[:n])
    with pytest.raises(AssertionError):
        gk.check_guard(other, n)                     # the wrong fill is a changed canary
