"""TEST INFRASTRUCTURE: the helpers both suites share.  CPU only: numpy, and what the callers pass in (the `orc` module, rustfhe_amd as R).
The GPU suite's own helpers are in tests/gpu_kit.py; the oracles in tests/pbs_oracle.py, tests/leveled_oracle.py and the *_oracle.py beside
them.  No test module is imported by another (tests/test_suite_layout.py): what two of them need lives here."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_N = {1024: 40, 2048: 24}      # the TLWE dimensions of the stage tests


def random_words(rng, shape):
    """uniform u32 words"""
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def i32(a):
    return np.array(a, np.int32)


def torus_err(a, b):
    """signed torus distance a - b of u32 words, a fraction in [-1/2, 1/2)"""
    d = (np.asarray(a, np.uint32) - np.asarray(b, np.uint32)).astype(np.uint32).view(np.int32).astype(np.float64)
    return d / 2.0 ** 32


def torus_dist(a, b):
    """|torus_err|, a fraction in [0, 1/2]"""
    return np.abs(torus_err(a, b))


def torus_dist_lsb(a, b):
    """|torus_err| in units of 2^-32, int64 (exact: the fraction is an int32 over 2^32)"""
    return (torus_dist(a, b) * 2.0 ** 32).astype(np.int64)


def phase_err(R, p, key0, cts, want, bits):
    """signed distance (torus fraction) of each phase from the encoding of `want`"""
    return torus_err(R.phases(p, key0, cts), R.encode_msgs(want, bits))


def load_example(name):
    """examples/<name>.py as a module of its own (the examples are scripts, not a package)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


_KEYS_2048 = []


def keys_2048(orc):
    """(parameters, key set) at N = 2048 with the default parameters from seed 2048, generated once per session"""
    if not _KEYS_2048:
        P = orc.Params(N=2048)
        _KEYS_2048.append((P, orc.Keys(P, 2048)))
    return _KEYS_2048[0]
