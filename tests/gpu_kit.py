"""TEST INFRASTRUCTURE: the helpers of the GPU suite.  torch and rustfhe_amd are imported inside the functions that need them, so the
module itself imports without a GPU (tests/test_suite_layout.py checks the guard's numpy half on the CPU).  What both suites share is in
tests/kit.py; the oracles in tests/pbs_oracle.py, tests/leveled_oracle.py and the *_oracle.py beside them; the drivers of the leveled
entry points and of the LUT circuits in tests/leveled_kit.py and tests/lut_circuit_kit.py."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

FILL = 0x5A5A5A5A
CANARY = 64             # words behind a guarded device output that must keep their bytes

# ---- contexts and launch shapes -------------------------------------------------------------------------------------------------------------
CONFIGS_1024 = [None, {"RTFHE_FORCE_WAVES": "1"}, {"RTFHE_FORCE_WAVES": "2"}, {"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_FORCE_WAVES": "8"},
                {"RTFHE_PAIR_RR": "0"}, {"RTFHE_PAIR4": "0"}, {"RTFHE_KS_MM_MIN": "0"}]
CONFIGS_2048 = [None, {"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_N2048_EO4": "0"}]


def env_id(env):
    """the id of a launch shape in a parametrize list"""
    return "default" if not env else ",".join("%s=%s" % kv for kv in env.items())


def engine(R, p, keys_bk, keys_ksk, monkeypatch=None, env=None, **kw):
    """a context on device 0 (or on kw's devices) created under `env`, which is read at creation only, with both keys loaded"""
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    try:
        e = R.Engine(p, 0, **kw) if "devices" not in kw else R.Engine(p, **kw)
    finally:
        if env:
            for k in env:
                monkeypatch.delenv(k)
    e.load_bk_torus(keys_bk)
    e.load_ksk(keys_ksk)
    return e


# ---- host arrays to the device and back -----------------------------------------------------------------------------------------------------
def to_device(a, dtype=np.int32):
    """None gives None; anything else is converted to `dtype` (np.int32 or np.uint32) in a copy of its own -- shared inputs are read-only --
    and arrives on the device as an int32 tensor of the same bytes"""
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype).view(np.int32)).cuda()


def words_of(t):
    """a device tensor's bytes as u32 words on the host"""
    return t.cpu().numpy().view(np.uint32)


# ---- guarded output buffers: the numpy half, then its torch wrapper -------------------------------------------------------------------------
def guarded(words, fill=FILL, canary=CANARY, init=None):
    """the host image u32[words + canary] of an output buffer: `fill` everywhere (or `init` in the payload), `canary` words of `fill` behind"""
    img = np.full(words + canary, fill, np.uint32)
    if init is not None:
        img[:words] = np.asarray(init, np.uint32).reshape(-1)
    return img


def check_guard(host_words, n, fill=FILL):
    """the payload host_words[:n]; every word behind it must still be `fill`"""
    if not (host_words[n:] == fill).all():
        raise AssertionError("words behind d_out were written")
    return host_words[:n]


def guarded_out(words, init=None):
    """guarded() on the device"""
    return to_device(guarded(words, init=init), np.uint32)


def read_guarded(d_out, words):
    """check_guard() of a guarded_out buffer after the stream has been synchronised"""
    return check_guard(words_of(d_out), words)


def acc_rows(kind, count, N):
    """what an accumulating product finds in its output: None (accumulate off), "fill" (the sentinel) or "random" words; u32[count][2][N]"""
    if kind is None:
        return None
    if kind == "fill":
        return np.full((count, 2, N), FILL, np.uint32)
    return np.random.default_rng(count * N).integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)


# ---- worlds: what a module's tests share per ring -------------------------------------------------------------------------------------------
class Worlds:
    """the lazily built worlds of one module-scoped fixture: worlds(*key) builds on first use, close() closes every world at teardown"""

    def __init__(self, build, close=lambda w: w.close()):
        self._build, self._close, self._made = build, close, {}

    def __call__(self, *key):
        if key not in self._made:
            self._made[key] = self._build(*key)
        return self._made[key]

    def close(self):
        for w in self._made.values():
            self._close(w)
        self._made.clear()


def memo(cache, args, compute):
    """compute() once per `cache` (a world's dict) and `args` -- arrays are keyed by shape, type and bytes -- and read-only after"""
    key = tuple((a.shape, a.dtype.str, a.tobytes()) if isinstance(a, np.ndarray) else tuple(a) if isinstance(a, list) else a for a in args)
    if key not in cache:
        got = compute()
        for arr in got if isinstance(got, tuple) else (got,):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        cache[key] = got
    return cache[key]


# ---- batch sizes from the device's CU count, and the oracle on several host threads ---------------------------------------------------------
THREADS = min(16, os.cpu_count() or 1)
_pool = ThreadPoolExecutor(THREADS)
_tls = threading.local()


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def sizes(N, C):
    """batch sizes that reach every launch shape of the default dispatch on a device of C CUs"""
    if N == 1024:
        return [1, C + C // 6, 2 * C + C // 3, 3 * C + C // 2, 4 * C, 4 * C + 1, 5 * C, 6 * C, 9 * C + 44]
    return [1, 37, C + 1, 2 * C + 1, 3 * C + 2, 4 * C, 4 * C + 76]


def forced_sizes(N, C):
    """the subset of sizes() that the forced launch shapes run"""
    return [1, C + C // 6, 2 * C + C // 3, 4 * C, 5 * C] if N == 1024 else [37, 2 * C + 1, 4 * C + 76]


def pmap(fn, items):
    return list(_pool.map(fn, items))


def oracle_plan(orc, N, backend=0):
    """an oracle plan of the calling thread's own (a plan carries transform scratch: one per thread)"""
    plans = _tls.__dict__.setdefault("plans", {})
    if (N, backend) not in plans:
        plans[N, backend] = orc.Plan(N, backend)
    return plans[N, backend]
