"""CPU: pins the oracle's FP64 transform (i) against the committed golden vectors that were produced by the
reference's own compiled spqlios and (ii) against that library's outputs on a longer seeded sequence: live, where
oracle/_ref has been built, and always against a recording of them (tests/golden/spqlios_live_N<N>.npz), bit for bit."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden


@pytest.mark.parametrize("N", [16, 1024, 2048])
def test_mirror_matches_golden_reference_vectors(orc, N):
    g = golden("fft_N%d.npz" % N)
    pl = orc.Plan(N)
    a, b = pl.tables()
    assert a.tobytes() == g["ifft_table"].tobytes(), "forward twiddle table differs from the reference build's"
    assert b.tobytes() == g["fft_table"].tobytes(), "inverse twiddle table differs from the reference build's"
    for src, exp in zip(g["fft_src"], g["fft_fwd"]):
        assert pl.ifft_i32(src).tobytes() == exp.tobytes()
    for src, exp in zip(g["inv_src"], g["inv_out"]):
        assert np.array_equal(pl.fft_u32(src), exp)


def test_whole_gate_golden(orc, params, keys, gold_gate):
    pl = orc.Plan(params.N)
    for g in range(len(gold_gate["ops"])):
        out = orc.gate(params, pl, int(gold_gate["ops"][g]), keys.bk_f, None, keys.ksk, gold_gate["in0"][g], gold_gate["in1"][g])
        assert np.array_equal(out, gold_gate["out"][g])
    assert orc.fnv64(keys.bk_f) == int(gold_gate["bk_f_fnv"])
    t0 = orc.gate_linear(params, orc.NAND, gold_gate["in0"][0], gold_gate["in1"][0])
    assert np.array_equal(orc.blind_rotate(params, pl, keys.bk_f, None, t0, 3), gold_gate["acc_steps3"])
    mux = orc.mux(params, pl, keys.bk_f, None, keys.ksk, gold_gate["in0"][2], gold_gate["in0"][0], gold_gate["in1"][1])
    assert np.array_equal(mux, gold_gate["mux_out"])


# argv: N, tests dir, mode, recording.  live: against oracle/_ref; record: the same, and the library's outputs saved to the recording
# (FNV-1a 64 digests of the exact outputs, Spqlios_poly_mul's words whole); replay: against the recording
_LIVE = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[2])
import orc
N, mode, path = int(sys.argv[1]), sys.argv[3], sys.argv[4]
pl = orc.Plan(N)
if mode == "replay":
    rec = np.load(path)
else:
    R = orc.ref_lib(); h = R.Spqlios_new(N)
    rec = {"fwd": np.zeros(60, np.uint64), "inv": np.zeros(60, np.uint64), "poly_mul": np.empty(N, np.uint32)}
rng = np.random.default_rng(N)
for t in range(60):
    src = [rng.integers(-32, 32, N), rng.integers(-2**31, 2**31, N), rng.integers(0, 2, N)][t % 3].astype(np.int32)
    mine = pl.ifft_i32(src)
    if mode != "replay":
        ref = np.empty(N); R.Spqlios_ifft_i32(h, ref.ctypes.data, src.ctypes.data)
        assert mine.tobytes() == ref.tobytes(), ("forward", t)
        rec["fwd"][t] = orc.fnv64(ref)
    assert orc.fnv64(mine) == int(rec["fwd"][t]), ("forward", t)
    spec = np.ascontiguousarray(mine * float(rng.integers(1, 2**20)))
    if mode != "replay":
        r2 = np.empty(N, np.uint32); R.Spqlios_fft_u32(h, r2.ctypes.data, spec.ctypes.data)
        assert np.array_equal(pl.fft_u32(spec), r2), ("inverse", t)
        rec["inv"][t] = orc.fnv64(r2)
    assert orc.fnv64(pl.fft_u32(spec)) == int(rec["inv"][t]), ("inverse", t)
a = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32); b = rng.integers(0, 64, N).astype(np.uint32)
if mode != "replay":
    R.Spqlios_poly_mul(h, rec["poly_mul"].ctypes.data, a.ctypes.data, b.ctypes.data)
r3 = rec["poly_mul"]
# Spqlios_poly_mul (off the hot path; only the reference's N=16 unit test calls it) is C++ built with the reference's
# -Ofast -march=native, where g++ contracts a*b-c to FMA: machine-dependent bits, so +-1 LSB is all that can be pinned.
d = (pl.poly_mul(a, b).astype(np.int64) - r3.astype(np.int64) + 2**31) % 2**32 - 2**31
assert np.abs(d).max() <= 1, d
if mode == "record":
    np.savez_compressed(path, **rec)
print("ok")
"""


@pytest.mark.parametrize("N", [16, 1024, 2048])
def test_mirror_matches_live_reference_library(orc, N):
    import os
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    recording = os.path.join(tests_dir, "golden", "spqlios_live_N%d.npz" % N)
    for mode in (["live"] if orc.have_ref() else []) + ["replay"]:
        # one N per process: the reference caches 2/N in a function-local static
        out = subprocess.run([sys.executable, "-c", _LIVE, str(N), tests_dir, mode, recording], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ok" in out.stdout, (mode, out.stderr[-2000:])


def test_whole_gate_with_live_reference_fft(orc, params, keys, gold_gate):
    if not orc.have_ref():
        pytest.skip("oracle/_ref not built")
    plr = orc.Plan(params.N).use_reference_fft()
    out = orc.gate(params, plr, orc.NAND, keys.bk_f, None, keys.ksk, gold_gate["in0"][1], gold_gate["in1"][1])
    assert np.array_equal(out, gold_gate["out"][1])
