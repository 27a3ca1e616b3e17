#!/usr/bin/env python3
"""Same-process A/B of the multi-bit blind rotation against the single-bit PBS (device buffers, device events): legs alternate round by round --
pbs_batch_dev (the parent path), pbs_batch_dev once more (the spread of the measurement itself), pbs_mb_batch_dev at g = 2 and at g = 3 -- at
count = 1, 64, 256 and 1,024 at N = 1024 and count = 1 and 1,024 at N = 2048, default dispatch (N = 1024: the workgroup shape, N = 2048: the
wave shape) and, at N = 1024, each shape forced.  Beside the times: the phase-error standard deviation of 1,024 outputs
of the constant-1/8 table per decomposition mode for the three paths, and the VGPR / LDS / scratch figures of the built kernels (the compiler's
remarks on rtfhe_pbs_mb.hip).  One JSON line each.  There is no pass mark.
usage: ab_pbs_mb.py [--steps 20] [--warmup 3] [--rounds 5] [--no-resources]"""
import argparse, json, os, re, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R
from rustfhe_amd import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-resources", action="store_true")
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()
COUNTS = {1024: (1, 64, 256, 1024), 2048: (1, 1024)}


def timed(legs):
    for f in legs.values():
        for _ in range(args.warmup): f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, f in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(per_round): f()
            b.record(st)
            b.synchronize()
            times[name].append(a.elapsed_time(b) / per_round)
    return {k: round(float(np.median(v)), 4) for k, v in times.items()}


def resources():
    """the compiler's kernel-resource remarks on the one unit that instantiates the multi-bit kernels"""
    flags = [f for f in B.CFLAGS if f not in ("-fPIC", "-pthread")]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(B.CSRC, "rtfhe_pbs_mb.hip"), "-o", os.path.join(d, "mb.s")],
                           capture_output=True, text=True, check=True)
    out, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: \s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"kernel": subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)}
            out.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


if not args.no_resources:
    for k in resources():
        print(json.dumps(k), flush=True)
    print(json.dumps({"dynamic_lds_bytes_at_n635": {"k_pbs_mb<10>": 2040 * 16 + 4 * (2 * 576 * 8 + 8192 + 640 * 4) + 2048 * 16,
                                                    "k_pbs_mb_wg": 2040 * 16 + 2048 * 16 + 6 * 576 * 8 + 16384 + 8192 + 640 * 4}}),      # twiddles, waves' carves, W
          flush=True)

for N in (1024, 2048):
    P = R.Params(N=N)
    rng = np.random.default_rng(N)
    e = R.Engine(P, 0)
    key0, key1, bk, ksk = R.keygen(P, 20261021)
    e.load_bk_torus(bk); e.load_ksk(ksk)
    mbk = {g: e.multibit_key(R.mbk_keygen(P, key0, key1, g, seed=g), g) for g in (2, 3)}
    print(json.dumps({"N": N, "n": P.n, "cus": torch.cuda.get_device_properties(0).multi_processor_count, "memory_bytes": e.memory_bytes()}), flush=True)
    bits = rng.integers(0, 2, 1024).astype(np.uint8)
    ct = R.encrypt_bits(P, key0, bits, 1)
    d_in = torch.from_numpy(ct.view(np.int32)).cuda()
    d_o = torch.empty_like(d_in)
    lut = e.lut(np.full((1, N), 0x20000000, np.uint32))
    for count in COUNTS[N]:
        legs = {"single": lambda: e.pbs_batch_dev(lut, d_in, d_o, count, None, st.cuda_stream),
                "single_again": lambda: e.pbs_batch_dev(lut, d_in, d_o, count, None, st.cuda_stream),
                "mb_g2": lambda: e.pbs_mb_batch_dev(mbk[2], lut, d_in, d_o, count, None, st.cuda_stream),
                "mb_g3": lambda: e.pbs_mb_batch_dev(mbk[3], lut, d_in, d_o, count, None, st.cuda_stream)}
        for shape in ((None, "wave", "wg") if N == 1024 else (None,)):
            if shape:
                os.environ["RTFHE_MB_SHAPE"] = shape
                run = {k: v for k, v in legs.items() if k.startswith("mb") or k == "single"}
            else:
                os.environ.pop("RTFHE_MB_SHAPE", None)
                run = legs
            ms = timed(run)
            print(json.dumps({"N": N, "count": count, "shape": shape or "default", "ms": ms,
                              "mb_g2_over_single": round(ms["mb_g2"] / ms["single"], 3), "mb_g3_over_single": round(ms["mb_g3"] / ms["single"], 3)}), flush=True)
        os.environ.pop("RTFHE_MB_SHAPE", None)
    if N == 1024:      # noise: 1,024 outputs per mode and path
        want = np.where(bits == 1, 0x20000000, 0xE0000000).astype(np.uint32)
        for mode, name in ((R._ffi.DECOMP_REFERENCE, "reference"), (R._ffi.DECOMP_ROUNDED, "rounded")):
            e.set_decomposition(mode)
            outs = {"single": e.pbs_batch(lut, ct), "mb_g2": e.pbs_mb_batch(mbk[2], lut, ct), "mb_g3": e.pbs_mb_batch(mbk[3], lut, ct)}
            row = {"N": N, "decomposition": name}
            for k, out in outs.items():
                d = (R.phases(P, key0, out) - want).astype(np.uint32).view(np.int32) / 2.0 ** 32
                row[k] = {"phase_error_std": round(float(d.std()), 5), "mean": round(float(d.mean()), 5), "max_abs": round(float(np.abs(d).max()), 5),
                          "wrong": int(np.sum(R.decrypt_bits(P, key0, out) != bits))}
            print(json.dumps(row), flush=True)
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
    lut.close()
    for k in mbk.values():
        k.close()
    e.close()
