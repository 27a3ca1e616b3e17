#!/usr/bin/env python3
"""Same-process A/B of the many-LUT PBS from an encrypted table against the same PBS from the plain table (device buffers, one engine per N):
legs alternate round by round -- the plain table at n_out = 1 twice (against itself: the noise floor), then plain and encrypted at n_out = 1, 2
and 4, all on four random tables (the encrypted one: their TRLWE encryptions under key1) picked by random indices.  Device events around each
leg.  Once per shape, a trivially encrypted table's words are compared with the plain table's.
usage: ab_pbs_enc.py [--steps 20] [--warmup 3]     (shapes: 1,024 / 8,192 gates at N = 1024, 1,024 at N = 2048)"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import rustfhe_amd as R

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
per_round = max(1, args.steps // args.rounds)
st = torch.cuda.current_stream()

for N, counts in ((1024, (1024, 8192)), (2048, (1024,))):
    P = R.Params(N=N)
    key0, key1, bk, ksk = R.keygen(P, 20261016)
    e = R.Engine(P, 0)
    e.load_bk_torus(bk); e.load_ksk(ksk)
    rng = np.random.default_rng(N)
    G = max(counts)
    d_in = torch.from_numpy(R.encrypt_bits(P, key0, rng.integers(0, 2, G).astype(np.uint8), 1).view(np.int32)).cuda()
    d_idx = torch.from_numpy(rng.integers(0, 4, G).astype(np.int32)).cuda()
    tv = rng.integers(0, 1 << 32, (4, N), dtype=np.uint64).astype(np.uint32)
    plain = e.lut(tv)
    enc = e.lut_encrypted(R.encrypt_lut(P, key1, tv, seed=N))
    triv = e.lut_encrypted(np.stack([tv, np.zeros_like(tv)], axis=1))
    for c in counts:
        outs = {"plain1": None, "plain1_again": None, "enc1": None, "plain2": None, "enc2": None, "plain4": None, "enc4": None, "triv1": None}
        for k in outs:
            outs[k] = torch.empty((G, int(k.replace("_again", "")[-1]), P.n + 1), dtype=torch.int32, device="cuda")
        run = lambda lut, k: (lambda o: e.pbs_many_batch_dev(lut, d_in, o, c, k, d_idx, st.cuda_stream))  # noqa: E731
        legs = {"plain1": run(plain, 1), "plain1_again": run(plain, 1), "enc1": run(enc, 1), "plain2": run(plain, 2), "enc2": run(enc, 2),
                "plain4": run(plain, 4), "enc4": run(enc, 4)}
        for name, f in legs.items():
            for _ in range(args.warmup): f(outs[name])
        run(triv, 1)(outs["triv1"])
        e.sync(st.cuda_stream)
        times = {k: [] for k in legs}
        for r in range(args.rounds):
            for name, f in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                for _ in range(per_round): f(outs[name])
                b.record(st)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / per_round)
        e.sync(st.cuda_stream)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"N": N, "gates": c, "steps_per_leg": per_round * args.rounds, **{k + "_ms": round(v, 4) for k, v in med.items()},
                          "plain_vs_itself_pct": round((med["plain1_again"] / med["plain1"] - 1) * 100, 2),
                          **{"enc%d_vs_plain%d_pct" % (k, k): round((med["enc%d" % k] / med["plain%d" % k] - 1) * 100, 2) for k in (1, 2, 4)},
                          "trivial_words_equal_plain": bool(torch.equal(outs["triv1"][:c], outs["plain1"][:c]))}), flush=True)
    plain.close(); enc.close(); triv.close(); e.close()
