"""Shared by tests/test_pack_host.py and tests/test_gpu_pack.py: torus distances, the noise bound of DESIGN.md 5.11 and the measurement of a
packed row's noise against its inputs' phases."""
import numpy as np

import pack_oracle as O
from kit import torus_dist_lsb

ALPHA = 2.0 ** -25


def sdist(a, b):
    """distance on the torus of u32 words, in LSB"""
    return torus_dist_lsb(a, b)


def noise_bound(params, key0, P, rep):
    """8 sqrt(sigma_r^2 + sigma_k^2) as a fraction of the torus: rounding of h = |key0| coefficients to 16 bits, and n t P rep key rows of
    alpha = 2^-25 in the worst case"""
    h = int(np.asarray(key0).sum())
    s_r = 2.0 ** -16 * np.sqrt(h / 12.0)
    s_k = ALPHA * np.sqrt(params.n * params.ks_t * P * rep)
    return 8.0 * np.sqrt(s_r * s_r + s_k * s_k)


def pack_noise(R, params, key0, key1, tlwe, out, P, pos, rep):
    """(largest distance of phase(out)[pos[p] + k] from phase(c[g][p]) over all run coefficients, largest distance from 0 outside every run),
    as fractions of the torus.  Runs must not overlap."""
    N = params.N
    ph_in = R.phases(params, key0, tlwe).astype(np.int64).reshape(-1, P)
    ph = R.trlwe_phase(params, key1, out).astype(np.int64)
    pos = O.default_pos(P, rep) if pos is None else np.asarray(pos, np.int64)
    want = np.zeros((ph.shape[0], N), np.int64)
    covered = np.zeros(N, bool)
    for p in range(P):
        for k in range(rep):
            u = (int(pos[p]) + k) % (2 * N)
            assert not covered[u % N], "overlapping runs"
            covered[u % N] = True
            want[:, u % N] = ph_in[:, p] if u < N else -ph_in[:, p]
    d = sdist(ph, want)
    inside = d[:, covered].max() / 2.0 ** 32
    outside = d[:, ~covered].max() / 2.0 ** 32 if (~covered).any() else 0.0
    return inside, outside
