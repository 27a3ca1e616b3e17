"""The one table of cases behind tests/test_encryptor_words.py and scripts/record_encryptor_words.py: every *_deterministic entry point of the
host-side encryptors (unseeded and seeded) and the four CPU expansions, run through rustfhe_amd at four parameter sets, each output reduced to
the SHA-256 of its little-endian bytes.  tests/golden/encryptor_words.json holds the digests as the code BEFORE the encryptor core
(rustfhe_amd/csrc/rtfhe_encrypt.hpp) gave them: a deterministic entry point returns the same words for ever."""
import ctypes as C
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encryptor_words.json")
M64 = 1 << 64
MASK_SEED = (np.arange(8, dtype=np.uint64) * 0x9E3779B1 + 0x243F6A88).astype(np.uint32)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).hexdigest()


def first_rows(rows):
    """Where a seeded object may start: row 0, across the carry into the nonce's high word, and the last rows there are."""
    return (0, (1 << 32) - 2, M64 - rows)


def param_sets(R):
    """name -> (parameters, what runs there).  "all": everything, both keys and the packing key; "ksk": the key-switch-shaped generators at
    base - 1 = 7 digit rows (the packing key must be refused); "default": the default set without the bootstrapping and packing keys."""
    return {"n20_N16": (R.Params(n=20, N=16, l=2, bgbit=8), "all"),
            "n37_N64": (R.Params(n=37, N=64, l=3, bgbit=6), "all"),        # n = 2 * 16 + 5: the cut last keystream block
            "n20_N16_ks4x3": (R.Params(n=20, N=16, l=2, bgbit=8, ks_t=4, ks_basebit=3), "ksk"),
            "default": (R.Params(), "default")}


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def keygen_with_keys(R, p, key0, key1, seed):
    """rtfhe_keygen_with_keys_deterministic, which the package wraps in no function of its own"""
    bk, ksk = np.empty(p.bk_words, np.uint32), np.empty(p.ksk_words, np.uint32)
    rc = R.load().rtfhe_keygen_with_keys_deterministic(C.byref(p), seed, _ptr(key0), _ptr(key1), _ptr(bk), _ptr(ksk))
    assert rc == 0, rc
    return bk, ksk


def _setup(R, p, scope):
    """What the cases of one parameter set share: its keys (keygen's own words are a case too) and the messages."""
    rng = np.random.default_rng(p.n * 4099 + p.N)
    count = 5
    key0, key1, bk, ksk = R.keygen(p, 7, want_bk=scope != "default", want_ksk=True)
    return SimpleNamespace(p=p, key0=key0, key1=key1, bk=bk, ksk=ksk, count=count,
                           bits=rng.integers(0, 2, count).astype(np.uint8), polys=rng.integers(-8, 9, (count, p.N)).astype(np.int32),
                           tv=rng.integers(0, 1 << 32, (3, p.N), dtype=np.uint64).astype(np.uint32),
                           bits0=rng.integers(0, 2, 33).astype(np.uint8), mu0=rng.integers(0, 1 << 32, 33, dtype=np.uint64).astype(np.uint32),
                           user0=rng.integers(0, 2, p.n).astype(np.int32), user1=rng.integers(0, 2, p.N).astype(np.int32))


def _seeded(fn, rows):
    """One seeded encryptor at every first row: {first_row: b}; the seed must come back as given."""
    out = {}
    for fr in first_rows(rows):
        seed, b = fn(fr)
        assert np.array_equal(seed, MASK_SEED)
        out["row%d" % fr] = b
    return out


# (name, the scopes it runs in, s -> array | {part: array}); R is the package, s what _setup returned
CASES = [
    ("keygen", ("all", "ksk", "default"), lambda R, s: {"key0": s.key0, "key1": s.key1, "ksk": s.ksk, **({} if s.bk is None else {"bk": s.bk})}),
    ("keygen_with_keys", ("all",), lambda R, s: dict(zip(("bk", "ksk"), keygen_with_keys(R, s.p, s.user0, s.user1, 11)))),
    ("packing_keygen", ("all",), lambda R, s: R.packing_keygen(s.p, s.key0, s.key1, seed=3)),
    ("ksk_expand_ref", ("all", "ksk"), lambda R, s: R.ksk_expand_ref(s.p, s.key0, s.key1, s.ksk, seed=5)),
    ("tlwe_bits", ("all", "default"), lambda R, s: R.encrypt_bits(s.p, s.key0, s.bits0, seed=21)),
    ("tlwe_torus", ("all", "default"), lambda R, s: R.encrypt_torus(s.p, s.key0, s.mu0, seed=22)),
    ("trlwe_torus", ("all", "default"), lambda R, s: R.encrypt_lut(s.p, s.key1, s.tv, seed=23)),
    ("trgsw_bits", ("all", "default"), lambda R, s: R.encrypt_selectors(s.p, s.key1, s.bits, seed=24)),
    ("trgsw_polys", ("all", "default"), lambda R, s: R.encrypt_trgsw_polys(s.p, s.key1, s.polys, seed=25)),
    ("trlwe_torus_seeded", ("all", "default"),
     lambda R, s: _seeded(lambda fr: R.encrypt_lut_seeded(s.p, s.key1, s.tv, noise_seed=33, seed=MASK_SEED, first_row=fr), 3)),
    ("trgsw_bits_seeded", ("all", "default"),
     lambda R, s: _seeded(lambda fr: R.encrypt_selectors_seeded(s.p, s.key1, s.bits, noise_seed=34, seed=MASK_SEED, first_row=fr), s.count * 2 * s.p.l)),
    ("trgsw_polys_seeded", ("all", "default"),
     lambda R, s: _seeded(lambda fr: R.encrypt_trgsw_polys_seeded(s.p, s.key1, s.polys, noise_seed=35, seed=MASK_SEED, first_row=fr), s.count * 2 * s.p.l)),
    ("packing_keygen_seeded", ("all",),
     lambda R, s: _seeded(lambda fr: R.packing_keygen_seeded(s.p, s.key0, s.key1, noise_seed=3, seed=MASK_SEED, first_row=fr), s.p.n * 24)),
    ("tlwe_bits_seeded", ("all", "default"),
     lambda R, s: _seeded(lambda fr: R.encrypt_bits_seeded(s.p, s.key0, s.bits0, noise_seed=31, seed=MASK_SEED, first_row=fr), 33)),
    ("tlwe_torus_seeded", ("all", "default"),
     lambda R, s: _seeded(lambda fr: R.encrypt_torus_seeded(s.p, s.key0, s.mu0, noise_seed=32, seed=MASK_SEED, first_row=fr), 33)),
    ("ksk_keygen_seeded", ("all", "ksk", "default"),
     lambda R, s: _seeded(lambda fr: R.ksk_keygen_seeded(s.p, s.key0, s.key1, noise_seed=36, seed=MASK_SEED, first_row=fr), _ksk_rows(s.p))),
    ("mask_expand", ("all", "default"), lambda R, s: {"row%d" % fr: R.mask_expand(s.p.N, MASK_SEED, 7, first_row=fr) for fr in first_rows(7)}),
    ("seeded_expand", ("all", "default"),
     lambda R, s: {"row%d" % fr: R.seeded_expand(s.p, MASK_SEED, _b_rows(s), group=2 * s.p.l, first_row=fr) for fr in first_rows(2 * s.p.l)}),
    ("tlwe_mask_expand", ("all", "default"), lambda R, s: {"row%d" % fr: R.tlwe_mask_expand(s.p.n, MASK_SEED, 33, first_row=fr) for fr in first_rows(33)}),
    ("tlwe_seeded_expand", ("all", "default"), lambda R, s: {"row%d" % fr: R.tlwe_seeded_expand(s.p, MASK_SEED, s.mu0, first_row=fr) for fr in first_rows(33)}),
]


def _ksk_rows(p):
    return p.N * p.ks_t * ((1 << p.ks_basebit) - 1)


def _b_rows(s):
    """2l rows of N words to expand as one TRGSW group"""
    return np.random.default_rng(s.p.N).integers(0, 1 << 32, (2 * s.p.l, s.p.N), dtype=np.uint64).astype(np.uint32)


def run(R, only=None):
    """{"<parameter set>/<case>[/<part>]": digest} of every case (only: of the parameter sets named)."""
    out = {}
    for name, (p, scope) in param_sets(R).items():
        if only is not None and name not in only:
            continue
        s = _setup(R, p, scope)
        for case, scopes, fn in CASES:
            if scope not in scopes:
                continue
            res = fn(R, s)
            for part, a in (res.items() if isinstance(res, dict) else [("", res)]):
                out["/".join(x for x in (name, case, part) if x)] = digest(a)
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
