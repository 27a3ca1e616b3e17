"""The key holder's side: key generation, encryption, decryption, phases, the CPU expansions of seeded objects and of compressed results, and the
file formats, through the host-only part of the C ABI (rtfhe_keygen.cpp, rtfhe_seeded.cpp, rtfhe_compress_plan.cpp, rtfhe_wire.cpp).  Nothing
here touches an Engine or needs a GPU.
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import ERR_INVALID, Params


class RtfheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rtfhe error %d: %s" % (code, msg))
        self.code = code


def _np(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _seed(seed):
    """A mask seed (include/rtfhe.h, "seeded ciphertexts"): u32[8], a ChaCha20 key -- public."""
    seed = _np(seed, np.uint32).reshape(-1)
    assert seed.size == 8, "a mask seed is u32[8]"
    return seed


# ---- host-side key generation / encryption (C ABI, no GPU needed) --------------------------------

def _unseeded_rc(name, params, seed, seed_at, args):
    """One unseeded call: the production form (seed None: everything from the OS CSPRNG) or its TEST-ONLY deterministic twin, which takes the
    integer seed before argument seed_at (0: ahead of the keys, in the key generators; 1: behind the key, in the encryptors).  Returns rc."""
    L = _ffi.load()
    if seed is None:
        return getattr(L, name)(C.byref(params), *args)
    return getattr(L, name + "_deterministic")(C.byref(params), *args[:seed_at], seed, *args[seed_at:])


def _unseeded(name, params, seed, seed_at, args, detail=""):
    rc = _unseeded_rc(name, params, seed, seed_at, args)
    if rc != 0:
        raise RtfheError(rc, name + " failed" + detail)


def keygen(params, seed=None, want_bk=True, want_ksk=True):
    """seed None (production): every key bit, mask and noise sample comes from the OS CSPRNG.  An integer seed selects the
    TEST-ONLY deterministic generator (rtfhe_keygen_deterministic: reproducible, NOT secure)."""
    key0 = np.empty(params.n, np.int32)
    key1 = np.empty(params.N, np.int32)
    bk = np.empty(params.bk_words, np.uint32) if want_bk else None
    ksk = np.empty(params.ksk_words, np.uint32) if want_ksk else None
    _unseeded("rtfhe_keygen", params, seed, 0, (_ptr(key0), _ptr(key1), _ptr(bk), _ptr(ksk)))
    return key0, key1, bk, ksk


def packing_keygen(params, key0, key1, seed=None):
    """The packing key of the lvl0 key key0 under the lvl1 key key1 (include/rtfhe.h: rtfhe_packing_keygen): u32[n][t][base-1][2][N], row
    (i, j, d) a TRLWE of the constant (d+1) key0[i] / 2^(basebit (j+1)) with alpha = 2^-25 (125 MB at the default parameters).  seed None
    (production): OS CSPRNG; an integer seed = TEST-ONLY deterministic generation.  Non-binary keys and ks parameters other than (8, 2) are
    refused."""
    key0, key1 = _np(key0, np.int32).reshape(-1), _np(key1, np.int32).reshape(-1)
    assert key0.size == params.n and key1.size == params.N
    pk = np.empty((params.n, params.ks_t, (1 << params.ks_basebit) - 1, 2, params.N), np.uint32)
    _unseeded("rtfhe_packing_keygen", params, seed, 0, (_ptr(key0), _ptr(key1), _ptr(pk)),
              " (non-binary key, or ks parameters other than t = 8, basebit = 2)")
    return pk


def mbk_words(params, g):
    """Words of a multi-bit bootstrapping key at g key bits per step (include/rtfhe.h: rtfhe_mbk_words); RtfheError for g outside {2, 3}."""
    w = _ffi.load().rtfhe_mbk_words(C.byref(params), int(g))
    if not w:
        raise RtfheError(ERR_INVALID, "rtfhe_mbk_words: g = %d is outside {2, 3} (or bad parameters)" % int(g))
    return w


def mbk_keygen(params, key0, key1, g, seed=None):
    """The multi-bit bootstrapping key of the lvl0 key key0 under the lvl1 key key1 (include/rtfhe.h: rtfhe_mbk_keygen): u32[n_trgsw][2][2l][N],
    for every group of g key bits a TRGSW sample per non-empty subset j of its bits, encrypting 1 exactly when the group's set bits are those
    of j; each sample in the layout of one bootstrapping-key entry, with its noise (1.5 x the bootstrapping key's size at g = 2, 2.33 x at
    g = 3).  Engine.multibit_key uploads it.  seed None (production): OS CSPRNG; an integer seed = TEST-ONLY deterministic generation.
    g outside {2, 3} and non-binary keys are refused."""
    key0, key1 = _np(key0, np.int32).reshape(-1), _np(key1, np.int32).reshape(-1)
    assert key0.size == params.n and key1.size == params.N
    words = mbk_words(params, g)
    out = np.empty((words // (4 * params.l * params.N), 2, 2 * params.l, params.N), np.uint32)
    _unseeded("rtfhe_mbk_keygen", params, seed, 0, (int(g), _ptr(key0), _ptr(key1), _ptr(out)), " (non-binary key)")
    return out


def trlwe_ksk_keygen(params, key_from, key_to, t, seed=None):
    """The TRLWE switching key from the lvl1 key key_from to the lvl1 key key_to for the exponents t (include/rtfhe.h:
    rtfhe_trlwe_ksk_keygen): u32[n_t][l][2][N], row (e, j) a TRLWE under key_to of -sigma_{t[e]}(key_from) * 2^(32 - (j+1) bgbit) with
    alpha = 2^-25.  key_from is key_to: automorphism keys; t = [1] with two keys: a re-keying key.  Engine.trlwe_switch_key uploads it.
    seed None (production): OS CSPRNG; an integer seed = TEST-ONLY deterministic generation.  Refused: non-binary keys, more than 64 or no
    exponents, an even t or one outside [1, 2N), an exponent given twice."""
    key_from, key_to = _np(key_from, np.int32).reshape(-1), _np(key_to, np.int32).reshape(-1)
    assert key_from.size == params.N and key_to.size == params.N
    t = _np(t, np.int32).reshape(-1)
    out = np.empty((t.size, params.l, 2, params.N), np.uint32)
    _unseeded("rtfhe_trlwe_ksk_keygen", params, seed, 2, (_ptr(key_from), _ptr(key_to), _ptr(t), t.size, _ptr(out)),
              " (non-binary key, or exponents that are not 1 .. 64 distinct odd numbers in [1, 2N))")
    return out


def trlwe_automorphism(x, t):
    """sigma_t : X -> X^t on polynomials of u32 coefficients, on the CPU (rtfhe_trlwe_automorphism): x u32[..][N] -> the same shape, x[j] at
    j t mod 2N mod N, negated when j t mod 2N >= N.  A TRLWE row u32[2][N] maps polynomial by polynomial; sigma_t of a plaintext is what a
    replace step of Engine.trlwe_auto_batch makes of the row's message."""
    x = _np(x, np.uint32)
    N = x.shape[-1] if x.ndim else 0
    out = np.empty_like(x)
    rc = _ffi.load().rtfhe_trlwe_automorphism(int(N), int(t), _ptr(x), _ptr(out), x.size // N if N else 0)
    if rc != 0:
        raise RtfheError(rc, "rtfhe_trlwe_automorphism failed (N = %d not a power of two, or t = %d even or outside [1, 2N))" % (N, int(t)))
    return out


def trace_exponents(N, steps):
    """The exponents of a partial trace of `steps` add steps: [N + 1, N/2 + 1, ...], step i being sigma_{N / 2^i + 1}.  After them exactly the
    coefficients that are multiples of 2^steps survive, multiplied by 2^steps (Engine.trlwe_auto_batch with add = all ones)."""
    N, steps = int(N), int(steps)
    if not (N >= 2 and N & (N - 1) == 0 and 0 <= steps and (N >> steps) >= 1):
        raise RtfheError(ERR_INVALID, "trace_exponents: N = %d must be a power of two and steps = %d within 0 .. log2 N" % (N, steps))
    return [(N >> i) + 1 for i in range(steps)]


def mb_roots(N):
    """The roots table of the multi-bit key combination (rtfhe_mb_roots): float64[2N][2], row t = (cos, sin) of pi t / N."""
    out = np.empty((2 * int(N) if 2 <= int(N) <= 1 << 20 else 1, 2), np.float64)      # (a refused N writes nothing)
    rc = _ffi.load().rtfhe_mb_roots(int(N), _ptr(out))
    if rc != 0:
        raise RtfheError(rc, "rtfhe_mb_roots: N = %d" % int(N))
    return out


def mb_point_exponents(N):
    """The point map of the multi-bit key combination (rtfhe_mb_point_exponents): int32[N/2], the odd exponent q_p of spectrum point
    p = m * 64 + lane of the device layout."""
    out = np.empty(int(N) // 2 if 128 <= int(N) <= 1 << 20 else 1, np.int32)      # (a refused N writes nothing)
    rc = _ffi.load().rtfhe_mb_point_exponents(int(N), _ptr(out))
    if rc != 0:
        raise RtfheError(rc, "rtfhe_mb_point_exponents: N = %d" % int(N))
    return out


def encrypt_bits(params, key0, bits, seed=None):
    """seed None (production): mask and noise from the OS CSPRNG; an integer seed = TEST-ONLY deterministic encryption."""
    bits = _np(bits, np.uint8).reshape(-1)
    key0 = _np(key0, np.int32)
    out = np.empty((bits.size, params.n + 1), np.uint32)
    _unseeded("rtfhe_tlwe_encrypt_bits", params, seed, 1, (_ptr(key0), _ptr(bits), _ptr(out), bits.size))
    return out


def encrypt_torus(params, key0, mu, seed=None):
    """encrypt_bits with the plaintext torus words mu (u32) given directly, e.g. encode_msgs(m, p) for programmable bootstrapping.
    seed None (production): OS CSPRNG; an integer seed = TEST-ONLY deterministic encryption."""
    mu = _np(mu, np.uint32).reshape(-1)
    key0 = _np(key0, np.int32)
    out = np.empty((mu.size, params.n + 1), np.uint32)
    _unseeded("rtfhe_tlwe_encrypt_torus", params, seed, 1, (_ptr(key0), _ptr(mu), _ptr(out), mu.size))
    return out


def encrypt_lut(params, key1, tv, seed=None):
    """TRLWE encryptions under the lvl1 key key1 of test polynomials tv (u32[n_lut][N] or one u32[N]): u32[n_lut][2][N] (b then a), the rows of
    an encrypted table (Engine.lut_encrypted).  Noise alpha = 2^-25 as the bootstrapping key's rows.  seed None (production): OS CSPRNG; an
    integer seed = TEST-ONLY deterministic encryption."""
    tv = _np(tv, np.uint32).reshape(-1, params.N)
    key1 = _np(key1, np.int32)
    out = np.empty((tv.shape[0], 2, params.N), np.uint32)
    _unseeded("rtfhe_trlwe_encrypt_torus", params, seed, 1, (_ptr(key1), _ptr(tv), _ptr(out), tv.shape[0]))
    return out


def encrypt_selectors(params, key1, bits, seed=None):
    """TRGSW encryptions under the lvl1 key key1 of the bits (u8[count]): u32[count][2][2l][N], each in the layout of one bootstrapping-key
    entry -- the encrypted address bits of a CMUX tree (Engine.selectors).  Noise alpha = 2^-25 as the bootstrapping key's.  seed None
    (production): OS CSPRNG; an integer seed = TEST-ONLY deterministic encryption."""
    bits = _np(bits, np.uint8).reshape(-1)
    key1 = _np(key1, np.int32)
    out = np.empty((bits.size, 2, 2 * params.l, params.N), np.uint32)
    _unseeded("rtfhe_trgsw_encrypt_bits", params, seed, 1, (_ptr(key1), _ptr(bits), _ptr(out), bits.size))
    return out


def encrypt_trgsw_polys(params, key1, mu, seed=None):
    """TRGSW encryptions under the lvl1 key key1 of the small-integer polynomials mu (int32[count][N] or one int32[N]): u32[count][2][2l][N],
    encrypt_selectors with mu(X) in the bit's place -- the encrypted weights of Engine.trlwe_mul_trgsw_batch (Engine.selectors uploads them).
    A constant polynomial mu = bit gives encrypt_selectors' words under the same seed.  seed None (production): OS CSPRNG; an integer seed =
    TEST-ONLY deterministic encryption."""
    mu = _np(mu, np.int32).reshape(-1, params.N)
    key1 = _np(key1, np.int32)
    out = np.empty((mu.shape[0], 2, 2 * params.l, params.N), np.uint32)
    _unseeded("rtfhe_trgsw_encrypt_polys", params, seed, 1, (_ptr(key1), _ptr(mu), _ptr(out), mu.shape[0]))
    return out


# ---- seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts"): a public seed and the b halves stand for the full rows -------------------

def mask_expand(N, seed, rows, first_row=0):
    """The masks of rows first_row .. first_row + rows - 1 of a seed at ring degree N (rtfhe_mask_expand): u32[rows][N], the ChaCha20 keystream
    of the seed with the row number in the nonce."""
    L = _ffi.load()
    a = np.empty((int(rows), int(N)), np.uint32)
    rc = L.rtfhe_mask_expand(int(N), _ptr(_seed(seed)), int(first_row), _ptr(a), int(rows))
    if rc != 0:
        raise RtfheError(rc, "rtfhe_mask_expand failed (N not a power of two in 16 .. 2048, or first_row + rows beyond 2^64)")
    return a


def seeded_expand(params, seed, b, group=1, first_row=0):
    """The full layout of a seeded object on the CPU (rtfhe_seeded_expand): b u32[rows][N] -> u32[rows / group][2][group][N], the b polynomials
    of each group, then their masks.  group: 1 for TRLWE rows, tables and the packing key, 2l for TRGSW sets and the bootstrapping key."""
    L = _ffi.load()
    b = _np(b, np.uint32).reshape(-1, params.N)
    rows, group = b.shape[0], int(group)
    out = np.empty(2 * b.size, np.uint32)
    rc = L.rtfhe_seeded_expand(C.byref(params), _ptr(_seed(seed)), int(first_row), _ptr(b), group, _ptr(out), rows)
    if rc != 0:
        raise RtfheError(rc, "rtfhe_seeded_expand failed (group < 1, rows not a multiple of group, or first_row + rows beyond 2^64)")
    return out.reshape(rows // group, 2, group, params.N)


def _seeded_encrypt(name, params, keys, msg, b, noise_seed, seed, first_row, count=()):
    """One seeded encryptor: the production form (noise_seed None: fresh seed from the OS, rows from 0) or its TEST-ONLY deterministic form
    (noise_seed, seed and first_row given).  keys / msg: the pointers of the key(s) and of the messages; count: the trailing count argument as a
    tuple, empty for the packing key."""
    L = _ffi.load()
    if noise_seed is None:
        assert seed is None and first_row == 0, "the production form draws its own seed and numbers rows from 0"
        seed = np.zeros(8, np.uint32)
        rc = getattr(L, name)(C.byref(params), *keys, *msg, _ptr(seed), _ptr(b), *count)
    else:
        seed = _seed(seed)
        if name in ("rtfhe_packing_keygen_seeded", "rtfhe_ksk_keygen_seeded"):
            rc = getattr(L, name + "_deterministic")(C.byref(params), int(noise_seed), *keys, _ptr(seed), int(first_row), _ptr(b))
        else:
            rc = getattr(L, name + "_deterministic")(C.byref(params), *keys, int(noise_seed), _ptr(seed), int(first_row), *msg, _ptr(b), *count)
    if rc != 0:
        raise RtfheError(rc, name + " failed (non-binary key, bad parameters, or rows beyond 2^64)")
    return seed, b


def encrypt_lut_seeded(params, key1, tv, noise_seed=None, seed=None, first_row=0):
    """encrypt_lut in seeded form: (seed, b) with b u32[n_lut][N] -- half of encrypt_lut's words; Engine.lut_encrypted_seeded uploads it and
    seeded_expand gives the full rows.  noise_seed None (production): a fresh public seed from the OS, the noise from a separate OS-seeded
    generator.  An integer noise_seed = TEST-ONLY deterministic noise, with the mask seed (u32[8]) and first_row given by the caller."""
    tv = _np(tv, np.uint32).reshape(-1, params.N)
    key1 = _np(key1, np.int32)
    b = np.empty((tv.shape[0], params.N), np.uint32)
    return _seeded_encrypt("rtfhe_trlwe_encrypt_torus_seeded", params, (_ptr(key1),), (_ptr(tv),), b, noise_seed, seed, first_row, (tv.shape[0],))


def encrypt_selectors_seeded(params, key1, bits, noise_seed=None, seed=None, first_row=0):
    """encrypt_selectors in seeded form: (seed, b) with b u32[count][2l][N]; Engine.selectors_seeded uploads it.  With bits = key0 this is the
    seeded bootstrapping key (Engine.load_bk_seeded).  noise_seed / seed / first_row as in encrypt_lut_seeded."""
    bits = _np(bits, np.uint8).reshape(-1)
    key1 = _np(key1, np.int32)
    b = np.empty((bits.size, 2 * params.l, params.N), np.uint32)
    return _seeded_encrypt("rtfhe_trgsw_encrypt_bits_seeded", params, (_ptr(key1),), (_ptr(bits),), b, noise_seed, seed, first_row, (bits.size,))


def encrypt_trgsw_polys_seeded(params, key1, mu, noise_seed=None, seed=None, first_row=0):
    """encrypt_trgsw_polys in seeded form: (seed, b) with b u32[count][2l][N].  noise_seed / seed / first_row as in encrypt_lut_seeded."""
    mu = _np(mu, np.int32).reshape(-1, params.N)
    key1 = _np(key1, np.int32)
    b = np.empty((mu.shape[0], 2 * params.l, params.N), np.uint32)
    return _seeded_encrypt("rtfhe_trgsw_encrypt_polys_seeded", params, (_ptr(key1),), (_ptr(mu),), b, noise_seed, seed, first_row, (mu.shape[0],))


def packing_keygen_seeded(params, key0, key1, noise_seed=None, seed=None, first_row=0):
    """packing_keygen in seeded form: (seed, b) with b u32[n][t][base-1][N]; Engine.packing_key_seeded uploads it.  noise_seed / seed /
    first_row as in encrypt_lut_seeded."""
    key0, key1 = _np(key0, np.int32).reshape(-1), _np(key1, np.int32).reshape(-1)
    assert key0.size == params.n and key1.size == params.N
    b = np.empty((params.n, params.ks_t, (1 << params.ks_basebit) - 1, params.N), np.uint32)
    return _seeded_encrypt("rtfhe_packing_keygen_seeded", params, (_ptr(key0), _ptr(key1)), (), b, noise_seed, seed, first_row)


# ---- seeded lvl0 ciphertexts (include/rtfhe.h, "seeded lvl0 ciphertexts"): a public seed and one b word per row stand for u32[rows][n+1] -------

def tlwe_mask_expand(n, seed, rows, first_row=0):
    """The masks of rows first_row .. first_row + rows - 1 of a seed at TLWE dimension n (rtfhe_tlwe_mask_expand): u32[rows][n], the keystream of
    mask_expand cut at n words."""
    L = _ffi.load()
    a = np.empty((int(rows), max(int(n), 0)), np.uint32)
    rc = L.rtfhe_tlwe_mask_expand(int(n), _ptr(_seed(seed)), int(first_row), _ptr(a), int(rows))
    if rc != 0:
        raise RtfheError(rc, "rtfhe_tlwe_mask_expand failed (n < 1, rows = 0, or first_row + rows beyond 2^64)")
    return a


def tlwe_seeded_expand(params, seed, b, first_row=0):
    """The full rows of a seeded lvl0 object on the CPU (rtfhe_tlwe_seeded_expand): b u32[rows] -> u32[rows][n+1], a[0 .. n) then b."""
    L = _ffi.load()
    b = _np(b, np.uint32).reshape(-1)
    out = np.empty((b.size, params.n + 1), np.uint32)
    rc = L.rtfhe_tlwe_seeded_expand(C.byref(params), _ptr(_seed(seed)), int(first_row), _ptr(b), _ptr(out), b.size)
    if rc != 0:
        raise RtfheError(rc, "rtfhe_tlwe_seeded_expand failed (n < 1, rows = 0, or first_row + rows beyond 2^64)")
    return out


def encrypt_bits_seeded(params, key0, bits, noise_seed=None, seed=None, first_row=0):
    """encrypt_bits in seeded form: (seed, b) with b u32[count], one word per bit; tlwe_seeded_expand gives encrypt_bits' rows and
    Engine.upload_tlwe_seeded makes them on the device.  noise_seed / seed / first_row as in encrypt_lut_seeded."""
    bits = _np(bits, np.uint8).reshape(-1)
    key0 = _np(key0, np.int32)
    b = np.empty(bits.size, np.uint32)
    return _seeded_encrypt("rtfhe_tlwe_encrypt_bits_seeded", params, (_ptr(key0),), (_ptr(bits),), b, noise_seed, seed, first_row, (bits.size,))


def encrypt_torus_seeded(params, key0, mu, noise_seed=None, seed=None, first_row=0):
    """encrypt_torus in seeded form: (seed, b) with b u32[count].  noise_seed / seed / first_row as in encrypt_lut_seeded."""
    mu = _np(mu, np.uint32).reshape(-1)
    key0 = _np(key0, np.int32)
    b = np.empty(mu.size, np.uint32)
    return _seeded_encrypt("rtfhe_tlwe_encrypt_torus_seeded", params, (_ptr(key0),), (_ptr(mu),), b, noise_seed, seed, first_row, (mu.size,))


def ksk_keygen_seeded(params, key0, key1, noise_seed=None, seed=None, first_row=0):
    """The key-switching key of keygen in seeded form: (seed, b) with b u32[N][t][base-1], one word per row (98 KB at the default parameters
    where the key is 62.5 MB); Engine.load_ksk_seeded uploads it.  noise_seed / seed / first_row as in encrypt_lut_seeded."""
    key0, key1 = _np(key0, np.int32).reshape(-1), _np(key1, np.int32).reshape(-1)
    assert key0.size == params.n and key1.size == params.N
    b = np.empty((params.N, params.ks_t, (1 << params.ks_basebit) - 1), np.uint32)
    return _seeded_encrypt("rtfhe_ksk_keygen_seeded", params, (_ptr(key0), _ptr(key1)), (), b, noise_seed, seed, first_row)


def keygen_seeded(params, seed=None):
    """The secret keys and both halves of the evaluation key in seeded form: (key0, key1, (bk_seed, bk_b), (ksk_seed, ksk_b)) for
    Engine.load_bk_seeded and Engine.load_ksk_seeded -- 15.7 MB at the default parameters where keygen's keys are 93.7 MB.  The bootstrapping key
    is encrypt_selectors_seeded with bits = key0; the two mask seeds are independent.  seed None (production): everything from the OS CSPRNG; an
    integer seed = TEST-ONLY deterministic generation (mask seeds and noise derived from it)."""
    key0, key1, _, _ = keygen(params, seed, want_bk=False, want_ksk=False)
    if seed is None:
        return key0, key1, encrypt_selectors_seeded(params, key1, key0), ksk_keygen_seeded(params, key0, key1)
    rng = np.random.default_rng(int(seed))
    masks = rng.integers(0, 1 << 32, (2, 8), dtype=np.uint64).astype(np.uint32)
    noise = [int(v) for v in rng.integers(0, 1 << 63, 2)]
    return (key0, key1, encrypt_selectors_seeded(params, key1, key0, noise_seed=noise[0], seed=masks[0]),
            ksk_keygen_seeded(params, key0, key1, noise_seed=noise[1], seed=masks[1]))


# ---- compressed results (include/rtfhe.h, "compressed results"): k-bit, bit-packed rows; the key holder expands them here ----------------------

def compressed_words(L, k):
    """W(L, k) = ceil(L k / 32): the u32 words of one compressed row of L values at k bits (rtfhe_compressed_words); 0 for k outside 2 .. 32."""
    return int(_ffi.load().rtfhe_compressed_words(int(L), int(k)))


def _compress_ck(rc, name):
    if rc != 0:
        raise RtfheError(rc, name + " failed (k outside 2 .. 32, a bad coefficient list, count * L not below 2^31, or overlapping buffers)")


def _row_words(L, k):
    """compressed_words for a call that goes on to use it: k outside 2 .. 32 is refused here"""
    W = compressed_words(L, k)
    if W == 0:
        raise RtfheError(ERR_INVALID, "k = %d is outside 2 .. 32 (or the row is empty)" % int(k))
    return W


def _coef(coef, P):
    if coef is None:
        return None
    coef = _np(coef, np.int32).reshape(-1)
    assert coef.size == int(P), "one coefficient per kept value"
    return coef


def tlwe_compress(n, k, tlwe):
    """lvl0 rows u32[count][n+1] -> u32[count][W(n+1, k)]: every word rounded to its top k bits (to nearest, ties up, wrapping) and the values
    packed into a little-endian bit stream (rtfhe_tlwe_compress) -- word for word what Engine.tlwe_compress_dev writes on the GPU."""
    n, k = int(n), int(k)
    tlwe = _np(tlwe, np.uint32).reshape(-1, n + 1)
    out = np.empty((tlwe.shape[0], _row_words(n + 1, k)), np.uint32)
    _compress_ck(_ffi.load().rtfhe_tlwe_compress(n, k, _ptr(tlwe), _ptr(out), tlwe.shape[0]), "rtfhe_tlwe_compress")
    return out


def tlwe_expand(n, k, words):
    """The inverse on the key holder's side (rtfhe_tlwe_expand): u32[count][W(n+1, k)] -> u32[count][n+1], each value back at the top of its
    word, within 2^(31-k) of the original; phases / decrypt_bits read the rows as they are."""
    n, k = int(n), int(k)
    words = _np(words, np.uint32).reshape(-1, _row_words(n + 1, k))
    out = np.empty((words.shape[0], n + 1), np.uint32)
    _compress_ck(_ffi.load().rtfhe_tlwe_expand(n, k, _ptr(words), _ptr(out), words.shape[0]), "rtfhe_tlwe_expand")
    return out


def trlwe_compress(N, k, trlwe, P, coef=None, stride=1):
    """TRLWE rows u32[count][2][N] (b then a) -> u32[count][W(N+P, k)]: the a polynomial, then b at the P kept coefficients coef (None:
    p * stride), rounded and packed as in tlwe_compress (rtfhe_trlwe_compress); what Engine.trlwe_compress_dev writes on the GPU."""
    N, k, P = int(N), int(k), int(P)
    trlwe = _np(trlwe, np.uint32).reshape(-1, 2, N)
    out = np.empty((trlwe.shape[0], _row_words(N + max(P, 0), k)), np.uint32)
    coef = _coef(coef, P)      # (kept in a name: _ptr holds an address, not the array)
    _compress_ck(_ffi.load().rtfhe_trlwe_compress(N, k, P, _ptr(coef), int(stride), _ptr(trlwe), _ptr(out), trlwe.shape[0]), "rtfhe_trlwe_compress")
    return out


def trlwe_expand(N, k, words, P, coef=None, stride=1):
    """The inverse (rtfhe_trlwe_expand): u32[count][W(N+P, k)] -> full rows u32[count][2][N] whose b is zero at the coefficients that were not
    kept (duplicates: the later entry wins); trlwe_phase and the extract calls read them as they are."""
    N, k, P = int(N), int(k), int(P)
    words = _np(words, np.uint32).reshape(-1, _row_words(N + max(P, 0), k))
    out = np.empty((words.shape[0], 2, N), np.uint32)
    coef = _coef(coef, P)      # (kept in a name: _ptr holds an address, not the array)
    _compress_ck(_ffi.load().rtfhe_trlwe_expand(N, k, P, _ptr(coef), int(stride), _ptr(words), _ptr(out), words.shape[0]), "rtfhe_trlwe_expand")
    return out


def trlwe_phase(params, key1, ct):
    """b - a * s of TRLWE ciphertexts u32[count][2][N] under key1: u32[count][N] (the plaintext plus the noise)."""
    L = _ffi.load()
    ct = _np(ct, np.uint32).reshape(-1, 2, params.N)
    key1 = _np(key1, np.int32)
    ph = np.empty((ct.shape[0], params.N), np.uint32)
    rc = L.rtfhe_trlwe_phase(C.byref(params), _ptr(key1), _ptr(ct), _ptr(ph), ct.shape[0])
    if rc != 0:
        raise RtfheError(rc, "rtfhe_trlwe_phase failed")
    return ph


def decrypt_bits(params, key0, cts):
    L = _ffi.load()
    cts = _np(cts, np.uint32).reshape(-1, params.n + 1)
    key0 = _np(key0, np.int32)
    bits = np.empty(cts.shape[0], np.uint8)
    rc = L.rtfhe_tlwe_decrypt_bits(C.byref(params), _ptr(key0), _ptr(cts), _ptr(bits), cts.shape[0])
    if rc != 0:
        raise RtfheError(rc, "rtfhe_tlwe_decrypt_bits failed")
    return bits


def phases(params, key0, cts):
    L = _ffi.load()
    cts = _np(cts, np.uint32).reshape(-1, params.n + 1)
    key0 = _np(key0, np.int32)
    ph = np.empty(cts.shape[0], np.uint32)
    rc = L.rtfhe_tlwe_phase(C.byref(params), _ptr(key0), _ptr(cts), _ptr(ph), cts.shape[0])
    if rc != 0:
        raise RtfheError(rc, "rtfhe_tlwe_phase failed")
    return ph


def ksk_expand_ref(params, key0, key1, ksk, seed=None):
    """The reference's KeySwitchingKey shape u32[N][t][base][n+1] (hom_nand/src/tlwe.rs:243-245) from the compact key:
    entries t = 1 .. base-1 copied, entry t = base encrypted afresh (seed: TEST ONLY, deterministic)."""
    key0, key1, ksk = _np(key0, np.int32), _np(key1, np.int32), _np(ksk, np.uint32).reshape(-1)
    base = 1 << params.ks_basebit
    out = np.empty(params.ksk_words // (base - 1) * base, np.uint32)
    rc = _unseeded_rc("rtfhe_ksk_expand_ref", params, seed, 0, (_ptr(key0), _ptr(key1), _ptr(ksk), _ptr(out)))
    if rc != 0:
        raise RuntimeError("rtfhe_ksk_expand_ref failed (%d)" % rc)
    return out.reshape(params.N, params.ks_t, base, params.n + 1)


# ---- wire format (flat files; include/rtfhe.h) ----------------------------------------------------

def save_keys(path, params, key0=None, key1=None, bk=None, ksk=None):
    L = _ffi.load()
    arrs = [None if a is None else _np(a, dt) for a, dt in ((key0, np.int32), (key1, np.int32), (bk, np.uint32), (ksk, np.uint32))]
    rc = L.rtfhe_keys_write(path.encode(), C.byref(params), *[_ptr(a) for a in arrs])
    if rc != 0:
        raise RtfheError(rc, "rtfhe_keys_write failed")


def load_keys(path, want_bk=True, want_ksk=True):
    """Returns (params, key0, key1, bk, ksk); sections absent from the file (or not wanted) come back as None."""
    L = _ffi.load()
    p, flags = Params(), C.c_uint32()
    if L.rtfhe_keys_read_header(path.encode(), C.byref(p), C.byref(flags)) != 0:
        raise RtfheError(ERR_INVALID, "not an rtfhe key file: " + path)
    f = flags.value
    key0 = np.empty(p.n, np.int32) if f & 4 else None
    key1 = np.empty(p.N, np.int32) if f & 4 else None
    bk = np.empty(p.bk_words, np.uint32) if (f & 1 and want_bk) else None
    ksk = np.empty(p.ksk_words, np.uint32) if (f & 2 and want_ksk) else None
    if L.rtfhe_keys_read(path.encode(), _ptr(key0), _ptr(key1), _ptr(bk), _ptr(ksk)) != 0:
        raise RtfheError(ERR_INVALID, "corrupt rtfhe key file (checksum or length): " + path)
    return p, key0, key1, bk, ksk


def save_tlwe(path, params, cts):
    L = _ffi.load()
    cts = _np(cts, np.uint32).reshape(-1, params.n + 1)
    if L.rtfhe_tlwe_write(path.encode(), params.n, _ptr(cts), cts.shape[0]) != 0:
        raise RtfheError(ERR_INVALID, "rtfhe_tlwe_write failed")


def load_tlwe(path):
    L = _ffi.load()
    n, count = C.c_int32(), C.c_uint64()
    if L.rtfhe_tlwe_read(path.encode(), C.byref(n), C.byref(count), None, 0) != 0:
        raise RtfheError(ERR_INVALID, "not an rtfhe ciphertext file: " + path)
    out = np.empty((count.value, n.value + 1), np.uint32)
    if L.rtfhe_tlwe_read(path.encode(), C.byref(n), C.byref(count), _ptr(out), count.value) != 0:
        raise RtfheError(ERR_INVALID, "corrupt rtfhe ciphertext file: " + path)
    return out


def write_compressed(path, words, k, n=None, N=None, coef=None):
    """Compressed rows with what it takes to expand them (rtfhe_compressed_write): n for lvl0 rows (tlwe_compress / Engine.tlwe_compress_dev), or
    N and the resolved list of kept coefficients for TRLWE rows -- rows compressed with coef None pass np.arange(P) * stride."""
    assert (n is None) != (N is None) and (N is None) == (coef is None), "either n (lvl0 rows) or N and coef (TRLWE rows)"
    kind, dim = (0, int(n)) if N is None else (1, int(N))
    coef = None if N is None else _np(coef, np.int32).reshape(-1)
    P = 0 if coef is None else coef.size
    words = _np(words, np.uint32).reshape(-1, _row_words(dim + (1 if N is None else P), k))
    if _ffi.load().rtfhe_compressed_write(path.encode(), kind, dim, int(k), P, _ptr(coef), _ptr(words), words.shape[0]) != 0:
        raise RtfheError(ERR_INVALID, "rtfhe_compressed_write failed")


def read_compressed(path):
    """Returns (words u32[count][W], k, n, N, coef): n set and N, coef None for lvl0 rows; N and coef set and n None for TRLWE rows -- the
    arguments of tlwe_expand(n, k, words) or trlwe_expand(N, k, words, len(coef), coef)."""
    L = _ffi.load()
    kind, dim, k, P, count = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    if L.rtfhe_compressed_read_header(path.encode(), C.byref(kind), C.byref(dim), C.byref(k), C.byref(P), C.byref(count)) != 0:
        raise RtfheError(ERR_INVALID, "not an rtfhe compressed file: " + path)
    coef = np.empty(P.value, np.int32) if kind.value == 1 else None
    words = np.empty((count.value, compressed_words(dim.value + (P.value if kind.value == 1 else 1), k.value)), np.uint32)
    if L.rtfhe_compressed_read(path.encode(), _ptr(coef), _ptr(words), count.value) != 0:
        raise RtfheError(ERR_INVALID, "corrupt rtfhe compressed file: " + path)
    return (words, k.value, None, dim.value, coef) if kind.value == 1 else (words, k.value, dim.value, None, None)
