"""CPU: every deterministic entry point of the host-side encryptors, unseeded and seeded, and the four CPU expansions return the words they
returned before the encryptor core (rustfhe_amd/csrc/rtfhe_encrypt.hpp) was shared between them -- SHA-256 for SHA-256 against
tests/golden/encryptor_words.json, recorded by scripts/record_encryptor_words.py from the tree before that change (tests/encryptor_kit.py holds
the cases).  The digests rest on libm giving the same log / cos / sqrt everywhere, as the oracle's keygen hash in tests/conftest.py does."""
import numpy as np
import pytest

import encryptor_kit as ek


@pytest.fixture(scope="module")
def golden():
    return ek.load_golden()


@pytest.mark.parametrize("name", ["n20_N16", "n37_N64", "n20_N16_ks4x3", "default"])
def test_every_deterministic_word_is_the_recorded_one(golden, name):
    import rustfhe_amd as R
    got = ek.run(R, only=(name,))
    want = {k: v for k, v in golden.items() if k.split("/")[0] == name}
    assert want and sorted(got) == sorted(want), "the table and the recorded file list the same outputs"
    bad = [k for k in sorted(want) if got[k] != want[k]]
    assert not bad, "words differ from the recorded ones: " + ", ".join(bad)


def test_the_recorded_file_covers_every_case_somewhere(golden):
    cases = {k.split("/")[1] for k in golden}
    assert cases == {c for c, _, _ in ek.CASES}
    assert {k.split("/")[0] for k in golden} == {"n20_N16", "n37_N64", "n20_N16_ks4x3", "default"}


def test_packing_key_is_refused_at_other_ks_parameters():
    import rustfhe_amd as R
    p, _ = ek.param_sets(R)["n20_N16_ks4x3"]
    key0, key1, _, _ = R.keygen(p, 7, want_bk=False, want_ksk=False)
    with pytest.raises(R.RtfheError) as e:
        R.packing_keygen(p, key0, key1, seed=3)
    assert e.value.code == R._ffi.ERR_INVALID
    with pytest.raises(R.RtfheError) as e:
        R.packing_keygen_seeded(p, key0, key1, noise_seed=3, seed=ek.MASK_SEED, first_row=0)
    assert e.value.code == R._ffi.ERR_INVALID


@pytest.mark.parametrize("name", ["n20_N16", "n37_N64"])
def test_a_constant_polynomial_equal_to_a_bit_gives_the_bits_form(name):
    """encrypt_trgsw_polys' docstring: a constant polynomial mu = bit gives encrypt_selectors' words under the same seed -- seeded form too"""
    import rustfhe_amd as R
    p, _ = ek.param_sets(R)[name]
    _, key1, _, _ = R.keygen(p, 7, want_bk=False, want_ksk=False)
    bits = np.array([1, 0, 1], np.uint8)
    mu = np.zeros((3, p.N), np.int32)
    mu[:, 0] = bits
    assert np.array_equal(R.encrypt_trgsw_polys(p, key1, mu, seed=9), R.encrypt_selectors(p, key1, bits, seed=9))
    for fr in ek.first_rows(3 * 2 * p.l):
        _, b_polys = R.encrypt_trgsw_polys_seeded(p, key1, mu, noise_seed=9, seed=ek.MASK_SEED, first_row=fr)
        _, b_bits = R.encrypt_selectors_seeded(p, key1, bits, noise_seed=9, seed=ek.MASK_SEED, first_row=fr)
        assert np.array_equal(b_polys, b_bits), fr


def test_striped_generation_gives_the_same_words_twice():
    """one generator per coefficient, striped over the threads: which thread makes which row changes nothing"""
    import rustfhe_amd as R
    p, _ = ek.param_sets(R)["n37_N64"]
    key0, key1, _, _ = R.keygen(p, 7, want_bk=False, want_ksk=False)
    assert np.array_equal(R.packing_keygen(p, key0, key1, seed=3), R.packing_keygen(p, key0, key1, seed=3))
