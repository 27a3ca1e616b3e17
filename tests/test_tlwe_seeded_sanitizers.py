"""CPU: the host-only unit of the seeded lvl0 ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule for rows of length n, the
seeded lvl0 encryptors, the seeded key-switching key, every argument check of the seeded lvl0 calls) compiled by g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and driven from a stand-alone C host (tests/c/tlwe_seeded_sanitize_main.c), together with rtfhe_seeded.cpp, whose
rtfhe_mask_expand the walk ties the new rule to.  Nothing in them makes a HIP call, so no device is needed, and nothing is loaded into Python."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_tlwe_seeded_unit_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_seeded.cpp"], "tlwe_seeded_sanitize_main.c", "tlwe seeded sanitizer walk ok", flags=["-pthread"], libs=["-lm"])
