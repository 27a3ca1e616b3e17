"""CPU: the host-only unit of the seeded ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule, the seeded encryptors, every argument
check of the seeded calls) compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C host
(tests/c/seeded_sanitize_main.c).  Nothing in it makes a HIP call, so no device is needed, and nothing is loaded into Python."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_seeded_unit_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_seeded.cpp"], "seeded_sanitize_main.c", "seeded sanitizer walk ok", flags=["-pthread"], libs=["-lm"])
