"""CPU: the host-only part of the TRLWE key switch -- the exponent rules of a switching key, the inverse exponents and every argument check of
rtfhe_trlwe_auto_batch[_dev] that needs no context (rustfhe_amd/csrc/rtfhe_trlwe_auto_plan.cpp), and the automorphism on the CPU
(rtfhe_trlwe_automorphism, rustfhe_amd/csrc/rtfhe_keygen.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven
from a stand-alone C host (tests/c/trlwe_auto_sanitize_main.c).  It runs before any HIP call, so no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_trlwe_auto_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_trlwe_auto_plan.cpp", "rustfhe_amd/csrc/rtfhe_keygen.cpp"], "trlwe_auto_sanitize_main.c",
           "trlwe auto sanitizer walk ok", flags=["-pthread"])
