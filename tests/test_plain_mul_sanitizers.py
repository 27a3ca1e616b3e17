"""CPU: the host-only part of rtfhe_plain_create and rtfhe_trlwe_mul_plain_batch[_dev] -- every argument check that needs no context
(rustfhe_amd/csrc/rtfhe_plain_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C
host (tests/c/plain_sanitize_main.c).  It runs before any HIP call, so no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_plain_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_plain_plan.cpp"], "plain_sanitize_main.c", "plain sanitizer walk ok")
