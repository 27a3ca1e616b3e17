"""CPU: the host-only part of rtfhe_dense_create and rtfhe_tlwe_dense_batch[_dev] -- every argument check that needs no context, the
correction words and the launch rule (rustfhe_amd/csrc/rtfhe_dense_plan.cpp) -- compiled by g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and driven from a stand-alone C host (tests/c/dense_sanitize_main.c).  It runs before any HIP call, so no device
is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_dense_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_dense_plan.cpp"], "dense_sanitize_main.c", "dense sanitizer walk ok")
