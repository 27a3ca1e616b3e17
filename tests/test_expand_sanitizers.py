"""CPU: the host-only part of the device-side expansion of compressed rows -- the RTFHE_COMPRESS_EXPAND checks as rtfhe_tlwe_expand_batch_dev /
rtfhe_trlwe_expand_batch_dev call them and the inverse map of the coefficient list, rtfhe_expand_inverse_map
(rustfhe_amd/csrc/rtfhe_compress_plan.cpp, with the coefficient list of rtfhe_extract_plan.cpp) -- compiled by g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and driven from a stand-alone C host (tests/c/expand_sanitize_main.c) with buffers of exact size.  Nothing is loaded
into Python, and no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_expand_plan_and_inverse_map_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_compress_plan.cpp", "rustfhe_amd/csrc/rtfhe_extract_plan.cpp"], "expand_sanitize_main.c", "expand sanitizer walk ok")
