"""CPU: the host-only part of rtfhe_pack_batch[_dev] -- every argument check that needs no context (rtfhe_pack_plan in
rustfhe_amd/csrc/rtfhe_extract_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C
host (tests/c/pack_sanitize_main.c).  It runs before any HIP call, so no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_pack_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_extract_plan.cpp"], "pack_sanitize_main.c", "pack sanitizer walk ok")
