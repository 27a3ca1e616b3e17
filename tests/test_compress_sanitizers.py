"""CPU: the host-only part of compressed results -- every argument check of rtfhe_tlwe_compress_batch_dev / rtfhe_trlwe_compress_batch_dev and
the CPU twins rtfhe_tlwe_compress / _expand and rtfhe_trlwe_compress / _expand (rustfhe_amd/csrc/rtfhe_compress_plan.cpp, with the coefficient
list of rtfhe_extract_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a stand-alone C host
(tests/c/compress_sanitize_main.c) at ragged shapes with buffers of exact size.  Nothing is loaded into Python, and no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_compress_plan_and_twins_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_compress_plan.cpp", "rustfhe_amd/csrc/rtfhe_extract_plan.cpp"], "compress_sanitize_main.c", "compress sanitizer walk ok")
