"""CPU: the host-only part of the multi-bit blind rotation -- the key's sizes, the roots table, the point map and every argument check that
needs no context (rustfhe_amd/csrc/rtfhe_mb_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a
stand-alone C host (tests/c/mb_sanitize_main.c).  It runs before any HIP call, so no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_mb_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_mb_plan.cpp"], "mb_sanitize_main.c", "mb sanitizer walk ok")
