"""CPU: the host-only part of rtfhe_cmux_circuit_create -- every check of a CMUX netlist's description and its levelisation
(rustfhe_amd/csrc/rtfhe_cmux_net_plan.cpp) -- compiled by g++ under AddressSanitizer + UndefinedBehaviorSanitizer and driven from a
stand-alone C host (tests/c/cmux_net_sanitize_main.c).  It runs before any HIP call, so no device is needed."""
import sanitize_kit as K


@K.needs_gcc_and_gxx
def test_cmux_net_plan_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_cmux_net_plan.cpp"], "cmux_net_sanitize_main.c", "cmux net sanitizer walk ok")
