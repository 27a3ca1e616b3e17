"""CPU: the oracle (test infrastructure) built once under AddressSanitizer + UndefinedBehaviorSanitizer and walked end to end
(SURVEY 5).  GPU sanitizers are not available on this pool; the device code shares no source with the oracle."""
import sanitize_kit as K


@K.needs_gcc
def test_oracle_under_asan_and_ubsan(tmp_path):
    K.walk(tmp_path, ["oracle/tfhe_oracle.c"], "oracle_sanitize_main.c", "oracle sanitizer walk ok", flags=["-ffp-contract=off", "-pthread"],
           libs=["-lm", "-lpthread"], timeout=900)


@K.needs_gcc_and_gxx
def test_product_host_sources_under_asan_and_ubsan(tmp_path):
    """The product's host-only sources (key generation / encryption, wire format) compiled by g++ under ASan + UBSan and driven
    from a C host: secure and deterministic keygen, encrypt -> decrypt, file round trips, corrupted and truncated files."""
    K.walk(tmp_path, ["rustfhe_amd/csrc/rtfhe_keygen.cpp", "rustfhe_amd/csrc/rtfhe_wire.cpp"], "host_sanitize_main.c", "host sanitizer walk ok", flags=["-pthread"],
           args=[tmp_path], timeout=600)
