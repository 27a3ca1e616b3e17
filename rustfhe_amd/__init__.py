"""rustfhe_amd -- MI355X (gfx950) engine for the HomNAND hot path of hideki1217/rusTfhe.

The product is the C-ABI shared library librtfhe_hip.so (include/rtfhe.h, rustfhe_amd/csrc/); this
package is the thin Python host side above it.  There is no CPU fallback anywhere in the package.
"""
from ._ffi import AND, ANDNY, COPY, NAND, NOT, OR, XOR, Params, load  # noqa: F401
from .client import (RtfheError, decrypt_bits, encrypt_bits, encrypt_lut, encrypt_selectors, encrypt_torus, encrypt_trgsw_polys, keygen, ksk_expand_ref, load_keys,  # noqa: F401
                     load_tlwe, mb_point_exponents, mb_roots, mbk_keygen, mbk_words, packing_keygen, phases, save_keys, save_tlwe, trlwe_phase,
                     encrypt_lut_seeded, encrypt_selectors_seeded, encrypt_trgsw_polys_seeded, mask_expand, packing_keygen_seeded, seeded_expand,
                     encrypt_bits_seeded, encrypt_torus_seeded, keygen_seeded, ksk_keygen_seeded, tlwe_mask_expand, tlwe_seeded_expand,
                     compressed_words, read_compressed, tlwe_compress, tlwe_expand, trlwe_compress, trlwe_expand, write_compressed,
                     trace_exponents, trlwe_automorphism, trlwe_ksk_keygen)
from .engine import Dense, Engine, FftPlan, Lut, MultibitKey, PackingKey, PlainPolys, Selectors, TrlweSwitchKey, demux_level_selector, device_link, pinned_empty, shard_range  # noqa: F401
from .pbs import decode_msgs, encode_msgs, lut_pack_layout, lut_polynomial, many_lut_polynomial  # noqa: F401
from .lut_circuit import LutCircuitRunner, LutNetlist, lut_ripple_adder  # noqa: F401
from .linear import dense_bias, dense_layer_bias, dense_layer_input, dense_layer_polys, dense_layer_trgsw  # noqa: F401
from .cmux_net import CmuxCircuit, CmuxNetlist, bdd_netlist, cmux_tree_netlist, trgsw_rotate_netlist  # noqa: F401

__all__ = ["Engine", "FftPlan", "Params", "RtfheError", "keygen", "ksk_expand_ref", "encrypt_bits", "decrypt_bits", "phases", "save_keys", "load_keys", "save_tlwe", "load_tlwe", "pinned_empty", "shard_range", "device_link",
           "Lut", "Selectors", "encrypt_torus", "encrypt_lut", "encrypt_selectors", "trlwe_phase", "encode_msgs", "decode_msgs", "lut_polynomial", "many_lut_polynomial", "LutNetlist", "LutCircuitRunner", "lut_ripple_adder",
           "CmuxNetlist", "CmuxCircuit", "bdd_netlist", "cmux_tree_netlist", "trgsw_rotate_netlist", "demux_level_selector",
           "PackingKey", "packing_keygen", "lut_pack_layout", "PlainPolys", "Dense", "dense_bias", "dense_layer_polys", "dense_layer_input", "dense_layer_bias", "encrypt_trgsw_polys", "dense_layer_trgsw",
           "mask_expand", "seeded_expand", "encrypt_lut_seeded", "encrypt_selectors_seeded", "encrypt_trgsw_polys_seeded", "packing_keygen_seeded",
           "tlwe_mask_expand", "tlwe_seeded_expand", "encrypt_bits_seeded", "encrypt_torus_seeded", "ksk_keygen_seeded", "keygen_seeded",
           "compressed_words", "tlwe_compress", "tlwe_expand", "trlwe_compress", "trlwe_expand", "write_compressed", "read_compressed",
           "MultibitKey", "mbk_keygen", "mbk_words", "mb_roots", "mb_point_exponents",
           "TrlweSwitchKey", "trlwe_ksk_keygen", "trlwe_automorphism", "trace_exponents",
           "NAND", "AND", "OR", "XOR", "NOT", "COPY", "ANDNY", "load"]
