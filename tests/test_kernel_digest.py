"""tools/kernel_digest.py: the mnemonic multiset it compares for kernels that are not byte-identical (no GPU)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_digest  # noqa: E402


def test_mnemonic_multiset_ignores_encoding_suffix_nops_and_padding():
    a = ["\tv_cndmask_b32_e32 v0, v1, v2, vcc", "\ts_nop 0", "\tv_fma_f32 v3, v4, v5, v6", "\ts_endpgm"]
    b = ["\tv_fma_f32 v9, v4, v5, v6", "\tv_cndmask_b32_e64 v0, v1, v2, s[0:1]", "\ts_endpgm",
         "\tv_cndmask_b32_e32 v0, s0, v0, vcc"]  # rescheduled, other encoding, no s_nop, padding past the end
    assert kernel_digest.mnemonics(a) == kernel_digest.mnemonics(b) == {"v_cndmask_b32": 1, "v_fma_f32": 1,
                                                                        "s_endpgm": 1}
    assert kernel_digest.mnemonics(a + ["\ts_waitcnt vmcnt(0)", "\ts_endpgm"]) != kernel_digest.mnemonics(a)
