"""CPU tests (no GPU) of the long time attention's plumbing: which entry points the network plans at which sequence length, and how the binding
table names them.  tests/test_abi_host.py holds the header, the prototypes, the macro and the exports of the built library to that table."""
import pytest


def test_attention_entries_by_sequence_length():
    from audio_inpainting_diffusion_amd.network import attention_entries
    old, long = ("aid_time_attention", "aid_time_attention_bwd"), ("aid_time_attention_long", "aid_time_attention_long_bwd")
    assert attention_entries(1) == old
    assert attention_entries(128) == old
    assert attention_entries(129) == long
    assert attention_entries(1024) == long
    with pytest.raises(NotImplementedError, match="1024"):
        attention_entries(1025)


def test_binding_table_names_the_long_entries_on_the_existing_structs():
    from audio_inpainting_diffusion_amd import _lib
    abi = _lib.ABIS[0]
    assert abi.header == "aid_kernels.h"
    assert abi.launches["aid_time_attention_long"] is _lib.AttentionParams is abi.launches["aid_time_attention"]
    assert abi.launches["aid_time_attention_long_bwd"] is _lib.AttentionBwdParams is abi.launches["aid_time_attention_bwd"]
    assert "AID_ATTN_LONG_MAX_T" in abi.macros


def test_bounds_of_both_kernel_families():
    from audio_inpainting_diffusion_amd import _lib
    assert _lib.AID_ATTN_LONG_MAX_T == 1024 and _lib.AID_ATTN_MAX_T == 128
