"""CPU-side contract of F.flash_attn_decode(impl="mfma") and of the rule and
switch behind impl=None."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402


def test_mfma_on_cpu_is_an_error_and_unknown_impl_a_value_error():
    q, k, v, _, _ = DO.make_inputs(2, 16, 2, 40, 64)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        F.flash_attn_decode(q, k, v, 7, impl="mfma")
    assert F.flash_attn_decode_on_hip(q, k, v, 7, impl="mfma")
    with pytest.raises(ValueError, match="impl must be.*'mfma'"):
        F.flash_attn_decode(q, k, v, 7, impl="wmma")


def test_env_switch_parsing():
    for s in ("auto", "hip", "mfma"):
        assert F._decode_env(s) == s
    assert F._decode_env() == os.environ.get("HETU_AMD_DECODE", "auto")
    with pytest.raises(ValueError, match="HETU_AMD_DECODE"):
        F._decode_env("torch")


@pytest.mark.parametrize("G", [1, 2, 4])
def test_auto_keeps_narrow_groups_on_the_valu_kernel(G):
    """profiles/r09_decode_mfma.md: the G = 4 control is within 1-7 % of
    the VALU kernel and which rows come out ahead changes from run to run,
    so the rule claims no G <= 4."""
    for D in (64, 128):
        for Bn, Hkv, L in ((1, 8, 2048), (16, 8, 8192), (64, 1, 8192)):
            assert not F._decode_auto_mfma(G, D, Bn, Hkv, L)
    assert F._decode_auto_mfma(8, 128, 16, 4, 8192)
