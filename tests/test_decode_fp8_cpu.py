"""CPU tests of the fp8 KV cache: the torch branches of
F.kv_cache_append_fp8 and of F.flash_attn_decode over e4m3 caches, the
dispatch errors that need no GPU, and the generator cache's default."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import decode_fp8_cases as C  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

B, L = 3, 300


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_append_torch_branch(D, S):
    H, Hkv = 4, 2
    for i, end in enumerate(([S, 130, L], [L + 3, 2, 130])):
        k, v = C.append_inputs(B, S, H, Hkv, D, seed=D + S + i)
        kc = torch.full((B, Hkv, L, D), 0x55, dtype=torch.uint8).view(C.FP8)
        vc = kc.clone()
        ks = torch.full((B, Hkv, L), 7.0)
        vs = ks.clone()
        before = (kc.clone(), ks.clone())
        F.kv_cache_append_fp8(k, v, kc, vc, ks, vs,
                              torch.tensor(end, dtype=torch.int32))
        C.check_append(k, kc, ks, before, end, f"K D{D} S{S} end{end}")
        C.check_append(v, vc, vs, before, end, f"V D{D} S{S} end{end}")


@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 64), (16, 2, 128)])
def test_decode_torch_branch_vs_oracle(H, Hkv, D):
    q, k, ks, v, vs = C.make_fp8_inputs(B, H, Hkv, L, D, seed=H + D)
    for n in (torch.tensor([0, 17, L + 5], dtype=torch.int32), 129):
        pk, pks = k.clone(), ks.clone()
        if isinstance(n, torch.Tensor):          # poison past kv_len
            for b, m in enumerate(n.tolist()):
                pk.view(torch.uint8)[b, :, m:] = 0x7F
                pks[b, :, m:] = float("nan")
        out, lse = F.flash_attn_decode(q, pk, v, n, k_scale=pks, v_scale=vs)
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        ref = DO.decode_ref(q, C.dequant(k, ks), C.dequant(v, vs), n)
        DO.check(out, lse, ref, f"torch branch {n}")


def test_dispatch_errors_without_a_gpu():
    q, k, ks, v, vs = C.make_fp8_inputs(2, 4, 2, 40, 64)
    bf = k.float().bfloat16()
    with pytest.raises(RuntimeError, match="needs k_scale"):
        F.flash_attn_decode(q, k, v, 3)
    with pytest.raises(RuntimeError, match="needs v_scale"):
        F.flash_attn_decode(q, k, v, 3, k_scale=ks)
    with pytest.raises(RuntimeError, match="k_scale given with a"):
        F.flash_attn_decode(q, bf, bf, 3, k_scale=ks, v_scale=vs)
    with pytest.raises(RuntimeError, match=r"k_cache is uint8.*\.view"):
        F.flash_attn_decode(q, k.view(torch.uint8), v.view(torch.uint8), 3,
                            k_scale=ks, v_scale=vs)
    with pytest.raises(RuntimeError, match="v_scale has shape"):
        F.flash_attn_decode(q, k, v, 3, k_scale=ks, v_scale=vs[:, :1])
    with pytest.raises(RuntimeError, match="k_scale is torch.float16"):
        F.flash_attn_decode(q, k, v, 3, k_scale=ks.half(), v_scale=vs)
    with pytest.raises(RuntimeError, match="q is not on the GPU"):
        F.flash_attn_decode(q, k, v, 3, impl="hip", k_scale=ks, v_scale=vs)
    with pytest.raises(RuntimeError, match=r"v_cache is uint8.*\.view"):
        F.kv_cache_append_fp8(q[:, None], q[:, None], k, v.view(torch.uint8),
                              ks, vs, torch.tensor([1, 1]))
    assert not F.flash_attn_decode_on_hip(q, k, v, k_scale=ks, v_scale=vs)


def test_generator_cache_default_and_fp8_allocation():
    from hetu_amd.engine.generator import LlamaGenerator, LlamaKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=256,
                      ffn_hidden=64, vocab=53, max_seq=32)
    c = LlamaKVCache(cfg, 2, 16, "cpu", torch.bfloat16)
    assert c.kv_dtype is None and not hasattr(c, "k_scale")
    assert c.k.dtype == c.v.dtype == torch.bfloat16
    assert c.k.shape == c.v.shape == (2, 2, 2, 16, 64)
    c8 = LlamaKVCache(cfg, 2, 16, "cpu", torch.bfloat16, kv_dtype="fp8")
    assert c8.k.dtype == c8.v.dtype == C.FP8 and c8.k.shape == c.k.shape
    assert c8.k_scale.shape == c8.v_scale.shape == (2, 2, 2, 16)
    assert c8.k_scale.dtype == torch.float32
    with pytest.raises(ValueError, match="kv_dtype"):
        LlamaKVCache(cfg, 2, 16, "cpu", torch.bfloat16, kv_dtype="int4")
    # the fp8 generator runs end to end on the torch branches: prefill and
    # one decode step fill rows 0 .. 5 of every layer, nothing else
    ids = torch.randint(0, cfg.vocab, (2, 6),
                        generator=torch.Generator().manual_seed(0))
    g = LlamaGenerator(cfg, DO.llama_state(cfg, 64),
                       device=torch.device("cpu"), dtype=torch.float32,
                       kv_dtype="fp8")
    with torch.no_grad():
        c8.kv_len.fill_(5)
        g._forward(ids[:, :5], c8, 0)
        c8.kv_len.fill_(6)
        logits = g._forward(ids[:, 5:6], c8, 5)
    assert torch.isfinite(logits).all()
    for sc in (c8.k_scale, c8.v_scale):
        assert (sc[..., :6] > 0).all() and (sc[..., 6:] == 0).all()
