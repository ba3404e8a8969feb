"""CPU tests of the packed prefill over the paged KV cache: the torch branches,
the argument errors, LlamaGenerator(prefill="packed") against "sequence"."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import prefill_paged_oracle as PO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402
from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache  # noqa: E402
from hetu_amd.models.llama import LlamaConfig  # noqa: E402


def call(c, **kw):
    return F.flash_attn_prefill_paged(c["q"], c["k_pool"], c["v_pool"],
                                      c["table"], c["cu_q"], c["kv_len"], **kw)


@pytest.mark.parametrize("PS", [32, 256])
def test_torch_branch_meets_fp64_reference(PS):
    c = PO.build(8, 2, PS, dtype=torch.float32)
    out, lse = call(c)
    ro, rl, _ = PO.ref(c)
    assert out.dtype == torch.float32 and lse.shape == (8, c["q"].shape[0])
    assert torch.allclose(out.double(), ro, rtol=1e-5, atol=1e-6)
    assert torch.equal(torch.isinf(lse.t()), torch.isinf(rl))
    assert torch.allclose(lse.t().double(), rl, rtol=1e-5)   # inf == inf
    assert (out[torch.isinf(rl)] == 0).all()


def test_packed_append_torch_branch_equals_a_loop():
    Hkv, Dh, PS, MP, P = 2, 16, 32, 3, 8
    g = torch.Generator().manual_seed(0)
    ns = [5, 0, 40, 3]                    # ragged, one empty chunk
    # in page 0; empty; crossing into a dropped page; past MP * PS
    end = torch.tensor([5, 7, 70, MP * PS + 1], dtype=torch.int32)
    cu = torch.tensor([0, 5, 5, 45, 48], dtype=torch.int32)
    table = torch.tensor([[6, 1, 2], [P, P, P], [3, P, 4], [5, 0, 7]],
                         dtype=torch.int32)
    k_new = torch.randn(48, Hkv, Dh, generator=g)
    v_new = torch.randn(48, Hkv, Dh, generator=g)
    kp = torch.full((P, Hkv, PS, Dh), PO.NAN)
    vp = torch.full((P, Hkv, PS, Dh), PO.NAN)
    want_k, want_v = kp.clone(), vp.clone()
    for b, n in enumerate(ns):
        for i in range(n):
            j = int(end[b]) - n + i
            page = int(table[b, j // PS]) if 0 <= j < MP * PS else -1
            if 0 <= page < P:
                want_k[page, :, j % PS] = k_new[int(cu[b]) + i]
                want_v[page, :, j % PS] = v_new[int(cu[b]) + i]
    F.kv_cache_append_paged(k_new, v_new, kp, vp, table, end, cu_q=cu)
    assert torch.equal(kp.nan_to_num(7.0), want_k.nan_to_num(7.0))
    assert torch.equal(vp.nan_to_num(7.0), want_v.nan_to_num(7.0))
    # 5 + (40 - 32 in the dropped page) + (3 - 1 past the end) rows landed
    assert int((~kp.isnan()).sum()) == (5 + 8 + 2) * Hkv * Dh


def test_argument_errors():
    c = PO.build(4, 2, 32, seqs=((0, 3), (2, 2)))
    with pytest.raises(ValueError, match="q is not on the GPU"):
        call(c, impl="hip")
    d64 = dict(c, q=c["q"][..., :64], k_pool=c["k_pool"][..., :64],
               v_pool=c["v_pool"][..., :64])
    with pytest.raises(ValueError, match="q is not on the GPU|head dim of q"):
        call(d64, impl="hip")
    odd = torch.zeros(4, 2, 48, PO.D, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="page size of k_pool"):
        call(dict(c, k_pool=odd, v_pool=odd))
    with pytest.raises(ValueError, match=r"cu_q \[B \+ 1\]"):
        call(dict(c, cu_q=c["cu_q"][:2]))
    cfg = LlamaConfig(n_layer=1, n_head=2, n_kv_head=1, hidden=256,
                      ffn_hidden=64, vocab=50, max_seq=16)
    with pytest.raises(ValueError, match="needs kv_layout='paged'"):
        LlamaGenerator(cfg, DO.llama_state(cfg, 64), prefill="packed")


@pytest.mark.parametrize("chunk", [None, 1, 64])
def test_generator_packed_equals_sequence_on_cpu(chunk):
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=512,
                      ffn_hidden=256, vocab=301, max_seq=160)
    state = DO.llama_state(cfg, 256)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g)
               for n in (3, 70, 131)]
    lens = [p.numel() for p in prompts]
    kw = dict(device=torch.device("cpu"), kv_layout="paged", page_size=32)
    seq = LlamaGenerator(cfg, state, **kw)
    pk = LlamaGenerator(cfg, state, prefill="packed", prefill_chunk=chunk,
                        **kw)
    with torch.no_grad():
        cache = PagedKVCache(cfg, lens, 32, kw["device"], torch.float32)
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        want = torch.cat([seq._forward(p.unsqueeze(0), cache.row(b), 0)
                          for b, p in enumerate(prompts)])
        cache = PagedKVCache(cfg, lens, 32, kw["device"], torch.float32)
        got = pk._prefill_packed(prompts, lens, cache)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), \
        (got - want).abs().max()
    a, b = seq.generate(prompts, 8), pk.generate(prompts, 8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
