"""CPU tests of the paged KV cache's torch branches (F.flash_attn_decode with
a block_table, F.kv_cache_append_paged) and of paged generation.

The gather form must equal F._decode_torch on the gathered dense cache
exactly, and that within the oracle's bounds; the append equals plain
indexing; paged greedy generation on ragged prompts returns, per prompt, the
tokens of the dense generator run on that prompt alone.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402


def scatter_pool(k, v, PS, seed=0, extra=1):
    """Dense [B, Hkv, L, D] caches -> pools [P, Hkv, PS, D] behind a randomly
    permuted table [B, L / PS]; `extra` pages belong to nobody."""
    B, Hkv, L, D = k.shape
    MP = L // PS
    P = B * MP + extra
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    table = perm[:B * MP].view(MP, B).t().contiguous().to(torch.int32)
    pools = []
    for t in (k, v):
        pool = torch.zeros(P, Hkv, PS, D, dtype=t.dtype)
        pages = t.view(B, Hkv, MP, PS, D).permute(0, 2, 1, 3, 4)
        pool[table.long()] = pages
        pools.append(pool)
    return pools[0], pools[1], table


@pytest.mark.parametrize("PS", [32, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_form_equals_dense_torch(PS, dtype):
    B, H, Hkv, L, D = 3, 8, 2, 256, 64
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, dtype=dtype, seed=PS)
    kp, vp, table = scatter_pool(k, v, PS)
    kv_len = torch.tensor([0, PS + 1, L], dtype=torch.int32)
    # whatever lies past a row's last needed page is never indexed
    table[0, :] = 10 ** 6
    table[1, 2:] = -7
    out, lse = F.flash_attn_decode(q, kp, vp, kv_len, impl="torch",
                                   block_table=table)
    ro, rl = F._decode_torch(q, k, v, kv_len, 1.0 / D ** 0.5)
    assert torch.equal(out, ro) and torch.equal(lse, rl)
    DO.check(out, lse, DO.decode_ref(q, k, v, kv_len), f"PS={PS} {dtype}")
    # an int length is the same call
    o2, l2 = F.flash_attn_decode(q[2:], kp, vp, L, impl="torch",
                                 block_table=table[2:])
    assert torch.equal(o2, out[2:]) and torch.equal(l2, lse[2:])


def test_gather_form_masks_out_of_range_page():
    B, H, Hkv, L, D, PS = 2, 4, 2, 128, 64, 32
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=3)
    kp, vp, table = scatter_pool(k, v, PS)
    kv_len = torch.tensor([L, 70], dtype=torch.int32)
    table[0, 1] = kp.shape[0]            # keys 32 .. 63 of row 0 vanish
    out, lse = F.flash_attn_decode(q, kp, vp, kv_len, impl="torch",
                                   block_table=table)
    keep = [j for j in range(L) if not 32 <= j < 64]
    r0 = DO.decode_ref(q[:1], k[:1, :, keep], v[:1, :, keep], L - 32)
    r1 = DO.decode_ref(q[1:], k[1:], v[1:], 70)
    DO.check(out, lse, tuple(torch.cat([a, b]) for a, b in zip(r0, r1)))


@pytest.mark.parametrize("S", [1, 5])
def test_append_torch_is_plain_indexing(S):
    B, Hkv, D, PS, MP, P = 3, 2, 64, 32, 3, 10
    g = torch.Generator().manual_seed(S)
    k_new = torch.randn(B, S, Hkv, D, generator=g)
    v_new = torch.randn(B, S, Hkv, D, generator=g)
    table = torch.randperm(P, generator=g)[:B * MP].view(B, MP) \
        .to(torch.int32)
    table[1, 1] = P                       # rows of this page are dropped
    end = torch.tensor([S, PS + 2, MP * PS + 2], dtype=torch.int32)
    kp = torch.randn(P, Hkv, PS, D, generator=g)
    vp = torch.randn(P, Hkv, PS, D, generator=g)
    want_k, want_v = kp.clone(), vp.clone()
    for b in range(B):
        for s in range(S):
            j = int(end[b]) - S + s
            page = int(table[b, j // PS]) if 0 <= j < MP * PS else -1
            if 0 <= page < P:
                want_k[page, :, j % PS] = k_new[b, s]
                want_v[page, :, j % PS] = v_new[b, s]
    F.kv_cache_append_paged(k_new, v_new, kp, vp, table, end)
    assert torch.equal(kp, want_k) and torch.equal(vp, want_v)


def test_generate_paged_matches_dense_per_prompt():
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=64,
                      ffn_hidden=96, vocab=97, max_seq=128)
    state = DO.llama_state(cfg, 96)
    dense = LlamaGenerator(cfg, state, device=torch.device("cpu"))
    paged = LlamaGenerator(cfg, state, device=torch.device("cpu"),
                           kv_layout="paged", page_size=32)
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g)
               for n in (5, 30, 9)]
    new = 40                              # every sequence crosses a page
    got = paged.generate(prompts, max_new_tokens=new)
    assert isinstance(got, list) and len(got) == len(prompts)
    for p, o in zip(prompts, got):
        want = dense.generate(p.unsqueeze(0), max_new_tokens=new)[0]
        assert torch.equal(o, want)
    # a rectangular batch keeps the tensor form; an eos cuts a ragged row
    rect = paged.generate(torch.stack([prompts[0], prompts[0]]),
                          max_new_tokens=3)
    assert rect.shape == (2, 8) and torch.equal(rect[0], got[0][:8])
    eos = int(got[0][7])
    cut = paged.generate(prompts[:1], max_new_tokens=new, eos_id=eos)[0]
    first = (got[0][5:] == eos).nonzero()[0].item()
    assert torch.equal(cut, got[0][:5 + first + 1])
    cache = PagedKVCache(cfg, [n + new for n in (5, 30, 9)], 32, "cpu",
                         torch.float32)
    assert cache.num_pages == 2 + 3 + 2 and cache.k.shape[1] == 7
    assert cache.block_table.tolist() == [[0, 3, 7], [1, 4, 6], [2, 5, 7]]
