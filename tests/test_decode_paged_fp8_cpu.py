"""CPU tests of fp8 page pools: the torch branches of F.flash_attn_decode and
F.kv_cache_append_paged over e4m3 code pools [P, Hkv, PS, D] with fp32 scale
pools [P, Hkv, PS], and the paged fp8 generator against the dense fp8 one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import decode_fp8_cases as C  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

B = 3


def raw(x):
    """Codes as bytes (torch.equal has no fp8 form); scales as they are."""
    return x.view(torch.uint8) if x.dtype == C.FP8 else x


def scatter(ins, PS, lens, seed, device="cpu"):
    """Dense (k, k_scale, v, v_scale) [B, Hkv, L(, D)] -> (pools, table, P):
    views of P pages of P + 2 behind a shuffled table whose pages interleave
    the sequences.  0x7F bytes / NaN scales fill rows at or past lens[b], the
    unowned page and the pages beyond P; unneeded entries hold garbage."""
    Bk, Hkv, L = ins[0].shape[:3]
    MP = L // PS
    P = Bk * MP + 1
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    table = perm[:Bk * MP].view(MP, Bk).t().contiguous()
    pools = []
    for t in ins:
        codes = t.dim() == 4
        bad = 0x7F if codes else float("nan")
        t = (t.view(torch.uint8) if codes else t.unsqueeze(-1)).cpu().clone()
        for b, n in enumerate(lens):
            t[b, :, n:] = bad
        big = torch.full((P + 2, Hkv, PS, t.shape[-1]), bad, dtype=t.dtype)
        big[table] = t.view(Bk, Hkv, MP, PS, -1).permute(0, 2, 1, 3, 4)
        big = big.to(device)[:P]
        pools.append(big.view(C.FP8) if codes else big[..., 0])
    for b, n in enumerate(lens):
        table[b, -(-n // PS):] = 2 ** 30 + b
    return pools, table.to(torch.int32).to(device), P


@pytest.mark.parametrize("PS", [32, 64])
def test_torch_branch_over_pools(PS):
    """Equal to the dense fp8 torch branch on the same values; a needed entry
    outside [0, P) masks its page."""
    H, Hkv, D, L = 8, 2, 64, 256
    ins = C.make_fp8_inputs(B, H, Hkv, L, D, seed=PS)
    q, k, ks, v, vs = ins
    lens = [0, PS + 1, L]
    n = torch.tensor(lens, dtype=torch.int32)
    (kp, ksp, vp, vsp), table, P = scatter(ins[1:], PS, lens, seed=PS)
    out, lse = F.flash_attn_decode(q, kp, vp, n, k_scale=ksp, v_scale=vsp,
                                   block_table=table)
    do, dl = F.flash_attn_decode(q, k, v, n, k_scale=ks, v_scale=vs)
    assert torch.equal(out, do) and torch.equal(lse, dl)
    table[2, 0] = P
    out, lse = F.flash_attn_decode(q, kp, vp, n, k_scale=ksp, v_scale=vsp,
                                   block_table=table)
    kd, vd = C.dequant(k, ks), C.dequant(v, vs)
    head = DO.decode_ref(q[:2], kd[:2], vd[:2], n[:2])
    tail = DO.decode_ref(q[2:], kd[2:, :, PS:], vd[2:, :, PS:], L - PS)
    DO.check(out, lse, tuple(torch.cat([a, b]) for a, b in zip(head, tail)))


@pytest.mark.parametrize("S", [1, 5])
def test_torch_append_is_the_dense_append_behind_the_table(S):
    H, Hkv, D, PS, MP, P = 4, 2, 64, 32, 3, 10
    k_new, v_new = C.append_inputs(B, S, H, Hkv, D, seed=S)
    table = torch.randperm(P, generator=torch.Generator().manual_seed(S)) \
        [:B * MP].view(B, MP).to(torch.int32)
    table[1, 1] = P                       # these rows are dropped
    end = torch.tensor([S, PS + 2, MP * PS + 2], dtype=torch.int32)
    dense = [torch.zeros(B, Hkv, MP * PS, D).to(C.FP8) for _ in range(2)] \
        + [torch.zeros(B, Hkv, MP * PS) for _ in range(2)]
    F.kv_cache_append_fp8(k_new, v_new, dense[0], dense[1], dense[2],
                          dense[3], end)
    pools = [torch.full((P, Hkv, PS, D), 0x55, dtype=torch.uint8).view(C.FP8)
             for _ in range(2)] + [torch.full((P, Hkv, PS), 7.0)
                                   for _ in range(2)]
    want = [p.clone() for p in pools]
    for b in range(B):
        for j in range(max(int(end[b]) - S, 0), min(int(end[b]), MP * PS)):
            if table[b, j // PS] < P:
                for w, d in zip(want, dense):
                    w[table[b, j // PS], :, j % PS] = d[b, :, j]
    F.kv_cache_append_paged(k_new, v_new, pools[0], pools[1], table, end,
                            k_scale=pools[2], v_scale=pools[3])
    for got, w in zip(pools, want):
        assert torch.equal(raw(got), raw(w))
    with pytest.raises(RuntimeError, match="fp8 pools need k_scale"):
        F.kv_cache_append_paged(k_new, v_new, pools[0], pools[1], table, end)
    with pytest.raises(RuntimeError, match="cu_q .* fp8"):
        F.kv_cache_append_paged(k_new[0], v_new[0], pools[0], pools[1], table,
                                end, cu_q=end, k_scale=pools[2],
                                v_scale=pools[3])


def test_generator_paged_fp8_matches_dense_fp8():
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=256,
                      ffn_hidden=64, vocab=53, max_seq=64)
    state = DO.llama_state(cfg, 64)
    kw = dict(device=torch.device("cpu"), dtype=torch.float32, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8 prefill kernel .* does not exist"):
        LlamaGenerator(cfg, state, kv_layout="paged", prefill="packed", **kw)
    c = PagedKVCache(cfg, [40, 9], 32, "cpu", torch.float32, kv_dtype="fp8")
    assert c.k.dtype == c.v.dtype == C.FP8 and c.k.shape == (2, 3, 2, 32, 64)
    assert c.k_scale.shape == c.v_scale.shape == (2, 3, 2, 32)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g)
               for n in (30, 5)]          # the first crosses a page
    paged = LlamaGenerator(cfg, state, kv_layout="paged", page_size=32, **kw)
    dense = LlamaGenerator(cfg, state, **kw)
    outs = paged.generate(prompts, max_new_tokens=6)
    for p, o in zip(prompts, outs):
        assert torch.equal(o, dense.generate(p[None], max_new_tokens=6)[0])
