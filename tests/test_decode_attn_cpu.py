"""F.flash_attn_decode on the CPU: the torch branch against the fp64 oracle
(decode_attn_oracle.py), bit-identity of the int-length path with the
composition the generators ran before the kernel existed, unchanged CPU
generation, and the impl="hip" error.

Bounds: bf16 results meet the bound the GPU test asks of the kernel
(3 * 2^-9 * max|v| per element, lse within 1e-3), which shows that bound is
attainable; fp32 results have no output rounding, so they get 2^-18 * max|v|
(fp32 accumulation over at most a few hundred keys is orders below it) and
1e-4 on lse.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

FP32_OUT_BOUND = 2.0 ** -18
FP32_LSE_BOUND = 1e-4


def _bounds(dtype):
    if dtype == torch.float32:
        return dict(out_bound=FP32_OUT_BOUND, lse_bound=FP32_LSE_BOUND)
    return {}


# ---- the composition F.flash_attn_decode replaces: the S == 1 case of the
# ---- `else` branch of LlamaGenerator._attn before this kernel, verbatim
def _old_decode_branch(qt, kk, vv, H, Hkv, scale, dtype):
    """qt [B, H, 1, dh]; kk, vv [B, Hkv, n, dh] (the visible slice)."""
    rep = H // Hkv
    kr = kk.repeat_interleave(rep, dim=1) if rep > 1 else kk
    vr = vv.repeat_interleave(rep, dim=1) if rep > 1 else vv
    scores = (qt.float() @ kr.float().transpose(-1, -2)) \
        * scale
    p = torch.softmax(scores, dim=-1)
    o = (p @ vr.float()).to(dtype)
    return o


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (8, 2), (32, 1)])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_torch_branch_vs_oracle_tensor_len(dtype, H, Hkv, D):
    B, L = 4, 37
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, dtype, seed=D + H)
    kv_len = torch.tensor([0, 1, L, L + 9], dtype=torch.int32)
    out, lse = F.flash_attn_decode(q, k, v, kv_len)
    assert out.dtype == dtype and out.shape == (B, H, D)
    assert lse.dtype == torch.float32 and lse.shape == (B, H)
    DO.check(out, lse, DO.decode_ref(q, k, v, kv_len), "tensor kv_len",
             **_bounds(dtype))
    # kv_len > L is clamped: same as L
    o2, l2 = F.flash_attn_decode(q[3:], k[3:], v[3:],
                                 torch.tensor([L], dtype=torch.int32))
    assert torch.equal(o2, out[3:]) and torch.equal(l2, lse[3:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [0, 1, 20, 37, 50])
def test_torch_branch_vs_oracle_int_len(dtype, n):
    q, k, v, _, _ = DO.make_inputs(2, 8, 2, 37, 64, dtype, seed=n)
    out, lse = F.flash_attn_decode(q, k, v, n, impl="torch")
    DO.check(out, lse, DO.decode_ref(q, k, v, n), f"int kv_len {n}",
             **_bounds(dtype))


def test_torch_branch_ignores_rows_past_kv_len():
    """Tensor lengths mask by selection: NaN past kv_len does not leak."""
    B, H, Hkv, L, D = 3, 6, 2, 21, 64
    q, k, v, kbig, vbig = DO.make_inputs(B, H, Hkv, L, D, torch.float32,
                                         seed=5, alloc=L + 4)
    kv_len = torch.tensor([0, 7, L - 1], dtype=torch.int32)
    ref = DO.decode_ref(q, k, v, kv_len)
    DO.poison(kbig, vbig, kv_len)
    out, lse = F.flash_attn_decode(q, k, v, kv_len)
    DO.check(out, lse, ref, "poisoned", **_bounds(torch.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_strided_views(dtype):
    """Layer slices of a [2, B, Hkv, L, D] cache and a q that is a view
    into a [B, 1, (H + 2 Hkv) D] qkv buffer give what contiguous copies
    give."""
    B, H, Hkv, L, D = 2, 6, 2, 19, 64
    g = torch.Generator().manual_seed(11)
    kc = torch.randn(2, B, Hkv, L, D, generator=g).to(dtype)
    vc = torch.randn(2, B, Hkv, L, D, generator=g).to(dtype)
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, generator=g).to(dtype)
    q = qkv[..., :H * D].view(B, 1, H, D)[:, 0]
    assert not q.is_contiguous()
    kv_len = torch.tensor([5, L], dtype=torch.int32)
    for n in (kv_len, 13):
        out, lse = F.flash_attn_decode(q, kc[1], vc[1], n)
        oc, lc = F.flash_attn_decode(q.contiguous(), kc[1].contiguous(),
                                     vc[1].contiguous(), n)
        assert torch.equal(out, oc) and torch.equal(lse, lc)
        DO.check(out, lse, DO.decode_ref(q, kc[1], vc[1], n), "strided",
                 **_bounds(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (6, 1)])
def test_int_path_bit_identical_to_old_composition(dtype, H, Hkv):
    B, L, D, n = 2, 40, 64, 23
    g = torch.Generator().manual_seed(H)
    # operands laid out as the generator has them: q [B, 1, H, dh] permuted,
    # the cache a layer of [n_layer, B, Hkv, L, dh]
    q4 = torch.randn(B, 1, H, D, generator=g).to(dtype)
    kc = torch.randn(2, B, Hkv, L, D, generator=g).to(dtype)
    vc = torch.randn(2, B, Hkv, L, D, generator=g).to(dtype)
    scale = 1.0 / math.sqrt(D)
    old = _old_decode_branch(q4.permute(0, 2, 1, 3), kc[1][:, :, :n],
                             vc[1][:, :, :n], H, Hkv, scale, dtype)
    old = old.permute(0, 2, 1, 3).reshape(B, 1, H * D)
    new, _ = F.flash_attn_decode(q4[:, 0], kc[1], vc[1], n, scale)
    assert torch.equal(new.reshape(B, 1, H * D), old)


# ---- generators: the parent's _attn, kept here as the reference step ------
def _llama_attn_parent(self, x, layer, cache, pos0):
    cfg = self.cfg
    B, S, _ = x.shape
    H, Hkv = cfg.n_head, cfg.n_kv_head
    dh = cfg.hidden // H
    qkv = x @ self.w[f"l{layer}.attn.wqkv.weight"].t()
    q, k, v = qkv.split([H * dh, Hkv * dh, Hkv * dh], dim=-1)
    q = q.view(B, S, H, dh)
    k = k.view(B, S, Hkv, dh)
    cos = self.cos[pos0:pos0 + S]
    sin = self.sin[pos0:pos0 + S]
    q = F.rope_fwd(q, cos, sin)
    k = F.rope_fwd(k, cos, sin)
    v = v.view(B, S, Hkv, dh)
    cache.k[layer][:, :, pos0:pos0 + S] = k.permute(0, 2, 1, 3)
    cache.v[layer][:, :, pos0:pos0 + S] = v.permute(0, 2, 1, 3)
    kk = cache.k[layer][:, :, :pos0 + S]
    vv = cache.v[layer][:, :, :pos0 + S]
    qt = q.permute(0, 2, 1, 3)
    rep = H // Hkv
    kr = kk.repeat_interleave(rep, dim=1) if rep > 1 else kk
    vr = vv.repeat_interleave(rep, dim=1) if rep > 1 else vv
    mask = None
    if S > 1:
        Skv = pos0 + S
        mask = torch.ones(S, Skv, dtype=torch.bool,
                          device=x.device).tril(diagonal=Skv - S)
    scores = (qt.float() @ kr.float().transpose(-1, -2)) \
        * self.scale
    if mask is not None:
        scores = scores.masked_fill(~mask, float("-inf"))
    p = torch.softmax(scores, dim=-1)
    o = (p @ vr.float()).to(x.dtype)
    o = o.permute(0, 2, 1, 3).reshape(B, S, H * dh)
    return o @ self.w[f"l{layer}.attn.wo.weight"].t()


def _gpt_attn_parent(self, x, layer, kcache, vcache, pos0, kv_len=None):
    cfg = self.cfg
    B, S, _ = x.shape
    H = cfg.n_head
    dh = cfg.hidden // H
    qkv = self._lin(x, f"h{layer}.attn.wqkv")
    q, k, v = qkv.chunk(3, -1)
    q = q.view(B, S, H, dh).permute(0, 2, 1, 3)
    kcache[layer][:, :, pos0:pos0 + S] = \
        k.view(B, S, H, dh).permute(0, 2, 1, 3)
    vcache[layer][:, :, pos0:pos0 + S] = \
        v.view(B, S, H, dh).permute(0, 2, 1, 3)
    kk = kcache[layer][:, :, :pos0 + S]
    vv = vcache[layer][:, :, :pos0 + S]
    scores = (q.float() @ kk.float().transpose(-1, -2)) * self.scale
    if S > 1:
        Skv = pos0 + S
        mask = torch.ones(S, Skv, dtype=torch.bool,
                          device=x.device).tril(diagonal=Skv - S)
        scores = scores.masked_fill(~mask, float("-inf"))
    o = (torch.softmax(scores, -1) @ vv.float()).to(x.dtype)
    o = o.permute(0, 2, 1, 3).reshape(B, S, H * dh)
    return self._lin(o, f"h{layer}.attn.wo")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_llama_generator_unchanged_on_cpu(dtype):
    from hetu_amd.engine.generator import LlamaGenerator, LlamaKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=64,
                      ffn_hidden=48, vocab=97, max_seq=32)
    state = DO.llama_state(cfg, 48)
    cpu = torch.device("cpu")
    new = LlamaGenerator(cfg, state, device=cpu, dtype=dtype)
    old = LlamaGenerator(cfg, state, device=cpu, dtype=dtype)
    old._attn = _llama_attn_parent.__get__(old)
    ids = torch.randint(0, cfg.vocab, (2, 12),
                        generator=torch.Generator().manual_seed(1))
    cn = LlamaKVCache(cfg, 2, 16, cpu, dtype)
    co = LlamaKVCache(cfg, 2, 16, cpu, dtype)
    with torch.no_grad():
        assert torch.equal(new._forward(ids[:, :5], cn, 0),
                           old._forward(ids[:, :5], co, 0))
        for pos in range(5, 12):
            ln = new._forward(ids[:, pos:pos + 1], cn, pos)
            lo = old._forward(ids[:, pos:pos + 1], co, pos)
            assert torch.equal(ln, lo), pos
    assert torch.equal(cn.k, co.k) and torch.equal(cn.v, co.v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpt_generator_unchanged_on_cpu(dtype):
    from hetu_amd.engine.generator import GPTGenerator
    from hetu_amd.models.gpt import GPTConfig
    cfg = GPTConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=64,
                    ffn_hidden=96, vocab=97, max_seq=32)
    state = DO.gpt_state(cfg, 96)
    cpu = torch.device("cpu")
    new = GPTGenerator(cfg, state, device=cpu, dtype=dtype)
    old = GPTGenerator(cfg, state, device=cpu, dtype=dtype)
    old._attn = _gpt_attn_parent.__get__(old)
    ids = torch.randint(0, cfg.vocab, (2, 12),
                        generator=torch.Generator().manual_seed(2))
    kn = torch.zeros(2, 2, 4, 16, 16, dtype=dtype)
    vn, ko, vo = (torch.zeros_like(kn) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(new._forward(ids[:, :5], kn, vn, 0),
                           old._forward(ids[:, :5], ko, vo, 0))
        for pos in range(5, 12):
            ln = new._forward(ids[:, pos:pos + 1], kn, vn, pos)
            lo = old._forward(ids[:, pos:pos + 1], ko, vo, pos)
            assert torch.equal(ln, lo), pos
    # and the public loop still runs end to end
    out = new.generate(ids[:, :5], max_new_tokens=3)
    assert out.shape == (2, 8)


def test_generate_single_token_prompt_cpu():
    from hetu_amd.engine.generator import LlamaGenerator
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=1, n_head=4, n_kv_head=2, hidden=64,
                      ffn_hidden=48, vocab=97, max_seq=32)
    gen = LlamaGenerator(cfg, DO.llama_state(cfg, 48),
                         device=torch.device("cpu"))
    out = gen.generate(torch.tensor([[3], [5]]), max_new_tokens=3)
    assert out.shape == (2, 4)


def test_errors():
    q, k, v, _, _ = DO.make_inputs(2, 4, 2, 9, 64)
    with pytest.raises(RuntimeError, match="impl='hip'"):
        F.flash_attn_decode(q, k, v, 5, impl="hip")
    with pytest.raises(ValueError, match="impl must be"):
        F.flash_attn_decode(q, k, v, 5, impl="fast")
    with pytest.raises(ValueError, match="need q"):
        F.flash_attn_decode(q[:, :, None], k, v, 5)
    assert not F.flash_attn_decode_on_hip(q, k, v)
