"""GPU tests of the split-KV decode attention kernel
(hetu_amd/ops/hip/attention_decode.hip) through F.flash_attn_decode.

Reference: the fp64 loop in decode_attn_oracle.py on the bf16 inputs.
Bound, per output element: |out - ref| <= 3 * 2^-9 * max_j |v[b, hkv, j, d]|
over the attended keys (one bf16 rounding of P where MFMA is used, one of
the output, one unit for fp32 accumulation and exp), and |lse - ref| <= 1e-3
(fp32 dots of at most 128 exact bf16 products; inputs keep |scale q.k| far
below 30).  tests/test_decode_attn_cpu.py shows the torch branch's bf16
output meets the same bound, so it is attainable.

Every case is a few launches on [3, Hkv, 2 BN + 44, D] caches; a reference
is computed once per shape and shared.
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = [(4, 4), (8, 2), (12, 4), (6, 1), (32, 1)]
SPLITS = [0, 1, 2, 3, 8]
B = 3


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    assert F.has_ext(), "HIP extension must be built and loaded on GPU"


def BN():
    return int(F.ext().decode_attn_tile())


def cache_len():
    return 2 * BN() + 44


def length_sets():
    """Rows of kv_len that together cover {0, 1, 15, 16, 17, BN-1, BN, BN+1,
    L-1, L}."""
    bn, L = BN(), cache_len()
    return [[0, 1, 15], [16, 17, bn - 1], [bn, bn + 1, L - 1], [L, 0, bn]]


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv):
    """CPU inputs and one oracle result per length set; never modified."""
    L = cache_len()
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=D + 7 * H + Hkv)
    refs = [DO.decode_ref(q, k, v, torch.tensor(ls)) for ls in length_sets()]
    return q, k, v, refs


def lens(ls):
    return torch.tensor(ls, dtype=torch.int32, device=dev())


def hip(q, k, v, n, ns=0, scale=None):
    return F.flash_attn_decode(q, k, v, n, scale, num_splits=ns, impl="hip")


@pytest.mark.parametrize("ns", SPLITS)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_accuracy_vs_oracle(D, H, Hkv, ns):
    q, k, v, refs = case(D, H, Hkv)
    qd, kd, vd = q.to(dev()), k.to(dev()), v.to(dev())
    for ls, ref in zip(length_sets(), refs):
        out, lse = hip(qd, kd, vd, lens(ls), ns)
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        worst = DO.check(out, lse, ref, f"D{D} H{H}/{Hkv} ns{ns} {ls}")
        print(f"D{D} H{H}/{Hkv} ns{ns} kv_len{ls}: "
              f"worst out err {worst:.3e} x vmax (bound {DO.OUT_BOUND:.3e})")


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2), (6, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_int_length(D, H, Hkv):
    q, k, v, _ = case(D, H, Hkv)
    n = BN() + 1
    out, lse = hip(q.to(dev()), k.to(dev()), v.to(dev()), n)
    DO.check(out, lse, DO.decode_ref(q, k, v, n), "int kv_len")


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (12, 4), (32, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_poison_past_kv_len(D, H, Hkv, ns):
    """The cache is a view of L rows inside a larger allocation; every row
    at index >= kv_len[b] is NaN, inside the view and beyond it."""
    bn, L = BN(), cache_len()
    q, k, v, kbig, vbig = DO.make_inputs(B, H, Hkv, L, D, seed=3,
                                         alloc=L + 20, device=dev())
    for ls in ([0, 17, bn], [bn - 1, bn + 1, L - 1], [1, 2 * bn, L + 5]):
        n = lens(ls)
        kb, vb = kbig.clone(), vbig.clone()
        ref = DO.decode_ref(q, k, v, n)          # from the clean values
        DO.poison(kb, vb, n.cpu())
        out, lse = hip(q, kb[:, :, :L], vb[:, :, :L], n, ns)
        DO.check(out, lse, ref, f"poison {ls} ns{ns}")
        if ls[-1] == L + 5:                      # clamped: same as L
            o2, l2 = hip(q, kb[:, :, :L], vb[:, :, :L],
                         lens(ls[:-1] + [L]), ns)
            assert torch.equal(out, o2) and torch.equal(lse, l2)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 128), (8, 2, 64)])
def test_rescale_on_a_late_or_early_peak(H, Hkv, D, where, ns):
    """One key scores about +25 above the rest: in the last tile of the
    last non-empty split (every earlier partial is rescaled, in the split
    and in the merge), then in the first tile."""
    L = cache_len()
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=9)
    G = H // Hkv
    scale = 1.0 / math.sqrt(D)
    j = L - 2 if where == "last" else 3
    k = k.clone()
    for b in range(B):
        for hk in range(Hkv):
            qg = q[b, hk * G].float()
            k[b, hk, j] = (qg * (25.0 / scale / qg.dot(qg))).to(k.dtype)
    n = torch.tensor([L, L, L], dtype=torch.int32)
    ref = DO.decode_ref(q, k, v, n)
    s = (k[0, 0].float() @ q[0, 0].float()) * scale
    assert s[j] - s[torch.arange(L) != j].max() > 15
    out, lse = hip(q.to(dev()), k.to(dev()), v.to(dev()), n.to(dev()), ns)
    DO.check(out, lse, ref, f"rescale {where} ns{ns}")


@pytest.mark.parametrize("H,Hkv,D", [(8, 2, 128), (4, 4, 64), (6, 1, 64)])
def test_strided_views_bit_equal_to_contiguous(H, Hkv, D):
    L = cache_len()
    g = torch.Generator().manual_seed(4)
    kc = torch.randn(2, B, Hkv, L, D, generator=g).bfloat16().to(dev())
    vc = torch.randn(2, B, Hkv, L, D, generator=g).bfloat16().to(dev())
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, generator=g).bfloat16() \
        .to(dev())
    q = qkv[..., :H * D].view(B, 1, H, D)[:, 0]
    assert not q.is_contiguous()
    n = lens([17, BN() + 1, L])
    for ns in (0, 1, 3):
        out, lse = hip(q, kc[1], vc[1], n, ns)
        oc, lc = hip(q.contiguous(), kc[1].clone(), vc[1].clone(), n, ns)
        assert torch.equal(out, oc) and torch.equal(lse, lc)
    DO.check(out, lse, DO.decode_ref(q, kc[1], vc[1], n), "strided")


@pytest.mark.parametrize("H,Hkv,D", [(8, 2, 128), (32, 1, 64)])
def test_determinism(H, Hkv, D):
    q, k, v, refs = case(D, H, Hkv)
    qd, kd, vd = q.to(dev()), k.to(dev()), v.to(dev())
    ls = length_sets()[2]
    res = {}
    for ns in (0, 1, 3):
        a = hip(qd, kd, vd, lens(ls), ns)
        b = hip(qd, kd, vd, lens(ls), ns)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), ns
        res[ns] = a
    # 1 vs 3 splits: both within the bound of the oracle, and of each other
    for ns in (1, 3):
        DO.check(*res[ns], refs[2], f"ns{ns}")
    vmax = refs[2][2]
    diff = (res[1][0].double().cpu() - res[3][0].double().cpu()).abs()
    assert (diff <= DO.OUT_BOUND * vmax).all()


def test_auto_split_rule_ignores_kv_len():
    """The launcher's choice is a function of B, Hkv, L and the CU count."""
    e = F.ext()
    assert e.decode_attn_num_splits(64, 32, 8192, 256) == 1
    assert e.decode_attn_num_splits(1, 8, 8192, 256) == 64
    assert e.decode_attn_num_splits(1, 1, 100, 256) == 2     # <= tiles
    assert e.decode_attn_num_splits(1, 1, 0, 256) == 1


def test_graph_capture_with_device_length():
    """One captured call; the cache grows and kv_len advances in place
    between replays, across a tile boundary."""
    bn, L = BN(), cache_len()
    H, Hkv, D = 8, 2, 128
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=21, device=dev())
    k, v = k.clone(), v.clone()
    start = [bn - 1, 5, 2 * bn - 2]          # row 0 crosses a tile boundary
    n = lens(start)
    hip(q, k, v, n)                          # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = hip(q, k, v, n)
    gen = torch.Generator().manual_seed(22)
    for step in range(3):
        for b in range(B):
            row = start[b] + step
            k[b, :, row] = torch.randn(Hkv, D, generator=gen).bfloat16() \
                .to(dev())
            v[b, :, row] = torch.randn(Hkv, D, generator=gen).bfloat16() \
                .to(dev())
        n.add_(1)
        g.replay()
        torch.cuda.synchronize()
        assert n.tolist() == [s + step + 1 for s in start]
        DO.check(out, lse, DO.decode_ref(q, k, v, n), f"replay {step}")


def test_impl_hip_errors():
    q, k, v, _, _ = DO.make_inputs(2, 4, 2, 40, 64, device=dev())
    n = lens([3, 40])
    hip(q, k, v, n)                                           # eligible
    with pytest.raises(RuntimeError, match="not bf16"):
        hip(q.float(), k.float(), v.float(), n)
    q32, k32, v32, _, _ = DO.make_inputs(2, 4, 2, 40, 32, device=dev())
    with pytest.raises(RuntimeError, match="head dim 32"):
        hip(q32, k32, v32, n)
    with pytest.raises(RuntimeError, match="not a multiple of Hkv"):
        hip(q[:, :3], k, v, n)
    wide = torch.randn(2, 4, 128, device=dev()).bfloat16()
    with pytest.raises(RuntimeError, match="non-unit last stride"):
        hip(wide[..., ::2], k, v, n)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        hip(q, k, v, n.cpu())
    # auto on the same inputs quietly serves them from the torch branch
    o, _ = F.flash_attn_decode(q.float(), k.float(), v.float(), n)
    assert o.dtype == torch.float32


def _teacher_force(gen_hip, gen_torch, fwd, ids):
    """Prefill 5 tokens, then 6 decode steps on fixed tokens; the two
    generators' logits within the tolerance test_fa_prefill_matches_fp32_path
    uses for the same kind of comparison."""
    with torch.no_grad():
        for g in (gen_hip, gen_torch):
            fwd(g, ids[:, :5], 0)
        for pos in range(5, 11):
            lh = fwd(gen_hip, ids[:, pos:pos + 1], pos).float().cpu()
            lt = fwd(gen_torch, ids[:, pos:pos + 1], pos).float().cpu()
            assert torch.isfinite(lh).all()
            err = (lh - lt).abs().max().item()
            assert torch.allclose(lh, lt, rtol=6e-2, atol=6e-2), \
                f"step {pos}: max abs err {err}"


def test_llama_generator_hip_vs_torch():
    from hetu_amd.engine.generator import LlamaGenerator, LlamaKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=512,
                      ffn_hidden=256, vocab=301, max_seq=64)
    state = DO.llama_state(cfg, 256)
    gens = [LlamaGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                           decode_impl=impl) for impl in ("hip", "torch")]
    caches = {id(g): LlamaKVCache(cfg, 2, 16, dev(), torch.bfloat16)
              for g in gens}
    ids = torch.randint(0, cfg.vocab, (2, 11),
                        generator=torch.Generator().manual_seed(1)).to(dev())

    def fwd(g, tok, pos):
        c = caches[id(g)]
        c.kv_len.fill_(pos + tok.shape[1])
        return g._forward(tok, c, pos)
    _teacher_force(gens[0], gens[1], fwd, ids)
    out = gens[0].generate(ids[:, :5], max_new_tokens=4)
    assert out.shape == (2, 9)


def test_gpt_generator_hip_vs_torch():
    from hetu_amd.engine.generator import GPTGenerator
    from hetu_amd.models.gpt import GPTConfig
    cfg = GPTConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=256,
                    ffn_hidden=512, vocab=301, max_seq=64)
    state = DO.gpt_state(cfg, 512)
    gens = [GPTGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                         decode_impl=impl) for impl in ("hip", "torch")]
    caches = {id(g): (torch.zeros(2, 2, 4, 16, 64, device=dev(),
                                  dtype=torch.bfloat16),
                      torch.zeros(2, 2, 4, 16, 64, device=dev(),
                                  dtype=torch.bfloat16),
                      torch.zeros(2, device=dev(), dtype=torch.int32))
              for g in gens}
    ids = torch.randint(0, cfg.vocab, (2, 11),
                        generator=torch.Generator().manual_seed(2)).to(dev())

    def fwd(g, tok, pos):
        kc, vc, n = caches[id(g)]
        n.fill_(pos + tok.shape[1])
        return g._forward(tok, kc, vc, pos, n)
    _teacher_force(gens[0], gens[1], fwd, ids)
    out = gens[0].generate(ids[:, :5], max_new_tokens=4)
    assert out.shape == (2, 9)
