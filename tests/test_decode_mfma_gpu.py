"""GPU tests of the MFMA decode attention kernel
(hetu_amd/ops/hip/attention_decode_mfma.hip) through
F.flash_attn_decode(impl="mfma").

Reference and bound are tests/decode_attn_oracle.py's: the fp64 loop on the
bf16 inputs, |out - ref| <= 3 * 2^-9 * max_j |v| per element (it budgets the
one bf16 rounding of P), |lse - ref| <= 1e-3.  Every case is a few launches
on [3, Hkv, 2 T + 44, D] caches, T = decode_attn_mfma_tile(); a reference is
computed once per shape and shared.
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

# a full tile, ragged tiles, MT = 1 / 2 / 4 head tiles, and G = 1
HEADS = [(8, 1), (16, 2), (20, 4), (32, 1), (40, 1), (64, 1), (4, 4)]
B = 3


def dev():
    return torch.device("cuda", 0)


def T():
    return int(F.ext().decode_attn_mfma_tile())


def cache_len():
    return 2 * T() + 44


def length_sets():
    t, L = T(), cache_len()
    return [[0, 1, 15], [16, 17, 31], [32, 33, t - 1], [t, t + 1, L - 1],
            [L, 0, t]]


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv):
    """CPU inputs and one oracle result per length set; never modified."""
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, cache_len(), D,
                                   seed=D + 7 * H + Hkv)
    refs = [DO.decode_ref(q, k, v, torch.tensor(ls)) for ls in length_sets()]
    return q, k, v, refs


def lens(ls):
    return torch.tensor(ls, dtype=torch.int32, device=dev())


def mfma(q, k, v, n, ns=0, scale=None):
    return F.flash_attn_decode(q, k, v, n, scale, num_splits=ns, impl="mfma")


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_accuracy_vs_oracle(D, H, Hkv, ns):
    q, k, v, refs = case(D, H, Hkv)
    qd, kd, vd = q.to(dev()), k.to(dev()), v.to(dev())
    for ls, ref in zip(length_sets(), refs):
        out, lse = mfma(qd, kd, vd, lens(ls), ns)
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        worst = DO.check(out, lse, ref, f"D{D} H{H}/{Hkv} ns{ns} {ls}")
        print(f"D{D} H{H}/{Hkv} ns{ns} kv_len{ls}: "
              f"worst out err {worst:.3e} x vmax (bound {DO.OUT_BOUND:.3e})")


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("H,Hkv", [(16, 2), (32, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_poison_past_kv_len(D, H, Hkv, ns):
    """Every cache row at index >= kv_len[b] is NaN, inside the [.., L, D]
    view and in the allocation beyond it."""
    t, L = T(), cache_len()
    q, k, v, kbig, vbig = DO.make_inputs(B, H, Hkv, L, D, seed=3,
                                         alloc=L + 20, device=dev())
    for ls in ([0, 17, t], [t - 1, t + 1, L - 1], [33, 2 * t, L + 5]):
        n = lens(ls)
        kb, vb = kbig.clone(), vbig.clone()
        ref = DO.decode_ref(q, k, v, n)          # from the clean values
        DO.poison(kb, vb, n.cpu())
        out, lse = mfma(q, kb[:, :, :L], vb[:, :, :L], n, ns)
        DO.check(out, lse, ref, f"poison {ls} ns{ns}")
        if ls[-1] == L + 5:                      # clamped: same as L
            o2, l2 = mfma(q, kb[:, :, :L], vb[:, :, :L],
                          lens(ls[:-1] + [L]), ns)
            assert torch.equal(out, o2) and torch.equal(lse, l2)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("H,Hkv,D", [(16, 2, 128), (32, 1, 64)])
def test_rescale_on_a_late_or_early_peak(H, Hkv, D, where, ns):
    """One key scores about +25 above the rest, in the last tile (every
    earlier partial is rescaled, in the wave, the block and the merge), then
    in the first."""
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
    s = (k[0, 0].float() @ q[0, 0].float()) * scale
    assert s[j] - s[torch.arange(L) != j].max() > 15
    out, lse = mfma(q.to(dev()), k.to(dev()), v.to(dev()), n.to(dev()), ns)
    DO.check(out, lse, DO.decode_ref(q, k, v, n), f"rescale {where} ns{ns}")


@pytest.mark.parametrize("H,Hkv,D", [(16, 2, 128), (32, 1, 64)])
def test_strided_views_and_repeats_are_bit_equal(H, Hkv, D):
    """A layer slice of a 5-D cache and q as a view into a fused qkv row
    against contiguous copies; the contiguous call twice."""
    L = cache_len()
    g = torch.Generator().manual_seed(4)
    kc = torch.randn(2, B, Hkv, L, D, generator=g).bfloat16().to(dev())
    vc = torch.randn(2, B, Hkv, L, D, generator=g).bfloat16().to(dev())
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, generator=g).bfloat16() \
        .to(dev())
    q = qkv[..., :H * D].view(B, 1, H, D)[:, 0]
    assert not q.is_contiguous()
    n = lens([17, T() + 1, L])
    for ns in (0, 1, 3):
        out, lse = mfma(q, kc[1], vc[1], n, ns)
        args = (q.contiguous(), kc[1].clone(), vc[1].clone(), n, ns)
        for _ in range(2):
            oc, lc = mfma(*args)
            assert torch.equal(out, oc) and torch.equal(lse, lc)
    DO.check(out, lse, DO.decode_ref(q, kc[1], vc[1], n), "strided")


def test_graph_capture_with_device_length():
    """One captured call; the cache grows and kv_len advances in place
    between replays, across a tile boundary."""
    t, L = T(), cache_len()
    H, Hkv, D = 16, 2, 128
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=21, device=dev())
    k, v = k.clone(), v.clone()
    start = [t - 1, 31, 2 * t - 2]           # rows 0 and 1 cross tiles
    n = lens(start)
    mfma(q, k, v, n)                         # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = mfma(q, k, v, n)
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
        DO.check(out, lse, DO.decode_ref(q, k, v, n), f"replay {step}")


def test_impl_mfma_errors():
    q, k, v, _, _ = DO.make_inputs(2, 4, 2, 40, 64, device=dev())
    n = lens([3, 40])
    with pytest.raises(RuntimeError, match="not bf16"):
        mfma(q.float(), k.float(), v.float(), n)
    q32, k32, v32, _, _ = DO.make_inputs(2, 4, 2, 40, 32, device=dev())
    with pytest.raises(RuntimeError, match="head dim 32"):
        mfma(q32, k32, v32, n)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        mfma(q, k, v, n.cpu())


def test_llama_generator_mfma_vs_torch():
    """Teacher-forced as test_llama_generator_hip_vs_torch, same tolerance."""
    from hetu_amd.engine.generator import LlamaGenerator, LlamaKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=16, n_kv_head=2, hidden=1024,
                      ffn_hidden=256, vocab=301, max_seq=64)
    state = DO.llama_state(cfg, 256)
    gm, gt = [LlamaGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                             decode_impl=impl) for impl in ("mfma", "torch")]
    caches = {id(g): LlamaKVCache(cfg, 2, 16, dev(), torch.bfloat16)
              for g in (gm, gt)}
    ids = torch.randint(0, cfg.vocab, (2, 11),
                        generator=torch.Generator().manual_seed(1)).to(dev())

    def fwd(g, tok, pos):
        c = caches[id(g)]
        c.kv_len.fill_(pos + tok.shape[1])
        return g._forward(tok, c, pos)
    with torch.no_grad():
        for g in (gm, gt):
            fwd(g, ids[:, :5], 0)
        for pos in range(5, 11):
            lm = fwd(gm, ids[:, pos:pos + 1], pos).float().cpu()
            lt = fwd(gt, ids[:, pos:pos + 1], pos).float().cpu()
            assert torch.isfinite(lm).all()
            assert torch.allclose(lm, lt, rtol=6e-2, atol=6e-2), \
                f"step {pos}: max abs err {(lm - lt).abs().max().item()}"
