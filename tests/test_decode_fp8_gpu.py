"""GPU tests of the fp8 KV cache: F.kv_cache_append_fp8
(hetu_amd/ops/hip/kv_cache_fp8.hip) and F.flash_attn_decode over e4m3 caches
with per-row scales (hetu_amd/ops/hip/attention_decode_fp8.hip).

Decode reference and bounds are tests/decode_attn_oracle.py's, on the
dequantized values (exact in fp64): the conversion to bf16 is exact and the
scales enter in fp32, so the three budgeted roundings are the same.  Caches
are [3, Hkv, 2 T + 44, D], T = decode_attn_fp8_tile().
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import decode_fp8_cases as C  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

HEADS = [(4, 4), (16, 2), (20, 4), (32, 1), (40, 1)]
B = 3


def dev():
    return torch.device("cuda", 0)


def T():
    return int(F.ext().decode_attn_fp8_tile())


def cache_len():
    return 2 * T() + 44


def length_sets():
    t, L = T(), cache_len()
    return [[0, 1, 15], [16, 17, 31], [32, 33, t - 1], [t, t + 1, L - 1],
            [L, 0, t]]


def lens(ls):
    return torch.tensor(ls, dtype=torch.int32, device=dev())


def ref_of(q, k, ks, v, vs, n, scale=None):
    return DO.decode_ref(q, C.dequant(k, ks), C.dequant(v, vs), n, scale)


def dec(q, k, ks, v, vs, n, ns=0, scale=None, impl="hip"):
    return F.flash_attn_decode(q, k, v, n, scale, num_splits=ns, impl=impl,
                               k_scale=ks, v_scale=vs)


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv):
    """CPU inputs and one oracle result per length set; never modified."""
    ins = C.make_fp8_inputs(B, H, Hkv, cache_len(), D, seed=D + 7 * H + Hkv)
    return ins, [ref_of(*ins, torch.tensor(ls)) for ls in length_sets()]


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("D", [64, 128])
def test_append_against_the_definition(D, S):
    """Rows at 0, before 0 (dropped), across a tile edge, at L - 1 and past
    L (dropped: the cache bytes there are unchanged)."""
    t, L, H, Hkv = T(), cache_len(), 4, 2
    for i, end in enumerate(([S, t + 2, L], [L + 3, 2, t + 2])):
        kd, vd = C.append_inputs(B, S, H, Hkv, D, D + S + i, dev())
        kc = torch.full((B, Hkv, L, D), 0x55, dtype=torch.uint8,
                        device=dev()).view(C.FP8)
        vc = kc.clone()
        ks = torch.full((B, Hkv, L), 7.0, device=dev())
        vs = ks.clone()
        before = (kc.clone(), ks.clone())
        F.kv_cache_append_fp8(kd, vd, kc, vc, ks, vs, lens(end), impl="hip")
        C.check_append(kd, kc, ks, before, end, f"K D{D} S{S} end{end}")
        C.check_append(vd, vc, vs, before, end, f"V D{D} S{S} end{end}")


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
def test_every_code_in_every_byte_lane(D, ns):
    """One attended V row per (b, hkv), together all 254 finite e4m3 codes,
    v_scale = 1, P = 1: out is the row exactly (e4m3 is exact in bf16; -0
    comes back as +0, the sum 0 + 1 * -0).  Then the row at T + 3 with a K
    row that takes all the weight, within the oracle's bound."""
    t, L, H, Hkv = T(), cache_len(), 4, 2
    q, k, ks, v, vs = C.make_fp8_inputs(B, H, Hkv, L, D, seed=5)
    finite = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                          dtype=torch.uint8)
    rows = finite.repeat(B * Hkv * D // 254 + 1)[:B * Hkv * D] \
        .view(B, Hkv, D).view(C.FP8)
    G, scale = H // Hkv, 1.0 / math.sqrt(D)
    for j in (0, t + 3):
        k2, ks2, v2, vs2 = k.clone(), ks.clone(), v.clone(), vs.clone()
        v2[:, :, j] = rows
        vs2[:, :, j] = 1.0
        for b in range(B):                   # a +25 score for the group's
            for hk in range(Hkv):            # first head, as the rescale test
                qg = q[b, hk * G].float()
                x = qg * (25.0 / scale / qg.dot(qg))
                ks2[b, hk, j] = x.abs().max() / 448
                k2[b, hk, j] = (x / ks2[b, hk, j]).to(C.FP8)
        n = torch.full((B,), j + 1, dtype=torch.int32)
        out, lse = dec(*(x.to(dev()) for x in (q, k2, ks2, v2, vs2, n)), ns)
        if j == 0:
            want = rows.float().repeat_interleave(G, dim=1)
            assert torch.equal(out.float().cpu(), want)
        DO.check(out, lse, ref_of(q, k2, ks2, v2, vs2, n), f"codes row {j}")


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
def test_accuracy_vs_oracle(D, H, Hkv, ns):
    ins, refs = case(D, H, Hkv)
    ind = [x.to(dev()) for x in ins]
    for ls, ref in zip(length_sets(), refs):
        out, lse = dec(*ind, lens(ls), ns)
        assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32
        worst = DO.check(out, lse, ref, f"D{D} H{H}/{Hkv} ns{ns} {ls}")
        print(f"D{D} H{H}/{Hkv} ns{ns} kv_len{ls}: "
              f"worst out err {worst:.3e} x vmax (bound {DO.OUT_BOUND:.3e})")


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("H,Hkv", [(16, 2), (32, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_poison_past_kv_len(D, H, Hkv, ns):
    """Bytes 0x7F (NaN) and NaN scales in every row at index >= kv_len[b],
    inside the [.., L, ..] views and in the allocation beyond them."""
    t, L = T(), cache_len()
    q, kb, ksb, vb, vsb = [x.to(dev()) for x in C.make_fp8_inputs(
        B, H, Hkv, L, D, seed=3, alloc=L + 20)]
    for ls in ([0, 17, t], [t - 1, t + 1, L - 1], [33, 2 * t, L + 5]):
        n = lens(ls)
        ref = ref_of(q, kb[:, :, :L], ksb[:, :, :L], vb[:, :, :L],
                     vsb[:, :, :L], n)           # from the clean values
        pk, pks, pv, pvs = kb.clone(), ksb.clone(), vb.clone(), vsb.clone()
        for b, m in enumerate(ls):
            pk.view(torch.uint8)[b, :, m:] = 0x7F
            pv.view(torch.uint8)[b, :, m:] = 0x7F
            pks[b, :, m:] = float("nan")
            pvs[b, :, m:] = float("nan")
        args = (q, pk[:, :, :L], pks[:, :, :L], pv[:, :, :L], pvs[:, :, :L])
        out, lse = dec(*args, n, ns)
        DO.check(out, lse, ref, f"poison {ls} ns{ns}")
        if ls[-1] == L + 5:                      # clamped: same as L
            o2, l2 = dec(*args, lens(ls[:-1] + [L]), ns)
            assert torch.equal(out, o2) and torch.equal(lse, l2)


@pytest.mark.parametrize("H,Hkv,D", [(16, 2, 128), (32, 1, 64)])
def test_strided_views_and_repeats_are_bit_equal(H, Hkv, D):
    """Layer slices of 5-D caches and scales, q a view into a fused qkv
    row, against contiguous copies; the contiguous call twice."""
    L = cache_len()
    _, k, ks, v, vs = [x.to(dev()) for x in C.make_fp8_inputs(
        2 * B, H, Hkv, L, D, seed=4)]
    k, ks, v, vs = [x.view(2, B, *x.shape[1:]) for x in (k, ks, v, vs)]
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D,
                      generator=torch.Generator().manual_seed(4)) \
        .bfloat16().to(dev())
    q = qkv[..., :H * D].view(B, 1, H, D)[:, 0]
    assert not q.is_contiguous()
    n = lens([17, T() + 1, L])
    for ns in (0, 1, 3):
        out, lse = dec(q, k[1], ks[1], v[1], vs[1], n, ns)
        args = (q.contiguous(), k[1].clone(), ks[1].clone(), v[1].clone(),
                vs[1].clone(), n, ns)
        for _ in range(2):
            oc, lc = dec(*args)
            assert torch.equal(out, oc) and torch.equal(lse, lc)
    DO.check(out, lse, ref_of(q, k[1], ks[1], v[1], vs[1], n), "strided")


def test_graph_capture_of_append_and_decode():
    """One graph: append, then attention.  Between replays new rows go into
    the captured k_new / v_new buffers and kv_len advances in place, across
    a tile edge; each replay against the oracle on the dequantized cache."""
    t, L = T(), cache_len()
    H, Hkv, D = 16, 2, 128
    q, k, ks, v, vs = [x.to(dev()) for x in C.make_fp8_inputs(
        B, H, Hkv, L, D, seed=21)]
    n = lens([t - 2, 30, 2 * t - 3])             # rows 0 and 2 cross tiles
    gen = torch.Generator().manual_seed(22)
    kn = torch.zeros(B, 1, Hkv, D, dtype=torch.bfloat16, device=dev())
    vn = torch.zeros_like(kn)

    def step():
        F.kv_cache_append_fp8(kn, vn, k, v, ks, vs, n, impl="hip")
        return dec(q, k, ks, v, vs, n)
    n.add_(1)
    step()                                       # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = step()
    for i in range(3):
        kn.copy_(torch.randn(B, 1, Hkv, D, generator=gen).bfloat16())
        vn.copy_(torch.randn(B, 1, Hkv, D, generator=gen).bfloat16())
        n.add_(1)
        g.replay()
        torch.cuda.synchronize()
        DO.check(out, lse, ref_of(q, k, ks, v, vs, n), f"replay {i}")
        b, r = 0, int(n[0]) - 1                  # the row went where n says
        assert torch.equal(ks[b, :, r].cpu(),
                           kn[b, 0].float().abs().amax(-1).cpu()
                           / torch.full((Hkv,), 448.0))


def test_errors_name_the_argument():
    q, k, ks, v, vs = [x.to(dev()) for x in C.make_fp8_inputs(2, 4, 2, 40, 64)]
    n = lens([3, 40])
    bf = k.float().bfloat16()
    with pytest.raises(RuntimeError, match="needs k_scale"):
        F.flash_attn_decode(q, k, v, n, impl="hip")
    with pytest.raises(RuntimeError, match="v_scale given with a"):
        F.flash_attn_decode(q, bf, bf, n, impl="hip", v_scale=vs)
    with pytest.raises(RuntimeError, match=r"k_cache is uint8.*\.view"):
        dec(q, k.view(torch.uint8), ks, v.view(torch.uint8), vs, n)
    with pytest.raises(RuntimeError, match="k_scale has shape"):
        dec(q, k, ks[:, :, :39], v, vs, n)
    with pytest.raises(RuntimeError, match="v_scale is torch.float64"):
        dec(q, k, ks, v, vs.double(), n)
    with pytest.raises(RuntimeError, match="kv_len is a CPU tensor"):
        dec(q, k, ks, v, vs, n.cpu())


def test_llama_generator_fp8_hip_vs_torch():
    """Teacher-forced as test_llama_generator_mfma_vs_torch, same config,
    steps and tolerance, both sides on fp8 caches: they see the same
    quantized rows up to the append's rounding.

    The kernel carries P as three bf16 parts, so its P.V is an fp32
    product like the torch branch's; with a single bf16 rounding of P the
    two sides quantized different second-layer rows and this tolerance was
    missed by up to 0.033 (profiles/r10_decode_fp8.md section 5)."""
    from hetu_amd.engine.generator import LlamaGenerator, LlamaKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=16, n_kv_head=2, hidden=1024,
                      ffn_hidden=256, vocab=301, max_seq=64)
    state = DO.llama_state(cfg, 256)
    gh, gt = [LlamaGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                             decode_impl=impl, kv_dtype="fp8")
              for impl in (None, "torch")]
    caches = {id(g): LlamaKVCache(cfg, 2, 16, dev(), torch.bfloat16,
                                  kv_dtype="fp8") for g in (gh, gt)}
    ids = torch.randint(0, cfg.vocab, (2, 11),
                        generator=torch.Generator().manual_seed(1)).to(dev())

    def fwd(g, tok, pos):
        c = caches[id(g)]
        c.kv_len.fill_(pos + tok.shape[1])
        return g._forward(tok, c, pos)
    with torch.no_grad():
        for g in (gh, gt):
            fwd(g, ids[:, :5], 0)
        for pos in range(5, 11):
            lh = fwd(gh, ids[:, pos:pos + 1], pos).float().cpu()
            lt = fwd(gt, ids[:, pos:pos + 1], pos).float().cpu()
            assert torch.isfinite(lh).all()
            assert torch.allclose(lh, lt, rtol=6e-2, atol=6e-2), \
                f"step {pos}: max abs err {(lh - lt).abs().max().item()}"
    assert caches[id(gh)].k.dtype == C.FP8
