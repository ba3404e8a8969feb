"""Head dim 64 in the v2 flash-attention kernels: the packed-varlen and the
fused-qkv entries, forward and backward, against the fp32 reference.

Tolerances are the ones the D = 128 tests of the same kernels use
(test_gpu_kernels, test_varlen_bwd_gpu).  The lengths cross every boundary of
the D = 64 geometry: an empty segment, one below a 16-key k-step, the 128-key
tile by one key, the 256-row block, a ragged tail, and rows of no segment.
"""
import math

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

D = 64
SCALE = 1.0 / math.sqrt(D)
LENS = [1, 63, 0, 129, 257, 300]
PAD = 5


def dev():
    return torch.device("cuda", 0)


def _close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs().max().item()
    print(f"{what}: max abs diff {err:.3e}")
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    assert torch.allclose(a, b, rtol=tol, atol=tol), f"{what}: max err {err}"


def _packed(lens, H, Hkv, seed=0, pad=PAD):
    g = torch.Generator().manual_seed(seed)
    T = sum(lens) + pad
    t = [torch.randn(T, h, D, generator=g).to(torch.bfloat16).to(dev())
         for h in (H, Hkv, Hkv, H)]
    cu = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).int()
    return t, cu


def _varlen(q, k, v, do, cu, causal, max_seqlen):
    e = F.ext()
    o, lse = e.flash_attn_varlen_fwd(q, k, v, cu.to(dev()), max_seqlen,
                                     causal, SCALE)
    dq, dk, dv = e.flash_attn_varlen_bwd(do, q, k, v, o, lse, cu.to(dev()),
                                         max_seqlen, causal, SCALE)
    return o, lse, dq, dk, dv


def _varlen_ref(H, Hkv, causal):
    """Per-segment fp32 reference on CPU."""
    (q, k, v, do), cu = _packed(LENS, H, Hkv)
    c = [t.cpu().float() for t in (q, k, v, do)]
    n = int(cu[-1])
    o = torch.zeros_like(c[0])
    lse = torch.zeros(H, c[0].shape[0])
    dq, dk, dv = (torch.zeros_like(t) for t in c[:3])
    for s0, s1 in zip(cu[:-1].tolist(), cu[1:].tolist()):
        if s1 <= s0:
            continue
        qs, ks, vs, ds = (t[s0:s1].permute(1, 0, 2).unsqueeze(0) for t in c)
        os_, ls = F._attn_ref_fwd(qs, ks, vs, causal, SCALE)
        r = F._attn_ref_bwd(ds, qs, ks, vs, os_, ls, causal, SCALE)
        o[s0:s1], lse[:, s0:s1] = os_[0].permute(1, 0, 2), ls[0]
        for dst, src in zip((dq, dk, dv), r):
            dst[s0:s1] = src[0].permute(1, 0, 2)
    return n, o, lse, dq, dk, dv


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)])
def test_varlen_fwd_bwd(H, Hkv, causal):
    (q, k, v, do), cu = _packed(LENS, H, Hkv)
    # the hint for one case, the default (T) for the others
    hint = 300 if (H, causal) == (2, True) else q.shape[0]
    o, lse, dq, dk, dv = _varlen(q, k, v, do, cu, causal, hint)
    n, o_r, lse_r, dq_r, dk_r, dv_r = _varlen_ref(H, Hkv, causal)
    _close(o[:n], o_r[:n], 3e-2, "out")
    _close(lse[:, :n], lse_r[:, :n], 1e-2, "lse")
    for name, a, b in (("dq", dq, dq_r), ("dk", dk, dk_r), ("dv", dv, dv_r)):
        _close(a, b, 5e-2, name)
        assert torch.count_nonzero(a[n:]).item() == 0, \
            f"{name}: rows of no segment must be zero"


@pytest.mark.parametrize("rope", [True, False])
def test_fused_qkv_fwd_bwd(rope):
    B, S, H, Hkv = 2, 300, 4, 2
    torch.manual_seed(0)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, dtype=torch.bfloat16,
                      device=dev())
    cos = sin = cc = ss = None
    if rope:
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
        fr = torch.outer(torch.arange(S, dtype=torch.float32), inv)
        cc, ss = fr.cos(), fr.sin()
        cos, sin = cc.to(dev()), ss.to(dev())
    qkv_cpu = qkv.cpu().float()
    o, lse = F.fused_qkv_attention_fwd(qkv, H, Hkv, D, cos, sin, True, None)
    o_r, lse_r = F.fused_qkv_attention_fwd(qkv_cpu, H, Hkv, D, cc, ss, True,
                                           None)
    _close(o, o_r, 3e-2, "fused out")
    _close(lse, lse_r, 1e-2, "fused lse")
    do = torch.randn_like(o)
    dqkv = F.fused_qkv_attention_bwd(do, qkv, o, lse, H, Hkv, D, cos, sin,
                                     True, None)
    d_r = F.fused_qkv_attention_bwd(do.cpu().float(), qkv_cpu, o_r, lse_r, H,
                                    Hkv, D, cc, ss, True, None)
    _close(dqkv, d_r, 6e-2, "fused dqkv")


def test_spiked_key_forces_rescale():
    """A key late in a 300-key segment outscores the running max of the last
    row, in its second 128-key tile: the O rescale and dq must follow."""
    (q, k, v, do), cu = _packed([300], 2, 2, seed=1, pad=0)
    k[200] = (q[299] * 4).to(torch.bfloat16)
    o, lse, dq, _, _ = _varlen(q, k, v, do, cu, True, 300)
    c = [t.cpu().float().permute(1, 0, 2).unsqueeze(0) for t in (q, k, v, do)]
    o_r, lse_r = F._attn_ref_fwd(c[0], c[1], c[2], True, SCALE)
    dq_r = F._attn_ref_bwd(c[3], c[0], c[1], c[2], o_r, lse_r, True, SCALE)[0]
    _close(o, o_r[0].permute(1, 0, 2), 3e-2, "spike out")
    _close(dq, dq_r[0].permute(1, 0, 2), 5e-2, "spike dq")


def test_mask_all_same_bits(monkeypatch):
    """The masked softmax / dS stage on every tile gives the bits of the
    interior / boundary split; S = 600 has interior tiles."""
    (q, k, v, do), cu = _packed([600], 2, 2, seed=2, pad=0)
    base = _varlen(q, k, v, do, cu, True, 600)
    monkeypatch.setenv("HETU_AMD_FA_MASK_ALL", "1")
    forced = _varlen(q, k, v, do, cu, True, 600)
    for name, a, b in zip(("out", "lse", "dq"), base[:3], forced[:3]):
        assert torch.equal(a, b), f"{name}: masked stage changes bits"


def test_varlen_and_fused_qkv_same_bits():
    """One segment through the packed entry and the same values through the
    fused-qkv entry: the same kernels, only the strides differ."""
    S, H = 300, 2
    (q, k, v, do), cu = _packed([S], H, H, seed=3, pad=0)
    o, lse, dq, dk, dv = _varlen(q, k, v, do, cu, True, S)
    qkv = torch.cat([q, k, v], dim=1).reshape(1, S, 3 * H * D).contiguous()
    e = F.ext()
    o2, lse2 = e.flash_attn_fwd_qkv(qkv, H, H, D, True, SCALE)
    dqkv = e.flash_attn_bwd_qkv(do.reshape(1, S, H * D), qkv, o2, lse2, H, H,
                                D, True, SCALE)
    assert torch.equal(o2.view(S, H, D), o), "out"
    got = dqkv.view(S, 3 * H, D).split(H, dim=1)
    for name, a, b in zip(("dq", "dk", "dv"), got, (dq, dk, dv)):
        assert torch.equal(a, b), name
