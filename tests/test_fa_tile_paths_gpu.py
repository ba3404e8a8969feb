"""The two tile paths of the 8-wave flash-attention forward and dq kernels:
the masked body on boundary tiles and the mask-free body on interior tiles
(the dkv kernel masks every tile and runs in every backward case here).

Every case is checked twice: against the fp32 reference with the project's
attention tolerances (test_gpu_kernels.py: 3e-2 for o, 1e-2 for lse, 5e-2
for the gradients, 6e-2 for the fused dqkv), and bit for bit against a run
under HETU_AMD_FA_MASK_ALL=1, which sends every tile through the masked
body.  Under GQA dk / dv are accumulated with fp32 atomics, so only the
reference check applies to them.

The dkv kernel has a single path today (a split was measured no faster), so
the switch comparison of dk / dv compares that kernel with itself and can
only fail on its inputs (lse, o); it is kept for the day the kernel gets a
second path.

Shapes are the smallest that reach every path: a single tile (the duplicate
prologue issue), one full 256-row block in which each wave has a different
boundary tile, ragged row and key tails over several blocks with a non-zero
first q tile, Skv > S (diag > 0), GQA, the fused-qkv strides and the packed
varlen segments of test_varlen_bwd_gpu.py.  Every entry is called on the
extension itself, so no case can pass through a torch branch.

What these tests cannot see is a boundary predicate that is too wide: a
tile sent through the masked body without need computes the same bits, and
only the benchmark shows it.
"""
import functools
import math
import os

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)
SWITCH = "HETU_AMD_FA_MASK_ALL"
TOL_O, TOL_LSE, TOL_GRAD, TOL_DQKV = 3e-2, 1e-2, 5e-2, 6e-2

# (S, Skv, H, Hkv)
DENSE = [
    (64, 64, 2, 2),
    (256, 256, 2, 2),
    (257, 257, 2, 2),
    (513, 513, 2, 2),
    (320, 320, 2, 2),
    (192, 448, 2, 2),
    (320, 320, 4, 2),
]
LENS = [1, 31, 32, 33, 63, 64, 65, 0, 255, 256, 257, 513, 300]
TAIL = 50


def dev():
    return torch.device("cuda", 0)


def _masked_everywhere(fn):
    """fn() with the switch set; the launchers read it at every launch."""
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = "1"
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


def _close(a, b, tol, what):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    err = (a - b).abs().max().item()
    print(f"{what}: max abs diff {err:.3e} (ref max {b.abs().max().item():.3e})")
    assert torch.allclose(a, b, rtol=tol, atol=tol), f"{what}: max abs err {err}"


def _same(a, b, what):
    assert torch.equal(a, b), (
        f"{what}: default and {SWITCH}=1 differ in "
        f"{(a != b).sum().item()} elements")


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev())


# ---- dense entries ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense(S, Skv, H, Hkv, causal):
    """Inputs, reference and both runs of one dense case (shared, read-only)."""
    assert SWITCH not in os.environ
    g = torch.Generator().manual_seed(S * 7 + Skv + H)
    q, do = _randn(g, 1, H, S, D), _randn(g, 1, H, S, D)
    k, v = _randn(g, 1, Hkv, Skv, D), _randn(g, 1, Hkv, Skv, D)
    e = F.ext()

    def run():
        o, lse = e.flash_attn_fwd(q, k, v, causal, SCALE, 2)
        return (o, lse) + tuple(
            e.flash_attn_bwd(do, q, k, v, o, lse, causal, SCALE, 2))

    got = run()
    again = run()
    masked = _masked_everywhere(run)
    c = [t.cpu().float() for t in (q, k, v, do)]
    orf, lser = F._attn_ref_fwd(c[0], c[1], c[2], causal, SCALE)
    ref = (orf, lser) + tuple(
        F._attn_ref_bwd(c[3], c[0], c[1], c[2], orf, lser, causal, SCALE))
    return dict(q=q, k=k, v=v, do=do, got=got, again=again, masked=masked,
                ref=ref)


NAMES = ("o", "lse", "dq", "dk", "dv")
TOLS = (TOL_O, TOL_LSE, TOL_GRAD, TOL_GRAD, TOL_GRAD)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,Skv,H,Hkv", DENSE)
def test_dense_reference(S, Skv, H, Hkv, causal):
    c = _dense(S, Skv, H, Hkv, causal)
    for name, tol, a, b in zip(NAMES, TOLS, c["got"], c["ref"]):
        _close(a, b, tol, f"dense {S}x{Skv} H={H}/{Hkv} causal={causal} {name}")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,Skv,H,Hkv", DENSE)
def test_dense_switch(S, Skv, H, Hkv, causal):
    c = _dense(S, Skv, H, Hkv, causal)
    names = NAMES if H == Hkv else NAMES[:3]
    for name, a, b in zip(names, c["got"], c["masked"]):
        _same(a, b, f"dense {S}x{Skv} H={H}/{Hkv} causal={causal} {name}")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,Skv,H,Hkv", [c for c in DENSE if c[2] == c[3]])
def test_dense_repeatable(S, Skv, H, Hkv, causal):
    """Two default runs: a race on the Q / dO staging would show as a
    difference."""
    c = _dense(S, Skv, H, Hkv, causal)
    for name, a, b in zip(NAMES, c["got"], c["again"]):
        assert torch.equal(a, b), f"{name}: two default runs differ"


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", [256, 513])
def test_v3_bit_equal_v2(S, causal):
    c = _dense(S, S, 2, 2, causal)
    o, lse = c["got"][:2]
    g3 = F.ext().flash_attn_bwd(c["do"], c["q"], c["k"], c["v"], o, lse,
                                causal, SCALE, 3)
    for name, a, b in zip(NAMES[2:], g3, c["got"][2:]):
        assert torch.equal(a, b), f"{name}: impl=3 differs from impl=2"


# ---- fused-qkv entries -----------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)])
def test_fused_qkv(H, Hkv, causal):
    B, S = 2, 320
    g = torch.Generator().manual_seed(11 + H)
    qkv = _randn(g, B, S, (H + 2 * Hkv) * D)
    do = _randn(g, B, S, H * D)
    e = F.ext()

    def run():
        o, lse = e.flash_attn_fwd_qkv(qkv, H, Hkv, D, causal, SCALE)
        return o, lse, e.flash_attn_bwd_qkv(do, qkv, o, lse, H, Hkv, D,
                                            causal, SCALE)

    got = run()
    masked = _masked_everywhere(run)
    qkv_c = qkv.cpu().float()
    orf, lser = F.fused_qkv_attention_fwd(qkv_c, H, Hkv, D, None, None,
                                          causal, None)
    dref = F.fused_qkv_attention_bwd(do.cpu().float(), qkv_c, orf, lser, H,
                                     Hkv, D, None, None, causal, None)
    what = f"fused H={H}/{Hkv} causal={causal}"
    _close(got[0], orf, TOL_O, what + " o")
    _close(got[1], lser, TOL_LSE, what + " lse")
    _close(got[2], dref, TOL_DQKV, what + " dqkv")
    _same(got[0], masked[0], what + " o")
    _same(got[1], masked[1], what + " lse")
    if H == Hkv:
        _same(got[2], masked[2], what + " dqkv")
    else:       # dk / dv sections come from fp32 atomics
        _same(got[2][..., :H * D], masked[2][..., :H * D], what + " dq")


# ---- packed varlen ---------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_varlen(causal):
    H = 2
    g = torch.Generator().manual_seed(5)
    T = sum(LENS) + TAIL
    q, k, v, do = (_randn(g, T, H, D) for _ in range(4))
    cu_h = torch.zeros(len(LENS) + 1, dtype=torch.int32)
    cu_h[1:] = torch.tensor(LENS, dtype=torch.int32).cumsum(0)
    cu = cu_h.to(dev())
    n = int(cu_h[-1])

    e = F.ext()
    max_len = max(LENS)

    def run():
        o, lse = e.flash_attn_varlen_fwd(q, k, v, cu, max_len, causal, SCALE)
        return (o, lse) + tuple(e.flash_attn_varlen_bwd(
            do, q, k, v, o, lse, cu, max_len, causal, SCALE))

    got = run()
    again = run()
    masked = _masked_everywhere(run)

    c = [t.cpu().float() for t in (q, k, v, do)]
    ref = [torch.zeros(T, H, D), torch.zeros(H, T)] + \
          [torch.zeros(T, H, D) for _ in range(3)]
    b = cu_h.tolist()
    for s0, s1 in zip(b[:-1], b[1:]):
        if s1 <= s0:
            continue
        qs, ks, vs, ds = (t[s0:s1].permute(1, 0, 2).unsqueeze(0) for t in c)
        o_s, lse_s = F._attn_ref_fwd(qs, ks, vs, causal, SCALE)
        grads = F._attn_ref_bwd(ds, qs, ks, vs, o_s, lse_s, causal, SCALE)
        ref[0][s0:s1] = o_s[0].permute(1, 0, 2)
        ref[1][:, s0:s1] = lse_s[0]
        for dst, src in zip(ref[2:], grads):
            dst[s0:s1] = src[0].permute(1, 0, 2)

    what = f"varlen causal={causal}"
    # o / lse rows past the last segment are not written
    _close(got[0][:n], ref[0][:n], TOL_O, what + " o")
    _close(got[1][:, :n], ref[1][:, :n], TOL_LSE, what + " lse")
    _same(got[0][:n], masked[0][:n], what + " o")
    _same(got[1][:, :n], masked[1][:, :n], what + " lse")
    for name, a, r, m, a2 in zip(NAMES[2:], got[2:], ref[2:], masked[2:],
                                 again[2:]):
        _close(a, r, TOL_GRAD, f"{what} {name}")
        _same(a, m, f"{what} {name}")
        assert torch.equal(a, a2), f"{what} {name}: two default runs differ"
