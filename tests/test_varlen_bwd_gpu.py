"""Single-kernel packed-varlen attention backward (flash_attn_varlen_bwd)
vs the fp32 reference, the per-segment composition, and under graph capture.

Shapes are the smallest that cross every boundary of the kernels: the
32-row wave / q-tile, the 64-key tile, the 256-row block, a multi-block
segment with a non-zero causal t_start, an empty segment and a length-1
segment, plus a tail of rows that belong to no segment.
"""
import functools
import math

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

D = 128
TOL = 5e-2          # the project's FA-backward tolerance (test_gpu_kernels)
LENS = [1, 31, 32, 33, 63, 64, 65, 0, 255, 256, 257, 513, 300]   # sum 1870
TAIL = 50
GQA_LENS = [65, 0, 257, 40]                                       # sum 362


def dev():
    return torch.device("cuda", 0)


def _require_binding():
    assert hasattr(F.ext(), "flash_attn_varlen_bwd"), \
        "extension has no flash_attn_varlen_bwd"


def _cu(lens):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    return cu


def _inputs(lens, tail, H, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    T = sum(lens) + tail

    def rnd(h):
        return torch.randn(T, h, D, generator=g).to(torch.bfloat16).to(dev())
    return dict(T=T, H=H, Hkv=Hkv, cu=_cu(lens), q=rnd(H), k=rnd(Hkv),
                v=rnd(Hkv), do=rnd(H))


def _run(x, causal, max_seqlen=None):
    """fwd + bwd through the public functional entry points."""
    cu = x["cu"].to(dev())
    o, lse = F.varlen_attention_fwd(x["q"], x["k"], x["v"], cu, causal,
                                    None, max_seqlen)
    dq, dk, dv = F.varlen_attention_bwd(x["do"], x["q"], x["k"], x["v"], o,
                                        lse, cu, causal, None, max_seqlen)
    return o, lse, dq, dk, dv


def _ref_bwd(x, o, lse, causal):
    """Per-segment F._attn_ref_bwd on CPU fp32; uncovered rows stay 0."""
    scale = 1.0 / math.sqrt(D)
    c = {n: x[n].cpu().float() for n in ("q", "k", "v", "do")}
    o, lse = o.cpu().float(), lse.cpu().float()
    dq = torch.zeros_like(c["q"])
    dk = torch.zeros_like(c["k"])
    dv = torch.zeros_like(c["v"])
    cu = x["cu"].tolist()
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        a = [t[s0:s1].permute(1, 0, 2).unsqueeze(0)
             for t in (c["do"], c["q"], c["k"], c["v"], o)]
        r = F._attn_ref_bwd(a[0], a[1], a[2], a[3], a[4],
                            lse[:, s0:s1].unsqueeze(0), causal, scale)
        dq[s0:s1] = r[0][0].permute(1, 0, 2)
        dk[s0:s1] = r[1][0].permute(1, 0, 2)
        dv[s0:s1] = r[2][0].permute(1, 0, 2)
    return dq, dk, dv


@functools.lru_cache(maxsize=None)
def _case(causal):
    """Non-GQA case, computed once per causal flag and shared (read-only)."""
    x = _inputs(LENS, TAIL, 2, 2, seed=0)
    o, lse, dq, dk, dv = _run(x, causal)
    return x, o, lse, (dq, dk, dv)


def _check(got, ref, what):
    for name, a, b in zip(("dq", "dk", "dv"), got, ref):
        a = a.detach().float().cpu()
        b = b.detach().float().cpu()
        assert torch.isfinite(a).all(), f"{what} {name}: non-finite"
        err = (a - b).abs().max().item()
        print(f"{what} {name}: max abs diff {err:.3e} "
              f"(ref max {b.abs().max().item():.3e})")
        assert torch.allclose(a, b, rtol=TOL, atol=TOL), \
            f"{what} {name}: max abs err {err}"


def test_binding_exists():
    _require_binding()


@pytest.mark.parametrize("causal", [True, False])
def test_numerics(causal):
    _require_binding()
    x, o, lse, got = _case(causal)
    assert x["T"] == 1920 and int(x["cu"][-1]) == 1870
    _check(got, _ref_bwd(x, o, lse, causal), f"varlen causal={causal}")
    for name, g in zip(("dq", "dk", "dv"), got):
        assert g.shape[0] == x["T"]
        assert torch.count_nonzero(g[-TAIL:]).item() == 0, \
            f"{name}: rows outside every segment must be exactly zero"


def test_numerics_gqa():
    _require_binding()
    x = _inputs(GQA_LENS, 0, 4, 2, seed=1)
    assert x["T"] == 362
    o, lse, dq, dk, dv = _run(x, True)
    _check((dq, dk, dv), _ref_bwd(x, o, lse, True), "varlen gqa")


@pytest.mark.parametrize("causal", [True, False])
def test_matches_per_segment_composition(causal):
    """The single-kernel path vs the Python loop over the dense
    F.flash_attn_bwd that it replaces."""
    _require_binding()
    x, o, lse, got = _case(causal)
    comp = [torch.zeros_like(x[n]) for n in ("q", "k", "v")]
    cu = x["cu"].tolist()
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        a = [t[s0:s1].permute(1, 0, 2).unsqueeze(0).contiguous()
             for t in (x["do"], x["q"], x["k"], x["v"], o)]
        ls = lse[:, s0:s1].unsqueeze(0).contiguous()
        r = F.flash_attn_bwd(a[0], a[1], a[2], a[3], a[4], ls, causal, None)
        for dst, src in zip(comp, r):
            dst[s0:s1] = src[0].permute(1, 0, 2)
    _check(got, comp, f"single-kernel vs composition causal={causal}")


def test_max_seqlen_hint():
    _require_binding()
    x, o, lse, got = _case(True)
    o2, lse2, dq, dk, dv = _run(x, True, max_seqlen=513)
    n = int(x["cu"][-1])
    assert torch.equal(o2[:n], o[:n]) and torch.equal(lse2[:, :n], lse[:, :n])
    for a, b in zip((dq, dk, dv), got):
        assert torch.equal(a, b)


def test_graph_capture_device_cu():
    """fwd + bwd captured once; cu rewritten in place between replays.
    A host sync inside either entry would fail the capture, and bounds
    read at capture time would make the second replay wrong."""
    _require_binding()
    x = _inputs([362], 0, 2, 2, seed=2)
    splits = ([0, 100, 300, 362, 362], [0, 257, 257, 330, 362])
    cu = torch.tensor(splits[0], dtype=torch.int32, device=dev())

    def step():
        o, lse = F.varlen_attention_fwd(x["q"], x["k"], x["v"], cu, True)
        return F.varlen_attention_bwd(x["do"], x["q"], x["k"], x["v"], o,
                                      lse, cu, True)

    eager = []
    for s in splits:
        cu.copy_(torch.tensor(s, dtype=torch.int32))
        eager.append([t.clone() for t in step()])
    torch.cuda.synchronize()

    cu.copy_(torch.tensor(splits[0], dtype=torch.int32))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for s, ref in zip(splits, eager):
        cu.copy_(torch.tensor(s, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("dq", "dk", "dv"), outs, ref):
            assert torch.isfinite(a.float()).all()
            assert torch.equal(a, b), f"replay cu={s}: {name} differs"
