"""F.linear_dgrad(impl="transposed") on the GPU: dx = gy @ w computed as
F.linear(gy, transpose2d(w)).

Shapes: (64, 40, 24) one partial tile of the transpose's 16-byte path,
(192, 320, 136) several tiles with ragged edges, (130, 257, 129) the
element path (odd N and K), (256, 512, 256) whole tiles, and a 3-D gy.

Bound (from the number formats, not from the kernels): the transpose is
exact, and both GEMM forms accumulate in fp32 and round to bf16 once, so
against the fp64 reference the transposed route's max error is at most
1.5x the library NN path's on the same inputs; the margin covers a
different summation order.
"""
import functools

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(64, 40, 24), (192, 320, 136), (130, 257, 129), (256, 512, 256)]


def dev():
    return torch.device("cuda", 0)


def _rand(R, C, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, C, generator=g).to(dtype).to(dev())


@functools.lru_cache(maxsize=None)
def _case(T, N, K):
    """inputs, fp64 reference and library result, computed once per shape"""
    gy, w = _rand(T, N, 100 + T + N), _rand(N, K, 200 + N + K)
    ref = gy.double() @ w.double()
    blas = F.linear_dgrad(gy, w, impl="blas")
    return gy, w, ref, blas


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_matches_reference(T, N, K):
    gy, w, ref, blas = _case(T, N, K)
    out = F.linear_dgrad(gy, w, impl="transposed")
    assert out.shape == (T, K) and out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()
    e_tr = (out.double() - ref).abs().max().item()
    e_blas = (blas.double() - ref).abs().max().item()
    print(f"T={T} N={N} K={K}: max err transposed {e_tr:.4g} "
          f"blas {e_blas:.4g}")
    assert e_tr <= 1.5 * e_blas


def test_3d_gy():
    gy, w, ref, blas = _case(192, 320, 136)
    gy3 = gy.reshape(3, 64, 320)
    out = F.linear_dgrad(gy3, w, impl="transposed")
    assert out.shape == (3, 64, 136)
    e_tr = (out.reshape(192, 136).double() - ref).abs().max().item()
    e_blas = (blas.double() - ref).abs().max().item()
    print(f"3-D gy: max err transposed {e_tr:.4g} blas {e_blas:.4g}")
    assert e_tr <= 1.5 * e_blas
    assert torch.equal(out.reshape(192, 136),
                       F.linear_dgrad(gy, w, impl="transposed"))


@pytest.mark.parametrize("T,N,K", [(192, 320, 136), (130, 257, 129)])
def test_two_calls_bit_equal(T, N, K):
    gy, w, _, _ = _case(T, N, K)
    assert torch.equal(F.linear_dgrad(gy, w, impl="transposed"),
                       F.linear_dgrad(gy, w, impl="transposed"))


def test_fp16():
    gy = _rand(64, 40, 1, torch.float16)
    w = _rand(40, 24, 2, torch.float16)
    ref = gy.double() @ w.double()
    e_tr = (F.linear_dgrad(gy, w, impl="transposed").double()
            - ref).abs().max().item()
    e_blas = (F.linear_dgrad(gy, w, impl="blas").double()
              - ref).abs().max().item()
    assert e_tr <= 1.5 * e_blas


def test_capture_replay_follows_new_weight():
    """nothing is cached: a captured call re-reads w on every replay"""
    T, N, K = 192, 320, 136
    gy = _rand(T, N, 11)
    w = _rand(N, K, 12).clone()
    w_new = _rand(N, K, 13)
    assert not torch.equal(w, w_new)
    eager_old = F.linear_dgrad(gy, w, impl="transposed").clone()
    eager_new = F.linear_dgrad(gy, w_new, impl="transposed").clone()
    assert not torch.equal(eager_old, eager_new)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.linear_dgrad(gy, w, impl="transposed")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_old)
    w.copy_(w_new)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_new)


def test_ineligible_raises():
    gy = _rand(64, 40, 1)
    with pytest.raises(RuntimeError):
        F.linear_dgrad(gy.float(), _rand(40, 24, 2).float(),
                       impl="transposed")
    with pytest.raises(RuntimeError):          # w's dtype differs from gy's
        F.linear_dgrad(gy, _rand(40, 24, 2).float(), impl="transposed")
    nc = _rand(40, 48, 3)[:, ::2]
    assert not nc.is_contiguous()
    with pytest.raises(RuntimeError):
        F.linear_dgrad(gy, nc, impl="transposed")


def test_linear_layer_graph_transposed_vs_blas(monkeypatch):
    """one biased linear layer: dx through the graph on both routes"""
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
    from hetu_amd.graph.ops import api as ht
    gen = torch.Generator().manual_seed(77)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)
    wv, bv = rnd(320, 136) * 0.05, rnd(320)
    xv, cv = rnd(192, 136).to(dev()), rnd(192, 320).to(dev())
    outs = {}
    for impl in ("transposed", "blas"):
        monkeypatch.setattr(F, "_HETU_DGRAD", impl)
        g = DefineAndRunGraph(f"dgrad_{impl}")
        push_graph(g)
        try:
            x = ht.placeholder((192, 136), dtype=torch.bfloat16, name="x")
            c = ht.placeholder((192, 320), dtype=torch.bfloat16, name="c")
            w = ht.variable(wv.clone(), name="w")
            b = ht.variable(bv.clone(), name="b")
            loss = ht.reduce_sum(ht.mul(ht.linear(x, w, b), c))
            (gx,) = ht.gradients(loss, [x])
        finally:
            pop_graph()
        ctx = prepare_run_context(g, dev(), use_comm=False)
        outs[impl] = g.run([gx], {x: xv, c: cv}, ctx=ctx)[0].clone()
    torch.cuda.synchronize()
    ref = cv.double() @ wv.to(dev()).double()
    e_tr = (outs["transposed"].double() - ref).abs().max().item()
    e_blas = (outs["blas"].double() - ref).abs().max().item()
    assert e_tr <= 1.5 * e_blas
