"""F.linear_dgrad on CPU: exactly torch.matmul(gy, w) for every impl that
may run there, and the graph's input gradient routes through it."""
import pytest
import torch

import hetu_amd.ops.functional as F


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("impl", [None, "auto", "blas"])
def test_2d_equals_matmul(dtype, impl):
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(96, 40, generator=g).to(dtype)
    w = torch.randn(40, 24, generator=g).to(dtype)
    out = F.linear_dgrad(gy, w, impl=impl)
    assert out.shape == (96, 24)
    assert torch.equal(out, torch.matmul(gy, w))


@pytest.mark.parametrize("impl", [None, "auto", "blas"])
def test_3d_equals_matmul(impl):
    g = torch.Generator().manual_seed(4)
    gy = torch.randn(4, 16, 40, generator=g)
    w = torch.randn(40, 24, generator=g)
    out = F.linear_dgrad(gy, w, impl=impl)
    assert out.shape == (4, 16, 24)
    assert torch.equal(out, torch.matmul(gy, w))
    assert torch.equal(out.reshape(64, 24),
                       F.linear_dgrad(gy.reshape(64, 40), w, impl=impl))


def test_cpu_never_takes_the_transposed_route(monkeypatch):
    # even for a shape the rule accepts, auto on CPU is the library, and
    # the forced route is an error, never a fallback
    monkeypatch.setattr(F, "_dgrad_auto_transposed", lambda T, N, K: True)
    gy = torch.randn(8, 256).to(torch.bfloat16)
    w = torch.randn(256, 256).to(torch.bfloat16)
    assert torch.equal(F.linear_dgrad(gy, w, impl="auto"),
                       torch.matmul(gy, w))
    with pytest.raises(RuntimeError):
        F.linear_dgrad(gy, w, impl="transposed")


def test_unknown_impl_rejected():
    with pytest.raises(ValueError):
        F.linear_dgrad(torch.zeros(4, 4), torch.zeros(4, 4), impl="fast")


def test_graph_input_gradient_goes_through_dispatch(monkeypatch):
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
    from hetu_amd.graph.ops import api as ht
    calls = []
    real = F.linear_dgrad

    def spy(gy, w, impl=None):
        calls.append((tuple(gy.shape), tuple(w.shape)))
        return real(gy, w, impl)
    monkeypatch.setattr(F, "linear_dgrad", spy)
    torch.manual_seed(5)
    wv, bv = torch.randn(6, 8), torch.randn(6)
    xv, cv = torch.randn(2, 5, 8), torch.randn(2, 5, 6)
    g = DefineAndRunGraph("dgrad_cpu")
    push_graph(g)
    try:
        x = ht.placeholder((2, 5, 8), name="x")
        c = ht.placeholder((2, 5, 6), name="c")
        w = ht.variable(wv.clone(), name="w")
        b = ht.variable(bv.clone(), name="b")
        loss = ht.reduce_sum(ht.mul(ht.linear(x, w, b), c))
        (gx,) = ht.gradients(loss, [x])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    out = g.run([gx], {x: xv, c: cv}, ctx=ctx)[0]
    assert calls == [((2, 5, 6), (6, 8))]
    assert torch.equal(out, torch.matmul(cv, wv))


@pytest.mark.parametrize("T,N,K,want", [
    # measured winners (scripts/bench_dgrad.py): (N -> K) at T tokens
    (32768, 12288, 4096, True), (32768, 4096, 4096, True),
    (32768, 16384, 4096, True), (32768, 4096, 16384, True),
    (16384, 12288, 4096, True), (8192, 16384, 4096, True),
    (8192, 4096, 4096, True), (32768, 50304, 4096, True),
    # near misses
    (8191, 4096, 4096, False),       # below the measured token range
    (4096, 16384, 4096, False),      # measured: ranges overlap
    (2048, 4096, 16384, False),      # measured: the library wins
    (32768, 4096, 2048, False),      # weight smaller than any measured
    (32768, 2048, 4096, False),
    (32768, 4097, 4096, False),      # no 16-byte transpose path
    (32768, 4096, 4100, False),
])
def test_auto_rule(T, N, K, want):
    assert F._dgrad_auto_transposed(T, N, K) is want
