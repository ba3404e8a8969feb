"""F.linear_wgrad on CPU: exactly torch.matmul(gy.t(), x) for every impl
that may run there, and the graph ops route through it."""
import pytest
import torch

import hetu_amd.ops.functional as F


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("impl", [None, "auto", "blas"])
def test_2d_equals_matmul(dtype, impl):
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(96, 40, generator=g).to(dtype)
    x = torch.randn(96, 24, generator=g).to(dtype)
    out = F.linear_wgrad(gy, x, impl=impl)
    assert out.shape == (40, 24)
    assert torch.equal(out, torch.matmul(gy.t(), x))


def test_flattened_3d_equals_matmul():
    g = torch.Generator().manual_seed(4)
    gy = torch.randn(4, 16, 40, generator=g)
    x = torch.randn(4, 16, 24, generator=g)
    want = torch.matmul(gy.reshape(64, 40).t(), x.reshape(64, 24))
    assert torch.equal(F.linear_wgrad(gy, x), want)
    assert torch.equal(F.linear_wgrad(gy, x, impl="blas"), want)


def test_eligible_shape_on_cpu_stays_on_library():
    gy = torch.randn(64, 256).to(torch.bfloat16)
    x = torch.randn(64, 256).to(torch.bfloat16)
    assert torch.equal(F.linear_wgrad(gy, x, impl="auto"),
                       torch.matmul(gy.t(), x))
    with pytest.raises(RuntimeError):
        F.linear_wgrad(gy, x, impl="hip")


def test_unknown_impl_rejected():
    with pytest.raises(ValueError):
        F.linear_wgrad(torch.zeros(4, 4), torch.zeros(4, 4), impl="fast")


def test_graph_weight_gradient_goes_through_dispatch(monkeypatch):
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
    from hetu_amd.graph.ops import api as ht
    calls = []
    real = F.linear_wgrad

    def spy(gy, x, impl=None):
        calls.append((tuple(gy.shape), tuple(x.shape)))
        return real(gy, x, impl)
    monkeypatch.setattr(F, "linear_wgrad", spy)
    torch.manual_seed(5)
    wv, bv = torch.randn(6, 8), torch.randn(6)
    xv, cv = torch.randn(2, 5, 8), torch.randn(2, 5, 6)
    g = DefineAndRunGraph("wgrad_cpu")
    push_graph(g)
    try:
        x = ht.placeholder((2, 5, 8), name="x")
        c = ht.placeholder((2, 5, 6), name="c")
        w = ht.variable(wv.clone(), name="w")
        b = ht.variable(bv.clone(), name="b")
        loss = ht.reduce_sum(ht.mul(ht.linear(x, w, b), c))
        (gw,) = ht.gradients(loss, [w])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    out = g.run([gw], {x: xv, c: cv}, ctx=ctx)[0]
    assert calls == [((2, 5, 6), (2, 5, 8))]
    assert torch.equal(out, torch.matmul(cv.reshape(10, 6).t(),
                                         xv.reshape(10, 8)))


@pytest.mark.parametrize("T,N,K,want", [
    # the four GPT-3 7B layer shapes, at the measured token counts
    (32768, 12288, 4096, True), (32768, 4096, 4096, True),
    (32768, 16384, 4096, True), (32768, 4096, 16384, True),
    (2048, 4096, 4096, True), (8192, 16384, 4096, True),
    # near misses
    (1984, 4096, 4096, False),       # contraction below the measured range
    (32768, 4096, 3840, False),      # 16x15 = 240 tiles: partial last round
    (32768, 2048, 8192, True),       # 8x32 = 256 tiles, folds
    (32768, 256, 65536, False),      # 1x256 = 256 tiles but no 8x4 fold
    (32768, 1024, 16384, False),     # 4x64 = 256 tiles, N/256 % 8 != 0
    (32768, 16384, 768, False),      # 64x3 = 192 tiles
    (32768, 2048, 1024, False),      # 32 tiles: folds, not a whole round
])
def test_auto_rule(T, N, K, want):
    assert F._wgrad_auto_hip(T, N, K) is want
