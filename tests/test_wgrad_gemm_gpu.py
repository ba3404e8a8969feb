"""Hand-written weight-gradient GEMM (ops/hip/gemm_wgrad.hip) behind
F.linear_wgrad(impl="hip"): dW [N, K] = gy[T, N]^T @ x[T, K].

Shapes are the smallest that reach every path of the kernel.  Contraction
lengths of 1, 2, 3, 4, 7 and 16 K-tiles of 64 tokens: shorter than the
prefetch depth, odd and even against a loop that takes two K-tiles per
iteration, and the smallest steady state.  Output grids of 1, 2, 3 and 9
tiles: non-square so a transposed output cannot hide, and 9 (> 8, not a
multiple of 8) for the XCD remap's row-major branch.  The 8x4 rectangle fold
that every large output takes needs N/256 % 8 == 0 and K/256 % 4 == 0, so
2048x1024 (32 tiles, one rectangle) and 4096x2048 (128 tiles: two rectangle
rows and columns, and a 16-id XCD chunk that a run of 32 straddles) cover
it; the output buffer is uninitialised, so a tile mapped twice or never
shows as a mismatch.

Bounds (from the number formats, not from the kernel): against the fp64
reference the hand kernel's max error is at most 1.5x the library's on the
same inputs
(both accumulate in fp32 and round once; the margin covers a different
summation tree), and every element is within one bf16 ulp of the library's.
"""
import functools

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

T_STEPS = [64, 128, 192, 256, 448, 1024]         # 1, 2, 3, 4, 7, 16 K-tiles
GRIDS = [(256, 256), (512, 256), (256, 768), (2304, 256)]
FOLD_SHAPES = [(64, 2048, 1024), (448, 2048, 1024), (128, 4096, 2048)]
SHAPES = ([(t, 256, 256) for t in T_STEPS] +
          [(t, n, k) for t in (448, 1024) for (n, k) in GRIDS[1:]] +
          FOLD_SHAPES)


def dev():
    return torch.device("cuda", 0)


def _rand(T, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, C, generator=g).to(torch.bfloat16).to(dev())


@functools.lru_cache(maxsize=None)
def _case(T, N, K):
    """inputs, fp64 reference and library result, computed once per shape"""
    gy, x = _rand(T, N, 1000 + T + N), _rand(T, K, 2000 + T + K)
    ref = gy.double().t() @ x.double()
    blas = torch.matmul(gy.t(), x)
    return gy, x, ref, blas


def _ulp_key(t):
    """bf16 -> integers ordered like the values, adjacent values 1 apart"""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _assert_within_one_ulp(a, b, what):
    d = (_ulp_key(a) - _ulp_key(b)).abs().max().item()
    assert d <= 1, f"{what}: {d} bf16 ulps apart"


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_matches_reference_and_library(T, N, K):
    gy, x, ref, blas = _case(T, N, K)
    hand = F.linear_wgrad(gy, x, impl="hip")
    assert hand.shape == (N, K) and hand.dtype == torch.bfloat16
    assert torch.isfinite(hand.float()).all()
    e_hand = (hand.double() - ref).abs().max().item()
    e_blas = (blas.double() - ref).abs().max().item()
    print(f"T={T} N={N} K={K}: max err hand {e_hand:.4g} blas {e_blas:.4g}")
    assert e_hand <= 1.5 * e_blas
    _assert_within_one_ulp(hand, blas, f"T={T} N={N} K={K} hand vs library")


def test_identity_gy_returns_x():
    x = _rand(256, 256, 7)
    eye = torch.eye(256, dtype=torch.bfloat16, device=dev())
    assert torch.equal(F.linear_wgrad(eye, x, impl="hip"), x)


def test_identity_x_returns_gy_transposed():
    gy = _rand(256, 256, 8)          # random, hence asymmetric
    eye = torch.eye(256, dtype=torch.bfloat16, device=dev())
    assert not torch.equal(gy, gy.t())
    assert torch.equal(F.linear_wgrad(gy, eye, impl="hip"), gy.t())


@pytest.mark.parametrize("T,N,K", [(192, 256, 256), (448, 2304, 256),
                                   (1024, 256, 768), (128, 4096, 2048)])
def test_deterministic(T, N, K):
    gy, x, _, _ = _case(T, N, K)
    first = F.linear_wgrad(gy, x, impl="hip")
    for i in range(10):
        again = F.linear_wgrad(gy, x, impl="hip")
        assert torch.equal(again, first), f"call {i + 2} differs"


def test_graph_capture_replay():
    T, N, K = 448, 512, 256
    gy, x = _rand(T, N, 31).clone(), _rand(T, K, 32).clone()
    feeds = [(_rand(T, N, 40 + i), _rand(T, K, 50 + i)) for i in range(3)]
    eager = []
    for a, b in feeds:
        gy.copy_(a)
        x.copy_(b)
        eager.append(F.linear_wgrad(gy, x, impl="hip").clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.linear_wgrad(gy, x, impl="hip")
    for (a, b), ref in zip(feeds, eager):
        gy.copy_(a)
        x.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def _ineligible():
    nc = _rand(256, 512, 5)[:, ::2]                  # non-contiguous gy
    assert not nc.is_contiguous()
    return {
        "N=384": (_rand(256, 384, 1), _rand(256, 256, 2)),
        "K=320": (_rand(256, 256, 1), _rand(256, 320, 2)),
        "T=100": (_rand(100, 256, 1), _rand(100, 256, 2)),
        "fp32": (_rand(256, 256, 1).float(), _rand(256, 256, 2).float()),
        "non-contiguous gy": (nc, _rand(256, 256, 2)),
    }


@pytest.mark.parametrize("name", ["N=384", "K=320", "T=100", "fp32",
                                  "non-contiguous gy"])
def test_hip_raises_and_auto_uses_library(name):
    gy, x = _ineligible()[name]
    with pytest.raises(RuntimeError):
        F.linear_wgrad(gy, x, impl="hip")
    assert torch.equal(F.linear_wgrad(gy, x, impl="auto"),
                       torch.matmul(gy.t(), x))


def _linear_grads(monkeypatch, impl):
    """one linear layer with bias, hidden 256, 512 tokens: grads of
    sum(y * c) with respect to x, w and b"""
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
    from hetu_amd.graph.ops import api as ht
    monkeypatch.setattr(F, "_HETU_WGRAD", impl)
    calls = []
    real = F.linear_wgrad

    def spy(gy, x, impl=None):
        calls.append(impl)
        return real(gy, x, impl)
    monkeypatch.setattr(F, "linear_wgrad", spy)
    gen = torch.Generator().manual_seed(77)

    def rnd(*shape):
        return torch.randn(*shape, generator=gen).to(torch.bfloat16)
    g = DefineAndRunGraph(f"wgrad_{impl}")
    push_graph(g)
    try:
        x = ht.placeholder((512, 256), dtype=torch.bfloat16, name="x")
        c = ht.placeholder((512, 256), dtype=torch.bfloat16, name="c")
        w = ht.variable(rnd(256, 256) * 0.05, name="w")
        b = ht.variable(rnd(256), name="b")
        loss = ht.reduce_sum(ht.mul(ht.linear(x, w, b), c))
        grads = ht.gradients(loss, [x, w, b])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, dev(), use_comm=False)
    out = g.run(list(grads), {x: rnd(512, 256).to(dev()),
                              c: rnd(512, 256).to(dev())}, ctx=ctx)
    torch.cuda.synchronize()
    assert calls, "the graph's weight gradient did not go through " \
                  "F.linear_wgrad"
    return [t.clone() for t in out]


def test_linear_layer_graph_hip_vs_blas(monkeypatch):
    gx_h, gw_h, gb_h = _linear_grads(monkeypatch, "hip")
    gx_b, gw_b, gb_b = _linear_grads(monkeypatch, "blas")
    assert gw_h.shape == (256, 256)
    _assert_within_one_ulp(gw_h, gw_b, "graph weight gradient")
    assert torch.equal(gx_h, gx_b)
    assert torch.equal(gb_h, gb_b)
