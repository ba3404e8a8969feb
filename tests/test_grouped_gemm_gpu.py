"""Grouped expert GEMM kernels (ops/hip/gemm_grouped.hip, the batched entry
of gemm_wgrad.hip) against fp64 matmuls of the same bf16 values.

Tolerance (derived): the output is one bf16 rounding (relative 2^-8 with
margin for the half-ulp 2^-9) of an fp32 sum of K products of magnitude
<= max|a| max|b|, each fp32 step off by at most 2^-24 of the running sum:
  |got - ref| <= 2^-8 |ref| + K 2^-22 max|a| max|b|.
"""
import pytest
import torch

from hetu_amd.ops import functional as F

from test_grouped_gemm_cpu import run_layer

pytestmark = pytest.mark.gpu
BN = F.GMM_N_TILE
# (P, seg, counts [G=3, P])
LAYOUTS = {
    "ragged": (1, 200, [[0], [200], [129]]),
    "straddle": (2, 96, [[96, 0], [1, 96], [0, 0]]),
    "edge": (1, 256, [[128], [127], [256]]),
}


def dev():
    return torch.device("cuda")


def rnd(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 2 - 1).to(torch.bfloat16)


def row_mask(counts, seg):
    G, P = counts.shape
    return (torch.arange(seg).view(1, 1, seg)
            < counts.view(G, P, 1)).reshape(G, P * seg, 1)


def check(got, ref, K, a, b):
    got = got.double().cpu()
    assert not torch.isnan(got).any()
    amax = a.float().nan_to_num().abs().max().item() * b.abs().max().item()
    excess = (got - ref).abs() - (2.0 ** -8 * ref.abs()
                                  + K * 2.0 ** -22 * amax)
    assert excess.max() <= 0, f"over the bound by {excess.max():.3e}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N", [BN, 2 * BN])
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("trans_b", [False, True])
def test_nn_nt_match_fp64(trans_b, K, N, layout):
    P, seg, counts = LAYOUTS[layout]
    counts = torch.tensor(counts, dtype=torch.int32)
    G, M = counts.shape[0], P * seg
    gen = torch.Generator().manual_seed(K + N + seg)
    a = rnd(gen, G, M, K)
    b = rnd(gen, G, N, K) if trans_b else rnd(gen, G, K, N)
    mask = row_mask(counts, seg)
    ref = (a.double() @ (b.double().transpose(1, 2) if trans_b
                         else b.double())) * mask
    a = torch.where(mask, a, torch.full_like(a, float("nan")))
    got = F.grouped_gemm(a.to(dev()), b.to(dev()), counts.to(dev()), seg,
                         trans_b=trans_b, impl="hip")
    assert got.shape == (G, M, N) and got.dtype == torch.bfloat16
    assert (got.cpu()[~mask.expand(G, M, N)] == 0).all()
    check(got, ref, K, a, b)


def test_counts_none_is_all_valid():
    gen = torch.Generator().manual_seed(5)
    a, b = rnd(gen, 2, 200, 192), rnd(gen, 2, 192, BN)
    got = F.grouped_gemm(a.to(dev()), b.to(dev()), impl="hip")
    check(got, a.double() @ b.double(), 192, a, b)


@pytest.mark.parametrize("M", [64, 192])
def test_tn_matches_fp64_and_linear_wgrad(M):
    gen = torch.Generator().manual_seed(M)
    a, b = rnd(gen, 2, M, 256).to(dev()), rnd(gen, 2, M, 256).to(dev())
    got = F.grouped_gemm_tn(a, b, impl="hip")
    check(got, a.double().cpu().transpose(1, 2) @ b.double().cpu(), M, a, b)
    for i in range(2):
        assert torch.equal(got[i], F.linear_wgrad(a[i], b[i], impl="hip"))


@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 300])
def test_moe_slot_counts(E, C):
    gen = torch.Generator().manual_seed(E * 1000 + C)
    fill = torch.randint(0, C + 1, (E,), generator=gen)
    fill[0], fill[-1] = C, 0          # E = 1: the empty row
    pos = torch.where(torch.arange(C).view(1, C) < fill.view(E, 1),
                      torch.randint(0, 99, (E, C), generator=gen), -1)
    got = F.moe_slot_counts(pos.to(dev()))
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu(), (pos >= 0).sum(1).to(torch.int32))
    if E == 1:
        full = F.moe_slot_counts(torch.zeros(1, C, dtype=torch.int64,
                                             device=dev()))
        assert full.tolist() == [C]


def test_capture_follows_counts_rewritten_on_device():
    gen = torch.Generator().manual_seed(9)
    a, b = rnd(gen, 3, 256, 64).to(dev()), rnd(gen, 3, 64, BN).to(dev())
    first = torch.tensor([[256], [0], [5]], dtype=torch.int32, device=dev())
    second = torch.tensor([[0], [130], [256]], dtype=torch.int32,
                          device=dev())
    counts = first.clone()
    F.grouped_gemm(a, b, counts, 256, impl="hip")       # warm-up, eager
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.grouped_gemm(a, b, counts, 256, impl="hip")
    for want in (second, first, second):
        counts.copy_(want)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, F.grouped_gemm(a, b, want, 256, impl="hip"))
        ref = (a.double() @ b.double()).cpu() * row_mask(want.cpu(), 256)
        check(out, ref, 64, a, b)


def test_layer_grouped_no_worse_than_bmm():
    # capacity 1.5: C = 192 slots, so every form takes its hand kernel and an
    # expert is one full row tile and one that is partly or wholly empty
    shape = dict(N=256, H=256, Fh=256, E=4, cap=1.5)
    ref = run_layer("bmm", torch.float32, dev(), **shape)
    err = {m: [(o.float() - r).abs().max().item() for o, r in
               zip(run_layer(m, torch.bfloat16, dev(), **shape), ref)]
           for m in ("grouped", "bmm")}
    names = ("y", "dx", "dw1", "dw2")
    for name, eg, eb in zip(names, err["grouped"], err["bmm"]):
        print(f"{name}: grouped {eg:.3e} bmm {eb:.3e}")
    for name, eg, eb in zip(names, err["grouped"], err["bmm"]):
        assert eg <= 2 * eb + 1e-6, (name, eg, eb)


@pytest.mark.parametrize("case", ["K96", "fp16", "counts_shape"])
def test_hip_errors(case):
    K = 96 if case == "K96" else 64
    dt = torch.float16 if case == "fp16" else torch.bfloat16
    a = torch.zeros(2, 128, K, dtype=dt, device=dev())
    b = torch.zeros(2, K, BN, dtype=dt, device=dev())
    counts = torch.zeros((3, 1) if case == "counts_shape" else (2, 1),
                         dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError):
        F.grouped_gemm(a, b, counts, 128, impl="hip")
