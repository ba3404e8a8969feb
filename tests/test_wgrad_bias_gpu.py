"""Bias variant of the hand weight-gradient GEMM (ops/hip/gemm_wgrad.hip)
behind F.linear_wgrad_bias(impl="hip"):
(dW [N, K] = gy^T @ x, db [N] = sum_t gy[t, :]) from one launch.

Shapes are those where the added code can go wrong.  (256, 256) at 1, 2, 3
and 7 K-tiles of 64 tokens: the prologue-only case, odd and even counts
against a loop that takes two K-tiles per iteration.  (512, 512): the
row-major remap with tiles_k = 2, where only the tk == 0 block of a tile row
may write db and tile row 1 lands at offset 256.  (768, 256): 3 tiles, a grid
that is no multiple of 8.  (2048, 1024): the 8x4 rectangle fold, exactly one
writer per tile row after the remap.

Bounds, from the number formats alone.  dW: bit-equal to the plain kernel
(the same MFMAs in the same order).  db on {-1, 0, 1} inputs: every partial
sum is an integer of magnitude <= 448, exact in fp32, and the totals are
checked to be bf16 numbers, so db equals the fp64 sum exactly.  db on
random-normal inputs, per column j:
  |db - ref| <= 2^-8 |ref| + (T/32 + 8) 2^-24 sum_t |gy[t, j]|
one bf16 rounding (half an ulp is at most 2^-8 relative) plus fp32
accumulation over T/32 sequential MFMA adds, each of a 32-term product sum
(the 8 allows for the tree inside one MFMA).
"""
import functools

import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

SHAPES = ([(t, 256, 256) for t in (64, 128, 192, 448)] +
          [(128, 512, 512), (64, 768, 256), (128, 2048, 1024)])


def dev():
    return torch.device("cuda", 0)


def _rand(T, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, C, generator=g).to(torch.bfloat16).to(dev())


@functools.lru_cache(maxsize=None)
def _normal_case(T, N, K):
    """random-normal operands, the plain kernel's dW, the fp64 column sums
    and the error bound of the module docstring, computed once per shape"""
    gy, x = _rand(T, N, 3000 + T + N), _rand(T, K, 4000 + T + K)
    plain = F.ext().gemm_wgrad_bf16(gy, x)
    ref = gy.double().sum(0)
    bound = 2.0 ** -8 * ref.abs() + \
        (T / 32 + 8) * 2.0 ** -24 * gy.double().abs().sum(0)
    return gy, x, plain, ref, bound


@functools.lru_cache(maxsize=None)
def _integer_case(T, N, K):
    """gy in {-1, 0, 1}; column 1 of every 256 all ones, column 2 all zeros"""
    g = torch.Generator().manual_seed(5000 + T + N)
    gy = torch.randint(-1, 2, (T, N), generator=g).to(torch.bfloat16)
    gy[:, 1::256] = 1
    gy[:, 2::256] = 0
    gy = gy.to(dev())
    return gy, _rand(T, K, 6000 + T + K), gy.double().sum(0)


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_dw_bit_equal_to_plain_kernel(T, N, K):
    gy, x, plain, _, _ = _normal_case(T, N, K)
    dw, db = F.linear_wgrad_bias(gy, x, impl="hip")
    assert dw.shape == (N, K) and dw.dtype == torch.bfloat16
    assert db.shape == (N,) and db.dtype == torch.bfloat16
    assert torch.equal(dw, plain)


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_db_exact_on_small_integers(T, N, K):
    gy, x, ref = _integer_case(T, N, K)
    # a property of the seeded input: the totals are bf16 numbers
    assert torch.equal(ref.to(torch.bfloat16).double(), ref)
    assert ref.abs().max().item() <= 448
    assert (ref[1::256] == T).all() and (ref[2::256] == 0).all()
    _, db = F.linear_wgrad_bias(gy, x, impl="hip")
    bad = (db.double() != ref).nonzero().flatten().tolist()
    assert not bad, (f"T={T} N={N} K={K}: {len(bad)} wrong columns, first "
                     f"{bad[:8]}: got {db[bad[:8]].tolist()} want "
                     f"{ref[bad[:8]].tolist()}")


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_db_random_normal_within_format_bound(T, N, K):
    gy, x, _, ref, bound = _normal_case(T, N, K)
    _, db = F.linear_wgrad_bias(gy, x, impl="hip")
    err = (db.double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"T={T} N={N} K={K}: max err/bound {worst:.3f}")
    assert (err <= bound).all(), f"max err/bound {worst:.3f}"


@pytest.mark.parametrize("T,N,K", SHAPES)
def test_db_fully_written_over_poisoned_memory(T, N, K):
    gy, x, _, ref, bound = _normal_case(T, N, K)
    torch.cuda.synchronize()
    poison = torch.full((N,), float("nan"), dtype=torch.bfloat16,
                        device=dev())
    torch.cuda.synchronize()
    del poison                       # the allocator hands this block to db
    _, db = F.linear_wgrad_bias(gy, x, impl="hip")
    assert torch.isfinite(db.float()).all()
    assert ((db.double() - ref).abs() <= bound).all()


def test_graph_capture_replay():
    T, N, K = 192, 512, 512
    gy, x = _rand(T, N, 61).clone(), _rand(T, K, 62)
    feeds = [_rand(T, N, 70 + i) for i in range(3)]
    eager = []
    for a in feeds:
        gy.copy_(a)
        dw, db = F.linear_wgrad_bias(gy, x, impl="hip")
        eager.append((dw.clone(), db.clone()))
    assert not torch.equal(eager[0][1], eager[1][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dw, db = F.linear_wgrad_bias(gy, x, impl="hip")
    for a, (dw_ref, db_ref) in zip(feeds, eager):
        gy.copy_(a)                  # rewritten in place, then replayed
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dw, dw_ref)
        assert torch.equal(db, db_ref)


@pytest.mark.parametrize("name", ["N=384", "K=320", "T=100", "fp32",
                                  "non-contiguous gy"])
def test_hip_raises_on_ineligible_input(name):
    nc = _rand(256, 512, 5)[:, ::2]
    gy, x = {
        "N=384": (_rand(256, 384, 1), _rand(256, 256, 2)),
        "K=320": (_rand(256, 256, 1), _rand(256, 320, 2)),
        "T=100": (_rand(100, 256, 1), _rand(100, 256, 2)),
        "fp32": (_rand(256, 256, 1).float(), _rand(256, 256, 2).float()),
        "non-contiguous gy": (nc, _rand(256, 256, 2)),
    }[name]
    with pytest.raises(RuntimeError):
        F.linear_wgrad_bias(gy, x, impl="hip")
    with pytest.raises(RuntimeError):
        F.ext().gemm_wgrad_bias_bf16(gy, x)
    # auto on the same input: the unfused pair, bit for bit
    dw, db = F.linear_wgrad_bias(gy, x, impl="auto")
    assert torch.equal(dw, torch.matmul(gy.t(), x))
    assert torch.equal(db, F.colsum(gy).to(gy.dtype))


def test_auto_fuses_where_the_wgrad_rule_admits(monkeypatch):
    """2048 tokens, 2048 x 8192: the smallest shape the rule admits (256
    tiles, folds); auto returns the fused kernel's db, and the unfused
    pair's with the switch off"""
    T, N, K = 2048, 2048, 8192
    assert F._wgrad_auto_hip(T, N, K)
    gy, x = _rand(T, N, 81), _rand(T, K, 82)
    dw_h, db_h = F.linear_wgrad_bias(gy, x, impl="hip")
    dw_a, db_a = F.linear_wgrad_bias(gy, x, impl="auto")
    assert torch.equal(dw_a, dw_h) and torch.equal(db_a, db_h)
    monkeypatch.setattr(F, "_HETU_WGRAD_BIAS", "0")
    dw_u, db_u = F.linear_wgrad_bias(gy, x, impl="auto")
    assert torch.equal(dw_u, dw_h)
    assert torch.equal(db_u, F.colsum(gy).to(gy.dtype))
    ref = gy.double().sum(0)
    bound = 2.0 ** -8 * ref.abs() + (T / 32 + 8) * 2.0 ** -24 * \
        gy.double().abs().sum(0)
    assert ((db_h.double() - ref).abs() <= bound).all()
