"""GPU tests of the paged KV cache: the PAGED decode kernels
(hetu_amd/ops/hip/attention_decode_paged.hip, attention_decode_mfma.hip) and
the append kernel (kv_cache_paged.hip) through hetu_amd.ops.functional.

The paged kernels run the dense kernels' arithmetic in the dense order, so
for the same values, kv_len and num_splits the result must be bit-identical
to the dense kernel's; against the fp64 oracle (decode_attn_oracle.py) the
bounds are that file's defaults.  Every pool is a view of P pages of an
allocation of P + 2, and NaN fills everything a kernel must not read: rows
past kv_len, the page nobody owns, the two pages beyond the view; table
entries past the last needed page point at a NaN page.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

B, L = 3, 512
HEADS = [(4, 4), (8, 2), (12, 2), (32, 1)]
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    assert F.has_ext(), "HIP extension must be built and loaded on GPU"


def length_rows(PS):
    """kv_len rows that together cover 0, 1, PS - 1, PS, PS + 1, 63 / 64 / 65,
    127 / 128 / 129 and L."""
    return [(0, 1, PS - 1), (PS, PS + 1, 63), (64, 65, 127), (128, 129, L)]


def scatter(k, v, PS, lens, seed):
    """Dense caches -> NaN-poisoned pools behind a random table whose pages
    interleave the sequences; returns (k_pool, v_pool, table, P)."""
    Bk, Hkv, Lk, D = k.shape
    MP = Lk // PS
    P = Bk * MP + 1                       # the last page of the permutation
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed))
    table = perm[:Bk * MP].view(MP, Bk).t().contiguous()
    pools = []
    for t in (k, v):
        t = t.clone()
        for b, n in enumerate(lens):
            t[b, :, n:] = NAN
        big = torch.full((P + 2, Hkv, PS, D), NAN, dtype=t.dtype,
                         device=t.device)
        big[table.to(t.device)] = t.view(Bk, Hkv, MP, PS, D) \
            .permute(0, 2, 1, 3, 4)
        pools.append(big[:P])
    for b, n in enumerate(lens):          # unneeded entries: the NaN page
        table[b, -(-n // PS):] = perm[-1]
    return pools[0], pools[1], table.to(torch.int32).to(k.device), P


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv, PS, row):
    lens = length_rows(PS)[row]
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, seed=D + H + row,
                                   device=dev())
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev())
    kp, vp, table, P = scatter(k, v, PS, lens, seed=PS + row)
    return q, k, v, kp, vp, table, kv_len, DO.decode_ref(q, k, v, kv_len)


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("PS", [32, 64, 256])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("impl", ["hip", "mfma"])
def test_paged_is_bit_identical_to_dense_and_meets_oracle(impl, D, H, Hkv,
                                                          PS, ns):
    for row in range(4):
        q, k, v, kp, vp, table, kv_len, ref = case(D, H, Hkv, PS, row)
        out, lse = F.flash_attn_decode(q, kp, vp, kv_len, num_splits=ns,
                                       impl=impl, block_table=table)
        do, dl = F.flash_attn_decode(q, k, v, kv_len, num_splits=ns,
                                     impl=impl)
        what = f"{impl} D={D} {H}/{Hkv} PS={PS} ns={ns} row {row}"
        DO.check(out, lse, ref, what)
        assert torch.equal(out, do) and torch.equal(lse, dl), what


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("PS", [32, 256])
@pytest.mark.parametrize("impl", ["hip", "mfma"])
def test_out_of_range_page_is_a_page_of_masked_keys(impl, PS, ns):
    """Entry 0 of row 2 (kv_len = L) set to P: out of range, yet inside the
    allocation, where NaN waits.  At PS = 256 and ns = 3 the first split owns
    no other key."""
    D, H, Hkv = 128, 8, 2
    q, k, v, kp, vp, table, kv_len, _ = case(D, H, Hkv, PS, 3)
    table = table.clone()
    table[2, 0] = kp.shape[0]
    out, lse = F.flash_attn_decode(q, kp, vp, kv_len, num_splits=ns,
                                   impl=impl, block_table=table)
    head = DO.decode_ref(q[:2], k[:2], v[:2], kv_len[:2])
    tail = DO.decode_ref(q[2:], k[2:, :, PS:], v[2:, :, PS:], L - PS)
    DO.check(out, lse, tuple(torch.cat([a, b]) for a, b in zip(head, tail)),
             f"{impl} PS={PS} ns={ns}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
def test_append_equals_torch_branch(S, D):
    Hkv, H, PS, MP, P = 2, 4, 32, 3, 10
    g = torch.Generator().manual_seed(S + D)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).bfloat16() \
        .to(dev())
    _, k_new, v_new = qkv.split([H * D, Hkv * D, Hkv * D], dim=-1)
    k_new, v_new = k_new.view(B, S, Hkv, D), v_new.view(B, S, Hkv, D)
    table = torch.randperm(P, generator=g)[:B * MP].view(B, MP) \
        .to(torch.int32)
    table[1, 1] = P                       # these rows are dropped
    table = table.to(dev())
    # rows in page 0; in a dropped page; past MP * PS (S = 5: three of them)
    end = torch.tensor([S, PS + 2, MP * PS + 2], dtype=torch.int32,
                       device=dev())
    layers = torch.randn(2, 2, P, Hkv, PS, D, generator=g).bfloat16() \
        .to(dev())
    want = layers.clone()
    F.kv_cache_append_paged(k_new, v_new, layers[0, 1], layers[1, 1], table,
                            end, impl="hip")
    F.kv_cache_append_paged(k_new, v_new, want[0, 1], want[1, 1], table, end,
                            impl="torch")
    assert torch.equal(layers, want)
    assert torch.equal(layers[0, 1, table[0, 0], :, S - 1], k_new[0, S - 1])


def test_capture_append_and_decode():
    D, H, Hkv, PS, MP = 128, 8, 2, 32, 4
    q, k, v, _, _ = DO.make_inputs(B, H, Hkv, MP * PS, D, seed=9,
                                   device=dev())
    kp, vp, table, _ = scatter(k, v, PS, [MP * PS] * B, seed=9)
    g = torch.Generator().manual_seed(9)
    k_new = torch.randn(B, 1, Hkv, D, generator=g).bfloat16().to(dev())
    v_new = torch.randn(B, 1, Hkv, D, generator=g).bfloat16().to(dev())
    kv_len = torch.tensor([30, 62, 100], dtype=torch.int32, device=dev())

    def step():
        F.kv_cache_append_paged(k_new, v_new, kp, vp, table, kv_len,
                                impl="hip")
        return F.flash_attn_decode(q, kp, vp, kv_len, impl="hip",
                                   block_table=table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = step()
    for i in range(3):                    # 31 / 63 / 101, then 32 / 64 (a
        kv_len.add_(1)                    # new page) / 102, then 33 / 65 / ..
        if i:
            table.copy_(table[[1, 0, 2]])     # rows 0 and 1 trade pages
        graph.replay()
        kd, vd, n, _ = F._decode_paged_gather(kp, vp, table, kv_len)
        DO.check(out, lse, DO.decode_ref(q, kd, vd, n), f"replay {i}")
        eo, el = step()
        assert torch.equal(out, eo) and torch.equal(lse, el), f"replay {i}"


def test_errors_and_auto():
    q, k, v, kp, vp, table, kv_len, ref = case(64, 8, 2, 32, 2)

    def hip(kp_, vp_, table_, **kw):
        return F.flash_attn_decode(q, kp_, vp_, kv_len, impl="hip",
                                   block_table=table_, **kw)
    odd = torch.zeros(4, 2, 48, 64, dtype=torch.bfloat16, device=dev())
    with pytest.raises(RuntimeError, match="page size of k_cache"):
        hip(odd, odd, table)
    with pytest.raises(RuntimeError, match="block_table is torch.int64"):
        hip(kp, vp, table.long())
    with pytest.raises(RuntimeError, match="block_table is not on the GPU"):
        hip(kp, vp, table.cpu())
    with pytest.raises(RuntimeError, match="block_table must be"):
        hip(kp, vp, table[:2])
    fp8 = kp.view(torch.uint8).view(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="block_table with an fp8 cache"):
        hip(fp8, fp8, table)
    # the extension's own checks hold when it is called directly
    with pytest.raises(RuntimeError, match="block_table must be a contiguous"):
        F.ext().flash_attn_decode_paged(q, kp, vp, table.long(), kv_len, 1.0)
    # auto serves an fp32 pool from the torch branch, bf16 from a kernel
    o32, _ = F.flash_attn_decode(q.float(), kp.float(), vp.float(), kv_len,
                                 block_table=table)
    assert o32.dtype == torch.float32
    out, lse = F.flash_attn_decode(q, kp, vp, kv_len, block_table=table)
    assert torch.equal(out, hip(kp, vp, table)[0])
    DO.check(out, lse, ref)


def test_llama_generator_paged_hip_vs_torch():
    """Teacher-forced, in the form of test_llama_generator_hip_vs_torch: the
    same config and the same rtol = atol = 6e-2 on logits; ragged prompts
    (5 and 9 tokens), PS = 32, and enough steps for both to cross a page."""
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=512,
                      ffn_hidden=256, vocab=301, max_seq=64)
    state = DO.llama_state(cfg, 256)
    lens, steps = (5, 9), 30
    ids = torch.randint(0, cfg.vocab, (2, max(lens) + steps),
                        generator=torch.Generator().manual_seed(1)).to(dev())
    logits = []
    for impl in ("hip", "torch"):
        g = LlamaGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                           decode_impl=impl, kv_layout="paged", page_size=32)
        cache = PagedKVCache(cfg, [n + steps for n in lens], 32, dev(),
                             torch.bfloat16)
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        with torch.no_grad():
            got = [torch.cat([g._forward(ids[b:b + 1, :n], cache.row(b), 0)
                              for b, n in enumerate(lens)])]
            for s in range(steps):
                tok = torch.stack([ids[b, n + s] for b, n in enumerate(lens)])
                cache.kv_len.add_(1)
                got.append(g._forward(tok.view(2, 1), cache, None))
        logits.append(torch.stack(got).float().cpu())
    assert torch.isfinite(logits[0]).all()
    err = (logits[0] - logits[1]).abs().amax(dim=(1, 2))
    assert torch.allclose(logits[0], logits[1], rtol=6e-2, atol=6e-2), \
        f"max abs err per step {err.tolist()}"
    out = g.generate([ids[0, :5], ids[1, :9]], max_new_tokens=4)
    assert [o.numel() for o in out] == [9, 13]
