"""GPU tests of the packed prefill over the paged KV cache: the kernel of
hetu_amd/ops/hip/attention_prefill_paged.hip and the packed append kernel of
kv_cache_paged.hip through hetu_amd.ops.functional, against the fp64 oracle
of prefill_paged_oracle.py with decode_attn_oracle's bounds:
|out - ref| <= 3 * 2^-9 * max |v| over the row's attended keys,
|lse - ref| <= 1e-3, rows that attend nothing exactly 0 / -inf.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import prefill_paged_oracle as PO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu
HEADS = [(4, 4), (8, 2), (6, 2), (32, 1)]        # GP = 1, 4, 2, 8


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    assert F.has_ext(), "HIP extension must be built and loaded on GPU"


@functools.lru_cache(maxsize=None)
def case(H, Hkv, PS, spike=False, seqs=PO.SEQS, seed=0):
    return PO.build(H, Hkv, PS, seqs=seqs, spike=spike, device=dev(),
                    seed=seed)


@functools.lru_cache(maxsize=None)
def oracle(H, Hkv, spike=False, seqs=PO.SEQS, drop=None):
    return PO.ref(case(H, Hkv, 32, spike, seqs), drop)


def run(c, **kw):
    return F.flash_attn_prefill_paged(c["q"], c["k_pool"], c["v_pool"],
                                      c["table"], c["cu_q"], c["kv_len"],
                                      impl="hip", **kw)


def check(res, ref, what):
    return DO.check(res[0], res[1].t(), ref, what)


@pytest.mark.parametrize("PS,spike", [(32, False), (256, False), (32, True)])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_kernel_meets_fp64_reference(H, Hkv, PS, spike):
    c = case(H, Hkv, PS, spike)
    assert not c["q"].is_contiguous()
    check(run(c), oracle(H, Hkv, spike), f"{H}/{Hkv} PS={PS} spike={spike}")


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_mask_all_equals_boundary_only(H, Hkv, monkeypatch):
    c = case(H, Hkv, 32)
    out, lse = run(c)
    monkeypatch.setenv("HETU_AMD_FA_MASK_ALL", "1")
    mo, ml = run(c)
    assert torch.equal(out, mo) and torch.equal(lse, ml)


@pytest.mark.parametrize("PS,entry", [(32, 0), (32, 7), (256, 0), (256, 1)])
def test_out_of_range_page_is_masked_keys(PS, entry):
    """One entry of the last sequence (449 + 63 keys) set to P, where NaN
    waits: entry 0 is the first page of every block's range, and at PS = 256
    whole 64-key tiles lie in the page."""
    H, Hkv = 8, 2
    c = dict(case(H, Hkv, PS))
    c["table"] = c["table"].clone()
    c["table"][-1, entry] = c["P"]
    res = run(c)
    assert torch.isfinite(res[0]).all()
    check(res, oracle(H, Hkv, drop=(4, entry * PS, (entry + 1) * PS)),
          f"PS={PS} entry {entry}")


def test_kv_len_below_n_and_max_q():
    seqs = ((-4, 9), (10, 40))            # kv_len = 5 with 9 rows
    c = case(8, 2, 32, seqs=seqs)
    out, lse = run(c)
    assert (out[:4] == 0).all() and (lse[:, :4] == float("-inf")).all()
    assert torch.isfinite(lse[:, 4:49]).all()
    check((out, lse), oracle(8, 2, seqs=seqs), "kv_len < n")
    mo, ml = run(c, max_q=40)
    assert torch.equal(out, mo) and torch.equal(lse, ml)


@pytest.mark.parametrize("D", [64, 128])
def test_packed_append_equals_torch_branch(D, Hkv=2, H=4, PS=32, MP=3, P=8):
    g = torch.Generator().manual_seed(D)
    cu = torch.tensor([0, 5, 5, 45, 48], dtype=torch.int32, device=dev())
    # in page 0; empty; crossing a dropped page; the last row past MP * PS
    end = torch.tensor([5, 7, 70, MP * PS + 1], dtype=torch.int32,
                       device=dev())
    table = torch.tensor([[6, 1, 2], [P, P, P], [3, P, 4], [5, 0, 7]],
                         dtype=torch.int32, device=dev())
    qkv = torch.randn(48, (H + 2 * Hkv) * D, generator=g).bfloat16().to(dev())
    _, k_new, v_new = (t.view(48, -1, D) for t in
                       qkv.split([H * D, Hkv * D, Hkv * D], dim=-1))
    got = torch.full((2, P, Hkv, PS, D), PO.NAN, dtype=torch.bfloat16,
                     device=dev())
    want = got.clone()
    for pools, impl in ((got, "hip"), (want, "torch")):
        F.kv_cache_append_paged(k_new, v_new, pools[0], pools[1], table, end,
                                cu_q=cu, impl=impl)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # what landed: 5 + (40 - 32 in the dropped page) + (3 - 1) rows a side
    assert int((~got.isnan()).sum()) == 2 * (5 + 8 + 2) * Hkv * D


def test_capture_append_and_prefill():
    H, Hkv, PS = 8, 2, 32
    rounds = [((0, 20), (40, 3), (100, 60)), ((20, 7), (43, 0), (160, 64)),
              ((27, 37), (43, 33), (224, 1))]
    cases = [case(H, Hkv, PS, seqs=s, seed=i) for i, s in enumerate(rounds)]
    T = max(c["q"].shape[0] for c in cases)
    c0 = cases[0]
    # the captured buffers, rewritten in place between the replays
    q = torch.zeros(T, H, PO.D, dtype=torch.bfloat16, device=dev())
    k_new = torch.zeros(T, Hkv, PO.D, dtype=torch.bfloat16, device=dev())
    v_new = torch.zeros_like(k_new)
    cu, kv_len, table = (c0[n].clone() for n in ("cu_q", "kv_len", "table"))
    kp, vp = c0["k_pool"].clone(), c0["v_pool"].clone()

    def load(c):
        n = c["q"].shape[0]
        q[:n] = c["q"]
        for b, (ctx, rows) in enumerate(c["seqs"]):
            lo = int(c["cu_q"][b])
            for new, dense in ((k_new, c["k"]), (v_new, c["v"])):
                new[lo:lo + rows] = dense[b, :, ctx:ctx + rows] \
                    .permute(1, 0, 2).to(dev())
        for dst, src in ((cu, "cu_q"), (kv_len, "kv_len"), (table, "table"),
                         (kp, "k_pool"), (vp, "v_pool")):
            dst.copy_(c[src])
        # blank the chunk's rows: the captured append has to write them
        blank = torch.full_like(k_new, PO.NAN)
        F.kv_cache_append_paged(blank, blank, kp, vp, table, kv_len, cu_q=cu,
                                impl="torch")

    def step():
        F.kv_cache_append_paged(k_new, v_new, kp, vp, table, kv_len, cu_q=cu,
                                impl="hip")
        return F.flash_attn_prefill_paged(q, kp, vp, table, cu, kv_len,
                                          impl="hip")
    load(c0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = step()
    for i, c in enumerate(cases):
        load(c)
        graph.replay()
        n = c["q"].shape[0]
        ref = PO.ref(c)
        DO.check(out[:n], lse.t()[:n], ref, f"replay {i}")
        assert (out[n:] == 0).all() and (lse[:, n:] == float("-inf")).all()


def test_generator_packed_and_chunked_against_fp32():
    """bf16 last-token logits against an fp32 CPU run: the packed and the
    chunked error at most twice that of today's prefill="sequence"."""
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=512,
                      ffn_hidden=256, vocab=301, max_seq=160)
    state = DO.llama_state(cfg, 256)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g)
               for n in (3, 70, 131)]
    lens = [p.numel() for p in prompts]

    def logits(device, dtype, **kw):
        gen = LlamaGenerator(cfg, state, device=device, dtype=dtype,
                             kv_layout="paged", page_size=32, **kw)
        ps = [p.to(device) for p in prompts]
        cache = PagedKVCache(cfg, lens, 32, device, dtype)
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        with torch.no_grad():
            if kw:
                return gen._prefill_packed(ps, lens, cache).float().cpu()
            return torch.cat([gen._forward(p.unsqueeze(0), cache.row(b), 0)
                              for b, p in enumerate(ps)]).float().cpu()
    want = logits(torch.device("cpu"), torch.float32)
    e_seq = (logits(dev(), torch.bfloat16) - want).abs().max().item()
    e_pk = (logits(dev(), torch.bfloat16, prefill="packed") - want) \
        .abs().max().item()
    e_ch = (logits(dev(), torch.bfloat16, prefill="packed", prefill_chunk=64)
            - want).abs().max().item()
    print(f"e_seq {e_seq:.4e} e_packed {e_pk:.4e} e_chunked {e_ch:.4e}")
    assert e_pk <= 2 * e_seq and e_ch <= 2 * e_seq, (e_seq, e_pk, e_ch)
