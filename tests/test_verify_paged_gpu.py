"""GPU tests of the split-KV verification attention over the paged cache
(hetu_amd/ops/hip/attention_verify_paged.hip) through
F.flash_attn_prefill_paged(impl="split"), against the fp64 oracle of
prefill_paged_oracle.py with decode_attn_oracle's bounds:
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
# one row; the whole sequence; over a 32-key wave / page edge; over the 128-key
# tile edge; an empty chunk; ending on the last row of the last page
SEQS = ((0, 1), (0, 5), (31, 2), (125, 8), (300, 0), (504, 8))
HEADS = [(4, 4), (8, 2), (6, 2), (32, 1)]   # 8, 32, 24, 256 rows: MT 1, 2, 2, 4
INF = float("inf")


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _require_ext():
    assert F.has_ext(), "HIP extension must be built and loaded on GPU"


@functools.lru_cache(maxsize=None)
def case(H, Hkv, PS, spike=False, seqs=SEQS, seed=0):
    return PO.build(H, Hkv, PS, seqs=seqs, spike=spike, device=dev(),
                    seed=seed)


@functools.lru_cache(maxsize=None)
def oracle(H, Hkv, spike=False, seqs=SEQS, drop=None):
    return PO.ref(case(H, Hkv, 32, spike, seqs), drop)


def run(c, **kw):
    return F.flash_attn_prefill_paged(c["q"], c["k_pool"], c["v_pool"],
                                      c["table"], c["cu_q"], c["kv_len"],
                                      impl="split", **kw)


def check(res, ref, what):
    return DO.check(res[0], res[1].t(), ref, what)


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("H,Hkv,PS,spike",
                         [(H, Hkv, PS, False) for H, Hkv in HEADS
                          for PS in (32, 256)] + [(8, 2, 32, True)])
def test_kernel_meets_fp64_reference(H, Hkv, PS, spike, ns):
    c = case(H, Hkv, PS, spike)
    assert not c["q"].is_contiguous()
    check(run(c, num_splits=ns), oracle(H, Hkv, spike),
          f"{H}/{Hkv} PS={PS} spike={spike} ns={ns}")


@pytest.mark.parametrize("ns", [0, 1, 3])
def test_kv_len_below_n_and_max_q(ns):
    seqs = ((-3, 8), (10, 4))             # kv_len = 5 with 8 rows
    c = case(8, 2, 32, seqs=seqs)
    out, lse = run(c, num_splits=ns)
    assert (out[:3] == 0).all() and (lse[:, :3] == -INF).all()
    assert torch.isfinite(lse[:, 3:12]).all()
    check((out, lse), oracle(8, 2, seqs=seqs), "kv_len < n")
    mo, ml = run(c, num_splits=ns, max_q=8)
    assert torch.equal(out, mo) and torch.equal(lse, ml)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("PS,entry", [(32, 0), (32, 15), (256, 1)])
def test_out_of_range_page_is_masked_keys(PS, entry, ns):
    """One entry of the last sequence (504 + 8 keys) set to P, where NaN
    waits: the first page, the page the chunk itself lies in, half the keys."""
    H, Hkv = 8, 2
    c = dict(case(H, Hkv, PS))
    c["table"] = c["table"].clone()
    c["table"][-1, entry] = c["P"]
    res = run(c, num_splits=ns)
    assert torch.isfinite(res[0]).all()
    check(res, oracle(H, Hkv, drop=(5, entry * PS, (entry + 1) * PS)),
          f"PS={PS} entry {entry} ns={ns}")


def test_capture_append_and_verify():
    """Append + impl="split" captured once and replayed over rounds that
    differ in cu_q, kv_len, table and pools: an empty chunk in round 1, a
    chunk crossing into a new page (60 + 8 rows, PS = 32) in round 2."""
    H, Hkv, PS = 8, 2, 32
    rounds = [((0, 8), (40, 3), (100, 5)), ((8, 7), (43, 0), (200, 8)),
              ((15, 1), (60, 8), (500, 2))]
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
                                max_q=8, impl="hip")
        return F.flash_attn_prefill_paged(q, kp, vp, table, cu, kv_len,
                                          max_q=8, impl="split")
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
        n = c["q"].shape[0]               # cu_q[B] + PO.TAIL rows
        DO.check(out[:n], lse.t()[:n], PO.ref(c), f"replay {i}")
        assert (out[n:] == 0).all() and (lse[:, n:] == -INF).all()


def test_generator_verification_chunks_against_fp32(monkeypatch):
    """bf16 logits of ALL rows of one verification chunk per sequence through
    impl="split" against an fp32 CPU run of the same forward: at most twice
    the error of the same tokens one at a time through the S = 1 paged decode
    path (the rule of test_generator_packed_and_chunked_against_fp32)."""
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=512,
                      ffn_hidden=256, vocab=301, max_seq=160)
    state = DO.llama_state(cfg, 256)
    g = torch.Generator().manual_seed(2)
    lens, ns = (3, 70, 131), (1, 4, 8)
    prompts = [torch.randint(0, cfg.vocab, (n,), generator=g) for n in lens]
    given = [torch.randint(0, cfg.vocab, (n,), generator=g) for n in ns]

    def logits(device, dtype, chunked):
        gen = LlamaGenerator(cfg, state, device=device, dtype=dtype,
                             kv_layout="paged", page_size=32)
        cache = PagedKVCache(cfg, [a + b for a, b in zip(lens, ns)], 32,
                             device, dtype)
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        head = gen.w["lm_head.weight"].t()
        with torch.no_grad():
            for b, p in enumerate(prompts):
                gen._forward(p.to(device).unsqueeze(0), cache.row(b), 0)
            if chunked:
                x, _ = gen._packed_hidden([t.to(device) for t in given],
                                          list(lens), cache, split=True)
                return (x @ head).float().cpu()
            rows = []
            for b, t in enumerate(given):  # today's path: one token a step
                for i in range(t.numel()):
                    cache.kv_len[b] = lens[b] + i + 1
                    rows.append(gen._hidden(t[i].to(device).view(1, 1),
                                            cache.row(b), None)[0] @ head)
            return torch.cat(rows).float().cpu()
    impls, real = [], F.flash_attn_prefill_paged
    monkeypatch.setattr(F, "flash_attn_prefill_paged", lambda *a, **kw: (
        impls.append(kw.get("impl")), real(*a, **kw))[1])
    want = logits(torch.device("cpu"), torch.float32, True)
    e_one = (logits(dev(), torch.bfloat16, False) - want).abs().max().item()
    e_split = (logits(dev(), torch.bfloat16, True) - want).abs().max().item()
    assert impls == [None] * cfg.n_layer + ["split"] * cfg.n_layer, impls
    print(f"e_one_at_a_time {e_one:.4e} e_split {e_split:.4e}")
    assert e_split <= 2 * e_one, (e_one, e_split)
