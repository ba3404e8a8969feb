"""GPU tests of the paged prefill and split-KV verification kernels at head
dim 64 (hetu_amd/ops/hip/attention_prefill_paged.hip and
attention_verify_paged.hip) through F.flash_attn_prefill_paged, against the
fp64 oracle of prefill_paged_oracle.py at D = 64 with decode_attn_oracle's
bounds: |out - ref| <= 3 * 2^-9 * max |v| over the row's attended keys,
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
HEADS = [(4, 4), (8, 2), (6, 2), (32, 1)]   # prefill GP 1, 4, 2, 8
# the verification test's chunks: one row; the whole sequence; over a 32-key
# wave / page edge; over the 128-key tile edge; empty; the last row of the
# last page.  With HEADS a KV head has up to 8, 32, 24, 256 M-rows.
VSEQS = ((0, 1), (0, 5), (31, 2), (125, 8), (300, 0), (504, 8))
INF = float("inf")


@pytest.fixture(autouse=True)
def _d64(monkeypatch):
    assert F.has_ext(), "HIP extension must be built and loaded on GPU"
    monkeypatch.setattr(PO, "D", 64)      # PO.build / PO.ref read it per call


@functools.lru_cache(maxsize=None)
def case(H, Hkv, PS, spike=False, seqs=PO.SEQS, seed=0):
    return PO.build(H, Hkv, PS, seqs=seqs, spike=spike,
                    device=torch.device("cuda", 0), seed=seed)


@functools.lru_cache(maxsize=None)
def oracle(H, Hkv, spike=False, seqs=PO.SEQS, drop=None):
    return PO.ref(case(H, Hkv, 32, spike, seqs), drop)


def run(c, impl, ref=None, what="", **kw):
    out, lse = F.flash_attn_prefill_paged(
        c["q"], c["k_pool"], c["v_pool"], c["table"], c["cu_q"], c["kv_len"],
        impl=impl, **kw)
    assert out.shape[-1] == 64 and not c["q"].is_contiguous()
    if ref is not None:
        DO.check(out, lse.t(), ref, what)
    return out, lse


@pytest.mark.parametrize("PS,spike", [(32, False), (256, False), (32, True)])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_prefill_meets_fp64_reference(H, Hkv, PS, spike):
    """Key 440 of the last sequence carries the spike: the fourth 128-key
    tile, so the running max jumps after the first."""
    run(case(H, Hkv, PS, spike), "hip", oracle(H, Hkv, spike),
        f"{H}/{Hkv} PS={PS} spike={spike}")


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
def test_prefill_mask_all_equals_boundary_only(H, Hkv, monkeypatch):
    c = case(H, Hkv, 32)
    out, lse = run(c, "hip")
    monkeypatch.setenv("HETU_AMD_FA_MASK_ALL", "1")
    mo, ml = run(c, "hip")
    assert torch.equal(out, mo) and torch.equal(lse, ml)


@pytest.mark.parametrize("PS,entry", [(32, 0), (32, 7), (64, 3), (256, 1)])
def test_prefill_out_of_range_page_is_masked_keys(PS, entry):
    """One entry of the last sequence (449 + 63 keys) set to P, where NaN
    waits: one group of a tile, one group of the chunk's own tile, two groups
    of one tile, two whole tiles."""
    H, Hkv = 8, 2
    c = dict(case(H, Hkv, PS))
    c["table"] = c["table"].clone()
    c["table"][-1, entry] = c["P"]
    out, _ = run(c, "hip",
                 oracle(H, Hkv, drop=(4, entry * PS, (entry + 1) * PS)),
                 f"PS={PS} entry {entry}")
    assert torch.isfinite(out).all()


def test_prefill_kv_len_below_n_and_max_q():
    seqs = ((-4, 9), (10, 40))            # kv_len = 5 with 9 rows
    c = case(8, 2, 32, seqs=seqs)
    out, lse = run(c, "hip", oracle(8, 2, seqs=seqs), "kv_len < n")
    assert (out[:4] == 0).all() and (lse[:, :4] == -INF).all()
    assert torch.isfinite(lse[:, 4:49]).all()
    mo, ml = run(c, "hip", max_q=40)
    assert torch.equal(out, mo) and torch.equal(lse, ml)


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("H,Hkv,PS,spike",
                         [(H, Hkv, PS, False) for H, Hkv in HEADS
                          for PS in (32, 256)] + [(8, 2, 32, True)])
def test_verify_meets_fp64_reference(H, Hkv, PS, spike, ns):
    c = case(H, Hkv, PS, spike, VSEQS)
    out, lse = run(c, "split", oracle(H, Hkv, spike, VSEQS),
                   f"{H}/{Hkv} PS={PS} spike={spike} ns={ns}", num_splits=ns)
    if (H, PS) == (8, 32) and not spike:
        # max_q picks the row tile: T x 4 heads -> MT = 4, 2 x 4 -> MT = 1
        mo, ml = run(c, "split", num_splits=ns, max_q=2)
        assert torch.equal(out, mo) and torch.equal(lse, ml)


def test_generator_dh64_packed_and_chunked_against_fp32():
    """bf16 last-token logits against an fp32 CPU run at dh = 64: the packed
    and the chunked error at most twice that of prefill="sequence" (the rule
    of the D = 128 test; at dh = 64 the sequence path's attention is fp32
    torch math)."""
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=256,
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
    gpu = torch.device("cuda", 0)
    want = logits(torch.device("cpu"), torch.float32)
    e_seq = (logits(gpu, torch.bfloat16) - want).abs().max().item()
    e_pk = (logits(gpu, torch.bfloat16, prefill="packed") - want) \
        .abs().max().item()
    e_ch = (logits(gpu, torch.bfloat16, prefill="packed", prefill_chunk=64)
            - want).abs().max().item()
    print(f"e_seq {e_seq:.4e} e_packed {e_pk:.4e} e_chunked {e_ch:.4e}")
    assert e_pk <= 2 * e_seq and e_ch <= 2 * e_seq, (e_seq, e_pk, e_ch)
