"""GPU tests of fp8 page pools: the PAGED kernel of attention_decode_fp8.hip
and the quantizing paged append of kv_cache_fp8.hip through F.  Bit-identical
to the dense fp8 kernel on the same values; decode_attn_oracle.py's own bounds
against fp64 on the dequantized values.  Pools: test_decode_paged_fp8_cpu's
scatter (0x7F bytes and NaN scales wherever a kernel must not read)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import decode_fp8_cases as C  # noqa: E402
from test_decode_paged_fp8_cpu import raw, scatter  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3


def dev():
    return torch.device("cuda", 0)


def cache_len():
    """2 T + 64 rounded up to a multiple of 256, so that every PS divides."""
    return -(-(2 * int(F.ext().decode_attn_fp8_tile()) + 64) // 256) * 256


def length_rows(PS):
    t, L = int(F.ext().decode_attn_fp8_tile()), cache_len()
    return [(0, 1, 31), (32, 33, PS - 1), (PS, PS + 1, t - 1), (t, t + 1, L)]


def dec(q, k, ks, v, vs, n, ns, table=None, impl="hip"):
    return F.flash_attn_decode(q, k, v, n, num_splits=ns, impl=impl,
                               k_scale=ks, v_scale=vs, block_table=table)


@functools.lru_cache(maxsize=None)
def case(D, H, Hkv, PS, row):
    """Device q, dense caches, pools, table, kv_len and the oracle's result;
    never modified."""
    lens = length_rows(PS)[row]
    ins = C.make_fp8_inputs(B, H, Hkv, cache_len(), D, seed=D + H + row)
    ref = DO.decode_ref(ins[0], C.dequant(ins[1], ins[2]),
                        C.dequant(ins[3], ins[4]), torch.tensor(lens))
    pools, table, _ = scatter(ins[1:], PS, lens, PS + row, dev())
    n = torch.tensor(lens, dtype=torch.int32, device=dev())
    return [x.to(dev()) for x in ins], pools, table, n, ref


@pytest.mark.parametrize("ns", [0, 1, 3])
@pytest.mark.parametrize("PS", [32, 64, 256])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (20, 4), (40, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_is_bit_identical_to_dense_and_meets_oracle(D, H, Hkv, PS, ns):
    for row in range(4):
        ins, (kp, ksp, vp, vsp), table, n, ref = case(D, H, Hkv, PS, row)
        out, lse = dec(ins[0], kp, ksp, vp, vsp, n, ns, table)
        do, dl = dec(*ins, n, ns)
        what = f"D={D} {H}/{Hkv} PS={PS} ns={ns} row {row}"
        DO.check(out, lse, ref, what)
        assert torch.equal(out, do) and torch.equal(lse, dl), what


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("PS", [32, 256])
def test_out_of_range_page_is_a_page_of_masked_keys(PS, ns):
    """Entry 0 of row 2 (kv_len = L) is P: out of range, inside the NaN
    allocation.  At PS = 256, ns = 3 the first split owns no other key."""
    L = cache_len()
    ins, (kp, ksp, vp, vsp), table, n, _ = case(128, 20, 4, PS, 3)
    table = table.clone()
    table[2, 0] = kp.shape[0]
    q = ins[0]
    out, lse = dec(q, kp, ksp, vp, vsp, n, ns, table)
    kd, vd = C.dequant(ins[1], ins[2]), C.dequant(ins[3], ins[4])
    head = DO.decode_ref(q[:2], kd[:2], vd[:2], n[:2])
    tail = DO.decode_ref(q[2:], kd[2:, :, PS:], vd[2:, :, PS:], L - PS)
    DO.check(out, lse, tuple(torch.cat([a, b]) for a, b in zip(head, tail)),
             f"PS={PS} ns={ns}")


def gathered(pool, table):
    """Pool [P', Hkv, PS(, D)] -> dense [B, Hkv, MP * PS(, D)] by the table."""
    x = pool[table.long()]                       # [B, MP, Hkv, PS(, D)]
    return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1, *x.shape[4:])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
def test_append_against_the_definition(S, D):
    """Rows at 0, before 0, across a page edge, at MP * PS - 1, past it, and
    behind an out-of-range id (check_append gets an end that drops those)."""
    H, Hkv, PS, MP, P = 4, 2, 32, 3, 10
    L = MP * PS
    table = torch.randperm(P, generator=torch.Generator().manual_seed(S + D)) \
        [:B * MP].view(B, MP).to(torch.int32).to(dev())
    table[2, 1] = P
    for i, end in enumerate(([S, PS + 2, L], [2, L + 2, PS + 6])):
        kd, vd = C.append_inputs(B, S, H, Hkv, D, D + S + i, dev())
        # layer 1 of 5-D allocations, P + 1 pages each
        before = [torch.full((2, P + 1, Hkv, PS, D), 0x55, dtype=torch.uint8,
                             device=dev()).view(C.FP8)] * 2 \
            + [torch.full((2, P + 1, Hkv, PS), 7.0, device=dev())] * 2
        big, want = ([x.clone() for x in before] for _ in range(2))
        e = torch.tensor(end, dtype=torch.int32, device=dev())
        for pools, impl in ((big, "hip"), (want, "torch")):
            kp, vp, ksp, vsp = [x[1, :P] for x in pools]
            F.kv_cache_append_paged(kd, vd, kp, vp, table, e, impl=impl,
                                    k_scale=ksp, v_scale=vsp)
        for got, w in zip(big, want):            # codes and scales: torch's
            assert torch.equal(raw(got), raw(w))
        landed = end[:2] + [end[2] if i == 0 else -S]
        for x, c, s in ((kd, 0, 2), (vd, 1, 3)):
            C.check_append(x, gathered(big[c][1], table),
                           gathered(big[s][1], table),
                           (gathered(before[c][1], table),
                            gathered(before[s][1], table)), landed,
                           f"side {c} D{D} S{S} end{end}")
        # layer 0, the page nobody owns and the page past the view
        free = [p for p in range(P + 1) if p not in table[table < P].tolist()]
        for got, b4 in zip(big, before):
            assert torch.equal(raw(got)[0], raw(b4)[0])
            assert torch.equal(raw(got)[1, free], raw(b4)[1, free])


def test_capture_append_and_decode():
    D, H, Hkv, PS, MP = 128, 20, 4, 32, 4
    ins = C.make_fp8_inputs(B, H, Hkv, MP * PS, D, seed=9)
    (kp, ksp, vp, vsp), table, _ = scatter(ins[1:], PS, [MP * PS] * B, 9,
                                           dev())
    q = ins[0].to(dev())
    g = torch.Generator().manual_seed(9)
    k_new = torch.randn(B, 1, Hkv, D, generator=g).bfloat16().to(dev())
    v_new = torch.randn(B, 1, Hkv, D, generator=g).bfloat16().to(dev())
    kv_len = torch.tensor([30, 62, 100], dtype=torch.int32, device=dev())

    def step():
        F.kv_cache_append_paged(k_new, v_new, kp, vp, table, kv_len,
                                impl="hip", k_scale=ksp, v_scale=vsp)
        return dec(q, kp, ksp, vp, vsp, kv_len, 0, table)
    step()                                # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = step()
    for i in range(3):                    # 32 / 64 open a new page at i = 1
        kv_len.add_(1)
        if i:
            table.copy_(table[[1, 0, 2]])     # rows 0 and 1 trade pages
        graph.replay()
        kd, vd = [C.dequant(gathered(c, table), gathered(s, table))
                  for c, s in ((kp, ksp), (vp, vsp))]
        DO.check(out, lse, DO.decode_ref(q, kd, vd, kv_len), f"replay {i}")
        eo, el = step()
        assert torch.equal(out, eo) and torch.equal(lse, el), f"replay {i}"


def test_errors_name_the_argument():       # cu_q + fp8: the CPU file
    ins, (kp, ksp, vp, vsp), table, n, ref = case(64, 4, 4, 32, 2)
    q = ins[0]
    with pytest.raises(RuntimeError, match="k_scale has shape"):
        dec(q, kp, ksp[:, :, :31], vp, vsp, n, 0, table)
    with pytest.raises(RuntimeError, match="block_table with an fp8 cache "
                       "needs k_scale and v_scale"):
        dec(q, kp, None, vp, vsp, n, 0, table)
    with pytest.raises(RuntimeError, match="block_table is torch.int64"):
        dec(q, kp, ksp, vp, vsp, n, 0, table.long())
    # auto, "hip" and "mfma" are the one kernel
    outs = [dec(q, kp, ksp, vp, vsp, n, 0, table, impl)
            for impl in (None, "hip", "mfma")]
    assert all(torch.equal(o[0], outs[0][0]) for o in outs)
    DO.check(*outs[0], ref)


def test_llama_generator_paged_fp8_hip_vs_torch():
    """Teacher-forced; test_llama_generator_fp8_hip_vs_torch's config and
    rtol = atol = 6e-2.  Prompts of 5 and 29 tokens, PS = 32: one crosses."""
    from hetu_amd.engine.generator import LlamaGenerator, PagedKVCache
    from hetu_amd.models.llama import LlamaConfig
    cfg = LlamaConfig(n_layer=2, n_head=16, n_kv_head=2, hidden=1024,
                      ffn_hidden=256, vocab=301, max_seq=64)
    state = DO.llama_state(cfg, 256)
    lens, steps = (5, 29), 6
    ids = torch.randint(0, cfg.vocab, (2, max(lens) + steps),
                        generator=torch.Generator().manual_seed(1)).to(dev())
    logits = []
    for impl in (None, "torch"):
        g = LlamaGenerator(cfg, state, device=dev(), dtype=torch.bfloat16,
                           decode_impl=impl, kv_layout="paged", page_size=32,
                           kv_dtype="fp8")
        cache = PagedKVCache(cfg, [n + steps for n in lens], 32, dev(),
                             torch.bfloat16, kv_dtype="fp8")
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        with torch.no_grad():
            got = [torch.cat([g._forward(ids[b:b + 1, :n], cache.row(b), 0)
                              for b, n in enumerate(lens)])]
            for s in range(steps):
                tok = torch.stack([ids[b, n + s] for b, n in enumerate(lens)])
                cache.kv_len.add_(1)
                got.append(g._forward(tok.view(2, 1), cache, None))
        logits.append(torch.stack(got).float().cpu())
    assert torch.isfinite(logits[0]).all() and cache.k.dtype == C.FP8
    err = (logits[0] - logits[1]).abs().amax(dim=(1, 2))
    assert torch.allclose(logits[0], logits[1], rtol=6e-2, atol=6e-2), \
        f"max abs err per step {err.tolist()}"
