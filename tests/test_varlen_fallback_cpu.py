"""CPU side of the packed-varlen backward contract: the per-segment
fallback returns zeros for rows of no segment, and the max_seqlen hint
reaches both graph ops."""
import torch

import hetu_amd.ops.functional as F


def test_fallback_zeroes_uncovered_rows_and_takes_max_seqlen():
    torch.manual_seed(0)
    T, H, D = 40, 2, 16
    cu = torch.tensor([0, 9, 9, 30], dtype=torch.int32)     # tail of 10
    q, k, v, do = (torch.randn(T, H, D) for _ in range(4))
    o, lse = F.varlen_attention_fwd(q, k, v, cu, True, max_seqlen=21)
    grads = F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True,
                                   max_seqlen=21)
    hinted = [g.clone() for g in grads]
    # fill the allocator's free blocks with garbage, then run again: an
    # uninitialised allocation would now show it in the tail rows
    junk = [torch.full((T, H, D), float("nan")) for _ in range(8)]
    del junk
    grads = F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True)
    for g, h in zip(grads, hinted):
        assert torch.count_nonzero(g[30:]).item() == 0
        assert torch.isfinite(g).all()
        assert torch.equal(g, h)
        assert g[:30].abs().max().item() > 0


def test_max_seqlen_attr_reaches_forward_and_grad_op():
    from hetu_amd.graph.graph import (DefineAndRunGraph, pop_graph,
                                      push_graph)
    from hetu_amd.graph.ops import api as ht
    g = DefineAndRunGraph("vl_hint")
    push_graph(g)
    try:
        q = ht.placeholder((8, 2, 16), name="q")
        k = ht.placeholder((8, 2, 16), name="k")
        v = ht.placeholder((8, 2, 16), name="v")
        c = ht.placeholder((3,), dtype=torch.int32, name="cu")
        o = ht.varlen_attention(q, k, v, c, max_seqlen=5)
        ht.gradients([ht.reduce_sum(o)], [q, k, v])
    finally:
        pop_graph()
    hints = {op.type: op.attrs.get("max_seqlen") for op in g.ops
             if op.type in ("VarlenAttention", "VarlenAttentionGrad")}
    assert hints == {"VarlenAttention": 5, "VarlenAttentionGrad": 5}
