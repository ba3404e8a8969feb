"""Expert-parallel MoE ops: capacity-based dispatch / combine over RCCL a2a.

Reference parity: HetuMoE — v1/python/hetu/layers/moe_layer.py (top-k gate,
capacity dispatch), gpu_ops/AllToAll.py and HAllToAll.py (flat +
hierarchical a2a).  MI355X-native: static [E, C] routing buffers keep every
shape graph-static (hipGraph-capturable); the a2a rides RCCL over xGMI,
optionally hierarchical across nodes (HETU_AMD_MOE_NODE_SIZE).

Layouts (P = ep group size, E = total experts, El = E/P local experts,
C = per-(source rank, expert) capacity):
  dispatch:  x [N, h], probs [N, E] ->
    expert_in  [El, P*C, h]   (rows from every source rank)
    combine_w  [N, K] fp32    (gate weight per used slot; 0 if dropped)
    meta:      pos [E, C] int64 (token index per slot, -1 pad) — kept as a
               graph tensor so combine/grads replay the routing
  combine: expert_out [El, P*C, h], combine_w, pos -> y [N, h]

Routing and the row movement on either side of the a2a go through the
ops.functional moe_* entry points (moe.hip kernels on a GPU, the torch
composition on CPU).
"""
from __future__ import annotations

import os

import torch

from ...ops import functional as F
from ...parallel.dstates import DistributedStates
from ..op import OpInterface
from ..tensor import TensorMeta
from .basics import _g, _make
from .comm import _my_index, _ranks


def _ep_ranks(op, ctx):
    ranks = op.attrs.get("ep_ranks")
    if ranks is None or ctx.comm is None:
        return [0]
    return list(ranks)


def _node_size():
    return int(os.environ.get("HETU_AMD_MOE_NODE_SIZE", "0"))


def _a2a(comm, ranks, x):
    from ...parallel.moe import alltoall, hierarchical_alltoall
    ns = _node_size()
    if ns > 1:
        return hierarchical_alltoall(comm, ranks, x, ns)
    return alltoall(comm, ranks, x)


class MoEDispatchOp(OpInterface):
    """inputs: x [N, h], probs [N, E]; outputs: expert_in [El, P*C, h],
    combine_w [N, K] (differentiable wrt probs), pos [E, C], slot_of
    [N, K]."""
    type = "MoEDispatch"

    def infer_meta(self, attrs, inputs):
        x, probs = inputs
        E, C, K = attrs["experts"], attrs["capacity"], attrs["k"]
        P = len(attrs.get("ep_ranks") or [0])
        El = E // P
        return [TensorMeta([El, P * C, x.shape[-1]], x.dtype),
                TensorMeta([x.shape[0], K], torch.float32),
                TensorMeta([E, C], torch.int64),
                TensorMeta([x.shape[0], K], torch.int64)]

    def deduce_states(self, op):
        x = op.inputs[0]
        for t in op.outputs:
            t.device_group = x.device_group
        # expert_in is sharded over the ep group (local experts); the rest
        # mirror x's token layout / are per-rank routing state
        if x.ds is not None:
            for t in op.outputs:
                t.ds = DistributedStates(x.ds.device_num, {-1: x.ds.device_num}
                                         if x.ds.device_num > 1 else {})

    def compute(self, op, inputs, ctx):
        x, probs = inputs
        a = op.attrs
        E, C, K = a["experts"], a["capacity"], a["k"]
        ranks = _ep_ranks(op, ctx)
        P = len(ranks)
        El = E // P
        pos, slot_of, idx, wk = F.moe_route(probs, C, K)
        send = F.moe_dispatch_rows(x, pos)
        if P > 1:
            # [E*C, h] = [P, El*C, h] blocks by destination rank
            recv = _a2a(ctx.comm, ranks, send)
            expert_in = recv.reshape(P, El, C, -1).transpose(0, 1) \
                .reshape(El, P * C, -1).contiguous()
        else:
            expert_in = send.reshape(El, C, -1)
            expert_in = expert_in.reshape(El, P * C, -1)
        return [expert_in, wk, pos, slot_of]

    def gradient(self, op, g):
        gr = _g(op.outputs[0])
        g_exp = g[0]
        g_w = g[1]
        grads = _make(gr, MoEDispatchGradOp(),
                      [t for t in [g_exp, g_w, op.outputs[2], op.outputs[3],
                                   op.inputs[0], op.inputs[1]]
                       if t is not None],
                      dict(op.attrs), name="moe_dispatch_grad")
        return [grads.output(0), grads.output(1)]


class MoEDispatchGradOp(OpInterface):
    """inputs: g_expert_in (may be zeros), g_combine_w, pos, slot_of, x,
    probs -> dx [N, h], dprobs [N, E]."""
    type = "MoEDispatchGrad"

    def infer_meta(self, attrs, inputs):
        x, probs = inputs[4], inputs[5]
        return [TensorMeta(x.shape, x.dtype),
                TensorMeta(probs.shape, probs.dtype)]

    def compute(self, op, inputs, ctx):
        g_exp, g_w, pos, slot_of, x, probs = inputs
        a = op.attrs
        E, C, K = a["experts"], a["capacity"], a["k"]
        ranks = _ep_ranks(op, ctx)
        P = len(ranks)
        El = E // P
        # reverse the a2a: expert_in grads back to source layout [E*C, h]
        if P > 1:
            back = g_exp.reshape(El, P, C, -1).transpose(0, 1) \
                .reshape(P * El * C, -1).contiguous()
            gsend = _a2a(ctx.comm, ranks, back)
        else:
            gsend = g_exp.reshape(E * C, -1)
        dx = F.moe_dispatch_rows_bwd(gsend.to(x.dtype), pos, slot_of)
        if g_w is not None:
            dprobs = F.moe_gate_bwd(g_w, slot_of, probs, C)
        else:
            dprobs = torch.zeros_like(probs)
        return [dx, dprobs]


class MoECombineOp(OpInterface):
    """inputs: expert_out [El, P*C, h], combine_w [N, K], pos [E, C],
    slot_of [N, K] -> y [N, h]."""
    type = "MoECombine"

    def infer_meta(self, attrs, inputs):
        eo, wk = inputs[0], inputs[1]
        return [TensorMeta([wk.shape[0], eo.shape[-1]], eo.dtype)]

    def deduce_states(self, op):
        src = op.attrs.get("out_ds")
        op.outputs[0].ds = src
        op.outputs[0].device_group = op.inputs[0].device_group

    @staticmethod
    def _gather_back(eo, pos, ranks, ctx, E, C, P, El):
        if P > 1:
            back = eo.reshape(El, P, C, -1).transpose(0, 1) \
                .reshape(P * El * C, -1).contiguous()
            recv = _a2a(ctx.comm, ranks, back)
        else:
            recv = eo.reshape(E * C, -1)
        return recv      # [E*C, h] rows in send-slot order

    def compute(self, op, inputs, ctx):
        eo, wk, pos, slot_of = inputs
        a = op.attrs
        E, C, K = a["experts"], a["capacity"], a["k"]
        ranks = _ep_ranks(op, ctx)
        P = len(ranks)
        El = E // P
        recv = self._gather_back(eo, pos, ranks, ctx, E, C, P, El)
        return [F.moe_combine_rows(recv, wk, slot_of)]

    def gradient(self, op, g):
        gr = _g(op.outputs[0])
        bwd = _make(gr, MoECombineGradOp(),
                    [g[0], op.inputs[0], op.inputs[1], op.inputs[2],
                     op.inputs[3]], dict(op.attrs), name="moe_combine_grad")
        return [bwd.output(0), bwd.output(1), None, None]


class MoECombineGradOp(OpInterface):
    """inputs: gy [N, h], expert_out, combine_w, pos, slot_of ->
    d_expert_out [El, P*C, h], d_combine_w [N, K]."""
    type = "MoECombineGrad"

    def infer_meta(self, attrs, inputs):
        eo, wk = inputs[1], inputs[2]
        return [TensorMeta(eo.shape, eo.dtype),
                TensorMeta(wk.shape, wk.dtype)]

    def compute(self, op, inputs, ctx):
        gy, eo, wk, pos, slot_of = inputs
        a = op.attrs
        E, C, K = a["experts"], a["capacity"], a["k"]
        ranks = _ep_ranks(op, ctx)
        P = len(ranks)
        El = E // P
        recv = MoECombineOp._gather_back(eo, pos, ranks, ctx, E, C, P, El)
        d_recv, dwk = F.moe_combine_rows_bwd(gy, recv, wk, pos, slot_of)
        # forward a2a of d_recv to expert layout
        if P > 1:
            recv2 = _a2a(ctx.comm, ranks, d_recv)
            d_eo = recv2.reshape(P, El, C, -1).transpose(0, 1) \
                .reshape(El, P * C, -1).contiguous()
        else:
            d_eo = d_recv.reshape(El, P * C, -1)
        return [d_eo, dwk]


class MoEGateOp(OpInterface):
    """Fused learned gate: logits [N, E] -> probs [N, E] (softmax, logits'
    dtype), aux [] fp32 (load-balance loss), z [] fp32 (router z-loss), and
    the saved lse [N] fp32, cnt [E] int32 (see ops.functional.moe_gate for
    the definitions).  MoEDispatchOp keeps routing from probs; its top-k is
    the one cnt counts."""
    type = "MoEGate"

    def infer_meta(self, attrs, inputs):
        lg = inputs[0]
        N, E = lg.shape
        return [TensorMeta([N, E], lg.dtype),
                TensorMeta([], torch.float32),
                TensorMeta([], torch.float32),
                TensorMeta([N], torch.float32),
                TensorMeta([E], torch.int32)]

    def deduce_states(self, op):
        lg = op.inputs[0]
        for t in op.outputs:
            t.device_group = lg.device_group
        src = lg.ds
        if src is None:
            return
        if src.partial > 1 or src.get_dim(1) > 1:
            raise ValueError(
                f"moe_gate: logits must be whole rows of tokens, got {src}")
        probs, aux, z, lse, cnt = op.outputs
        probs.ds = lse.ds = src
        # statistics are per rank over the rank's own tokens: the token
        # split (dim 0) becomes a partial, i.e. the global value is the sum
        # over ranks; a duplicate factor stays a duplicate
        states = {(-2 if d == 0 else d): n for d, n in src.states.items()}
        order = [(-2 if d == 0 else d) for d in src.order]
        aux.ds = z.ds = cnt.ds = DistributedStates(src.device_num, states,
                                                   order)

    def compute(self, op, inputs, ctx):
        probs, _, _, lse, _, cnt, aux, z = F.moe_gate(inputs[0],
                                                      op.attrs["k"])
        return [probs, aux, z, lse, cnt]

    def gradient(self, op, g):
        ups = list(g[:3])
        if all(u is None for u in ups):
            return [None]
        gr = _g(op.outputs[0])
        attrs = dict(op.attrs)
        attrs["has"] = [u is not None for u in ups]
        bwd = _make(gr, MoEGateGradOp(),
                    [u for u in ups if u is not None]
                    + [op.inputs[0], op.outputs[3], op.outputs[4]],
                    attrs, name="moe_gate_grad")
        return [bwd.output()]


class MoEGateGradOp(OpInterface):
    """inputs: the present ones of (g_probs, g_aux, g_z) as flagged by
    attrs["has"], then logits, lse, cnt -> dlogits [N, E]."""
    type = "MoEGateGrad"

    def infer_meta(self, attrs, inputs):
        lg = inputs[-3]
        return [TensorMeta(lg.shape, lg.dtype)]

    def deduce_states(self, op):
        lg = op.inputs[-3]
        op.outputs[0].ds = lg.ds
        op.outputs[0].device_group = lg.device_group

    def compute(self, op, inputs, ctx):
        it = iter(inputs[:-3])
        g_probs, g_aux, g_z = [next(it) if h else None
                               for h in op.attrs["has"]]
        logits, lse, cnt = inputs[-3:]
        return [F.moe_gate_grad(g_probs, g_aux, g_z, logits, lse, cnt)]
