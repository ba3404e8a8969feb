#!/usr/bin/env python3
"""GPT-MoE training with expert parallelism + hierarchical all-to-all
(reference HetuMoE examples).

Run: python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 \
       --master-addr 127.0.0.1 examples/moe/train_moe.py
Set HETU_AMD_MOE_NODE_SIZE to enable the 3-phase hierarchical a2a.

--aux-coef A / --z-coef Z add A * (load-balance loss) + Z * (router z-loss)
to the training loss (the fused gate, ht.moe_gate) and print both with the
largest expert's share of this rank's token choices every 10 steps.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))
import torch  # noqa: E402

from hetu_amd.engine.runner import prepare_run_context  # noqa: E402
from hetu_amd.graph.graph import (DefineAndRunGraph, pop_graph,  # noqa
                                  push_graph)
from hetu_amd.graph.ops import api as ht  # noqa: E402
from hetu_amd.graph.ops.optim import Adam  # noqa: E402
from hetu_amd.nn.moe import MoEMLP  # noqa: E402
from hetu_amd.nn.parallel import ParallelSpec  # noqa: E402
from hetu_amd.parallel.comm import comm_backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aux-coef", type=float, default=0.0)
    ap.add_argument("--z-coef", type=float, default=0.0)
    args = ap.parse_args()
    gate_losses = bool(args.aux_coef or args.z_coef)
    comm = comm_backend()
    device = comm.device
    spec = ParallelSpec(dp=comm.world_size) if comm.world_size > 1 else None
    N, H, F, E = 512, 256, 1024, 8
    g = DefineAndRunGraph("moe")
    push_graph(g)
    try:
        x = ht.placeholder((N, H), name="x",
                           ds=spec.ds_tokens(0) if spec else None,
                           device_group=spec.device_group if spec else None)
        tgt = ht.placeholder((N, H), name="tgt",
                             ds=spec.ds_tokens(0) if spec else None,
                             device_group=spec.device_group if spec else None)
        moe = MoEMLP(H, F, E, spec=spec, k=2, gate_type="topk",
                     aux_loss_coef=args.aux_coef, z_loss_coef=args.z_coef)
        loss = ht.mse_loss(moe(x), tgt)
        fetches = []
        if gate_losses:
            # this rank's statistics over its own tokens
            fetches = [moe.aux_loss, moe.z_loss, moe.gate_counts]
            # add_n: the per-rank scalars are partial sums under a token
            # split, which the n-ary sum accepts
            loss = ht.add_n([loss] + [ht.mul(t, coef) for coef, t in
                                      ((args.aux_coef, moe.aux_loss),
                                       (args.z_coef, moe.z_loss)) if coef])
        train_op = Adam(lr=1e-3).minimize(loss)
    finally:
        pop_graph()
    ctx = prepare_run_context(g, device)
    torch.manual_seed(3 + comm.rank)
    for step in range(30):
        xd = torch.randn(N, H, device=device)
        td = torch.randn(N, H, device=device)
        lv, _, *gl = g.run([loss, train_op] + fetches, {x: xd, tgt: td},
                           ctx=ctx)
        if comm.rank == 0 and step % 10 == 0:
            line = f"step {step} loss {float(lv):.4f}"
            if gate_losses:
                share = float(gl[2].max()) / float(gl[2].sum())
                line += (f" aux {float(gl[0]):.4f} z {float(gl[1]):.4f}"
                         f" max expert share {share:.4f}")
            print(line)


if __name__ == "__main__":
    main()
