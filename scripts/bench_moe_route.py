#!/usr/bin/env python3
"""MoE routing / dispatch / combine: the HIP kernels of moe.hip against the
torch composition they replaced (the same hetu_amd.ops.functional entry
points with the "moe" family forced to the torch branch, which is what the
graph ops ran before the kernels existed).

Shape: bf16, N=16384 tokens, h=4096, E=16 experts, K=2, capacity factor
1.25 (C=2560), fixed seed.  Expert GEMMs are not part of any unit.  Both
sides run in this process on the same inputs, alternating round by round;
each round is a device-event window over `--iters` calls after a warm-up of
both.  Needs a GPU; prints one JSON line.

    python scripts/bench_moe_route.py [--iters 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

N, H, E, K, CAP, SEED = 16384, 4096, 16, 2, 1.25, 0
C = max(1, int(CAP * K * N / E))
LIVE = F._TORCH_FB - {"moe"}
FORCED = F._TORCH_FB | {"moe"}


def window_ms(fn, iters, fb):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    F._TORCH_FB = fb
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    F._TORCH_FB = LIVE
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_route: needs a GPU")
    assert hasattr(F.ext(), "moe_assign_slots")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(SEED)
    bf = torch.bfloat16
    # gate output stand-in: every row is a permutation of (j+1)/136, which
    # sums to 1 and stays tie-free in bf16, so both sides must route alike;
    # 60 % of the tokens put their top value on experts 0..3, which
    # overfills those (drops in both rounds) and underfills the rest
    vals = (torch.arange(E, dtype=torch.float32) + 1) / (E * (E + 1) // 2)
    probs = vals[torch.rand(N, E, generator=g).argsort(-1)]
    rows = torch.nonzero(torch.rand(N, generator=g) < 0.6).squeeze(1)
    top = probs[rows].argmax(-1)
    tgt = torch.randint(0, 4, (rows.numel(),), generator=g)
    a, b = probs[rows, top].clone(), probs[rows, tgt].clone()
    probs[rows, top], probs[rows, tgt] = b, a
    probs = probs.to(bf).to(dev)
    x = torch.randn(N, H, generator=g).to(bf).to(dev)
    gy = torch.randn(N, H, generator=g).to(bf).to(dev)
    recv = torch.randn(E * C, H, generator=g).to(bf).to(dev)
    gsend = torch.randn(E * C, H, generator=g).to(bf).to(dev)
    g_w = torch.randn(N, K, generator=g).to(dev)

    F._TORCH_FB = FORCED
    ref_route = F.moe_route(probs, C, K)
    F._TORCH_FB = LIVE
    pos, slot_of, idx, wk = F.moe_route(probs, C, K)
    routing_equal = all(torch.equal(a, b) for a, b in
                        zip((pos, slot_of, idx, wk), ref_route))
    assert routing_equal, "the two sides route differently"
    dropped = int((slot_of < 0).sum())
    empty_slots = int((pos < 0).sum())

    def route():
        return F.moe_route(probs, C, K)

    def dispatch():
        return F.moe_dispatch_rows(x, pos)

    def combine():
        return F.moe_combine_rows(recv, wk, slot_of)

    def combine_bwd():
        return F.moe_combine_rows_bwd(gy, recv, wk, pos, slot_of)

    def dispatch_bwd():
        return (F.moe_dispatch_rows_bwd(gsend, pos, slot_of),
                F.moe_gate_bwd(g_w, slot_of, probs, C))

    def total():
        p, s, _, w = F.moe_route(probs, C, K)
        send = F.moe_dispatch_rows(x, p)
        y = F.moe_combine_rows(recv, w, s)
        d_recv, dwk = F.moe_combine_rows_bwd(gy, recv, w, p, s)
        dx = F.moe_dispatch_rows_bwd(gsend, p, s)
        dprobs = F.moe_gate_bwd(dwk, s, probs, C)
        return send, y, d_recv, dx, dprobs

    units = {"route": route, "dispatch": dispatch, "combine": combine,
             "combine_bwd": combine_bwd, "dispatch_bwd": dispatch_bwd,
             "total_fwd_bwd": total}
    sides = {"hip": LIVE, "composed": FORCED}
    for fn in units.values():
        for fb in sides.values():
            window_ms(fn, 2, fb)
    times = {(u, s): [] for u in units for s in sides}
    for _ in range(args.rounds):            # alternate the sides
        for u, fn in units.items():
            for s, fb in sides.items():
                times[(u, s)].append(window_ms(fn, args.iters, fb))
    res = {"bench": "moe_route", "N": N, "h": H, "E": E, "K": K, "C": C,
           "dtype": "bf16", "iters": args.iters, "rounds": args.rounds,
           "routing_equal": routing_equal, "dropped_choices": dropped,
           "empty_slots": empty_slots}
    for u in units:
        for s in sides:
            ts = times[(u, s)]
            res[f"{u}_{s}_ms"] = {"median": round(statistics.median(ts), 4),
                                  "min": round(min(ts), 4),
                                  "max": round(max(ts), 4)}
        res[f"{u}_composed_over_hip"] = round(
            statistics.median(times[(u, "composed")])
            / statistics.median(times[(u, "hip")]), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
