#!/usr/bin/env python3
"""Fused MoE gate (moe.hip moe_gate_fwd / moe_gate_grad) against the kernels
it replaces and against its own torch branch.

Shape: bf16, N=16384 tokens, K=2, E in {16, 64, 256}, fixed seed.
  forward   fused: F.moe_gate (softmax + top-k + psum/cnt/aux/z)
            base:  F.softmax_fwd + ext().moe_topk (no loss statistics)
            torch: the torch branch of F.moe_gate ("moe" family forced)
  backward  fused: F.moe_gate_grad (g_probs, g_aux, g_z)
            base:  g_probs + coef * cnt (broadcast add) + F.softmax_bwd
            torch: the torch branch of F.moe_gate_grad
All sides run in this process on the same inputs, alternating round by
round; each round is a device-event window over `--iters` calls after a
warm-up of all.  The GB/s figures divide the [N, E] traffic a stage must
move (forward: read logits, write probs; backward: read logits and g_probs,
write dlogits) by the fused median.  Needs a GPU; prints one JSON line per E.

    python scripts/bench_moe_gate.py [--iters 10] [--rounds 7]
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

N, K, SEED = 16384, 2, 0
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


def bench(E, iters, rounds):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(SEED)
    bf = torch.bfloat16
    logits = torch.randn(N, E, generator=g).to(bf).to(dev)
    g_probs = torch.randn(N, E, generator=g).to(bf).to(dev)
    g_aux = torch.tensor(0.01, device=dev)
    g_z = torch.tensor(0.001, device=dev)
    out = F.moe_gate(logits, K)
    probs, lse, cnt = out[0], out[3], out[5]
    coef_cnt = (cnt.float() * (0.01 * E / (N * N))).to(bf)

    def fwd_fused():
        return F.moe_gate(logits, K)

    def fwd_base():
        p = F.softmax_fwd(logits)
        return p, F.ext().moe_topk(p, K)

    def bwd_fused():
        return F.moe_gate_grad(g_probs, g_aux, g_z, logits, lse, cnt)

    def bwd_base():
        return F.softmax_bwd(g_probs + coef_cnt, probs)

    units = {"fwd": {"fused": (fwd_fused, LIVE), "base": (fwd_base, LIVE),
                     "torch": (fwd_fused, FORCED)},
             "bwd": {"fused": (bwd_fused, LIVE), "base": (bwd_base, LIVE),
                     "torch": (bwd_fused, FORCED)}}
    for sides in units.values():
        for fn, fb in sides.values():
            window_ms(fn, 2, fb)
    times = {(u, s): [] for u, sides in units.items() for s in sides}
    for _ in range(rounds):                 # alternate the sides
        for u, sides in units.items():
            for s, (fn, fb) in sides.items():
                times[(u, s)].append(window_ms(fn, iters, fb))
    res = {"bench": "moe_gate", "N": N, "E": E, "K": K, "dtype": "bf16",
           "iters": iters, "rounds": rounds}
    for (u, s), ts in times.items():
        res[f"{u}_{s}_ms"] = {"median": round(statistics.median(ts), 4),
                              "min": round(min(ts), 4),
                              "max": round(max(ts), 4)}
    nbytes = {"fwd": 2 * N * E * 2, "bwd": 3 * N * E * 2}
    for u, b in nbytes.items():
        ms = statistics.median(times[(u, "fused")])
        res[f"{u}_fused_GBps"] = round(b / ms / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_gate: needs a GPU")
    assert hasattr(F.ext(), "moe_gate_fwd")
    for E in (16, 64, 256):
        print(json.dumps(bench(E, args.iters, args.rounds)), flush=True)


if __name__ == "__main__":
    main()
