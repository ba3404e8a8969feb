#!/usr/bin/env python3
"""Weight-gradient GEMM dW = gy^T @ x: the hand kernel
(F.linear_wgrad(impl="hip") -> ops/hip/gemm_wgrad.hip) against hipBLASLt
(impl="blas" -> torch.matmul(gy.t(), x)) on the four GPT-3 7B layer shapes
at T = 32768 tokens.

Both sides run in this process on the same random-normal bf16 operands,
alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of both.  FLOPs are 2*T*N*K from the shapes.
Outputs are compared at the timed sizes: every element of the hand
kernel's result within one bf16 ulp of the library's, and its max error
against an fp64 reference at most 1.5x the library's ("numerics_ok").
A shape belongs on the hand kernel under impl="auto" only if its result is
right and its [min-max] range lies entirely below the library's
("hand_wins").  Needs a GPU; prints one JSON line per shape and exits
non-zero if any shape fails the output comparison.

    python scripts/bench_wgrad.py [--iters 10] [--rounds 7] [--tokens 32768]
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

# (N, K) of qkv, attention out-proj, fc and proj of GPT-3 7B (hidden 4096)
LAYER_SHAPES = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]
MFMA_PEAK = 2.5e15      # dense bf16 FLOP/s, MI355X


def window_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def ulp_key(t):
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, default=32768)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wgrad: needs a GPU")
    dev = torch.device("cuda", 0)
    T = args.tokens
    all_ok = True
    for si, (N, K) in enumerate(LAYER_SHAPES):
        g = torch.Generator().manual_seed(si)
        gy = torch.randn(T, N, generator=g).to(torch.bfloat16).to(dev)
        x = torch.randn(T, K, generator=g).to(torch.bfloat16).to(dev)
        sides = {"hand": lambda: F.linear_wgrad(gy, x, impl="hip"),
                 "blas": lambda: F.linear_wgrad(gy, x, impl="blas")}
        # same results first (also warms both sides up)
        hand, blas = sides["hand"](), sides["blas"]()
        ulps = (ulp_key(hand) - ulp_key(blas)).abs()
        ref = gy.double().t() @ x.double()
        err = {n: (o.double() - ref).abs().max().item()
               for n, o in (("hand", hand), ("blas", blas))}
        del ref
        numerics_ok = (int(ulps.max().item()) <= 1
                       and err["hand"] <= 1.5 * err["blas"])
        all_ok = all_ok and numerics_ok
        for fn in sides.values():
            window_ms(fn, 3)
        times = {n: [] for n in sides}
        for _ in range(args.rounds):            # alternate the sides
            for n, fn in sides.items():
                times[n].append(window_ms(fn, args.iters))
        flops = 2.0 * T * N * K
        res = {"bench": "wgrad", "T": T, "N": N, "K": K, "dtype": "bf16",
               "iters": args.iters, "rounds": args.rounds,
               "max_ulp_hand_vs_blas": int(ulps.max().item()),
               "frac_elements_differing": round(
                   (ulps > 0).float().mean().item(), 6),
               "max_err_vs_fp64": err, "numerics_ok": numerics_ok}
        for n, ts in times.items():
            med = statistics.median(ts)
            res[n + "_ms"] = {"median": round(med, 4),
                              "min": round(min(ts), 4),
                              "max": round(max(ts), 4)}
            res[n + "_pflops"] = round(flops / (med * 1e-3) / 1e15, 3)
            res[n + "_of_mfma_peak"] = round(
                flops / (med * 1e-3) / MFMA_PEAK, 3)
        res["hand_wins"] = (numerics_ok
                            and max(times["hand"]) < min(times["blas"]))
        res["blas_over_hand"] = round(statistics.median(times["blas"])
                                      / statistics.median(times["hand"]), 3)
        print(json.dumps(res), flush=True)
        del gy, x, hand, blas, ulps
    if not all_ok:
        sys.exit("bench_wgrad: hand kernel output outside the bounds")


if __name__ == "__main__":
    main()
