#!/usr/bin/env python3
"""Weight + bias gradient of a Linear: the fused kernel
(F.linear_wgrad_bias(impl="hip") -> the bias variant in
ops/hip/gemm_wgrad.hip) against the unfused pair it replaces
(F.linear_wgrad(impl="hip") + F.colsum), on the four GPT-3 7B layer shapes
at T = 32768 and 8192 tokens.  Also the GEMM alone with and without the
bias variant ("kernel_bias" against "kernel_plain"): what the tk == 0
blocks' 17th MFMA per phase costs per grid.

All four sides run in this process on the same random-normal bf16 operands,
alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of every side.  Outputs are compared at the
timed sizes: dW bit-equal to the plain kernel's, db within
2^-8 |ref| + (T/32 + 8) 2^-24 sum|gy| of the fp64 column sums per column
("numerics_ok").  The fused side belongs under impl="auto" only if its
result is right and its [min-max] range lies entirely below the unfused
pair's ("fused_wins").  Needs a GPU; prints one JSON line per shape and
exits non-zero if a shape fails the output comparison or a shape that
F._wgrad_bias_auto_fused admits does not win.

    python scripts/bench_wgrad_bias.py [--iters 10] [--rounds 7]
                                       [--tokens 32768 8192]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", type=int, nargs="+", default=[32768, 8192])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wgrad_bias: needs a GPU")
    dev = torch.device("cuda", 0)
    ext = F.ext()
    failed = []
    for T in args.tokens:
        for si, (N, K) in enumerate(LAYER_SHAPES):
            g = torch.Generator().manual_seed(si)
            gy = torch.randn(T, N, generator=g).to(torch.bfloat16).to(dev)
            x = torch.randn(T, K, generator=g).to(torch.bfloat16).to(dev)

            def unfused():
                return (F.linear_wgrad(gy, x, impl="hip"),
                        F.colsum(gy).to(gy.dtype))
            sides = {
                "fused": lambda: F.linear_wgrad_bias(gy, x, impl="hip"),
                "unfused": unfused,
                "kernel_bias": lambda: ext.gemm_wgrad_bias_bf16(gy, x),
                "kernel_plain": lambda: ext.gemm_wgrad_bf16(gy, x),
            }
            # same results first (also warms the sides up)
            dw_f, db_f = sides["fused"]()
            dw_u, db_u = sides["unfused"]()
            ref = gy.double().sum(0)
            bound = 2.0 ** -8 * ref.abs() + \
                (T / 32 + 8) * 2.0 ** -24 * gy.double().abs().sum(0)
            err_f = (db_f.double() - ref).abs()
            err_u = (db_u.double() - ref).abs()
            dw_equal = bool(torch.equal(dw_f, dw_u))
            numerics_ok = dw_equal and bool((err_f <= bound).all())
            for fn in sides.values():
                window_ms(fn, 3)
            times = {n: [] for n in sides}
            for _ in range(args.rounds):            # alternate the sides
                for n, fn in sides.items():
                    times[n].append(window_ms(fn, args.iters))
            res = {"bench": "wgrad_bias", "T": T, "N": N, "K": K,
                   "tiles": (N // 256) * (K // 256), "dtype": "bf16",
                   "iters": args.iters, "rounds": args.rounds,
                   "dw_bit_equal": dw_equal,
                   "db_max_err_over_bound": {
                       "fused": round((err_f / bound).max().item(), 4),
                       "unfused": round((err_u / bound).max().item(), 4)},
                   "db_elements_differing": int((db_f != db_u).sum().item()),
                   "numerics_ok": numerics_ok}
            for n, ts in times.items():
                res[n + "_ms"] = {"median": round(statistics.median(ts), 4),
                                  "min": round(min(ts), 4),
                                  "max": round(max(ts), 4)}
            med = {n: statistics.median(ts) for n, ts in times.items()}
            res["fused_wins"] = (numerics_ok and
                                 max(times["fused"]) < min(times["unfused"]))
            res["unfused_over_fused"] = round(med["unfused"] / med["fused"], 4)
            res["saved_us"] = round((med["unfused"] - med["fused"]) * 1e3, 1)
            res["bias_blocks_cost_us"] = round(
                (med["kernel_bias"] - med["kernel_plain"]) * 1e3, 1)
            res["kernel_bias_over_plain"] = round(
                med["kernel_bias"] / med["kernel_plain"], 4)
            res["auto_fuses"] = F._wgrad_bias_auto_fused(T, N, K, "1")
            print(json.dumps(res), flush=True)
            if not numerics_ok or (res["auto_fuses"]
                                   and not res["fused_wins"]):
                failed.append((T, N, K))
            del gy, x, dw_f, dw_u, db_f, db_u, ref, bound
    if failed:
        sys.exit(f"bench_wgrad_bias: wrong output or no win on {failed}")


if __name__ == "__main__":
    main()
