#!/usr/bin/env python3
"""Input-gradient GEMM dx = gy @ W: the transposed-copy route
(F.linear_dgrad(impl="transposed") -> ops/hip/transpose.hip, then the
forward's TN form F.linear(gy, Wt)) against hipBLASLt's NN form
(impl="blas" -> torch.matmul(gy, W)) on the four GPT-3 7B layer shapes at
T = 32768 .. 2048 tokens, and on the LM head at T = 32768.

Both sides run in this process on the same random-normal bf16 operands,
alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of both.  The transposed side times
transpose + GEMM together; the transpose alone is timed as well, next to a
contiguous copy_ of the same tensor (the bandwidth yardstick), for the
kernel's default block order (along input rows) and for order 0 (along
output rows).  FLOPs are 2*T*N*K, bytes 2 * 2*N*K.
A shape belongs on the transposed route under impl="auto" only if its
[min-max] range lies entirely below the library's ("transposed_wins").
Needs a GPU; prints one JSON line per row and exits non-zero if a row that
F._dgrad_auto_transposed routes to the transposed side does not win, or if
the two sides' outputs differ by more than the bound of tests/test_dgrad_gpu.

    python scripts/bench_dgrad.py [--iters 10] [--rounds 7]
                                  [--tokens 32768,16384,8192,4096,2048]
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

# (N, K) = (out, in features) of qkv, attention out-proj, fc and proj of
# GPT-3 7B (hidden 4096); dgrad contracts over N
LAYER_SHAPES = [(12288, 4096), (4096, 4096), (16384, 4096), (4096, 16384)]
LM_HEAD = (50304, 4096)


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


def stats(ts):
    return {"median": round(statistics.median(ts), 4),
            "min": round(min(ts), 4), "max": round(max(ts), 4)}


def run_row(T, N, K, seed, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    gy = torch.randn(T, N, generator=g, device=dev).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g, device=dev).to(torch.bfloat16)
    wt_buf = torch.empty(K, N, dtype=w.dtype, device=dev)
    cp_buf = torch.empty_like(w)
    sides = {
        "transposed": lambda: F.linear_dgrad(gy, w, impl="transposed"),
        "blas": lambda: F.linear_dgrad(gy, w, impl="blas"),
        "transpose_only": lambda: F.ext().transpose2d(w, wt_buf),
        "transpose_only_order0": lambda: F.ext().transpose2d(w, wt_buf, 0),
        "copy_only": lambda: cp_buf.copy_(w),
    }
    # outputs first (also warms both sides up): both accumulate in fp32 and
    # round once, so against fp64 the errors are within 1.5x of each other
    tr, bl = sides["transposed"](), sides["blas"]()
    rows = slice(0, min(T, 1024))          # bound the fp64 reference's size
    ref = gy[rows].double() @ w.double()
    err = {n: (o[rows].double() - ref).abs().max().item()
           for n, o in (("transposed", tr), ("blas", bl))}
    del ref
    numerics_ok = err["transposed"] <= 1.5 * err["blas"]
    frac_diff = (tr != bl).float().mean().item()
    for fn in sides.values():
        window_ms(fn, 3)
    times = {n: [] for n in sides}
    for _ in range(rounds):                # alternate the sides
        for n, fn in sides.items():
            times[n].append(window_ms(fn, iters))
    flops = 2.0 * T * N * K
    nbytes = 4.0 * N * K                   # read + write of 2-byte elements
    res = {"bench": "dgrad", "T": T, "N": N, "K": K, "dtype": "bf16",
           "iters": iters, "rounds": rounds, "max_err_vs_fp64": err,
           "frac_elements_differing": round(frac_diff, 6),
           "numerics_ok": numerics_ok}
    for n, ts in times.items():
        res[n + "_ms"] = stats(ts)
    for n in ("transposed", "blas"):
        res[n + "_pflops"] = round(
            flops / (statistics.median(times[n]) * 1e-3) / 1e15, 3)
    for n in ("transpose_only", "transpose_only_order0", "copy_only"):
        res[n + "_tbps"] = round(
            nbytes / (statistics.median(times[n]) * 1e-3) / 1e12, 3)
    res["transpose_over_copy"] = round(
        statistics.median(times["transpose_only"])
        / statistics.median(times["copy_only"]), 3)
    res["transposed_wins"] = (numerics_ok and max(times["transposed"])
                              < min(times["blas"]))
    res["blas_over_transposed"] = round(
        statistics.median(times["blas"])
        / statistics.median(times["transposed"]), 3)
    res["auto_routes_transposed"] = F._dgrad_auto_transposed(T, N, K)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", default="32768,16384,8192,4096,2048")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dgrad: needs a GPU")
    dev = torch.device("cuda", 0)
    tokens = [int(t) for t in args.tokens.split(",")]
    rows = [(T, N, K) for T in tokens for (N, K) in LAYER_SHAPES]
    rows.append((32768,) + LM_HEAD)
    bad = []
    for i, (T, N, K) in enumerate(rows):
        res = run_row(T, N, K, i, args.iters, args.rounds, dev)
        if not res["numerics_ok"]:
            bad.append(f"T={T} N={N} K={K}: output outside the bounds")
        if res["auto_routes_transposed"] and not res["transposed_wins"]:
            bad.append(f"T={T} N={N} K={K}: auto routes it to the transposed "
                       "side, whose range is not below the library's")
    if bad:
        sys.exit("bench_dgrad: " + "; ".join(bad))


if __name__ == "__main__":
    main()
