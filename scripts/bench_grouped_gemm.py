#!/usr/bin/env python3
"""Grouped expert GEMMs (ops/hip/gemm_grouped.hip and the batched entry of
gemm_wgrad.hip) against what the expert block runs today: torch.matmul on
the padded [E, C, h] buffers for the forward, and BatchMatMulTNOp's
transposing copy + torch.matmul for the two gradients.

Shapes (bf16, one rank, so P = 1 and seg = C):
  8x13   h=2048 f=8192  E=8  C=5120   (examples/moe/train_moe_8x13.py at
                                        N=16384 tokens, k=2, capacity 1.25)
  route  h=4096 f=16384 E=16 C=2560   (scripts/bench_moe_route.py's routing)
each at a balanced fill (every expert 0.8 C slots) and at the skewed fill
that F.moe_route gives on bench_moe_route's skewed gate output.  Empty slot
rows hold zeros on both sides, as dispatch leaves them, so the outputs are
comparable as they are; every timed row is checked against the library.

Units: the three forms on the first GEMM's operands (nn: x @ w1, nt:
dh1 @ w1^T, tn: x^T @ dh1), the two N tiles of the hand kernel (nn256,
nt256: hand kernel only), and forward + backward of the two-GEMM block
(gelu from the same kernels on both sides).  Both sides run in this
process, alternating round by round; a round is a device-event window over
--iters calls.  TF/s counts the valid rows only.  Needs a GPU; prints one
JSON line per (shape, fill).

    python scripts/bench_grouped_gemm.py [--iters 10] [--rounds 7]
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

SHAPES = {"8x13": (2048, 8192, 8, 5120), "route": (4096, 16384, 16, 2560)}
N_TOK, TOPK = 16384, 2


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


def skewed_counts(E, C, dev):
    """Filled slots per expert after F.moe_route on bench_moe_route's gate
    stand-in: 60 % of the tokens put their top value on experts 0..3."""
    g = torch.Generator().manual_seed(0)
    vals = (torch.arange(E, dtype=torch.float32) + 1) / (E * (E + 1) // 2)
    probs = vals[torch.rand(N_TOK, E, generator=g).argsort(-1)]
    rows = torch.nonzero(torch.rand(N_TOK, generator=g) < 0.6).squeeze(1)
    top = probs[rows].argmax(-1)
    tgt = torch.randint(0, 4, (rows.numel(),), generator=g)
    a, b = probs[rows, top].clone(), probs[rows, tgt].clone()
    probs[rows, top], probs[rows, tgt] = b, a
    pos = F.moe_route(probs.to(torch.bfloat16).to(dev), C, TOPK)[0]
    return F.moe_slot_counts(pos).reshape(E, 1)


def lib_nt(a, b):
    return torch.matmul(a, b.transpose(1, 2).contiguous())


def lib_tn(a, b):
    return torch.matmul(a.transpose(1, 2).contiguous(), b)


def close(got, ref, K):
    """Two bf16 roundings of fp32 sums in different orders: one bf16 ulp of
    the result plus the fp32 summation error of either side."""
    ref = ref.float()
    bound = 2.0 ** -7 * ref.abs() + K * 2.0 ** -21 * 9.0
    return bool(((got.float() - ref).abs() <= bound).all())


def run(shape, fill, args, dev):
    h, f, E, C = SHAPES[shape]
    counts = (torch.full((E, 1), int(0.8 * C), dtype=torch.int32, device=dev)
              if fill == "balanced" else skewed_counts(E, C, dev))
    mask = (torch.arange(C, device=dev).view(1, C) < counts).unsqueeze(-1)
    valid = int(counts.sum())
    gen = torch.Generator(device=dev).manual_seed(1)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=gen, device=dev) * scale) \
            .to(torch.bfloat16)
    x, dh1, geo = rnd(E, C, h) * mask, rnd(E, C, f) * mask, rnd(E, C, h) * mask
    w1, w2 = rnd(E, h, f, scale=0.02), rnd(E, f, h, scale=0.02)
    ext = F.ext()

    def hip_block():
        h1 = F.grouped_gemm(x, w1, counts, C, impl="hip")
        act = F.gelu_fwd(h1)
        eo = F.grouped_gemm(act, w2, counts, C, impl="hip")
        dact = F.grouped_gemm(geo, w2, counts, C, trans_b=True, impl="hip")
        dw2 = F.grouped_gemm_tn(act, geo, impl="hip")
        d1 = F.gelu_bwd(dact, h1)
        dx = F.grouped_gemm(d1, w1, counts, C, trans_b=True, impl="hip")
        return eo, dx, F.grouped_gemm_tn(x, d1, impl="hip"), dw2

    def lib_block():
        h1 = torch.matmul(x, w1)
        act = F.gelu_fwd(h1)
        eo = torch.matmul(act, w2)
        dact = lib_nt(geo, w2)
        dw2 = lib_tn(act, geo)
        d1 = F.gelu_bwd(dact, h1)
        return eo, lib_nt(d1, w1), lib_tn(x, d1), dw2

    # unit -> (hand kernel, library or None, contraction length, flops/row)
    units = {
        "nn": (lambda: F.grouped_gemm(x, w1, counts, C, impl="hip"),
               lambda: torch.matmul(x, w1), h, 2 * h * f),
        "nt": (lambda: F.grouped_gemm(dh1, w1, counts, C, trans_b=True,
                                      impl="hip"),
               lambda: lib_nt(dh1, w1), f, 2 * h * f),
        "tn": (lambda: F.grouped_gemm_tn(x, dh1, impl="hip"),
               lambda: lib_tn(x, dh1), C, 2 * h * f),
        "nn256": (lambda: ext.grouped_gemm_bf16(x, w1, counts, C, False, 256),
                  None, h, 2 * h * f),
        "nt256": (lambda: ext.grouped_gemm_bf16(dh1, w1, counts, C, True,
                                                256), None, f, 2 * h * f),
        "block_fwd_bwd": (hip_block, lib_block, max(h, f, C), 12 * h * f),
    }
    res = {"bench": "grouped_gemm", "shape": shape, "fill": fill, "h": h,
           "f": f, "E": E, "C": C, "valid_rows": valid,
           "valid_share": round(valid / (E * C), 4), "n_tile": F.GMM_N_TILE,
           "iters": args.iters, "rounds": args.rounds}
    times = {}
    for u, (hip, lib, K, _) in units.items():
        got = hip()
        ref = lib() if lib is not None else \
            units[u[:2]][1]()
        pairs = zip(got, ref) if isinstance(got, tuple) else [(got, ref)]
        res[f"{u}_matches_library"] = all(close(g_, r_, K) for g_, r_ in pairs)
        del got, ref, pairs
        times[u] = {"hip": [], "lib": []}
    for _ in range(args.rounds):                # alternate the sides
        for u, (hip, lib, _, _) in units.items():
            times[u]["hip"].append(window_ms(hip, args.iters))
            if lib is not None:
                times[u]["lib"].append(window_ms(lib, args.iters))
    for u, (_, lib, _, flops_row) in units.items():
        for side, ts in times[u].items():
            if ts:
                res[f"{u}_{side}_ms"] = {
                    "median": round(statistics.median(ts), 4),
                    "min": round(min(ts), 4), "max": round(max(ts), 4)}
        med = statistics.median(times[u]["hip"])
        res[f"{u}_hip_valid_tflops"] = round(valid * flops_row / med / 1e9, 1)
        if lib is not None:
            res[f"{u}_lib_over_hip"] = round(
                statistics.median(times[u]["lib"]) / med, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="8x13,route")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_grouped_gemm: needs a GPU")
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        for fill in ("balanced", "skewed"):
            run(shape, fill, args, dev)


if __name__ == "__main__":
    main()
