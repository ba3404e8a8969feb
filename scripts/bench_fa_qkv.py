#!/usr/bin/env python3
"""Fused-qkv flash attention forward and backward at the flagship shape
(GPT-3 7B: B=16, S=2048, H=Hkv=32, D=128, causal, bf16), each with the
default tile dispatch (mask-free body on interior tiles) and with
HETU_AMD_FA_MASK_ALL=1 (masked body on every tile).

Both sides run in this process on the same random-normal operands,
alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of every side.  The launchers read the
switch at every launch, so it is flipped in os.environ between windows.
The outputs of the two sides are compared first: they must be bit-equal.
Reports median [min-max] per side; a side is ahead only if its range lies
entirely below the other's ("default_wins").  On a tree without the switch
both sides time the same kernels, which gives that tree's figures (and the
noise floor of the comparison).  Needs a GPU; one JSON line per direction.

    python scripts/bench_fa_qkv.py [--iters 10] [--rounds 7]
                                   [--batch 16] [--seq 2048] [--heads 32]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

D = 128
SWITCH = "HETU_AMD_FA_MASK_ALL"


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


def with_switch(on, fn, *args):
    if on:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    try:
        return fn(*args)
    finally:
        os.environ.pop(SWITCH, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--heads", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fa_qkv: needs a GPU")
    dev = torch.device("cuda", 0)
    ext = F.ext()
    B, S, H = args.batch, args.seq, args.heads
    scale = 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * D, generator=g).to(torch.bfloat16).to(dev)
    do = torch.randn(B, S, H * D, generator=g).to(torch.bfloat16).to(dev)

    def fwd():
        return ext.flash_attn_fwd_qkv(qkv, H, H, D, True, scale)

    o, lse = with_switch(False, fwd)

    def bwd():
        return ext.flash_attn_bwd_qkv(do, qkv, o, lse, H, H, D, True, scale)

    # causal FLOPs: half of the S x S square; fwd 2 GEMMs, bwd 5 + delta
    gemm = 2.0 * B * H * S * S * D / 2
    failed = []
    for name, fn, n_gemm in (("fwd", fwd, 2), ("bwd", bwd, 5)):
        a = with_switch(False, fn)
        b = with_switch(True, fn)
        a = a if isinstance(a, (tuple, list)) else (a,)
        b = b if isinstance(b, (tuple, list)) else (b,)
        equal = all(bool(torch.equal(x, y)) for x, y in zip(a, b))
        # one untimed round: the first window after a change of kernel runs
        # up to 10 % slow on either side (clocks), which is not the subject
        for on in (False, True):
            with_switch(on, window_ms, fn, args.iters)
        times = {"default": [], "mask_all": []}
        for _ in range(args.rounds):                # alternate the sides
            times["default"].append(with_switch(False, window_ms, fn,
                                                args.iters))
            times["mask_all"].append(with_switch(True, window_ms, fn,
                                                 args.iters))
        res = {"bench": "fa_qkv", "dir": name, "B": B, "S": S, "H": H, "D": D,
               "causal": True, "dtype": "bf16", "iters": args.iters,
               "rounds": args.rounds, "bit_equal": equal}
        for n, ts in times.items():
            res[n + "_ms"] = {"median": round(statistics.median(ts), 4),
                              "min": round(min(ts), 4),
                              "max": round(max(ts), 4)}
        med = {n: statistics.median(ts) for n, ts in times.items()}
        res["default_tflops"] = round(n_gemm * gemm / med["default"] / 1e9, 1)
        res["default_wins"] = max(times["default"]) < min(times["mask_all"])
        res["mask_all_over_default"] = round(
            med["mask_all"] / med["default"], 4)
        print(json.dumps(res), flush=True)
        if not equal:
            failed.append(name)
        del a, b
    if failed:
        sys.exit(f"bench_fa_qkv: the two tile dispatches differ in {failed}")


if __name__ == "__main__":
    main()
