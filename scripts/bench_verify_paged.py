#!/usr/bin/env python3
"""Split-KV verification attention (F.flash_attn_prefill_paged(impl="split"))
against its alternatives, the method of bench_decode_paged.py: every side in
this process, alternating round by round, `--rounds` device-event windows of
`--iters` calls after a warm-up, median [min-max]; a side is "ahead" of
another only if its range lies entirely below.  The outputs of all sides are
compared first.

Sides per row (B sequences, a chunk of n tokens at the end of kv_len keys):
  split     impl="split": the keys read once per step, spread over splits
  prefill   impl="hip" on the same input: the packed prefill kernel, what runs
            without the split kernel
  decode*n  n successive paged S = 1 decode calls (impl=None, the generator's
            routing between the VALU and the MFMA kernel) at lengths
            kv_len - n + 1 .. kv_len: what a generator without verification
            pays for n tokens
  decode    one S = 1 decode call on the same cache: the bandwidth floor
  torch     --head-dim 64 only: impl="torch", what these inputs ran before the
            kernels served D = 64

TB/s counts the cache bytes of the step (K and V of kv_len keys per sequence
and KV head) over the split side's median.  Needs a GPU; prints one JSON line
per row.

    python scripts/bench_verify_paged.py [--shapes 32/8,32/32] [--batches 1,16]
        [--kv 2048,8192] [--chunks 2,4,8] [--page 64] [--head-dim 128]
        [--md FILE]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402
from bench_decode_attn import stats, window_ms  # noqa: E402
from bench_decode_paged import relation  # noqa: E402

D = 128
SIDES = ("split", "prefill", "decode*n", "decode")


def run_row(H, Hkv, PS, B, kv, n, iters, rounds, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    MP = -(-kv // PS)
    P = B * MP
    q = torch.randn(B * n, H, D, generator=g, device=dev).bfloat16()
    kp = torch.randn(P, Hkv, PS, D, generator=g, device=dev).bfloat16()
    vp = torch.randn(P, Hkv, PS, D, generator=g, device=dev).bfloat16()
    table = torch.randperm(P, generator=g, device=dev).to(torch.int32) \
        .view(B, MP)
    cu_q = torch.arange(0, B * n + 1, n, dtype=torch.int32, device=dev)
    kv_len = torch.full((B,), kv, dtype=torch.int32, device=dev)
    lens = [kv_len - n + i + 1 for i in range(n)]
    qs = [q.view(B, n, H, D)[:, i] for i in range(n)]    # strided views
    scale = 1.0 / math.sqrt(D)

    def packed(impl):
        return F.flash_attn_prefill_paged(q, kp, vp, table, cu_q, kv_len,
                                          scale, max_q=n, impl=impl)[0]

    def decode_n():
        return [F.flash_attn_decode(qs[i], kp, vp, lens[i], scale,
                                    block_table=table)[0] for i in range(n)]
    sides = {"split": lambda: packed("split"),
             "prefill": lambda: packed("hip"), "decode*n": decode_n,
             "decode": lambda: F.flash_attn_decode(
                 qs[-1], kp, vp, kv_len, scale, block_table=table)[0]}
    if D != 128:
        sides["torch"] = lambda: packed("torch")
    res = {"bench": "verify_paged", "H": H, "Hkv": Hkv, "D": D, "PS": PS,
           "B": B, "kv_len": kv, "n": n}
    got = sides["split"]().float()
    if D != 128:
        res["max_abs_diff_vs_torch"] = round(
            (got - sides["torch"]().float()).abs().max().item(), 5)
    res["max_abs_diff_vs_prefill"] = round(
        (got - sides["prefill"]().float()).abs().max().item(), 5)
    res["max_abs_diff_vs_decode"] = round(
        (got.view(B, n, H, D) - torch.stack(decode_n(), 1).float())
        .abs().max().item(), 5)
    for fn in sides.values():
        window_ms(fn, 2)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    cache_bytes = 2 * B * Hkv * kv * D * 2
    res["split_TBps"] = round(cache_bytes / res["split_ms"]["median"] / 1e9, 3)
    for s in list(sides)[1:]:
        res["split_vs_" + s] = relation(times["split"], times[s])
    print(json.dumps(res), flush=True)
    return res


def md_table(rows):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]"
    sides = SIDES if D == 128 else SIDES + ("torch",)
    head = ["H/Hkv", "B", "kv_len", "n"] + [s + " ms" for s in sides] + \
        ["split TB/s"] + ["split vs " + s for s in sides[1:]]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        cells = [f"{r['H']}/{r['Hkv']}", r["B"], r["kv_len"], r["n"]] + \
            [rng(r[s + "_ms"]) for s in sides] + [r["split_TBps"]] + \
            [r["split_vs_" + s] for s in sides[1:]]
        out.append("| " + " | ".join(str(c) for c in cells) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="32/8,32/32", help="H/Hkv pairs")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--kv", default="2048,8192")
    ap.add_argument("--chunks", default="2,4,8")
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128))
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    global D
    D = args.head_dim
    if not torch.cuda.is_available():
        sys.exit("bench_verify_paged: needs a GPU")
    dev = torch.device("cuda", 0)

    def ints(s):
        return [int(x) for x in s.split(",")]
    rows = []
    for shape in args.shapes.split(","):
        H, Hkv = (int(x) for x in shape.split("/"))
        for B in ints(args.batches):
            for kv in ints(args.kv):
                for n in ints(args.chunks):
                    rows.append(run_row(H, Hkv, args.page, B, kv, n,
                                        args.iters, args.rounds, dev))
                torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows))


if __name__ == "__main__":
    main()
