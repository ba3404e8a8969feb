#!/usr/bin/env python3
"""Paged fp8 decode attention against the dense fp8 kernel on the same values
and against the paged bf16 kernel on the dequantized values, the method of
bench_decode_paged.py: every side in this process, alternating round by
round, `--rounds` device-event windows of `--iters` calls after a warm-up.

Per row (H/Hkv/D, B, kv_len): the dense fp8 kernel, the paged fp8 kernel at
each page size behind a shuffled block table, and the paged bf16 kernel
F.flash_attn_decode picks for the shape at the last page size.  A side is
"ahead" of another only if its [min-max] range lies entirely below.  --append
times the quantizing paged append (S = 1) against the dense fp8 append
instead.  Needs a GPU; prints one JSON line per row and exits non-zero if a
paged fp8 output is not bit-identical to the dense fp8 kernel's.

    python scripts/bench_decode_paged_fp8.py [--shapes 32/8/128,32/1/128,...]
        [--batches 1,16,64] [--lens 2048,8192] [--pages 32,64,256]
        [--append] [--md FILE]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402
from bench_decode_attn import stats, window_ms  # noqa: E402
from bench_decode_paged import relation  # noqa: E402

FP8 = torch.float8_e4m3fn


def to_pool(t, PS, table):
    """Dense [B, Hkv, L, ...] -> pool [P, Hkv, PS, ...] behind the table
    (codes travel as bytes)."""
    raw = t.view(torch.uint8) if t.dtype == FP8 else t
    B, Hkv, L = raw.shape[:3]
    pool = torch.empty(B * (L // PS), Hkv, PS, *raw.shape[3:],
                       dtype=raw.dtype, device=raw.device)
    x = raw.view(B, Hkv, L // PS, PS, *raw.shape[3:])
    pool[table.long()] = x.transpose(1, 2)
    return pool.view(FP8) if t.dtype == FP8 else pool


def timed(sides, iters, rounds):
    for fn in sides.values():
        window_ms(fn, 3)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    return times


def run_row(B, H, Hkv, D, n, pages, iters, rounds, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, H, D, generator=g, device=dev).bfloat16()
    k = (torch.randn(B, Hkv, n, D, generator=g, device=dev) * 8).to(FP8)
    v = (torch.randn(B, Hkv, n, D, generator=g, device=dev) * 8).to(FP8)
    ks = (1 + torch.rand(B, Hkv, n, generator=g, device=dev)) / 16
    vs = (1 + torch.rand(B, Hkv, n, generator=g, device=dev)) / 16
    kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    sides = {"dense_fp8": lambda: F.flash_attn_decode(
        q, k, v, kv_len, k_scale=ks, v_scale=vs)}
    ref = sides["dense_fp8"]()
    same = True
    for PS in pages:
        table = torch.randperm(B * (n // PS), generator=g, device=dev) \
            .view(B, n // PS).to(torch.int32)
        pools = [to_pool(t, PS, table) for t in (k, v, ks, vs)]

        def paged(pools=pools, table=table):
            return F.flash_attn_decode(q, pools[0], pools[1], kv_len,
                                       k_scale=pools[2], v_scale=pools[3],
                                       block_table=table)
        sides[f"paged{PS}"] = paged
        got = paged()
        same = same and torch.equal(got[0], ref[0]) \
            and torch.equal(got[1], ref[1])
    kb = to_pool((k.float() * ks.unsqueeze(-1)).bfloat16(), PS, table)
    vb = to_pool((v.float() * vs.unsqueeze(-1)).bfloat16(), PS, table)
    sides["paged_bf16"] = lambda: F.flash_attn_decode(q, kb, vb, kv_len,
                                                      block_table=table)
    times = timed(sides, iters, rounds)
    res = {"bench": "decode_paged_fp8", "B": B, "H": H, "Hkv": Hkv, "D": D,
           "kv_len": n, "bit_identical": same}
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
        if s.startswith("paged") and s != "paged_bf16":
            res[s + "_vs_dense_fp8"] = relation(ts, times["dense_fp8"])
    res["paged_fp8_vs_paged_bf16"] = relation(times[f"paged{pages[-1]}"],
                                              times["paged_bf16"])
    print(json.dumps(res), flush=True)
    return res


def run_append(B, Hkv, D, n, PS, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(B)
    k_new = torch.randn(B, 1, Hkv, D, generator=g, device=dev).bfloat16()
    v_new = torch.randn(B, 1, Hkv, D, generator=g, device=dev).bfloat16()
    kc = torch.zeros(B, Hkv, n, D, device=dev).to(FP8)
    vc = torch.zeros_like(kc)
    ksc = torch.zeros(B, Hkv, n, device=dev)
    vsc = torch.zeros_like(ksc)
    kp = torch.zeros(B * (n // PS), Hkv, PS, D, device=dev).to(FP8)
    vp = torch.zeros_like(kp)
    ksp = torch.zeros(B * (n // PS), Hkv, PS, device=dev)
    vsp = torch.zeros_like(ksp)
    table = torch.randperm(B * (n // PS), generator=g, device=dev) \
        .view(B, n // PS).to(torch.int32)
    end = torch.full((B,), n // 2, dtype=torch.int32, device=dev)
    sides = {"dense_fp8_append": lambda: F.kv_cache_append_fp8(
                 k_new, v_new, kc, vc, ksc, vsc, end, impl="hip"),
             "paged_fp8_append": lambda: F.kv_cache_append_paged(
                 k_new, v_new, kp, vp, table, end, impl="hip", k_scale=ksp,
                 v_scale=vsp)}
    times = timed(sides, iters, rounds)
    res = {"bench": "kv_append_paged_fp8", "B": B, "Hkv": Hkv, "D": D,
           "PS": PS, "paged_vs_dense": relation(times["paged_fp8_append"],
                                                times["dense_fp8_append"])}
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    print(json.dumps(res), flush=True)
    return res


def md_table(rows, pages):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]"
    head = ["H/Hkv", "D", "B", "kv_len", "dense fp8 ms"]
    for PS in pages:
        head += [f"PS={PS} ms", "vs dense fp8"]
    head += ["paged bf16 ms", f"PS={pages[-1]} vs paged bf16"]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        cells = [f"{r['H']}/{r['Hkv']}", r["D"], r["B"], r["kv_len"],
                 rng(r["dense_fp8_ms"])]
        for PS in pages:
            cells += [rng(r[f"paged{PS}_ms"]), r[f"paged{PS}_vs_dense_fp8"]]
        cells += [rng(r["paged_bf16_ms"]), r["paged_fp8_vs_paged_bf16"]]
        out.append("| " + " | ".join(str(c) for c in cells) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--lens", default="2048,8192")
    ap.add_argument("--pages", default="32,64,256")
    ap.add_argument("--shapes", default="32/32/128,32/8/128,32/4/128,32/1/128",
                    help="H/Hkv/D triples")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_paged_fp8: needs a GPU")
    dev = torch.device("cuda", 0)
    pages = [int(x) for x in args.pages.split(",")]
    batches = [int(x) for x in args.batches.split(",")]
    shapes = [tuple(int(x) for x in s.split("/"))
              for s in args.shapes.split(",")]
    if args.append:
        for B in batches:
            run_append(B, shapes[0][1], shapes[0][2], 2048, pages[0],
                       args.iters, args.rounds, dev)
        return
    rows = []
    for i, (H, Hkv, D) in enumerate(shapes):
        for B in batches:
            for n in (int(x) for x in args.lens.split(",")):
                rows.append(run_row(B, H, Hkv, D, n, pages, args.iters,
                                    args.rounds, dev, i))
                torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows, pages))
    if not all(r["bit_identical"] for r in rows):
        sys.exit("bench_decode_paged_fp8: a paged output differs from the "
                 "dense fp8 kernel's")


if __name__ == "__main__":
    main()
