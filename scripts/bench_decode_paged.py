#!/usr/bin/env python3
"""Paged decode attention against the dense kernel on the same values, the
method of bench_decode_attn.py: every side in this process, alternating round
by round, `--rounds` device-event windows of `--iters` calls after a warm-up.

Per row (H/Hkv/D, B, kv_len): the dense kernel F.flash_attn_decode picks for
the shape (VALU or MFMA, by _decode_auto_mfma), the paged variant of the same
kernel at each page size behind a shuffled block table, and, with --gather,
the torch gather composition (impl="torch") that impl=None would otherwise
fall to.  A side is "ahead" of another only if its [min-max] range lies
entirely below.  --append times kv_cache_append_paged (S = 1) against the
dense cache's slice assignment instead.  Needs a GPU; prints one JSON line
per row and exits non-zero if a paged output is not bit-identical to the
dense kernel's.

    python scripts/bench_decode_paged.py [--shapes 32/32/128,32/8/128,...]
        [--batches 1,16,64] [--lens 2048,8192] [--pages 32,64,256]
        [--gather] [--append] [--md FILE]
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
from bench_decode_attn import stats, window_ms  # noqa: E402


def to_pool(t, PS, table):
    B, Hkv, L, D = t.shape
    pool = torch.empty(B * (L // PS), Hkv, PS, D, dtype=t.dtype,
                       device=t.device)
    pool[table.long()] = t.view(B, Hkv, L // PS, PS, D).permute(0, 2, 1, 3, 4)
    return pool


def relation(a, b):
    """a against b by disjoint min-max ranges."""
    if max(a) < min(b):
        return "ahead"
    return "behind" if min(a) > max(b) else "overlapping"


def run_row(B, H, Hkv, D, n, pages, gather, iters, rounds, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, H, D, generator=g, device=dev).bfloat16()
    k = torch.randn(B, Hkv, n, D, generator=g, device=dev).bfloat16()
    v = torch.randn(B, Hkv, n, D, generator=g, device=dev).bfloat16()
    kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    impl = "mfma" if F._decode_auto_mfma(H // Hkv, D, B, Hkv, n) else "hip"
    sides = {"dense": lambda: F.flash_attn_decode(q, k, v, kv_len, impl=impl)}
    ref = sides["dense"]()
    same = True
    for PS in pages:
        table = torch.randperm(B * (n // PS), generator=g, device=dev) \
            .view(B, n // PS).to(torch.int32)
        kp, vp = to_pool(k, PS, table), to_pool(v, PS, table)

        def paged(kp=kp, vp=vp, table=table, impl=impl):
            return F.flash_attn_decode(q, kp, vp, kv_len, impl=impl,
                                       block_table=table)
        sides[f"paged{PS}"] = paged
        got = paged()
        same = same and torch.equal(got[0], ref[0]) \
            and torch.equal(got[1], ref[1])
        if gather and PS == pages[-1]:
            sides["gather"] = lambda kp=kp, vp=vp, table=table: \
                F.flash_attn_decode(q, kp, vp, kv_len, impl="torch",
                                    block_table=table)
    for fn in sides.values():
        window_ms(fn, 3)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    res = {"bench": "decode_paged", "B": B, "H": H, "Hkv": Hkv, "D": D,
           "kv_len": n, "kernel": impl, "bit_identical": same}
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
        if s.startswith("paged"):
            res[s + "_vs_dense"] = relation(ts, times["dense"])
    if gather:
        res["paged_vs_gather"] = relation(times[f"paged{pages[-1]}"],
                                          times["gather"])
    print(json.dumps(res), flush=True)
    return res


def run_append(B, Hkv, D, n, PS, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(B)
    k_new = torch.randn(B, 1, Hkv, D, generator=g, device=dev).bfloat16()
    v_new = torch.randn(B, 1, Hkv, D, generator=g, device=dev).bfloat16()
    kc = torch.zeros(B, Hkv, n, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    kp = torch.zeros(B * (n // PS), Hkv, PS, D, dtype=torch.bfloat16,
                     device=dev)
    vp = torch.zeros_like(kp)
    table = torch.randperm(B * (n // PS), generator=g, device=dev) \
        .view(B, n // PS).to(torch.int32)
    end = torch.full((B,), n // 2, dtype=torch.int32, device=dev)
    pos = n // 2 - 1

    def dense():
        kc[:, :, pos:pos + 1] = k_new.permute(0, 2, 1, 3)
        vc[:, :, pos:pos + 1] = v_new.permute(0, 2, 1, 3)
    sides = {"slice_assign": dense,
             "paged_append": lambda: F.kv_cache_append_paged(
                 k_new, v_new, kp, vp, table, end, impl="hip")}
    for fn in sides.values():
        window_ms(fn, 3)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    res = {"bench": "kv_append_paged", "B": B, "Hkv": Hkv, "D": D, "PS": PS,
           "append_vs_slice": relation(times["paged_append"],
                                       times["slice_assign"])}
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    print(json.dumps(res), flush=True)
    return res


def md_table(rows, pages):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]"
    head = ["H/Hkv", "B", "kv_len", "kernel", "dense ms"]
    for PS in pages:
        head += [f"PS={PS} ms", "vs dense"]
    if rows and "gather_ms" in rows[0]:
        head += ["gather ms", "paged vs gather"]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        cells = [f"{r['H']}/{r['Hkv']}", r["B"], r["kv_len"], r["kernel"],
                 rng(r["dense_ms"])]
        for PS in pages:
            cells += [rng(r[f"paged{PS}_ms"]), r[f"paged{PS}_vs_dense"]]
        if "gather_ms" in r:
            cells += [rng(r["gather_ms"]), r["paged_vs_gather"]]
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
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_paged: needs a GPU")
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
                rows.append(run_row(B, H, Hkv, D, n, pages, args.gather,
                                    args.iters, args.rounds, dev, i))
                torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows, pages))
    if not all(r["bit_identical"] for r in rows):
        sys.exit("bench_decode_paged: a paged output differs from the dense "
                 "kernel's")


if __name__ == "__main__":
    main()
