#!/usr/bin/env python3
"""Paged prefill attention (F.flash_attn_prefill_paged) against what it
replaces, the method of bench_decode_paged.py: every side in this process,
alternating round by round, `--rounds` device-event windows of `--iters`
calls after a warm-up, median [min-max]; a side is "ahead" of another only if
its range lies entirely below.

Sides per row:
  kernel    one launch over the packed rows and the page pools
  gather    per sequence: its pages gathered into contiguous K / V, its q
            rows copied to [1, H, n, D], F.flash_attn_fwd (causal, with the
            cached context): the composition a generator would run without
            the kernel
  varlen    context 0 and H == Hkv only: F.varlen_attention_fwd on the same
            packed rows, the same arithmetic without the table, so the
            difference is what paging and the (token, head) rows cost
  torch     --head-dim 64 only, in place of gather: impl="torch", what these
            inputs ran before the kernel served D = 64 (the fp32 loop over
            sequences that reads cu_q and kv_len on the host)

kernel_TBps counts the pages a call must read (K and V of every sequence's
keys, once per KV head) over the kernel's median.

Rows: "ragged" = 16 prompts of 200-2000 tokens from a fixed seed at context
0; "chunk/C" = a 512-token chunk per sequence (--batch sequences) behind C
cached keys.  Needs a GPU; prints one JSON line per row.

    python scripts/bench_prefill_paged.py [--shapes 32/8,32/32]
        [--contexts 0,2048,8192] [--batch 8] [--page 64] [--head-dim 128]
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


def run_row(name, H, Hkv, PS, seqs, iters, rounds, dev, seed=0):
    """seqs: (context, n) per sequence."""
    base = "gather" if D == 128 else "torch"
    g = torch.Generator(device=dev).manual_seed(seed)
    B = len(seqs)
    lens = [c + n for c, n in seqs]
    need = [-(-n // PS) for n in lens]
    P, MP = sum(need), max(need)
    cu = [0]
    for _, n in seqs:
        cu.append(cu[-1] + n)
    T = cu[-1]
    q = torch.randn(T, H, D, generator=g, device=dev).bfloat16()
    kp = torch.randn(P, Hkv, PS, D, generator=g, device=dev).bfloat16()
    vp = torch.randn(P, Hkv, PS, D, generator=g, device=dev).bfloat16()
    perm = torch.randperm(P, generator=g, device=dev).to(torch.int32)
    table = torch.full((B, MP), P, dtype=torch.int32, device=dev)
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = perm[at:at + n]
        at += n
    cu_q = torch.tensor(cu, dtype=torch.int32, device=dev)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(D)
    max_q = max(n for _, n in seqs)

    def kernel():
        return F.flash_attn_prefill_paged(q, kp, vp, table, cu_q, kv_len,
                                          scale, max_q=max_q, impl="hip")

    def gather():
        outs = []
        for b, kv in enumerate(lens):
            ids = table[b, :need[b]].long()
            kd = kp[ids].permute(1, 0, 2, 3).reshape(1, Hkv, -1, D)[:, :, :kv]
            vd = vp[ids].permute(1, 0, 2, 3).reshape(1, Hkv, -1, D)[:, :, :kv]
            qb = q[cu[b]:cu[b + 1]].permute(1, 0, 2).unsqueeze(0)
            outs.append(F.flash_attn_fwd(qb.contiguous(), kd.contiguous(),
                                         vd.contiguous(), True, scale)[0])
        return outs

    def torch_side():
        return F.flash_attn_prefill_paged(q, kp, vp, table, cu_q, kv_len,
                                          scale, max_q=max_q, impl="torch")
    sides = {"kernel": kernel, base: gather if D == 128 else torch_side}
    res = {"bench": "prefill_paged", "row": name, "H": H, "Hkv": Hkv,
           "D": D, "PS": PS, "B": B, "T": T, "kv_total": sum(lens)}
    got = kernel()[0]
    if D == 128:
        want = torch.cat([o[0].permute(1, 0, 2) for o in gather()])
    else:
        want = torch_side()[0]
    res["max_abs_diff_vs_" + base] = round(
        (got.float() - want.float()).abs().max().item(), 5)
    if D == 128 and H == Hkv and all(c == 0 for c, _ in seqs):
        # the packed new rows are the pools' content, laid out densely
        kd = torch.cat([kp[table[b, :need[b]].long()].permute(1, 0, 2, 3)
                        .reshape(Hkv, -1, D)[:, :lens[b]].permute(1, 0, 2)
                        for b in range(B)]).contiguous()
        vd = torch.cat([vp[table[b, :need[b]].long()].permute(1, 0, 2, 3)
                        .reshape(Hkv, -1, D)[:, :lens[b]].permute(1, 0, 2)
                        for b in range(B)]).contiguous()
        sides["varlen"] = lambda: F.varlen_attention_fwd(
            q, kd, vd, cu_q, True, scale, max_seqlen=max_q)
    for fn in sides.values():
        window_ms(fn, 2)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    res["kernel_TBps"] = round(2 * sum(lens) * Hkv * D * 2
                               / res["kernel_ms"]["median"] / 1e9, 3)
    res["kernel_vs_" + base] = relation(times["kernel"], times[base])
    if "varlen" in times:
        res["kernel_vs_varlen"] = relation(times["kernel"], times["varlen"])
    print(json.dumps(res), flush=True)
    return res


def md_table(rows):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]" \
            if d else "-"
    base = "gather" if D == 128 else "torch"
    head = ["row", "H/Hkv", "B", "T", "keys", "kernel ms", base + " ms",
            "kernel vs " + base, "varlen ms", "kernel vs varlen"]
    if D != 128:
        head[-2:] = ["kernel TB/s"]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        cells = [r["row"], f"{r['H']}/{r['Hkv']}", r["B"], r["T"],
                 r["kv_total"], rng(r["kernel_ms"]), rng(r[base + "_ms"]),
                 r["kernel_vs_" + base], rng(r.get("varlen_ms")),
                 r.get("kernel_vs_varlen", "-")]
        if D != 128:
            cells[-2:] = [r["kernel_TBps"]]
        out.append("| " + " | ".join(str(c) for c in cells) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="32/8,32/32", help="H/Hkv pairs")
    ap.add_argument("--contexts", default="0,2048,8192")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128))
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    global D
    D = args.head_dim
    if not torch.cuda.is_available():
        sys.exit("bench_prefill_paged: needs a GPU")
    dev = torch.device("cuda", 0)
    ragged = torch.randint(200, 2001, (16,),
                           generator=torch.Generator().manual_seed(0))
    rows = []
    for shape in args.shapes.split(","):
        H, Hkv = (int(x) for x in shape.split("/"))
        rows.append(run_row("ragged", H, Hkv, args.page,
                            [(0, int(n)) for n in ragged], args.iters,
                            args.rounds, dev))
        for c in (int(x) for x in args.contexts.split(",")):
            rows.append(run_row(f"chunk/{c}", H, Hkv, args.page,
                                [(c, 512)] * args.batch, args.iters,
                                args.rounds, dev))
            torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows))


if __name__ == "__main__":
    main()
