"""Flash attention at head dim 64: the v2 kernels against what the same calls
ran before they took D = 64.

  varlen  F.varlen_attention_fwd / _bwd (one launch over all segments)
          vs the per-segment loop over the dense v1 kernels (a host sync,
          a slice, a permute and a copy around every segment)
  fused   F.fused_qkv_attention_fwd / _bwd on [B, S, (H+2Hkv) D]
          vs slice / transpose copies + dense v1 forward and backward, what
          the model builders ran at dh = 64

bf16, causal, H/Hkv 16/16 and 32/8; T = 16384 in 64 ragged segments (fixed
seed), fused [B, S] = [8, 2048].  Both sides in one process, alternating round
by round, `--rounds` device-event windows of `--iters` calls after a warm-up,
median [min-max]; a side is "ahead" only if the ranges do not overlap.
Needs a GPU; prints one JSON line per row.

  python scripts/bench_fa_d64.py [--iters 20] [--rounds 7] [--md FILE]
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

D = 64
SCALE = 1.0 / math.sqrt(D)


def ragged_lens(total, n, seed=0):
    """n segment lengths >= 1 summing to `total`."""
    g = torch.Generator().manual_seed(seed)
    cuts = torch.randperm(total - 1, generator=g)[:n - 1].sort().values + 1
    edges = [0] + cuts.tolist() + [total]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def loop_fwd(q, k, v, cu):
    out = torch.empty_like(q)
    lse = torch.empty(q.shape[1], q.shape[0], dtype=torch.float32,
                      device=q.device)
    b = cu.tolist()
    for s0, s1 in zip(b[:-1], b[1:]):
        a = [t[s0:s1].permute(1, 0, 2).unsqueeze(0).contiguous()
             for t in (q, k, v)]
        o, l = F.flash_attn_fwd(a[0], a[1], a[2], True, SCALE)
        out[s0:s1] = o[0].permute(1, 0, 2)
        lse[:, s0:s1] = l[0]
    return out, lse


def loop_bwd(do, q, k, v, o, lse, cu):
    grads = [torch.zeros_like(t) for t in (q, k, v)]
    b = cu.tolist()
    for s0, s1 in zip(b[:-1], b[1:]):
        a = [t[s0:s1].permute(1, 0, 2).unsqueeze(0).contiguous()
             for t in (do, q, k, v, o)]
        ls = lse[:, s0:s1].unsqueeze(0).contiguous()
        r = F.flash_attn_bwd(a[0], a[1], a[2], a[3], a[4], ls, True, SCALE)
        for dst, src in zip(grads, r):
            dst[s0:s1] = src[0].permute(1, 0, 2)
    return grads


def split_qkv(qkv, H, Hkv):
    B, S, _ = qkv.shape
    q4 = qkv.view(B, S, H + 2 * Hkv, D)
    return [q4[:, :, a:b].permute(0, 2, 1, 3).contiguous()
            for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv))]


def copies_fwd(qkv, H, Hkv):
    B, S, _ = qkv.shape
    q, k, v = split_qkv(qkv, H, Hkv)
    o, lse = F.flash_attn_fwd(q, k, v, True, SCALE)
    return o.permute(0, 2, 1, 3).reshape(B, S, H * D).contiguous(), lse


def copies_bwd(do, qkv, o, lse, H, Hkv):
    B, S, _ = qkv.shape
    q, k, v = split_qkv(qkv, H, Hkv)
    d4, o4 = (t.view(B, S, H, D).permute(0, 2, 1, 3).contiguous()
              for t in (do, o))
    r = F.flash_attn_bwd(d4, q, k, v, o4, lse, True, SCALE)
    return torch.cat(r, dim=1).permute(0, 2, 1, 3).reshape(B, S, -1) \
        .contiguous()


def measure(res, sides, iters, rounds):
    for fn in sides.values():
        window_ms(fn, 2)
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    res["new_vs_before"] = relation(times["new"], times["before"])
    res["speedup"] = round(res["before_ms"]["median"]
                           / res["new_ms"]["median"], 2)
    print(json.dumps(res), flush=True)
    return res


def run_varlen(H, Hkv, T, nseg, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    lens = ragged_lens(T, nseg)
    cu = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).int().to(dev)
    q, do = (torch.randn(T, H, D, generator=g, device=dev).bfloat16()
             for _ in range(2))
    k, v = (torch.randn(T, Hkv, D, generator=g, device=dev).bfloat16()
            for _ in range(2))
    ms = max(lens)
    o, lse = F.varlen_attention_fwd(q, k, v, cu, True, SCALE, ms)
    o_b, lse_b = loop_fwd(q, k, v, cu)
    rows = []
    base = {"bench": "fa_d64", "path": "varlen", "H": H, "Hkv": Hkv,
            "T": T, "segments": nseg, "max_seqlen": ms}
    rows.append(measure(
        dict(base, dir="fwd", max_abs_diff=round(
            (o.float() - o_b.float()).abs().max().item(), 5)),
        {"new": lambda: F.varlen_attention_fwd(q, k, v, cu, True, SCALE, ms),
         "before": lambda: loop_fwd(q, k, v, cu)}, iters, rounds))
    dq = F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True, SCALE, ms)[0]
    dq_b = loop_bwd(do, q, k, v, o_b, lse_b, cu)[0]
    rows.append(measure(
        dict(base, dir="bwd", max_abs_diff=round(
            (dq.float() - dq_b.float()).abs().max().item(), 5)),
        {"new": lambda: F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True,
                                               SCALE, ms),
         "before": lambda: loop_bwd(do, q, k, v, o_b, lse_b, cu)},
        iters, rounds))
    return rows


def run_fused(H, Hkv, B, S, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g,
                      device=dev).bfloat16()
    do = torch.randn(B, S, H * D, generator=g, device=dev).bfloat16()
    o, lse = F.fused_qkv_attention_fwd(qkv, H, Hkv, D, None, None, True,
                                       SCALE)
    o_b, lse_b = copies_fwd(qkv, H, Hkv)
    rows = []
    base = {"bench": "fa_d64", "path": "fused_qkv", "H": H, "Hkv": Hkv,
            "B": B, "S": S}
    rows.append(measure(
        dict(base, dir="fwd", max_abs_diff=round(
            (o.float() - o_b.float()).abs().max().item(), 5)),
        {"new": lambda: F.fused_qkv_attention_fwd(qkv, H, Hkv, D, None, None,
                                                  True, SCALE),
         "before": lambda: copies_fwd(qkv, H, Hkv)}, iters, rounds))
    d = F.fused_qkv_attention_bwd(do, qkv, o, lse, H, Hkv, D, None, None,
                                  True, SCALE)
    d_b = copies_bwd(do, qkv, o_b, lse_b, H, Hkv)
    rows.append(measure(
        dict(base, dir="bwd", max_abs_diff=round(
            (d.float() - d_b.float()).abs().max().item(), 5)),
        {"new": lambda: F.fused_qkv_attention_bwd(do, qkv, o, lse, H, Hkv, D,
                                                  None, None, True, SCALE),
         "before": lambda: copies_bwd(do, qkv, o_b, lse_b, H, Hkv)},
        iters, rounds))
    return rows


def md_table(rows):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]"
    head = ["path", "dir", "H/Hkv", "new ms", "before ms", "before / new",
            "new vs before", "max abs diff"]
    out = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        cells = [r["path"], r["dir"], f"{r['H']}/{r['Hkv']}",
                 rng(r["new_ms"]), rng(r["before_ms"]), r["speedup"],
                 r["new_vs_before"], r["max_abs_diff"]]
        out.append("| " + " | ".join(str(c) for c in cells) + " |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="16/16,32/8", help="H/Hkv pairs")
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fa_d64: needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for shape in args.shapes.split(","):
        H, Hkv = (int(x) for x in shape.split("/"))
        rows += run_varlen(H, Hkv, 16384, 64, args.iters, args.rounds, dev)
        rows += run_fused(H, Hkv, 8, 2048, args.iters, args.rounds, dev)
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows))


if __name__ == "__main__":
    main()
