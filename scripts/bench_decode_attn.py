#!/usr/bin/env python3
"""Decode attention (one query token per sequence over a bf16 KV cache):
the split-KV HIP kernel (F.flash_attn_decode(impl="hip") ->
ops/hip/attention_decode.hip) against the composition it replaces, the
S == 1 case of the `else` branch of LlamaGenerator._attn before the kernel
(slice, repeat_interleave over the KV heads, fp32 casts, two matmuls and a
softmax), copied below and fed the same cache.

Both sides run in this process on the same random-normal bf16 operands,
alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of both.  A contiguous copy_ of the K and V
caches (the bandwidth yardstick: it reads AND writes the bytes the kernel
only reads) is timed in the same rounds.  Bytes that must move:
2 * B * Hkv * kv_len * D * 2 (each cached K and V row once as bf16).
The kernel belongs on the auto route for a shape only if its [min-max] range
lies entirely below the composition's ("hip_wins").
Needs a GPU; prints one JSON line per row and exits non-zero if a row that
F.flash_attn_decode's auto rule sends to the kernel does not win, or if the
two sides' outputs differ by more than two bf16 roundings of max|v|.

    python scripts/bench_decode_attn.py [--iters 20] [--rounds 7]
                                        [--batches 1,16,64]
                                        [--lens 512,2048,8192] [--md FILE]
                                        [--shapes 32/32/128,32/8/128,16/16/64]
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

# (H, Hkv, D)
HEAD_SHAPES = [(32, 32, 128), (32, 8, 128), (16, 16, 64)]


def composition(qt, kcache, vcache, n, H, Hkv, scale, dtype):
    """qt [B, H, 1, dh]; the caches [B, Hkv, L, dh]; n visible rows."""
    kk = kcache[:, :, :n]
    vv = vcache[:, :, :n]
    rep = H // Hkv
    kr = kk.repeat_interleave(rep, dim=1) if rep > 1 else kk
    vr = vv.repeat_interleave(rep, dim=1) if rep > 1 else vv
    scores = (qt.float() @ kr.float().transpose(-1, -2)) \
        * scale
    p = torch.softmax(scores, dim=-1)
    o = (p @ vr.float()).to(dtype)
    return o


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


def run_row(B, H, Hkv, D, n, seed, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    q = torch.randn(B, H, D, generator=g, device=dev).to(torch.bfloat16)
    k = torch.randn(B, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16)
    v = torch.randn(B, Hkv, n, D, generator=g, device=dev).to(torch.bfloat16)
    kv_len = torch.full((B,), n, dtype=torch.int32, device=dev)
    k2, v2 = torch.empty_like(k), torch.empty_like(v)
    scale = 1.0 / math.sqrt(D)
    qt = q.unsqueeze(2)
    sides = {
        "hip": lambda: F.flash_attn_decode(q, k, v, kv_len, scale,
                                           impl="hip"),
        "composition": lambda: composition(qt, k, v, n, H, Hkv, scale,
                                           torch.bfloat16),
        "copy": lambda: (k2.copy_(k), v2.copy_(v)),
    }
    oh = sides["hip"]()[0].float()
    oc = sides["composition"]().squeeze(2).float()
    max_diff = (oh - oc).abs().max().item()
    # each side rounds its output to bf16 once: two roundings of max|v|
    numerics_ok = max_diff <= 2 * 2.0 ** -9 * v.float().abs().max().item()
    del oh, oc
    for fn in sides.values():
        window_ms(fn, 3)
    times = {s: [] for s in sides}
    for _ in range(rounds):                # alternate the sides
        for s, fn in sides.items():
            times[s].append(window_ms(fn, iters))
    nbytes = 2.0 * B * Hkv * n * D * 2
    med = {s: statistics.median(ts) for s, ts in times.items()}
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ns = int(F.ext().decode_attn_num_splits(B, Hkv, n, cus))
    res = {"bench": "decode_attn", "B": B, "H": H, "Hkv": Hkv, "D": D,
           "kv_len": n, "splits": ns, "blocks": B * Hkv * ns,
           "iters": iters, "rounds": rounds,
           "max_diff_hip_vs_composition": max_diff,
           "numerics_ok": numerics_ok}
    for s, ts in times.items():
        res[s + "_ms"] = stats(ts)
    res["hip_tbps"] = round(nbytes / (med["hip"] * 1e-3) / 1e12, 3)
    res["composition_tbps"] = round(
        nbytes / (med["composition"] * 1e-3) / 1e12, 3)
    # the copy moves the same bytes (and writes them as well)
    res["copy_tbps_read"] = round(nbytes / (med["copy"] * 1e-3) / 1e12, 3)
    res["hip_bw_over_copy_bw"] = round(med["copy"] / med["hip"], 3)
    res["composition_over_hip"] = round(med["composition"] / med["hip"], 2)
    res["hip_wins"] = (numerics_ok
                       and max(times["hip"]) < min(times["composition"]))
    res["auto_routes_hip"] = F.flash_attn_decode_on_hip(q, k, v, kv_len)
    print(json.dumps(res), flush=True)
    return res


def md_table(rows):
    def rng(d):
        return f"{d['median']:.4f} [{d['min']:.4f}-{d['max']:.4f}]"
    out = ["| H/Hkv | D | B | kv_len | splits | blocks | HIP ms | "
           "composition ms | copy_ ms | HIP TB/s | HIP / copy_ bandwidth | "
           "composition / HIP | HIP wins |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(
            f"| {r['H']}/{r['Hkv']} | {r['D']} | {r['B']} | {r['kv_len']} | "
            f"{r['splits']} | {r['blocks']} | {rng(r['hip_ms'])} | "
            f"{rng(r['composition_ms'])} | {rng(r['copy_ms'])} | "
            f"{r['hip_tbps']:.3f} | {r['hip_bw_over_copy_bw']:.2f} | "
            f"{r['composition_over_hip']:.1f}x | "
            f"{'yes' if r['hip_wins'] else 'NO'} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--lens", default="512,2048,8192")
    ap.add_argument("--shapes", default=",".join(
        "/".join(str(x) for x in s) for s in HEAD_SHAPES),
        help="H/Hkv/D triples")
    ap.add_argument("--md", default="", help="also write a markdown table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_attn: needs a GPU")
    dev = torch.device("cuda", 0)
    rows, bad = [], []
    i = 0
    for (H, Hkv, D) in (tuple(int(x) for x in s.split("/"))
                        for s in args.shapes.split(",")):
        for B in (int(x) for x in args.batches.split(",")):
            for n in (int(x) for x in args.lens.split(",")):
                res = run_row(B, H, Hkv, D, n, i, args.iters, args.rounds,
                              dev)
                i += 1
                rows.append(res)
                tag = f"H={H}/{Hkv} D={D} B={B} kv_len={n}"
                if not res["numerics_ok"]:
                    bad.append(f"{tag}: outputs differ by "
                               f"{res['max_diff_hip_vs_composition']}")
                if res["auto_routes_hip"] and not res["hip_wins"]:
                    bad.append(f"{tag}: auto routes it to the kernel, whose "
                               "range is not below the composition's")
                torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(md_table(rows))
    if bad:
        sys.exit("bench_decode_attn: " + "; ".join(bad))


if __name__ == "__main__":
    main()
