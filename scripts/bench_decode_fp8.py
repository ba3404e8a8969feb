"""fp8 KV cache: the fp8 decode kernel against the bf16 kernel impl=None picks
for the same shape and against copy_ of the fp8 caches, then the quantizing
append against the slice assignment it replaces.

scripts/bench_decode_attn.py's protocol: the sides of a row in one process,
alternating, 7 rounds x 20 calls, device events, median [min-max] of the
rounds.  TB/s counts cache and scale bytes of the attended rows.

    python scripts/bench_decode_fp8.py [--out FILE.md]
"""
import argparse
import statistics
import sys

import torch

import hetu_amd.ops.functional as F

ROUNDS, CALLS = 7, 20
GRID = [(32, 32, 128), (32, 8, 128), (32, 4, 128), (32, 1, 128), (16, 16, 64)]
FP8 = torch.float8_e4m3fn


def time_sides(sides):
    """sides: list of callables -> per side (median, min, max) ms per call."""
    ms = [[] for _ in sides]
    for f in sides:
        f()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for i, f in enumerate(sides):
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / CALLS)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def fmt(t):
    return f"{t[0]:.4f} [{t[1]:.4f}-{t[2]:.4f}]"


def decode_rows(out):
    dev = torch.device("cuda", 0)
    out("| H/Hkv | D | B | kv_len | fp8 ms | TB/s | bf16 ms | TB/s | "
        "copy_ ms | bf16 / fp8 | ceiling | ranges |")
    out("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for H, Hkv, D in GRID:
        for B in (1, 16, 64):
            for n in (512, 2048, 8192):
                q = torch.randn(B, H, D, device=dev).bfloat16()
                kb = torch.randn(B, Hkv, n, D, device=dev).bfloat16()
                vb = torch.randn(B, Hkv, n, D, device=dev).bfloat16()
                k8, v8 = (kb * 8).to(FP8), (vb * 8).to(FP8)
                ks = torch.rand(B, Hkv, n, device=dev) / 8 + 0.01
                vs = torch.rand(B, Hkv, n, device=dev) / 8 + 0.01
                kv = torch.full((B,), n, dtype=torch.int32, device=dev)
                dk, dv = torch.empty_like(k8), torch.empty_like(v8)
                f8, bf, cp = time_sides([
                    lambda: F.flash_attn_decode(q, k8, v8, kv, k_scale=ks,
                                                v_scale=vs),
                    lambda: F.flash_attn_decode(q, kb, vb, kv),
                    lambda: (dk.copy_(k8), dv.copy_(v8))])
                b8 = 2 * B * Hkv * n * (D + 4)
                bb = 2 * B * Hkv * n * D * 2
                disjoint = "disjoint" if f8[2] < bf[1] or bf[2] < f8[1] \
                    else "overlap"
                slower = " (fp8 slower)" if f8[0] > bf[0] else ""
                out(f"| {H}/{Hkv} | {D} | {B} | {n} | {fmt(f8)} | "
                    f"{b8 / f8[0] / 1e9:.2f} | {fmt(bf)} | "
                    f"{bb / bf[0] / 1e9:.2f} | {fmt(cp)} | "
                    f"{bf[0] / f8[0]:.2f}{slower} | "
                    f"{4 * D / (2 * D + 8):.2f} | {disjoint} |")
                del kb, vb, k8, v8, dk, dv


def append_rows(out):
    dev = torch.device("cuda", 0)
    Hkv, D, L, H = 8, 128, 4096, 32
    out("")
    out("| B | append fp8 us | slice assignment (bf16 cache) us |")
    out("|---|---|---|")
    for B in (16, 64):
        qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, device=dev).bfloat16()
        k = torch.randn(B, 1, Hkv, D, device=dev).bfloat16()
        v = qkv[..., (H + Hkv) * D:].view(B, 1, Hkv, D)
        k8 = torch.zeros(B, Hkv, L, D, device=dev, dtype=FP8)
        v8 = torch.zeros_like(k8)
        ks = torch.zeros(B, Hkv, L, device=dev)
        vs = torch.zeros_like(ks)
        kb = torch.zeros(B, Hkv, L, D, device=dev, dtype=torch.bfloat16)
        vb = torch.zeros_like(kb)
        end = torch.full((B,), 1000, dtype=torch.int32, device=dev)

        def assign():
            kb[:, :, 999:1000] = k.permute(0, 2, 1, 3)
            vb[:, :, 999:1000] = v.permute(0, 2, 1, 3)
        a8, sl = time_sides([
            lambda: F.kv_cache_append_fp8(k, v, k8, v8, ks, vs, end), assign])
        us = [tuple(1e3 * x for x in t) for t in (a8, sl)]
        out(f"| {B} | {us[0][0]:.1f} [{us[0][1]:.1f}-{us[0][2]:.1f}] | "
            f"{us[1][0]:.1f} [{us[1][1]:.1f}-{us[1][2]:.1f}] |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fh = open(args.out, "w") if args.out else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    decode_rows(out)
    append_rows(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
