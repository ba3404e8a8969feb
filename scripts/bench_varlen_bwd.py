#!/usr/bin/env python3
"""Packed-varlen attention backward: the single-kernel path
(F.varlen_attention_bwd -> flash_attn_varlen_bwd) against the per-segment
composition it replaced (host `.tolist()`, then slice copies + the dense
F.flash_attn_bwd + scatter copies for every segment).

Shape: T=16384 packed tokens, H=32, D=128, causal, bf16, 64 ragged segment
lengths drawn from a fixed seed.  Both sides run in this process on the same
inputs, alternating round by round; each round is a device-event window over
`--iters` calls after a warm-up of both.  Needs a GPU; prints one JSON line.

    python scripts/bench_varlen_bwd.py [--iters 20] [--rounds 7]
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

T, H, D, NSEG, SEED = 16384, 32, 128, 64, 0


def ragged_lengths(total=T, n=NSEG, seed=SEED):
    """n positive lengths summing to total, spread ~10x between the
    shortest and the longest."""
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(n, generator=g) * 0.9 + 0.1
    lens = torch.clamp((w / w.sum() * total).long(), min=1)
    lens[lens.argmax()] += total - int(lens.sum())
    assert int(lens.sum()) == total and int(lens.min()) >= 1
    return lens.tolist()


def per_segment_bwd(dout, q, k, v, out, lse, cu_seqlens, causal, scale):
    """The composition varlen_attention_bwd was before the single-kernel
    path (still the CPU / other-D fallback)."""
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    cu = cu_seqlens.tolist()
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        args = [t[s0:s1].permute(1, 0, 2).unsqueeze(0).contiguous()
                for t in (dout, q, k, v, out)]
        ls = lse[:, s0:s1].unsqueeze(0).contiguous()
        dqs, dks, dvs = F.flash_attn_bwd(args[0], args[1], args[2], args[3],
                                         args[4], ls, causal, scale)
        dq[s0:s1] = dqs[0].permute(1, 0, 2)
        dk[s0:s1] = dks[0].permute(1, 0, 2)
        dv[s0:s1] = dvs[0].permute(1, 0, 2)
    return dq, dk, dv


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_varlen_bwd: needs a GPU")
    assert hasattr(F.ext(), "flash_attn_varlen_bwd")
    dev = torch.device("cuda", 0)
    lens = ragged_lengths()
    cu = torch.zeros(NSEG + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    cu = cu.to(dev)
    g = torch.Generator().manual_seed(SEED + 1)
    q, k, v, do = (torch.randn(T, H, D, generator=g).to(torch.bfloat16)
                   .to(dev) for _ in range(4))
    scale = 1.0 / math.sqrt(D)
    o, lse = F.varlen_attention_fwd(q, k, v, cu, True, scale)

    def single():
        return F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True, scale)

    def single_hint():
        return F.varlen_attention_bwd(do, q, k, v, o, lse, cu, True, scale,
                                      max(lens))

    def composed():
        return per_segment_bwd(do, q, k, v, o, lse, cu, True, scale)

    # same results first (and the warm-up of every shape both sides use)
    diffs = [(a.float() - b.float()).abs().max().item()
             for a, b in zip(single(), composed())]
    hint_equal = all(torch.equal(a, b)
                     for a, b in zip(single(), single_hint()))
    sides = {"single_kernel": single, "single_kernel_max_seqlen": single_hint,
             "per_segment": composed}
    for fn in sides.values():
        window_ms(fn, 3)
    times = {n: [] for n in sides}
    for _ in range(args.rounds):            # alternate the sides
        for n, fn in sides.items():
            times[n].append(window_ms(fn, args.iters))
    res = {"bench": "varlen_bwd", "T": T, "H": H, "D": D, "nseg": NSEG,
           "causal": True, "dtype": "bf16", "min_len": min(lens),
           "max_len": max(lens), "iters": args.iters, "rounds": args.rounds,
           "max_abs_diff_dq_dk_dv": diffs,
           "max_seqlen_hint_bit_equal": hint_equal}
    for n, ts in times.items():
        res[n + "_ms"] = {"median": round(statistics.median(ts), 4),
                          "min": round(min(ts), 4), "max": round(max(ts), 4)}
    res["per_segment_over_single_kernel"] = round(
        statistics.median(times["per_segment"])
        / statistics.median(times["single_kernel"]), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
