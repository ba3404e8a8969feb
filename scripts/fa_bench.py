#!/usr/bin/env python3
"""A/B microbench: every flash-attention variant (impl=1/2/3) forward and
backward, TF/s on random data.  Args: S=<seq> B=<batch> Hkv=<kv heads>."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hetu_amd.ops.functional as F

dev = torch.device("cuda", 0)
B, H, Hkv, S, D = 4, 32, 32, 2048, 128
for a in sys.argv[1:]:
    k, v = a.split("=")
    if k == "S": S = int(v)
    if k == "B": B = int(v)
    if k == "Hkv": Hkv = int(v)
torch.manual_seed(0)
q = torch.randn(B, H, S, D, dtype=torch.bfloat16, device=dev)
kk = torch.randn(B, Hkv, S, D, dtype=torch.bfloat16, device=dev)
vv = torch.randn(B, Hkv, S, D, dtype=torch.bfloat16, device=dev)
scale = D ** -0.5
ext = F.ext()

def bench(fn, iters=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters

for causal in (True, False):
    flops = 4 * B * H * S * S * D * (0.5 if causal else 1.0)
    o, lse = ext.flash_attn_fwd(q, kk, vv, causal, scale)
    do = torch.randn_like(o)
    for impl in (1, 2):
        t = bench(lambda: ext.flash_attn_fwd(q, kk, vv, causal, scale, impl),
                  iters=30 if impl > 1 else 5)
        print(f"fwd v{impl} causal={causal}: {t*1e3:.3f} ms  "
              f"{flops/t/1e12:.0f} TF/s")
    ref = ext.flash_attn_bwd(do, q, kk, vv, o, lse, causal, scale, 2)
    for impl in (1, 2, 3) if H == Hkv else (1, 2):
        g = ext.flash_attn_bwd(do, q, kk, vv, o, lse, causal, scale, impl)
        errs = [(a.float() - b.float()).abs().max().item()
                for a, b in zip(g, ref)]
        tb = bench(lambda: ext.flash_attn_bwd(do, q, kk, vv, o, lse, causal,
                                              scale, impl),
                   iters=10 if impl > 1 else 3)
        print(f"bwd v{impl} causal={causal}: {tb*1e3:.3f} ms  "
              f"{2.5*flops/tb/1e12:.0f} TF/s  (vs v2 dq/dk/dv "
              f"{errs[0]:.2e}/{errs[1]:.2e}/{errs[2]:.2e})")
