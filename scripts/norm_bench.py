"""Micro-timing for norm kernels at the 7B bench shape."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import hetu_amd.ops.functional as F

def bench(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000  # us

def calls(R=32768, D=4096, dtype=torch.bfloat16):
    """name -> zero-argument call, for every public norm function."""
    x, r, dy, ds = (torch.randn(R, D, dtype=dtype, device="cuda")
                    for _ in range(4))
    w = torch.randn(D, dtype=dtype, device="cuda")
    b = torch.randn(D, dtype=dtype, device="cuda")
    _, mean, rstd = F.layernorm_fwd(x, w, b, 1e-5)
    _, rs = F.rmsnorm_fwd(x, w, 1e-6)
    return {
        "ln fwd": lambda: F.layernorm_fwd(x, w, b, 1e-5),
        "ln bwd": lambda: F.layernorm_bwd(dy, x, w, mean, rstd),
        "rms fwd": lambda: F.rmsnorm_fwd(x, w, 1e-6),
        "rms bwd": lambda: F.rmsnorm_bwd(dy, x, w, rs),
        "ln fwd_res": lambda: F.layernorm_fwd_res(x, r, w, b, 1e-5),
        "ln bwd_res": lambda: F.layernorm_bwd_res(dy, x, w, mean, rstd, ds),
        "rms fwd_res": lambda: F.rmsnorm_fwd_res(x, r, w, 1e-6),
        "rms bwd_res": lambda: F.rmsnorm_bwd_res(dy, x, w, rs, ds),
    }, (x, w, b)

if __name__ == "__main__":
    fns, (x, w, b) = calls()
    for name, fn in fns.items():
        print(f"{name:11s} {bench(fn):8.1f} us")
    # numerics vs fp32 torch
    y = fns["ln fwd"]()[0]
    ln = torch.nn.functional.layer_norm(x.float(), x.shape[-1:], w.float(),
                                        b.float(), 1e-5)
    print("ln fwd err", (y.float() - ln).abs().max().item())
