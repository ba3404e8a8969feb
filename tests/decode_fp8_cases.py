"""Input builders and the append check shared by tests/test_decode_fp8_cpu.py
and tests/test_decode_fp8_gpu.py.  The fp8 KV cache format: e4m3 codes
[B, Hkv, L, D] and one fp32 scale per cached row [B, Hkv, L];
value = float(code) * scale[row]."""
import torch

FP8 = torch.float8_e4m3fn


def make_fp8_inputs(B, H, Hkv, L, D, seed=0, alloc=None):
    """CPU q [B, H, D] bf16, code and scale allocations [.., alloc, ..] built
    directly (no append).  Neighbouring keys' scales differ by at least 2^6
    in both caches (2^-4 u against 2^-11 u', u, u' in [1, 2)), so a scale
    applied to the wrong key misses the bound; values stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    A = L if alloc is None else alloc
    q = torch.randn(B, H, D, generator=g).bfloat16()
    out = [q]
    for big_first in (0, 1):
        codes = (torch.randn(B, Hkv, A, D, generator=g) * 8).to(FP8)
        u = 1 + torch.rand(B, Hkv, A, generator=g)
        big = (torch.arange(A) % 2 == big_first)
        out += [codes, torch.where(big, 2.0 ** -4 * u, 2.0 ** -11 * u)]
    return out                       # q, k, k_scale, v, v_scale


def dequant(codes, scale):
    """Exact in fp64."""
    return codes.cpu().double() * scale.cpu().double().unsqueeze(-1)


def append_inputs(B, S, H, Hkv, D, seed=0, device="cpu"):
    """bf16 k_new (contiguous) and v_new (a view into a fused qkv row) on
    `device`; row magnitudes span 2^-6 .. 2^6 and one row is all zero."""
    g = torch.Generator().manual_seed(seed)
    mag = 2.0 ** torch.randint(-6, 7, (2, B, S, Hkv, 1), generator=g).float()
    mag[0, 0, 0, 0] = 2.0 ** -6
    mag[0, 0, 0, 1] = 2.0 ** 6
    k = (torch.randn(B, S, Hkv, D, generator=g) * mag[0]).bfloat16()
    k[-1, -1, -1] = 0
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).bfloat16()
    v = qkv[..., (H + Hkv) * D:].view(B, S, Hkv, D)
    v.copy_((v.float() * mag[1]).bfloat16())
    v = qkv.to(device)[..., (H + Hkv) * D:].view(B, S, Hkv, D)
    assert not v.is_contiguous()
    return k.to(device), v


def check_append(x, cache, scale, before, end, what):
    """Rows end[b] - S + s of cache / scale against the definition from x
    [B, S, Hkv, D]; every other row equals `before` (cache, scale) bit for
    bit.  Prints whether the codes equal torch's own cast."""
    x = x.cpu().float()
    c8, sc = cache.cpu(), scale.cpu()
    c0, s0 = before[0].cpu().clone(), before[1].cpu().clone()
    B, S = x.shape[:2]
    L = c8.shape[2]
    same = True
    for b in range(B):
        for s in range(S):
            r = int(end[b]) - S + s
            if not 0 <= r < L:
                continue                           # dropped
            xr = x[b, s]
            amax = xr.abs().amax(-1)
            want = amax / torch.full_like(amax, 448.0)      # IEEE division
            assert torch.equal(sc[b, :, r], want), f"{what}: scale {b},{s}"
            code = c8[b, :, r].float()
            err = (code * want[:, None] - xr).abs()
            lim = 2.0 ** -4 * xr.abs() + 2.0 ** -10 * want[:, None]
            assert (err <= lim).all(), f"{what}: element bound {b},{s}"
            top = code.gather(-1, xr.abs().argmax(-1, keepdim=True))[:, 0]
            assert (top.abs()[amax > 0] == 448).all(), f"{what}: amax code"
            assert (code[amax == 0] == 0).all(), f"{what}: zero row"
            ref = torch.where(want[:, None] == 0, torch.zeros_like(xr),
                              xr / want[:, None]).clamp(-448, 448).to(FP8)
            same &= torch.equal(ref.view(torch.uint8),
                                c8[b, :, r].view(torch.uint8))
            c0[b, :, r] = c8[b, :, r]
            s0[b, :, r] = sc[b, :, r]
    assert torch.equal(c0.view(torch.uint8), c8.view(torch.uint8)), \
        f"{what}: a row outside the append changed"
    assert torch.equal(s0, sc), f"{what}: a scale outside the append changed"
    print(f"{what}: codes bit-equal to torch's cast of x / scale: {same}")
