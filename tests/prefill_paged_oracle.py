"""fp64 oracle and input builder for F.flash_attn_prefill_paged, shared by
tests/test_prefill_paged_cpu.py and tests/test_prefill_paged_gpu.py.

A batch is a list of (context, n): n packed query rows at the end of
context + n cached keys.  The oracle is a plain fp64 loop over (b, h, row).
"""
import math

import torch

import decode_attn_oracle as DO

NAN = float("nan")
D, L = 128, 512
# one row; pure prefill over a 256-row block, tile and page edges; context +
# chunk ending on a tile edge; an empty chunk; the last row of the last page
SEQS = ((0, 1), (0, 257), (63, 65), (300, 0), (449, 63))
TAIL = 3                                  # packed rows past cu_q[B]


def build(H, Hkv, PS, seqs=SEQS, spike=False, dtype=torch.bfloat16,
          device="cpu", seed=0):
    """-> dict: q [T, H, D] (a strided view; T = rows + TAIL), k_pool / v_pool
    (views of P pages of an allocation of P + 2), table, cu_q, kv_len, P and
    the dense k / v [B, Hkv, L, D].  NaN fills every pool row at or past
    kv_len, the page nobody owns and the two pages beyond the view; unneeded
    table entries point at the NaN page; pages of the sequences interleave.
    spike: a key late in the last sequence's context scores about 20 above
    the rest, in a tile after the first (the running max jumps there)."""
    B, MP = len(seqs), L // PS
    lens = [c + n for c, n in seqs]
    cu = [0]
    for _, n in seqs:
        cu.append(cu[-1] + n)
    T = cu[-1] + TAIL
    # q, k and v do not depend on PS: one oracle run serves every page size
    qbuf = torch.randn(T, (H + 2) * D,
                       generator=torch.Generator().manual_seed(seed + H))
    g = torch.Generator().manual_seed(seed + PS)
    _, k, v, _, _ = DO.make_inputs(B, H, Hkv, L, D, dtype=torch.float32,
                                   seed=seed + H)
    if spike:
        qbuf.view(T, H + 2, D)[cu[-2]:cu[-1], :, 0] = 8.0
        k[-1, :, lens[-1] - seqs[-1][1] - 9, 0] = 28.0
    q = qbuf.to(dtype).to(device)[:, :H * D].view(T, H, D)
    k, v = k.to(dtype), v.to(dtype)
    P = B * MP + 1
    perm = torch.randperm(P, generator=g)
    table = perm[:B * MP].view(MP, B).t().contiguous()
    pools = []
    for t in (k, v):
        t = t.clone()
        for b, n in enumerate(lens):
            t[b, :, max(n, 0):] = NAN
        big = torch.full((P + 2, Hkv, PS, D), NAN, dtype=dtype)
        big[table] = t.view(B, Hkv, MP, PS, D).permute(0, 2, 1, 3, 4)
        pools.append(big.to(device)[:P])
    for b, n in enumerate(lens):
        table[b, -(-max(n, 0) // PS):] = perm[-1]
    i32 = dict(dtype=torch.int32, device=device)
    return dict(q=q, k_pool=pools[0], v_pool=pools[1], P=P,
                table=table.to(**i32), cu_q=torch.tensor(cu, **i32),
                kv_len=torch.tensor(lens, **i32), k=k, v=v, seqs=seqs)


def ref(c, drop=None, scale=None):
    """-> (out [T, H, D], lse [T, H], vmax [T, H, D]) in float64; drop =
    (b, j0, j1) removes keys j0 .. j1 - 1 of sequence b."""
    q64, k64, v64 = (c[n].detach().cpu().double() for n in ("q", "k", "v"))
    T, H, _ = q64.shape
    G = H // k64.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    out = torch.zeros(T, H, D, dtype=torch.float64)
    lse = torch.full((T, H), float("-inf"), dtype=torch.float64)
    vmax = torch.zeros(T, H, D, dtype=torch.float64)
    cu, lens = c["cu_q"].tolist(), c["kv_len"].tolist()
    for b, kv in enumerate(lens):
        n = cu[b + 1] - cu[b]
        kv = min(max(kv, 0), L)
        keep = torch.ones(L, dtype=torch.bool)
        if drop is not None and drop[0] == b:
            keep[drop[1]:drop[2]] = False
        for h in range(H):
            for i in range(n):
                vis = keep[:max(kv - n + i + 1, 0)]
                if not vis.any():
                    continue
                kk, vv = k64[b, h // G, :len(vis)][vis], \
                    v64[b, h // G, :len(vis)][vis]
                s = (kk @ q64[cu[b] + i, h]) * scale
                t = cu[b] + i
                lse[t, h] = torch.logsumexp(s, 0)
                out[t, h] = torch.exp(s - lse[t, h]) @ vv
                vmax[t, h] = vv.abs().amax(0)
    return out, lse, vmax
