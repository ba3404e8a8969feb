"""fp64 oracle, input builders and the error bound for F.flash_attn_decode,
shared by tests/test_decode_attn_cpu.py and tests/test_decode_attn_gpu.py.

The oracle is a plain loop over (b, h) on the CPU in float64 on the values
the kernel is given (bf16 inputs are exact in fp64).
"""
import math

import torch

# per output element: |out - ref| <= OUT_BOUND * max_j |v[b, hkv, j, d]| over
# the attended keys: one bf16 rounding of P (MFMA only), one bf16 rounding
# of the output, one unit for fp32 accumulation and exp -- 2^-9 each
OUT_BOUND = 3 * 2.0 ** -9
LSE_BOUND = 1e-3


def decode_ref(q, k, v, kv_len, scale=None):
    """q [B, H, D], k / v [B, Hkv, L, D], kv_len int or [B] ->
    (out [B, H, D] f64, lse [B, H] f64, vmax [B, H, D] f64)."""
    q64, k64, v64 = (t.detach().cpu().double() for t in (q, k, v))
    B, H, D = q64.shape
    Hkv, L = k64.shape[1], k64.shape[2]
    G = H // Hkv
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if isinstance(kv_len, torch.Tensor):
        lens = [int(x) for x in kv_len.detach().cpu().tolist()]
    else:
        lens = [int(kv_len)] * B
    out = torch.zeros(B, H, D, dtype=torch.float64)
    lse = torch.full((B, H), float("-inf"), dtype=torch.float64)
    vmax = torch.zeros(B, H, D, dtype=torch.float64)
    for b in range(B):
        n = min(max(lens[b], 0), L)
        if n == 0:
            continue
        for h in range(H):
            kk, vv = k64[b, h // G, :n], v64[b, h // G, :n]
            s = (kk @ q64[b, h]) * scale
            lse[b, h] = torch.logsumexp(s, 0)
            out[b, h] = torch.exp(s - lse[b, h]) @ vv
            vmax[b, h] = vv.abs().amax(0)
    return out, lse, vmax


def check(out, lse, ref, what="", out_bound=OUT_BOUND, lse_bound=LSE_BOUND):
    """Assert the issue's bounds; rows with kv_len == 0 must be exactly
    out = 0, lse = -inf.  Returns the worst out error in units of vmax."""
    ro, rl, vmax = ref
    o = out.detach().cpu().double()
    l = lse.detach().cpu().double()
    assert o.shape == ro.shape and l.shape == rl.shape, what
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    empty = torch.isinf(rl)
    assert torch.equal(torch.isinf(l) & (l < 0), empty), \
        f"{what}: lse -inf pattern differs"
    assert (o[empty] == 0).all(), f"{what}: kv_len == 0 row is not zero"
    err = (o - ro).abs()
    lim = out_bound * vmax
    worst = (err / vmax.clamp_min(1e-30))[~empty].max().item() \
        if (~empty).any() else 0.0
    assert (err <= lim).all(), \
        f"{what}: out error {worst:.3e} x vmax exceeds {out_bound:.3e}"
    if (~empty).any():
        le = (l - rl)[~empty].abs().max().item()
        assert le <= lse_bound, f"{what}: lse error {le:.3e}"
    return worst


def make_inputs(B, H, Hkv, L, D, dtype=torch.bfloat16, seed=0, alloc=None,
                device="cpu"):
    """randn q [B, H, D] and caches [B, Hkv, L, D] (|scale q.k| stays far
    below 30).  alloc > L makes the caches views of the first L rows of a
    [B, Hkv, alloc, D] allocation."""
    g = torch.Generator().manual_seed(seed)
    A = L if alloc is None else alloc
    q = torch.randn(B, H, D, generator=g).to(dtype).to(device)
    kbig = torch.randn(B, Hkv, A, D, generator=g).to(dtype).to(device)
    vbig = torch.randn(B, Hkv, A, D, generator=g).to(dtype).to(device)
    return q, kbig[:, :, :L], vbig[:, :, :L], kbig, vbig


def poison(kbig, vbig, kv_len):
    """NaN in every K and V row at index >= kv_len[b], inside the view and
    beyond it."""
    for b, n in enumerate(kv_len.tolist()):
        n = max(int(n), 0)
        kbig[b, :, n:] = float("nan")
        vbig[b, :, n:] = float("nan")


# ---- tiny generator weights (engine/generator.py state-dict names) ------
def llama_state(cfg, ffn, seed=0):
    g = torch.Generator().manual_seed(seed)
    hid, dh = cfg.hidden, cfg.hidden // cfg.n_head
    qkv_rows = (cfg.n_head + 2 * cfg.n_kv_head) * dh

    def w(*shape):
        return torch.randn(*shape, generator=g) * 0.05
    state = {"wte.weight": w(cfg.vocab, hid), "lnf.weight": torch.ones(hid),
             "lm_head.weight": w(cfg.vocab, hid)}
    for i in range(cfg.n_layer):
        state[f"l{i}.ln1.weight"] = torch.ones(hid)
        state[f"l{i}.ln2.weight"] = torch.ones(hid)
        state[f"l{i}.attn.wqkv.weight"] = w(qkv_rows, hid)
        state[f"l{i}.attn.wo.weight"] = w(hid, hid)
        state[f"l{i}.mlp.w_in.weight"] = w(2 * ffn, hid)
        state[f"l{i}.mlp.w_out.weight"] = w(hid, ffn)
    return state


def gpt_state(cfg, ffn, seed=0):
    g = torch.Generator().manual_seed(seed)
    hid = cfg.hidden

    def w(*shape):
        return torch.randn(*shape, generator=g) * 0.05
    state = {"wte.weight": w(cfg.vocab, hid),
             "wpe.weight": w(cfg.max_seq, hid),
             "lnf.weight": torch.ones(hid), "lnf.bias": w(hid),
             "lm_head.weight": w(cfg.vocab, hid)}
    for i in range(cfg.n_layer):
        for ln in ("ln1", "ln2"):
            state[f"h{i}.{ln}.weight"] = torch.ones(hid)
            state[f"h{i}.{ln}.bias"] = w(hid)
        for name, (o, n) in (("attn.wqkv", (3 * hid, hid)),
                             ("attn.wo", (hid, hid)),
                             ("mlp.wfc", (ffn, hid)),
                             ("mlp.wproj", (hid, ffn))):
            state[f"h{i}.{name}.weight"] = w(o, n)
            state[f"h{i}.{name}.bias"] = w(o)
    return state
