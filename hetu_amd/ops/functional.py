"""Kernel dispatch: hand-written HIP/CDNA4 extension on GPU, torch on CPU.

Every hot op of the reference kernel set
(/root/reference/hetu/impl/kernel/ — RMSNorm.cu, FusedLayerNorm.cu,
SwiGLU.cu, rotary.cu, Softmax.cu, SoftmaxCrossEntropySparse.cu,
VocabParallelCrossEntropyLoss.cu, Dropout.cu, EmbeddingLookup.cu,
Optimizers.cu AdamCuda, FlashAttention.cu, MatMul.cu) has an MI355X-native
equivalent here. On a ROCm GPU the call MUST go through the in-tree
_hetu_hip extension (hand-written gfx950 kernels); if the extension is
missing on a CUDA/HIP device we raise — no silent eager fallback. On CPU the
plain torch implementations below serve as the numerics reference used by
the unit tests.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch

_EXT = None
_EXT_ERR = None


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        import importlib.util
        here = os.path.dirname(__file__)
        cands = [os.path.join(here, "hip", f) for f in
                 os.listdir(os.path.join(here, "hip"))
                 if f.startswith("_hetu_hip") and f.endswith(".so")] \
            if os.path.isdir(os.path.join(here, "hip")) else []
        if not cands:
            raise ImportError("_hetu_hip extension not built "
                              "(run python setup.py build_ext --inplace)")
        spec = importlib.util.spec_from_file_location("_hetu_hip", cands[0])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _EXT = mod
    except Exception as e:  # noqa: BLE001
        _EXT_ERR = e
        _EXT = None
    return _EXT


def ext():
    e = _load_ext()
    if e is None:
        raise RuntimeError(
            f"hetu_amd HIP extension required on GPU but not available: "
            f"{_EXT_ERR}")
    return e


def has_ext() -> bool:
    return _load_ext() is not None


def _gpu(*ts) -> bool:
    return any(isinstance(t, torch.Tensor) and t.is_cuda for t in ts)


# Debug bisect switch: HETU_AMD_TORCH_FALLBACK="fa,ln,adam,..." routes the
# named kernel families to the plain-torch reference implementations even
# on GPU (they are device-agnostic).  Families: fa, qkvfa, ln, rms, gelu,
# silu, swiglu, adam, ce, vce, embed, softmax, rope, dropout, moe.
_TORCH_FB = frozenset(
    s for s in os.environ.get("HETU_AMD_TORCH_FALLBACK", "").split(",") if s)


def _use_hip(family: str, *ts) -> bool:
    return _gpu(*ts) and family not in _TORCH_FB


# Debug bisect switch: HETU_AMD_FA1=1 routes dense flash attention to the
# v1 kernels (impl=1); otherwise the extension picks the variant by shape.
_FA_IMPL = 1 if os.environ.get("HETU_AMD_FA1", "")[:1] == "1" else 0


# ---------------------------------------------------------------------------
# RMSNorm / LayerNorm, plain and with the fused residual add (reference
# RMSNorm.cu, FusedLayerNorm.cu:455-760).  On GPU all eight go through the
# extension's two entry points, norm_fwd and norm_bwd.
# ---------------------------------------------------------------------------

def _opt(t, dtype=None):
    if t is None:
        return None
    t = t.contiguous()
    return t if dtype is None else t.to(dtype)


def _norm_fwd_hip(x, resid, w, b, eps):
    """LayerNorm when b is given, else RMSNorm; s = x + resid is normed and
    returned when resid is given.  Returns (y, [s,] [mean,] rstd)."""
    return tuple(ext().norm_fwd(x.contiguous(), _opt(resid),
                                _opt(w, x.dtype), _opt(b, x.dtype), eps))


def _norm_bwd_hip(dy, x, w, mean, rstd, dresid=None):
    """LayerNorm when mean is given; dresid is added into dx.
    Returns (dx, dw, [db])."""
    return tuple(ext().norm_bwd(dy.contiguous(), x.contiguous(),
                                _opt(w, x.dtype), _opt(mean),
                                rstd.contiguous(), _opt(dresid)))


def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """returns (y, rstd[rows] fp32)"""
    if _use_hip("rms", x):
        return _norm_fwd_hip(x, None, w, None, eps)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    y = (xf * rstd) * w.float()
    return y.to(x.dtype), rstd.squeeze(-1)


def rmsnorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor,
                rstd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if _use_hip("rms", x):
        return _norm_bwd_hip(dy, x, w, None, rstd)
    xf, dyf, wf = x.float(), dy.float(), w.float()
    r = rstd.unsqueeze(-1)
    xhat = xf * r
    wdy = dyf * wf
    c = (wdy * xhat).mean(-1, keepdim=True)
    dx = (wdy - xhat * c) * r
    dw = (dyf * xhat).reshape(-1, x.shape[-1]).sum(0)
    return dx.to(x.dtype), dw.to(w.dtype)


def layernorm_fwd(x, w, b, eps):
    """returns (y, mean[rows] fp32, rstd[rows] fp32)"""
    if _use_hip("ln", x):
        return _norm_fwd_hip(x, None, w, b, eps)
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = xf.var(-1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mean) * rstd * w.float() + b.float()
    return y.to(x.dtype), mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(dy, x, w, mean, rstd):
    if _use_hip("ln", x):
        return _norm_bwd_hip(dy, x, w, mean, rstd)
    xf, dyf, wf = x.float(), dy.float(), w.float()
    mu = mean.unsqueeze(-1)
    r = rstd.unsqueeze(-1)
    xhat = (xf - mu) * r
    wdy = dyf * wf
    c1 = wdy.mean(-1, keepdim=True)
    c2 = (wdy * xhat).mean(-1, keepdim=True)
    dx = (wdy - c1 - xhat * c2) * r
    D = x.shape[-1]
    dw = (dyf * xhat).reshape(-1, D).sum(0)
    db = dyf.reshape(-1, D).sum(0)
    return dx.to(x.dtype), dw.to(w.dtype), db.to(w.dtype)


def rmsnorm_fwd_res(x, resid, w, eps):
    """Fused residual-add + RMSNorm: s = x + resid; y = RMS(s).
    Returns (y, s, rstd)."""
    if _use_hip("rms", x):
        return _norm_fwd_hip(x, resid, w, None, eps)
    s = x + resid
    y, rstd = rmsnorm_fwd(s, w, eps)
    return y, s, rstd


def rmsnorm_bwd_res(dy, s, w, rstd, ds_ext=None):
    """returns (dsum = dRMS/ds (+ ds_ext), dw); dsum is the grad of both
    add inputs."""
    if _use_hip("rms", s):
        return _norm_bwd_hip(dy, s, w, None, rstd, ds_ext)
    dx, dw = rmsnorm_bwd(dy, s, w, rstd)
    if ds_ext is not None:
        dx = dx + ds_ext
    return dx, dw


def layernorm_fwd_res(x, resid, w, b, eps):
    """Fused residual-add + LayerNorm: s = x + resid; y = LN(s).
    Returns (y, s, mean, rstd)."""
    if _use_hip("ln", x):
        return _norm_fwd_hip(x, resid, w, b, eps)
    s = x + resid
    y, mean, rstd = layernorm_fwd(s, w, b, eps)
    return y, s, mean, rstd


def layernorm_bwd_res(dy, s, w, mean, rstd, ds_ext=None):
    """returns (dsum = dLN/ds (+ ds_ext), dw, db); dsum is the grad of
    both add inputs."""
    if _use_hip("ln", s):
        return _norm_bwd_hip(dy, s, w, mean, rstd, ds_ext)
    dx, dw, db = layernorm_bwd(dy, s, w, mean, rstd)
    if ds_ext is not None:
        dx = dx + ds_ext
    return dx, dw, db


# ---------------------------------------------------------------------------
# SwiGLU: y = silu(x1) * x2 over last-dim halves (reference SwiGLU.cu:14,30)
# ---------------------------------------------------------------------------

def swiglu_fwd(x):
    if _use_hip("swiglu", x):
        return ext().swiglu_fwd(x.contiguous())
    x1, x2 = x.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(x1) * x2).to(x.dtype)


def swiglu_bwd(dy, x):
    if _use_hip("swiglu", x):
        return ext().swiglu_bwd(dy.contiguous(), x.contiguous())
    x1, x2 = x.float().chunk(2, dim=-1)
    dyf = dy.float()
    sig = torch.sigmoid(x1)
    silu = x1 * sig
    dsilu = sig * (1 + x1 * (1 - sig))
    dx1 = dyf * x2 * dsilu
    dx2 = dyf * silu
    return torch.cat([dx1, dx2], dim=-1).to(x.dtype)


def colsum(x2d: torch.Tensor) -> torch.Tensor:
    """Column sum of a 2-D tensor -> fp32 [C].  On GPU: hand HIP kernel
    (reduce.hip) — also the hipGraph-replay-safe replacement for the
    at::native column reduce, which returns garbage from the 2nd replay of
    a captured step on some shapes (ROCm 7.2; see
    profiles/r02_capture_replay_bug.md)."""
    if _use_hip("colsum", x2d):
        return ext().colsum(x2d.contiguous())
    return x2d.float().sum(0)


# ---------------------------------------------------------------------------
# Activations (fused fwd/bwd; reference Gelu.cu / Activation.cu)
# ---------------------------------------------------------------------------

def gelu_fwd(x):
    if _use_hip("gelu", x):
        return ext().gelu_fwd(x.contiguous())
    return torch.nn.functional.gelu(x, approximate="tanh")


def gelu_bwd(dy, x):
    if _use_hip("gelu", x):
        return ext().gelu_bwd(dy.contiguous(), x.contiguous())
    xf = x.float()
    c = 0.7978845608028654  # sqrt(2/pi)
    a = 0.044715
    t = torch.tanh(c * (xf + a * xf ** 3))
    dt = (1 - t * t) * c * (1 + 3 * a * xf * xf)
    return (dy.float() * (0.5 * (1 + t) + 0.5 * xf * dt)).to(x.dtype)


def silu_fwd(x):
    if _use_hip("silu", x):
        return ext().silu_fwd(x.contiguous())
    return torch.nn.functional.silu(x)


def silu_bwd(dy, x):
    if _use_hip("silu", x):
        return ext().silu_bwd(dy.contiguous(), x.contiguous())
    s = torch.sigmoid(x.float())
    return (dy.float() * s * (1 + x.float() * (1 - s))).to(x.dtype)


# ---------------------------------------------------------------------------
# RoPE (reference rotary.cu:97-185; NeoX-style half rotation)
# ---------------------------------------------------------------------------

def rope_fwd(x, cos, sin, interleaved: bool = False):
    """x: [B, S, H, D] (or [S, H, D] packed); cos/sin: [S, D/2] fp32."""
    if _use_hip("rope", x):
        return ext().rope_fwd(x.contiguous(), cos.contiguous(),
                              sin.contiguous())
    return _rope_ref(x, cos, sin, False)


def rope_bwd(dy, cos, sin, interleaved: bool = False):
    if _use_hip("rope", dy):
        return ext().rope_bwd(dy.contiguous(), cos.contiguous(),
                              sin.contiguous())
    return _rope_ref(dy, cos, sin, True)


def _rope_ref(x, cos, sin, backward: bool):
    xf = x.float()
    D = x.shape[-1]
    x1, x2 = xf[..., :D // 2], xf[..., D // 2:]
    shape = [1] * x.ndim
    shape[-3] = cos.shape[0]   # seq dim of [B, S, H, D] or packed [S, H, D]
    shape[-1] = D // 2
    c = cos.reshape(shape)
    s = sin.reshape(shape)
    if backward:
        s = -s
    y1 = x1 * c - x2 * s
    y2 = x2 * c + x1 * s
    return torch.cat([y1, y2], dim=-1).to(x.dtype)


# ---------------------------------------------------------------------------
# Softmax (row; reference Softmax.cu:151,202,315)
# ---------------------------------------------------------------------------

def softmax_fwd(x, dim=-1):
    # the HIP kernel vectorizes rows by 8; narrow rows (e.g. MoE gate
    # logits over a handful of experts) take the torch path
    if _use_hip("softmax", x) and dim in (-1, x.ndim - 1) \
            and x.shape[-1] % 8 == 0:
        return ext().softmax_fwd(x.contiguous())
    return torch.softmax(x.float(), dim=dim).to(x.dtype)


def softmax_bwd(dy, y, dim=-1):
    if _use_hip("softmax", dy) and dim in (-1, dy.ndim - 1) \
            and dy.shape[-1] % 8 == 0:
        return ext().softmax_bwd(dy.contiguous(), y.contiguous())
    dyf, yf = dy.float(), y.float()
    dx = (dyf - (dyf * yf).sum(dim, keepdim=True)) * yf
    return dx.to(dy.dtype)


# ---------------------------------------------------------------------------
# Sparse softmax cross-entropy (reference SoftmaxCrossEntropySparse.cu)
# and TP-sharded vocab-parallel CE (VocabParallelCrossEntropyLoss.cu:15,70)
# ---------------------------------------------------------------------------

def softmax_ce_fwd(logits, labels, ignore_index: int = -100):
    """logits [N, V], labels [N] -> (loss[N] fp32, logsumexp[N] fp32)."""
    if _use_hip("ce", logits):
        return ext().softmax_ce_fwd(logits.contiguous(),
                                    labels.contiguous(), ignore_index)
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    mask = labels != ignore_index
    safe = labels.clamp(min=0)
    picked = lf.gather(-1, safe.unsqueeze(-1)).squeeze(-1)
    loss = torch.where(mask, lse - picked, torch.zeros_like(lse))
    return loss, lse


def softmax_ce_bwd(dloss, logits, labels, lse, ignore_index: int = -100):
    if _use_hip("ce", logits):
        return ext().softmax_ce_bwd(dloss.contiguous(), logits.contiguous(),
                                    labels.contiguous(), lse.contiguous(),
                                    ignore_index)
    lf = logits.float()
    p = torch.exp(lf - lse.unsqueeze(-1))
    mask = (labels != ignore_index)
    safe = labels.clamp(min=0)
    onehot = torch.zeros_like(lf).scatter_(-1, safe.unsqueeze(-1), 1.0)
    g = (p - onehot) * (dloss * mask.to(dloss.dtype)).unsqueeze(-1)
    return g.to(logits.dtype)


def vocab_parallel_ce_local_stats(logits, labels, vocab_start, vocab_end,
                                  ignore_index: int = -100):
    """Per-rank stage of the vocab-parallel CE: local max, local sum-exp (at
    given max), and predicted-logit for labels owned by this shard.
    Cross-rank max/sum allreduce happens at op level (see graph/ops/loss.py).
    """
    if _use_hip("vce", logits):
        return ext().vp_ce_local(logits.contiguous(), labels.contiguous(),
                                 vocab_start, vocab_end, ignore_index)
    lf = logits.float()
    lmax = lf.max(-1).values
    in_shard = (labels >= vocab_start) & (labels < vocab_end) & \
               (labels != ignore_index)
    local_idx = (labels - vocab_start).clamp(min=0, max=lf.shape[-1] - 1)
    picked = lf.gather(-1, local_idx.unsqueeze(-1)).squeeze(-1)
    picked = torch.where(in_shard, picked, torch.zeros_like(picked))
    return lmax, picked


# ---------------------------------------------------------------------------
# Dropout (Philox-seeded, stateless; reference Dropout.cu)
# ---------------------------------------------------------------------------

def dropout_fwd(x, p: float, seed: int, offset: int):
    if p <= 0.0:
        return x, None
    if _use_hip("dropout", x):
        return ext().dropout_fwd(x.contiguous(), p, seed, offset)
    g = torch.Generator(device="cpu").manual_seed(seed + offset)
    mask = (torch.rand(x.shape, generator=g, device=x.device) >= p)
    y = x * mask.to(x.dtype) / (1.0 - p)
    return y, mask


def dropout_bwd(dy, mask, p: float, seed: int, offset: int):
    if p <= 0.0:
        return dy
    if _use_hip("dropout", dy):
        return ext().dropout_bwd(dy.contiguous(), mask, p, seed, offset)
    return dy * mask.to(dy.dtype) / (1.0 - p)


# ---------------------------------------------------------------------------
# Embedding (reference EmbeddingLookup.cu)
# ---------------------------------------------------------------------------

def embedding_fwd(table, ids):
    if _use_hip("embed", table):
        return ext().embedding_fwd(table.contiguous(), ids.contiguous())
    return table[ids]


def embedding_bwd(dy, ids, num_rows: int):
    if _use_hip("embed", dy):
        return ext().embedding_bwd(dy.contiguous(), ids.contiguous(),
                                   num_rows)
    D = dy.shape[-1]
    g = torch.zeros(num_rows, D, dtype=torch.float32, device=dy.device)
    g.index_add_(0, ids.reshape(-1), dy.reshape(-1, D).float())
    return g.to(dy.dtype)


# ---------------------------------------------------------------------------
# Fused Adam (reference Optimizers.cu:145 AdamCuda — m/v update + bias corr
# + weight decay in one pass; fp32 master weights)
# ---------------------------------------------------------------------------

def adam_step(param32, grad, m, v, lr, beta1, beta2, eps, weight_decay,
              step, param_out16: Optional[torch.Tensor] = None,
              bc_dev: Optional[torch.Tensor] = None):
    """bc_dev: optional fp32 device tensor [2] = (1-b1^t, 1-b2^t); when
    given, the kernel reads bias corrections from it — this keeps a
    hipGraph-captured train step correct across replays (the host updates
    the pinned source of bc_dev between replays)."""
    if _use_hip("adam", param32):
        ext().adam_step(param32, grad, m, v, lr, beta1, beta2, eps,
                        weight_decay, step,
                        param_out16 if param_out16 is not None
                        else grad.new_empty(0),
                        bc_dev if bc_dev is not None
                        else param32.new_empty(0))
        return
    gf = grad.float()
    if weight_decay != 0.0:
        gf = gf + weight_decay * param32
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    update = (m / bc1) / (torch.sqrt(v / bc2) + eps)
    param32.add_(update, alpha=-lr)
    if param_out16 is not None:
        param_out16.copy_(param32.to(param_out16.dtype))


# ---------------------------------------------------------------------------
# Flash attention (reference FlashAttention.cu wraps flash_attn 2;
# here: hand-written CDNA4 MFMA kernel, see ops/hip/attention.hip)
# ---------------------------------------------------------------------------

def flash_attn_fwd(q, k, v, causal: bool, scale: Optional[float] = None):
    """q,k,v: [B, H, S, D] (kv may have fewer heads - GQA).
    Returns (out, lse[B,H,S] fp32)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _use_hip("fa", q):
        return ext().flash_attn_fwd(q.contiguous(), k.contiguous(),
                                    v.contiguous(), causal, scale, _FA_IMPL)
    return _attn_ref_fwd(q, k, v, causal, scale)


def flash_attn_bwd(dout, q, k, v, out, lse, causal: bool,
                   scale: Optional[float] = None):
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if _use_hip("fa", q):
        return ext().flash_attn_bwd(dout.contiguous(), q.contiguous(),
                                    k.contiguous(), v.contiguous(),
                                    out.contiguous(), lse.contiguous(),
                                    causal, scale, _FA_IMPL)
    return _attn_ref_bwd(dout, q, k, v, out, lse, causal, scale)


def _repeat_kv(k, n_head):
    if k.shape[1] == n_head:
        return k
    rep = n_head // k.shape[1]
    return k.repeat_interleave(rep, dim=1)


def _attn_ref_fwd(q, k, v, causal, scale):
    B, H, S, D = q.shape
    kf = _repeat_kv(k, H).float()
    vf = _repeat_kv(v, H).float()
    qf = q.float()
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        Skv = kf.shape[2]
        mask = torch.ones(S, Skv, dtype=torch.bool, device=q.device).tril(
            diagonal=Skv - S)
        scores = scores.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(scores, dim=-1)
    p = torch.exp(scores - lse.unsqueeze(-1))
    out = torch.matmul(p, vf)
    return out.to(q.dtype), lse


def _attn_ref_bwd(dout, q, k, v, out, lse, causal, scale):
    # delta MUST come from the global (dout . out) rowsum, not the local
    # (dp*p).sum: under ring attention this reference runs per KV block
    # with the global lse, where the two differ.
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    kf = _repeat_kv(k, H).float()
    vf = _repeat_kv(v, H).float()
    qf, dof = q.float(), dout.float()
    scores = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        Skv = kf.shape[2]
        mask = torch.ones(S, Skv, dtype=torch.bool, device=q.device).tril(
            diagonal=Skv - S)
        scores = scores.masked_fill(~mask, float("-inf"))
    p = torch.exp(scores - lse.unsqueeze(-1).float())
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * out.float()).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    if Hkv != H:
        rep = H // Hkv
        dk = dk.reshape(B, Hkv, rep, -1, D).sum(2)
        dv = dv.reshape(B, Hkv, rep, -1, D).sum(2)
    return dq.to(q.dtype), dk.to(k.dtype), dv.to(v.dtype)


# ---------------------------------------------------------------------------
# Decode attention: one query token per sequence against a KV cache read in
# place (ops/hip/attention_decode.hip; docs/KERNELS.md "Decode attention")
# ---------------------------------------------------------------------------

_DECODE_IMPLS = (None, "torch", "hip")


def _decode_hip_ineligible(q, k_cache, v_cache, kv_len) -> Optional[str]:
    """Why ops/hip/attention_decode.hip cannot take this input, or None."""
    ts = (("q", q), ("k_cache", k_cache), ("v_cache", v_cache))
    for name, t in ts:
        if not t.is_cuda:
            return f"{name} is not on the GPU"
        if t.dtype != torch.bfloat16:
            return f"{name} is {t.dtype}, not bf16"
    if q.shape[-1] not in (64, 128):
        return f"head dim {q.shape[-1]} is not 64 or 128"
    if k_cache.shape[1] < 1 or q.shape[1] % k_cache.shape[1]:
        return (f"H ({q.shape[1]}) is not a multiple of Hkv "
                f"({k_cache.shape[1]})")
    if isinstance(kv_len, torch.Tensor):
        if not kv_len.is_cuda:
            return "kv_len is a CPU tensor (pass an int or a device tensor)"
        if kv_len.dtype != torch.int32:
            return f"kv_len is {kv_len.dtype}, not int32"
    for name, t in ts:
        if t.stride(-1) != 1:
            return f"{name} has a non-unit last stride"
        # (the stride of a size-1 dim is never multiplied by anything)
        if any(s % 8 for s, n in zip(t.stride()[:-1], t.shape) if n > 1) \
                or t.data_ptr() % 16:
            return f"{name} is not 16-byte aligned in every stride"
    return None


def _decode_auto_hip(B: int, Hkv: int, L: int) -> bool:
    """Where the HIP kernel was ahead of the composition it replaces with
    disjoint min-max ranges in scripts/bench_decode_attn.py
    (profiles/r05_decode_attention.md, per-shape table): all 27 rows, bf16,
    D = 128 at H/Hkv 32/32 and 32/8 and D = 64 at 16/16, B in {1, 16, 64},
    kv_len in {512, 2048, 8192}, by 4.2-36x.  The smallest row (B = 1,
    kv_len 512) is the kernel's floor of two launches, 12 us against the
    composition's 73-85 us, so no corner goes to the torch branch.  A
    further 18 rows at H/Hkv 32/4, 32/1 and 24/4 (section 3a there) win by
    2.1-52x.  Shapes between and beyond the measured ones pass without
    having been timed: that part is extrapolated."""
    return True


def _decode_check_shapes(q, k_cache, v_cache):
    if q.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4 \
            or k_cache.shape != v_cache.shape \
            or k_cache.shape[0] != q.shape[0] \
            or k_cache.shape[3] != q.shape[2]:
        raise ValueError(
            "flash_attn_decode: need q [B, H, D] and k_cache, v_cache "
            f"[B, Hkv, L, D]; got {tuple(q.shape)}, {tuple(k_cache.shape)}, "
            f"{tuple(v_cache.shape)}")


def _decode_torch(q, k_cache, v_cache, kv_len, scale):
    """fp32 math on the given inputs, one rounding to q's dtype.  An int
    length slices the cache and repeats the KV heads, the composition the
    generators ran before the kernel existed (bit-identical to it); a
    tensor length masks, by selection: rows past kv_len[b] may hold
    anything."""
    B, H, D = q.shape
    Hkv, L = k_cache.shape[1], k_cache.shape[2]
    rep = H // Hkv
    qt = q.unsqueeze(2)                                   # [B, H, 1, D]
    if not isinstance(kv_len, torch.Tensor):
        n = min(max(int(kv_len), 0), L)
        kk = k_cache[:, :, :n]
        vv = v_cache[:, :, :n]
        kr = kk.repeat_interleave(rep, dim=1) if rep > 1 else kk
        vr = vv.repeat_interleave(rep, dim=1) if rep > 1 else vv
        scores = (qt.float() @ kr.float().transpose(-1, -2)) * scale
        p = torch.softmax(scores, dim=-1)
        o = (p @ vr.float()).to(q.dtype)
        return o.squeeze(2), torch.logsumexp(scores, dim=-1).squeeze(-1)
    n = kv_len.to(q.device).clamp(0, L).view(B, 1, 1)
    valid = torch.arange(L, device=q.device).view(1, 1, L) < n   # [B, 1, L]
    keep = valid.unsqueeze(-1)                                   # [B, 1, L, 1]
    kf = torch.where(keep, k_cache.float(), 0.0)
    vf = torch.where(keep, v_cache.float(), 0.0)
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = (qt.float() @ kf.transpose(-1, -2)) * scale         # [B,H,1,L]
    scores = scores.masked_fill(~valid.unsqueeze(1), float("-inf"))
    lse = torch.logsumexp(scores, dim=-1)                        # [B, H, 1]
    p = torch.where(valid.unsqueeze(1),
                    torch.exp(scores - lse.unsqueeze(-1)), 0.0)
    o = (p @ vf).to(q.dtype)
    return o.squeeze(2), lse.squeeze(-1)


def flash_attn_decode_on_hip(q, k_cache, v_cache, kv_len=0, impl=None) -> bool:
    """Whether flash_attn_decode sends this call to the HIP kernel (with
    impl="hip" always: an ineligible input is then an error there).  The
    generators ask before they choose between the device length tensor and
    the Python int, which keeps the torch branch on its slicing form."""
    if impl == "torch":
        return False
    if impl == "hip":
        return True
    return (_decode_hip_ineligible(q, k_cache, v_cache, kv_len) is None
            and "fa" not in _TORCH_FB
            and _decode_auto_hip(q.shape[0], k_cache.shape[1],
                                 k_cache.shape[2]))


def flash_attn_decode(q, k_cache, v_cache, kv_len, scale=None,
                      num_splits: int = 0, impl=None):
    """Attention of ONE new token per sequence over a KV cache.

    q [B, H, D]; k_cache, v_cache [B, Hkv, L, D] (H % Hkv == 0), taken with
    their strides: a layer slice of a [n_layer, B, Hkv, L, D] cache and a q
    that is a view into a fused qkv output are read in place.  kv_len is an
    int (every row attends keys 0 .. kv_len-1) or an int32 tensor [B]; it
    is clamped to [0, L] and rows of the cache past it may hold anything.
    Returns (out [B, H, D] in q's dtype, lse [B, H] fp32 = log sum_j
    exp(scale * q.k_j), the definition flash_attn_fwd uses); kv_len == 0
    gives out = 0, lse = -inf.

    impl: "hip" = the split-KV kernel (bf16, D 64 or 128, GPU; an error on
    anything else, never a fallback); "torch" = fp32 torch math; None = the
    kernel where it is eligible and measured ahead, else torch.  num_splits
    (HIP only): 0 lets the launcher choose from B, Hkv, L and the CU count
    (never from the values of kv_len, so a captured graph stays valid);
    >= 1 forces it."""
    if impl not in _DECODE_IMPLS:
        raise ValueError("flash_attn_decode: impl must be None, 'torch' or "
                         f"'hip', got {impl!r}")
    _decode_check_shapes(q, k_cache, v_cache)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if not flash_attn_decode_on_hip(q, k_cache, v_cache, kv_len, impl):
        return _decode_torch(q, k_cache, v_cache, kv_len, scale)
    why = _decode_hip_ineligible(q, k_cache, v_cache, kv_len)
    if why is not None:
        raise RuntimeError(f"flash_attn_decode(impl='hip'): {why}")
    if not isinstance(kv_len, torch.Tensor):
        # a fill kernel, not a host-to-device copy
        n = min(max(int(kv_len), 0), k_cache.shape[2])
        kv_len = torch.full((q.shape[0],), n, dtype=torch.int32,
                            device=q.device)
    out, lse = ext().flash_attn_decode(q, k_cache, v_cache, kv_len,
                                       float(scale), int(num_splits))
    return out, lse


# ---------------------------------------------------------------------------
# GEMM — hand-written MFMA bf16 kernel for the transformer hot path;
# library (hipBLASLt via torch.matmul) for general shapes.
# ---------------------------------------------------------------------------

# GEMM routing.  Three GEMMs per linear layer (profiles/r03_wgrad_gemm.md):
#   forward x @ W^T (TN): hipBLASLt via F.linear (~1.6 PF/s on the
#     transformer shapes).  The 128^2 hand kernel (ops/hip/gemm.hip, ~910
#     TF) loses there; HETU_AMD_GEMM=hip forces it for tests and
#     microbenchmarks.
#   dgrad gy @ W (NN): linear_dgrad() below.  The library's NN form runs at
#     ~1.35 PF/s, so for large shapes W is copied to W^T
#     (ops/hip/transpose.hip) and the forward's TN form is called instead
#     (profiles/r04_dgrad_layout.md).
#   wgrad gy^T @ x (NT over tokens): linear_wgrad() below, which picks
#     between the library and the 256^2 transposed-read hand kernel
#     (ops/hip/gemm_wgrad.hip) per shape.
_HETU_GEMM = os.environ.get("HETU_AMD_GEMM", "blas")  # hip | blas
_HETU_WGRAD = os.environ.get("HETU_AMD_WGRAD", "auto")  # auto | hip | blas
_WGRAD_IMPLS = ("auto", "hip", "blas")


def _wgrad_hip_eligible(gy2, x2) -> bool:
    """What ops/hip/gemm_wgrad.hip takes: full 256x256 output tiles and
    whole 64-token K-tiles of contiguous bf16 GPU operands."""
    return (gy2.is_cuda and x2.is_cuda and gy2.device == x2.device
            and gy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16
            and gy2.is_contiguous() and x2.is_contiguous()
            and gy2.shape[0] == x2.shape[0] and gy2.shape[0] > 0
            and gy2.shape[0] % 64 == 0
            and gy2.shape[1] > 0 and gy2.shape[1] % 256 == 0
            and x2.shape[1] > 0 and x2.shape[1] % 256 == 0)


def _wgrad_auto_hip(T: int, N: int, K: int) -> bool:
    """Shape classes where the hand kernel beat hipBLASLt with
    non-overlapping min-max ranges in scripts/bench_wgrad.py
    (profiles/r03_wgrad_gemm.md, per-shape table): outputs of 256, 768 and
    1024 tiles of 256x256 (16x16, 48x16, 64x16, 16x64), at T = 2048, 8192
    and 32768 tokens (1.17-1.26x).  What those have in common is the rule:
    whole rounds of the 256 CUs at one block per CU, and a tile grid the
    kernel folds into 8x4 rectangles per XCD (N/256 % 8 == 0, K/256 % 4
    == 0) so the operand panels are shared through L2.  Other multiples of
    256 tiles (512, 1280, ...) have the same properties but were not
    timed: that part is extrapolated.  A partial last round (the library's
    stream-K balances it, this kernel does not), grids without the fold
    and shorter contractions stay on the library."""
    tn, tk = N // 256, K // 256
    return tn % 8 == 0 and tk % 4 == 0 and (tn * tk) % 256 == 0 and T >= 2048


_HETU_WGRAD_BIAS = os.environ.get("HETU_AMD_WGRAD_BIAS", "1")  # 1 | 0


def _wgrad_bias_auto_fused(T: int, N: int, K: int, switch=None) -> bool:
    """Whether linear_wgrad_bias(impl="auto") takes the fused kernel for an
    eligible [T, N] x [T, K] input: exactly where _wgrad_auto_hip admits
    the shape, unless HETU_AMD_WGRAD_BIAS=0 (then the unfused pair runs
    everywhere, so both sides can be profiled from one tree).

    scripts/bench_wgrad_bias.py (profiles/r06_wgrad_bias.md, per-shape
    table) times fused against linear_wgrad + colsum on the four layer
    shapes at T = 32768 and 8192, all of which _wgrad_auto_hip admits; the
    table there states which rows are ahead with disjoint min-max ranges.
    Shapes the wgrad rule admits but the script does not time (other
    multiples of 256 tiles, T between the measured ones) pass untimed:
    that part is extrapolated."""
    switch = _HETU_WGRAD_BIAS if switch is None else switch
    return str(switch) != "0" and _wgrad_auto_hip(T, N, K)


class _DbRequest:
    """linear_wgrad_bias asks linear_wgrad for the column sums of gy: the
    hand-kernel routes fill `db` from the same launch, the library routes
    leave it None."""
    __slots__ = ("db",)

    def __init__(self):
        self.db = None


# set only for the duration of linear_wgrad_bias's call of linear_wgrad,
# which stays the one place that routes a weight-gradient GEMM
_wgrad_db_request = None


def _wgrad_hand_kernel(gy2, x2, req, fuse: bool):
    if req is not None and fuse:
        dw, req.db = ext().gemm_wgrad_bias_bf16(gy2, x2)
        return dw
    return ext().gemm_wgrad_bf16(gy2, x2)


def linear_wgrad(gy, x, impl=None):
    """Weight gradient of y = x @ W^T: dW [N, K] = gy[..., N]^T @ x[..., K]
    over the flattened leading (token) dims.

    impl: "blas" = torch.matmul (hipBLASLt); "hip" = the hand kernel, an
    error if the input is not eligible (never a fallback); "auto" = the
    hand kernel where it measured faster, else the library.  None takes
    HETU_AMD_WGRAD (default auto)."""
    global _wgrad_db_request
    req, _wgrad_db_request = _wgrad_db_request, None
    impl = _HETU_WGRAD if impl is None else impl
    if impl not in _WGRAD_IMPLS:
        raise ValueError(f"linear_wgrad: impl must be one of {_WGRAD_IMPLS}, "
                         f"got {impl!r}")
    gy2 = gy.reshape(-1, gy.shape[-1])
    x2 = x.reshape(-1, x.shape[-1])
    if impl == "hip":
        if not _wgrad_hip_eligible(gy2, x2):
            raise RuntimeError(
                "linear_wgrad(impl='hip') needs contiguous bf16 GPU operands "
                "with N % 256 == 0, K % 256 == 0 and T % 64 == 0; got "
                f"gy {tuple(gy2.shape)} {gy2.dtype} x {tuple(x2.shape)} "
                f"{x2.dtype} contiguous={gy2.is_contiguous()},"
                f"{x2.is_contiguous()} device={gy2.device}")
        return _wgrad_hand_kernel(gy2, x2, req, True)
    if (impl == "auto" and _gpu(gy2, x2) and _wgrad_hip_eligible(gy2, x2)
            and _wgrad_auto_hip(gy2.shape[0], gy2.shape[1], x2.shape[1])):
        return _wgrad_hand_kernel(
            gy2, x2, req, _wgrad_bias_auto_fused(
                gy2.shape[0], gy2.shape[1], x2.shape[1]))
    return torch.matmul(gy2.t(), x2)


def linear_wgrad_bias(gy, x, impl=None):
    """Weight and bias gradient of y = x @ W^T + b in one call:
    (dW [N, K] = gy^T @ x, db [N] = sum over tokens of gy, in gy's dtype).

    dW is linear_wgrad(gy, x, impl), so the routing rules are its rules and
    live there.  Where that call runs the hand kernel it runs the bias
    variant (ops/hip/gemm_wgrad.hip: the column sums ride the MFMA fragments
    the GEMM already holds; dW comes out bit-identical) and db is a product
    of the same launch; where it runs the library, db = colsum(gy).
      impl "blas": torch.matmul + colsum.
      impl "hip":  the fused kernel, an error if the input is not eligible
                   (never a fallback).
      impl "auto": the fused kernel exactly where _wgrad_auto_hip admits the
                   shape (_wgrad_bias_auto_fused; HETU_AMD_WGRAD_BIAS=0
                   turns the fusion off), else linear_wgrad + colsum, which
                   is bit for bit what two separate ops compute.
    None takes HETU_AMD_WGRAD (default auto)."""
    global _wgrad_db_request
    req = _DbRequest()
    _wgrad_db_request = req
    try:
        dw = linear_wgrad(gy, x, impl)
    finally:
        _wgrad_db_request = None
    if req.db is not None:
        return dw, req.db
    return dw, colsum(gy.reshape(-1, gy.shape[-1])).to(gy.dtype)


_HETU_DGRAD = os.environ.get("HETU_AMD_DGRAD", "auto")  # auto|transposed|blas
_DGRAD_IMPLS = ("auto", "transposed", "blas")


def _dgrad_transposed_eligible(gy, w) -> bool:
    """What the transposed route takes: a contiguous 2-D bf16/fp16 weight
    on the GPU that holds gy, of gy's dtype (ops/hip/transpose.hip moves
    2-byte elements)."""
    return (gy.is_cuda and w.is_cuda and gy.device == w.device
            and w.dim() == 2 and w.is_contiguous() and gy.dim() >= 1
            and w.dtype in (torch.bfloat16, torch.float16)
            and gy.dtype == w.dtype and gy.shape[-1] == w.shape[0])


def _dgrad_auto_transposed(T: int, N: int, K: int) -> bool:
    """Shape classes where transpose + TN GEMM beat the library's NN GEMM
    with non-overlapping min-max ranges in scripts/bench_dgrad.py
    (profiles/r04_dgrad_layout.md, per-shape table).

    Measured: (N -> K) 12288->4096, 4096->4096, 16384->4096 and 4096->16384
    at T = 32768, 16384 and 8192 tokens, and the LM head 50304->4096 at
    T = 32768: all thirteen rows win, 1.08-1.16x, in three runs.  At
    T = 4096 the four layer shapes win by 2-9 % in two runs and 16384->4096
    overlaps in the third; at T = 2048 the transpose costs more than the
    faster GEMM form saves on all four.
    What the winning rows have in common is the rule: at least 8192 tokens
    and a weight of at least 4096 x 4096 whose sides are multiples of 8
    (the transpose kernel's 16-byte path).  Token counts between the
    measured ones, other weight sizes of that class, and the LM head below
    T = 32768 pass the rule without having been timed: that part is
    extrapolated.  T = 4096 is left on the library because its win did
    not repeat."""
    return (T >= 8192 and N >= 4096 and K >= 4096
            and N % 8 == 0 and K % 8 == 0)


def linear_dgrad(gy, w, impl=None):
    """Input gradient of y = x @ W^T: dx[..., K] = gy[..., N] @ w[N, K].

    impl: "blas" = torch.matmul(gy, w) (hipBLASLt NN form); "transposed" =
    copy w to Wt [K, N] with the HIP transpose kernel and run the forward's
    TN form F.linear(gy, Wt), an error if the input is not eligible (never
    a fallback); "auto" = the transposed route where it measured faster,
    else the library, and always the library on CPU.  None takes
    HETU_AMD_DGRAD (default auto).  The copy lives only inside the call:
    nothing is cached, so it can never be stale."""
    impl = _HETU_DGRAD if impl is None else impl
    if impl not in _DGRAD_IMPLS:
        raise ValueError(f"linear_dgrad: impl must be one of {_DGRAD_IMPLS}, "
                         f"got {impl!r}")
    if impl == "blas":
        return torch.matmul(gy, w)
    eligible = _dgrad_transposed_eligible(gy, w)
    if impl == "transposed" and not eligible:
        raise RuntimeError(
            "linear_dgrad(impl='transposed') needs a contiguous 2-D bf16 or "
            "fp16 GPU weight of gy's dtype and device; got "
            f"gy {tuple(gy.shape)} {gy.dtype} {gy.device} w {tuple(w.shape)} "
            f"{w.dtype} {w.device} contiguous={w.is_contiguous()}")
    if impl == "transposed" or (
            eligible and _dgrad_auto_transposed(
                gy.numel() // max(gy.shape[-1], 1), w.shape[0], w.shape[1])):
        gy2 = gy.reshape(-1, gy.shape[-1])
        dx = torch.nn.functional.linear(gy2, ext().transpose2d(w))
        return dx.reshape(*gy.shape[:-1], w.shape[1])
    return torch.matmul(gy, w)


def linear(x, w, bias=None, trans_w: bool = True):
    """x [..., K] @ (w [N, K] if trans_w else w [K, N]) + bias."""
    if _gpu(x) and _HETU_GEMM == "hip" and x.dtype == torch.bfloat16 \
            and trans_w:
        xs = x.reshape(-1, x.shape[-1]).contiguous()
        M, K = xs.shape
        N = w.shape[0]
        if M % 128 == 0 and N % 128 == 0 and K % 64 == 0:
            y = ext().gemm_bf16(xs, w.contiguous(), trans_w)
            if bias is not None:
                y = y + bias
            return y.reshape(*x.shape[:-1], N)
    if bias is not None and trans_w:
        # F.linear hits the hipBLASLt bias-epilogue path (one GEMM, no
        # separate broadcast-add kernel over the [M, N] output)
        return torch.nn.functional.linear(x, w.to(x.dtype),
                                          bias.to(x.dtype))
    wm = w.t() if trans_w else w
    if bias is not None:
        xs = x.reshape(-1, x.shape[-1])
        y = torch.addmm(bias.to(x.dtype), xs, wm.to(x.dtype))
        return y.reshape(*x.shape[:-1], wm.shape[-1])
    return torch.matmul(x, wm.to(x.dtype))


# ---------------------------------------------------------------------------
# Blockwise quantization (reference quantization.cu / Quantization.h;
# bitsandbytes-style fp4/nf4/int8 with per-block absmax)
# ---------------------------------------------------------------------------

_FP4_CODE = torch.tensor([
    0.0, 0.0052083333, 0.6666667, 1.0, 0.3333333, 0.5, 0.1666667, 0.25,
    -0.0, -0.0052083333, -0.6666667, -1.0, -0.3333333, -0.5,
    -0.1666667, -0.25])
_NF4_CODE = torch.tensor([
    -1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
    -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
    0.07958029955625534, 0.16093020141124725, 0.24611230194568634,
    0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
    0.7229568362236023, 1.0])


def quantize_blockwise(x: torch.Tensor, qtype: str = "nf4",
                       blocksize: int = 64):
    """returns (packed uint8, absmax fp32 [nblocks])."""
    if _use_hip("quant", x):
        return tuple(ext().quantize_blockwise(x.contiguous(), qtype,
                                              blocksize))
    flat = x.float().reshape(-1)
    n = flat.numel()
    nblk = (n + blocksize - 1) // blocksize
    pad = nblk * blocksize - n
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    blocks = flat.reshape(nblk, blocksize)
    absmax = blocks.abs().amax(-1)
    if qtype == "int8":
        inv = torch.where(absmax > 0, 127.0 / absmax,
                          torch.zeros_like(absmax))
        q = torch.round(blocks * inv.unsqueeze(-1)) + 128
        return q.reshape(-1)[:n].to(torch.uint8), absmax
    code = _NF4_CODE if qtype == "nf4" else _FP4_CODE
    inv = torch.where(absmax > 0, 1.0 / absmax, torch.zeros_like(absmax))
    norm = blocks * inv.unsqueeze(-1)
    idx = (norm.unsqueeze(-1) - code).abs().argmin(-1).to(torch.uint8)
    idx = idx.reshape(-1)[:n]
    hi, lo = idx[0::2], idx[1::2]
    return (hi << 4) | lo, absmax


def dequantize_blockwise(q: torch.Tensor, absmax: torch.Tensor,
                         qtype: str, blocksize: int, numel: int,
                         dtype=torch.float32) -> torch.Tensor:
    if _use_hip("quant", q):
        return ext().dequantize_blockwise(q, absmax, qtype, blocksize,
                                          numel, dtype)
    if qtype == "int8":
        s = absmax.repeat_interleave(blocksize)[:numel] / 127.0
        return ((q.float() - 128) * s).to(dtype)
    code = _NF4_CODE if qtype == "nf4" else _FP4_CODE
    hi, lo = (q >> 4).long(), (q & 15).long()
    vals = torch.stack([code[hi], code[lo]], -1).reshape(-1)[:numel]
    s = absmax.repeat_interleave(blocksize)[:numel]
    return (vals * s).to(dtype)


def matmul_4bit(x: torch.Tensor, qweight: torch.Tensor,
                absmax: torch.Tensor, qtype: str, blocksize: int,
                shape) -> torch.Tensor:
    """y = x @ dequant(W)^T (reference matmul4bit: dequant then GEMM —
    weight stays 4-bit in HBM, dequant streams through once)."""
    w = dequantize_blockwise(qweight, absmax, qtype, blocksize,
                             shape[0] * shape[1], x.dtype).reshape(shape)
    return x @ w.t()


def fused_qkv_attention_fwd(qkv, n_head: int, n_kv_head: int, head_dim: int,
                            cos=None, sin=None, causal: bool = True,
                            scale: Optional[float] = None):
    """Fused attention over the qkv GEMM output [B, S, (H+2Hkv)*D]:
    in-place RoPE on the q|k sections (optional), then flash attention
    reading q/k/v as strided views — zero slice/transpose copies.
    Mutates qkv (rotation is linear, so backward never needs the
    pre-rotation values).  Returns (o [B,S,H*D], lse [B,H,S])."""
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if _use_hip("qkvfa", qkv):
        e = ext()
        if cos is not None:
            e.rope_qk_inplace(qkv, cos.contiguous(), sin.contiguous(),
                              n_head + n_kv_head, head_dim, 1)
        o, lse = e.flash_attn_fwd_qkv(qkv, n_head, n_kv_head, head_dim,
                                      causal, scale)
        return o, lse
    # CPU reference: same math with views
    B, S, _ = qkv.shape
    H, Hkv, D = n_head, n_kv_head, head_dim
    qkv4 = qkv.view(B, S, H + 2 * Hkv, D)
    if cos is not None:
        qkv4[:, :, :H + Hkv] = _rope_ref(qkv4[:, :, :H + Hkv], cos, sin,
                                         False).to(qkv.dtype)
    q = qkv4[:, :, :H].permute(0, 2, 1, 3)
    k = qkv4[:, :, H:H + Hkv].permute(0, 2, 1, 3)
    v = qkv4[:, :, H + Hkv:].permute(0, 2, 1, 3)
    o, lse = _attn_ref_fwd(q, k, v, causal, scale)
    return o.permute(0, 2, 1, 3).reshape(B, S, H * D).contiguous(), lse


def fused_qkv_attention_bwd(dout, qkv, out, lse, n_head: int,
                            n_kv_head: int, head_dim: int, cos=None,
                            sin=None, causal: bool = True,
                            scale: Optional[float] = None):
    """Backward of fused_qkv_attention: returns dqkv [B,S,(H+2Hkv)*D]
    (RoPE backward applied in place on the dq|dk sections)."""
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if _use_hip("qkvfa", qkv):
        e = ext()
        dqkv = e.flash_attn_bwd_qkv(dout.contiguous(), qkv,
                                    out.contiguous(), lse.contiguous(),
                                    n_head, n_kv_head, head_dim, causal,
                                    scale)
        if cos is not None:
            e.rope_qk_inplace(dqkv, cos.contiguous(), sin.contiguous(),
                              n_head + n_kv_head, head_dim, -1)
        return dqkv
    B, S, _ = qkv.shape
    H, Hkv, D = n_head, n_kv_head, head_dim
    qkv4 = qkv.view(B, S, H + 2 * Hkv, D)   # already rotated
    q = qkv4[:, :, :H].permute(0, 2, 1, 3)
    k = qkv4[:, :, H:H + Hkv].permute(0, 2, 1, 3)
    v = qkv4[:, :, H + Hkv:].permute(0, 2, 1, 3)
    do4 = dout.view(B, S, H, D).permute(0, 2, 1, 3)
    o4 = out.view(B, S, H, D).permute(0, 2, 1, 3)
    dq, dk, dv = _attn_ref_bwd(do4, q, k, v, o4, lse, causal, scale)
    dqkv = torch.cat([dq, dk, dv], dim=1).permute(0, 2, 1, 3) \
        .reshape(B, S, (H + 2 * Hkv) * D).contiguous()
    if cos is not None:
        d4 = dqkv.view(B, S, H + 2 * Hkv, D)
        d4[:, :, :H + Hkv] = _rope_ref(d4[:, :, :H + Hkv], cos, sin,
                                       True).to(dqkv.dtype)
    return dqkv


def varlen_attention_fwd(q, k, v, cu_seqlens, causal: bool = True,
                         scale: Optional[float] = None,
                         max_seqlen: Optional[int] = None):
    """Packed-varlen attention (reference ParallelAttention.cc packed
    path / FlashAttention.cu mha_varlen_fwd): q/k/v [T, H, D] with
    cu_seqlens [n+1] delimiting the packed sequences; each segment attends
    only within itself.  On GPU (D=128, no GQA mismatch constraint): ONE
    kernel launch with device-side cu offsets — no host loop, no
    `.tolist()` sync; blocks beyond a segment's tiles exit early.
    max_seqlen (optional) only shrinks the launch grid: None sizes it by
    T; a value must be >= the longest segment — a too-small value
    SILENTLY drops the rows past it (they are never computed).
    Returns (out [T, H, D], lse [H, T])."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    T, H, D = q.shape
    if _use_hip("varlen", q) and D == 128:
        cu32 = cu_seqlens.to(device=q.device, dtype=torch.int32)
        o, lse = ext().flash_attn_varlen_fwd(
            q.contiguous(), k.contiguous(), v.contiguous(), cu32,
            T if max_seqlen is None else int(max_seqlen), causal, scale)
        return o, lse
    out = torch.empty_like(q)
    lse = torch.empty(H, T, dtype=torch.float32, device=q.device)
    cu = cu_seqlens.tolist()
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        qs = q[s0:s1].permute(1, 0, 2).unsqueeze(0)
        ks = k[s0:s1].permute(1, 0, 2).unsqueeze(0)
        vs = v[s0:s1].permute(1, 0, 2).unsqueeze(0)
        o, l = flash_attn_fwd(qs.contiguous(), ks.contiguous(),
                              vs.contiguous(), causal, scale)
        out[s0:s1] = o[0].permute(1, 0, 2)
        lse[:, s0:s1] = l[0]
    return out, lse


def varlen_attention_bwd(dout, q, k, v, out, lse, cu_seqlens,
                         causal: bool = True,
                         scale: Optional[float] = None,
                         max_seqlen: Optional[int] = None):
    """Backward of varlen_attention_fwd -> (dq, dk, dv), packed like
    q/k/v.  On GPU (D=128): three launches (delta, dq, dkv) over all
    segments with device-side cu offsets — no host sync, so a packed
    step can be hipGraph-captured.  Rows that belong to no segment
    (t >= cu[-1]) come back ZERO on every path.  max_seqlen: see
    varlen_attention_fwd (too small silently drops rows)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    T, H, D = q.shape
    if _use_hip("varlen", q) and D == 128:
        cu32 = cu_seqlens.to(device=q.device, dtype=torch.int32)
        dq, dk, dv = ext().flash_attn_varlen_bwd(
            dout.contiguous(), q.contiguous(), k.contiguous(),
            v.contiguous(), out.contiguous(), lse.contiguous(), cu32,
            T if max_seqlen is None else int(max_seqlen), causal, scale)
        return dq, dk, dv
    # CPU / other-D / HETU_AMD_TORCH_FALLBACK=varlen: per-segment loop
    dq = torch.zeros_like(q)
    dk = torch.zeros_like(k)
    dv = torch.zeros_like(v)
    cu = cu_seqlens.tolist()
    for s0, s1 in zip(cu[:-1], cu[1:]):
        if s1 <= s0:
            continue
        args = [t[s0:s1].permute(1, 0, 2).unsqueeze(0).contiguous()
                for t in (dout, q, k, v, out)]
        ls = lse[:, s0:s1].unsqueeze(0).contiguous()
        dqs, dks, dvs = flash_attn_bwd(args[0], args[1], args[2], args[3],
                                       args[4], ls, causal, scale)
        dq[s0:s1] = dqs[0].permute(1, 0, 2)
        dk[s0:s1] = dks[0].permute(1, 0, 2)
        dv[s0:s1] = dvs[0].permute(1, 0, 2)
    return dq, dk, dv


# ---------------------------------------------------------------------------
# hipBLASLt epilogue-fused MLP pieces (ltgemm.cpp): gelu folded into the
# fc GEMM (GELU_AUX_BIAS) and dgelu+bias-grad into the backward GEMM
# (DGELU_BGRAD).  CPU path = the exact reference composition.
# ---------------------------------------------------------------------------

# per-direction capability: this hipBLASLt build (gfx950) has DGELU_BGRAD
# solutions but NO GELU_AUX_BIAS solutions, so the forward composes while
# the backward still fuses dgelu + bias-grad into the dgrad GEMM
_LT_FWD = [None]
_LT_BWD = [None]


def linear_gelu_aux(x2d, w, b):
    """returns (gelu(x@w^T+b), pre-gelu aux)."""
    if _use_hip("ltgemm", x2d) and _LT_FWD[0] is not False:
        try:
            out = tuple(ext().lt_linear_gelu_aux(x2d.contiguous(),
                                                 w.contiguous(),
                                                 b.contiguous()))
            _LT_FWD[0] = True
            return out
        except RuntimeError as e:
            if "no algo" not in str(e):
                raise
            # no GELU_AUX solutions: compose (bias still fused via
            # F.linear; gelu = hand HIP kernel; aux = pre-gelu kept)
            _LT_FWD[0] = False
            print("[hetu_amd] hipBLASLt GELU_AUX epilogue unavailable, "
                  "composing the MLP forward")
    h = torch.nn.functional.linear(x2d, w.to(x2d.dtype), b.to(x2d.dtype))
    return gelu_fwd(h), h


def dgelu_bgrad(dy2d, w, aux):
    """returns (dgelu(dy@w, aux), colsum(dgelu(...)))."""
    if _use_hip("ltgemm", dy2d) and _LT_BWD[0] is not False:
        try:
            out = tuple(ext().lt_dgelu_bgrad(dy2d.contiguous(),
                                             w.contiguous(),
                                             aux.contiguous()))
            _LT_BWD[0] = True
            return out
        except RuntimeError as e:
            if "no algo" not in str(e):
                raise
            _LT_BWD[0] = False
            print("[hetu_amd] hipBLASLt DGELU_BGRAD epilogue unavailable, "
                  "composing the MLP backward")
    da = linear_dgrad(dy2d, w.to(dy2d.dtype))
    dh = gelu_bwd(da, aux)
    return dh, colsum(dh).to(dh.dtype)


# ---------------------------------------------------------------------------
# MoE routing / layout (moe.hip; reference TopKIdx.cu, LayoutTransform.cu,
# ReverseLayoutTransform).  N tokens, E experts, C slots per expert, K
# choices per token:
#   pos     [E, C] int64   token index held by each slot, -1 if empty
#   slot_of [N, K] int64   flat slot e*C + q of choice k, -1 if dropped
#   wk      [N, K] fp32    gate weight of choice k, 0 if dropped
# Routing policy: rounds k = 0..K-1 in order; within a round tokens queue at
# their expert in increasing token index, behind the slots earlier rounds
# filled; a choice is kept iff its queue position is < C.  The HIP top-k
# breaks ties towards the lower expert index (torch.topk leaves tie order
# unspecified).  The torch branches are the composition the graph ops used
# before the kernels existed; they serve CPU, HETU_AMD_TORCH_FALLBACK=moe
# and K / E beyond the kernel limits.
# ---------------------------------------------------------------------------

MOE_MAX_K = 8
MOE_MAX_E = 2048


def _moe_hip(K: int, E: int, *ts) -> bool:
    return (_use_hip("moe", *ts) and 1 <= K <= MOE_MAX_K and K <= E
            and E <= MOE_MAX_E)


def _moe_route_torch(probs: torch.Tensor, E: int, C: int, K: int):
    """Greedy capacity routing.  Returns pos [E, C] int64 (-1 pad),
    combine scatter info: slot_of [N, K] int64 (flat index into E*C, -1 if
    dropped), topk idx [N, K], weights [N, K].

    Fully static shapes: no nonzero/boolean-mask gathers, so the routing
    is hipGraph-capturable and never syncs the host (dropped tokens
    scatter into a sacrificial slot E*C instead)."""
    N = probs.shape[0]
    dev = probs.device
    w, idx = probs.topk(K, dim=-1)                      # [N, K]
    # pos with one extra dummy slot at index E*C for dropped tokens
    pos_fl = torch.full((E * C + 1,), -1, dtype=torch.int64, device=dev)
    slot_of = torch.full((N, K), -1, dtype=torch.int64, device=dev)
    toks = torch.arange(N, dtype=torch.int64, device=dev)
    base = torch.zeros(E, dtype=torch.int64, device=dev)
    for k in range(K):
        e = idx[:, k]                                   # [N]
        onehot = torch.nn.functional.one_hot(e, E)      # [N, E]
        order = onehot.cumsum(0) * onehot               # 1-based rank
        q = (order.gather(1, e.unsqueeze(1)).squeeze(1) - 1) + base[e]
        keep = q < C
        flat = torch.where(keep, e * C + q,
                           torch.full_like(q, E * C))  # dummy if dropped
        pos_fl.scatter_(0, flat, toks)
        slot_of[:, k] = torch.where(keep, flat,
                                    torch.full_like(flat, -1))
        # recount filled slots per expert (robust to same-slot rewrites)
        base = (pos_fl[:E * C].reshape(E, C) >= 0).sum(-1)
    pos = pos_fl[:E * C].reshape(E, C)
    wk = torch.where(slot_of >= 0, w, torch.zeros_like(w))
    return pos, slot_of, idx, wk


def moe_route(probs: torch.Tensor, C: int, K: int):
    """probs [N, E] -> (pos [E, C], slot_of [N, K], idx [N, K] int64,
    wk [N, K] fp32).  Values compare in fp32."""
    E = probs.shape[1]
    if _moe_hip(K, E, probs):
        idx, w = ext().moe_topk(probs.contiguous(), K)
        pos, slot_of, wk = ext().moe_assign_slots(idx, w, E, C)
        return pos, slot_of, idx, wk
    return _moe_route_torch(probs.float(), E, C, K)


def moe_dispatch_rows(x: torch.Tensor, pos: torch.Tensor, out=None):
    """x [N, h], pos [E, C] -> send [E*C, h]: row s is x[pos[s]], zeros
    for an empty slot.  `out` (HIP path only) receives the rows."""
    if _use_hip("moe", x):
        return ext().moe_dispatch_rows(x.contiguous(), pos.contiguous(), out)
    # static-shape gather: dropped slots read token 0 and are masked
    pf = pos.view(-1)
    send = x[pf.clamp(min=0)] * (pf >= 0).unsqueeze(-1).to(x.dtype)
    if out is not None:
        out.copy_(send)
        return out
    return send


def moe_dispatch_rows_bwd(gsend: torch.Tensor, pos: torch.Tensor,
                          slot_of: torch.Tensor):
    """gsend [E*C, h] -> dx [N, h]: dx[t] = sum of the gsend rows of t's
    kept slots (fp32 accumulation, one rounding on the HIP path)."""
    N, K = slot_of.shape
    if _use_hip("moe", gsend) and 1 <= K <= MOE_MAX_K:
        return ext().moe_dispatch_rows_bwd(gsend.contiguous(),
                                           slot_of.contiguous())
    dx = gsend.new_zeros(N, gsend.shape[-1])
    pf = pos.view(-1)
    dx.index_add_(0, pf.clamp(min=0),
                  (gsend * (pf >= 0).unsqueeze(-1)).to(dx.dtype))
    return dx


def moe_gate_bwd(g_w: torch.Tensor, slot_of: torch.Tensor,
                 probs: torch.Tensor, C: int):
    """g_w [N, K] -> dprobs [N, E] (dtype of probs): g_w lands on the
    expert of every kept choice, zero elsewhere."""
    K = slot_of.shape[1]
    if _moe_hip(K, probs.shape[1], probs):
        return ext().moe_gate_bwd(g_w.float().contiguous(),
                                  slot_of.contiguous(), probs, C)
    # dprobs: combine_w = probs.gather(topk) masked -> scatter g_w
    dprobs = torch.zeros_like(probs)
    wmask = (slot_of >= 0).to(probs.dtype)
    # idx recomputed from probs (same topk order)
    _, idx = probs.float().topk(K, dim=-1)
    dprobs.scatter_(1, idx, (g_w.to(probs.dtype) * wmask))
    return dprobs


def moe_combine_rows(recv: torch.Tensor, wk: torch.Tensor,
                     slot_of: torch.Tensor):
    """recv [E*C, h] -> y [N, h]: y[t] = sum_k wk[t,k] * recv[slot_of[t,k]]
    over kept k."""
    N, K = slot_of.shape
    if _use_hip("moe", recv) and 1 <= K <= MOE_MAX_K:
        return ext().moe_combine_rows(recv.contiguous(),
                                      wk.float().contiguous(),
                                      slot_of.contiguous())
    y = recv.new_zeros(N, recv.shape[-1])
    for k in range(K):
        sl = slot_of[:, k]
        rows = recv[sl.clamp(min=0)]
        # wk is already 0 for dropped slots (masked at routing)
        y += rows * wk[:, k].unsqueeze(-1).to(rows.dtype)
    return y


def moe_combine_rows_bwd(gy: torch.Tensor, recv: torch.Tensor,
                         wk: torch.Tensor, pos: torch.Tensor,
                         slot_of: torch.Tensor, out=None):
    """-> (d_recv [E*C, h], dwk [N, K] fp32): d_recv[s] = gy[t] * wk[t,k]
    for the (t, k) holding slot s, zeros for an empty slot;
    dwk[t,k] = <gy[t], recv[slot_of[t,k]]> in fp32, 0 if dropped.  `out`
    (HIP path only) receives d_recv."""
    N, K = slot_of.shape
    if _use_hip("moe", gy) and 1 <= K <= MOE_MAX_K:
        return tuple(ext().moe_combine_rows_bwd(
            gy.contiguous(), recv.contiguous(), wk.float().contiguous(),
            pos.contiguous(), slot_of.contiguous(), out))
    # d_recv [E*C, h]: rows scattered from gy * w (slot E*C is the
    # sacrificial target for dropped entries — static shapes)
    h = gy.shape[-1]
    EC = pos.numel()
    d_fl = gy.new_zeros(EC + 1, h)
    for k in range(K):
        sl = slot_of[:, k]
        tgt = torch.where(sl >= 0, sl, torch.full_like(sl, EC))
        d_fl.scatter_(0, tgt.unsqueeze(-1).expand(-1, h),
                      gy * wk[:, k].unsqueeze(-1).to(gy.dtype))
    d_recv = d_fl[:EC]
    # d_combine_w: dot(gy[token], recv[slot]); 0 where dropped
    dwk = torch.zeros_like(wk)
    for k in range(K):
        sl = slot_of[:, k]
        dot = (gy.float() * recv[sl.clamp(min=0)].float()).sum(-1)
        dwk[:, k] = dot * (sl >= 0).to(dot.dtype)
    if out is not None:
        out.copy_(d_recv)
        d_recv = out
    return d_recv, dwk


# ---------------------------------------------------------------------------
# Fused MoE gate (moe.hip (h)): softmax + top-k + the load-balance and router
# z-loss statistics in one pass.  For logits [N, E] and K choices:
#   lse[t]  = logsumexp_e float(logits[t, e])       p32 = exp(logits - lse)
#   probs   = p32 rounded once to the logits' dtype
#   idx, w  = top-K of the stored probs row (value desc, expert index asc,
#             compared as fp32) -- what moe_route(probs, C, K) selects
#   cnt[e]  = #{(t, k): idx[t, k] == e}, before capacity dropping
#   psum[e] = sum_t p32[t, e]
#   aux     = E / N^2 * sum_e psum[e] * cnt[e]      (value K when uniform)
#   z       = 1 / N * sum_t lse[t]^2
# Backward, cnt held constant:
#   dp      = g_probs + g_aux * E / N^2 * cnt
#   dlogits = p32 * (dp - <p32, dp>) + g_z * 2 / N * lse * p32
# The extension entry points are moe_gate_fwd / moe_gate_grad
# (moe_gate_bwd is the dispatch gate scatter above).
# ---------------------------------------------------------------------------

MOE_GATE_MAX_BLOCKS = 1024     # grid cap of the fused gate's forward kernel


def moe_gate(logits: torch.Tensor, K: int):
    """logits [N, E] -> (probs [N, E], idx [N, K] int64, w [N, K] fp32,
    lse [N] fp32, psum [E] fp32, cnt [E] int32, aux [] fp32, z [] fp32)."""
    N, E = logits.shape
    if not 1 <= K <= E:
        raise ValueError(f"moe_gate: need 1 <= K <= E, got K={K}, E={E}")
    if N >= 1 and _moe_hip(K, E, logits):
        return tuple(ext().moe_gate_fwd(logits.contiguous(), K))
    xf = logits.float()
    lse = torch.logsumexp(xf, dim=-1)
    p32 = torch.softmax(xf, dim=-1)
    probs = p32.to(logits.dtype)
    # stable descending sort == (value desc, index asc); topk leaves the
    # tie order unspecified
    w, idx = torch.sort(probs.float(), dim=-1, descending=True, stable=True)
    w, idx = w[:, :K].contiguous(), idx[:, :K].contiguous()
    cnt = torch.zeros(E, dtype=torch.int32, device=logits.device)
    cnt.scatter_add_(0, idx.reshape(-1),
                     torch.ones(N * K, dtype=torch.int32,
                                device=logits.device))
    psum = colsum(p32)        # no at::native column reduce on a GPU
    # the two scalars are formed in fp64 and rounded once, as in the kernel
    aux = ((psum.double() * cnt.double()).sum() * (E / float(N * N))).float()
    z = ((lse.double() ** 2).sum() / N).float()
    return probs, idx, w, lse, psum, cnt, aux, z


def moe_gate_grad(g_probs: Optional[torch.Tensor],
                  g_aux: Optional[torch.Tensor],
                  g_z: Optional[torch.Tensor], logits: torch.Tensor,
                  lse: torch.Tensor, cnt: torch.Tensor) -> torch.Tensor:
    """Backward of moe_gate -> dlogits [N, E].  g_probs [N, E], g_aux and
    g_z (one-element tensors, read on the device) may each be None (zero)."""
    N, E = logits.shape
    if N >= 1 and _moe_hip(1, E, logits):
        def scalar(t):
            return None if t is None else \
                t.to(device=logits.device, dtype=torch.float32).reshape(())
        gp = None if g_probs is None else \
            g_probs.to(logits.dtype).contiguous()
        return ext().moe_gate_grad(gp, scalar(g_aux), scalar(g_z),
                                   logits.contiguous(),
                                   lse.float().contiguous(),
                                   cnt.to(torch.int32).contiguous())
    xf = logits.float()
    l = lse.float().unsqueeze(-1)
    p = torch.exp(xf - l)
    dp = torch.zeros_like(xf) if g_probs is None else g_probs.float()
    if g_aux is not None:
        dp = dp + (g_aux.float().reshape(()) * (E / float(N * N))) \
            * cnt.float()
    dl = p * (dp - (p * dp).sum(-1, keepdim=True))
    if g_z is not None:
        dl = dl + (g_z.float().reshape(()) * (2.0 / N)) * l * p
    return dl.to(logits.dtype)
