"""Brute-force fp64 oracle of the fused MoE gate (ops.functional.moe_gate).

Definitions, for logits [N, E] as stored and K choices per token:
  lse[t]  = logsumexp_e logits[t, e]
  p[t, e] = exp(logits[t, e] - lse[t])
  psum[e] = sum_t p[t, e]
  idx, w  = top-K of a given probs row: value descending, expert index
            ascending, values compared as fp32
  cnt[e]  = #{(t, k): idx[t, k] == e}
  aux     = E / N^2 * sum_e psum[e] * cnt[e]
  z       = 1 / N * sum_t lse[t]^2
  dp      = g_probs + g_aux * E / N^2 * cnt
  dlogits = p * (dp - sum_e p * dp) + g_z * 2 / N * lse * p
Everything is computed in float64 on the CPU from the stored values.
"""
import numpy as np
import torch


def gate_inputs(N, E, dtype, seed, step=0.25):
    """Tie-free logits: each row a random permutation of {step * j : j < E}
    (exact in bf16 / fp16 / fp32 for step 0.25 and E <= 256, and in fp32
    for step 1/32 and E <= 2048).  Neighbouring probabilities differ by a
    factor e^step, far above any rounding for step = 0.25."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randperm(E, generator=g).double() * step for _ in range(N)]
    return torch.stack(rows).to(dtype)


def topk_rule(probs, K):
    """Tie-rule top-K of stored probs -> (idx [N, K] int64, w [N, K] fp32,
    cnt [E] int64).  A stable ascending sort of the negated fp32 values is
    the order (value descending, expert index ascending)."""
    pf = probs.detach().cpu().float()
    E = pf.shape[1]
    order = np.argsort(-pf.numpy(), axis=1, kind="stable")[:, :K]
    idx = torch.from_numpy(np.ascontiguousarray(order)).long()
    w = pf.gather(1, idx)
    cnt = torch.bincount(idx.reshape(-1), minlength=E)
    return idx, w, cnt


def gate_forward(logits, K, probs=None):
    """fp64 reference.  Routing (idx, w, cnt) is taken from `probs` when
    given (the stored probs of the code under test), else from the oracle's
    own probabilities rounded to the logits' dtype."""
    x = logits.detach().cpu().double()
    N, E = x.shape
    lse = torch.logsumexp(x, dim=-1)
    p = torch.exp(x - lse[:, None])
    if probs is None:
        probs = p.to(logits.dtype)
    idx, w, cnt = topk_rule(probs, K)
    psum = p.sum(0)
    aux = (psum * cnt.double()).sum() * E / (N * N)
    z = (lse * lse).sum() / N
    return {"probs": p, "lse": lse, "psum": psum, "idx": idx, "w": w,
            "cnt": cnt, "aux": aux, "z": z}


def gate_backward(logits, cnt, g_probs=None, g_aux=None, g_z=None):
    """fp64 dlogits for upstream g_probs [N, E], scalars g_aux, g_z (None =
    zero); also returns max |dp| for the tolerance."""
    x = logits.detach().cpu().double()
    N, E = x.shape
    lse = torch.logsumexp(x, dim=-1, keepdim=True)
    p = torch.exp(x - lse)
    dp = torch.zeros_like(x) if g_probs is None \
        else g_probs.detach().cpu().double()
    if g_aux is not None:
        dp = dp + float(g_aux) * E / (N * N) * cnt.cpu().double()
    dl = p * (dp - (p * dp).sum(-1, keepdim=True))
    if g_z is not None:
        dl = dl + float(g_z) * 2.0 / N * lse * p
    return dl, float(dp.abs().max())


# relative rounding of one store in each dtype (the issue's figures)
RTOL = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11,
        torch.float32: 1e-5}
# absolute floor where a stored value underflows its format: fp32 arithmetic
# may flush results below the smallest fp32 normal (2^-126) to zero, which
# also bounds what bf16 (same exponent range) can lose; fp16 goes subnormal
# below 2^-14 and then rounds to a multiple of 2^-24 (half a step: 2^-25)
ATOL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25,
        torch.float32: 2.0 ** -126}


def check_forward(out, ref, logits, K, exact_routing=True):
    """Assert one forward result (the 8-tuple of F.moe_gate) against the
    oracle `ref` with the derived bounds; returns nothing."""
    probs, idx, w, lse, psum, cnt, aux, z = [t.detach().cpu() for t in out]
    N, E = logits.shape
    dt = logits.dtype
    assert probs.dtype == dt and idx.dtype == torch.int64
    assert w.dtype == lse.dtype == psum.dtype == torch.float32
    assert aux.dtype == z.dtype == torch.float32
    assert aux.ndim == 0 and z.ndim == 0
    # routing is exact: the tie rule applied to the STORED probs
    ridx, rw, rcnt = topk_rule(probs, K)
    assert torch.equal(idx, ridx)
    assert torch.equal(w, rw)
    assert torch.equal(cnt.long(), rcnt)
    if exact_routing:
        assert torch.equal(idx, ref["idx"])
        assert torch.equal(cnt.long(), ref["cnt"])
    # probs: one rounding of an fp32 value good to a few ulp
    err = (probs.double() - ref["probs"]).abs()
    bound = RTOL[dt] * ref["probs"] + ATOL[dt]
    assert bool((err <= bound).all()), float((err - bound).max())
    # lse
    err = (lse.double() - ref["lse"]).abs()
    bound = 1e-6 * ref["lse"].abs() + E * 2.0 ** -24
    assert bool((err <= bound).all()), float((err - bound).max())
    # psum: fp32 summation of N terms in [0, 1]
    ptol = (N + 8) * 2.0 ** -24
    err = (psum.double() - ref["psum"]).abs()
    assert bool((err <= ptol * ref["psum"] + 1e-37).all()), float(err.max())
    # aux: the psum bounds weighted by cnt
    c = rcnt.double()
    ref_aux = (ref["psum"] * c).sum() * E / (N * N)
    tol = ptol * float(ref_aux)
    assert abs(float(aux) - float(ref_aux)) <= tol, (float(aux),
                                                     float(ref_aux), tol)
    assert abs(float(z) - float(ref["z"])) <= 1e-5 * float(ref["z"]) + 1e-30


def check_backward(dl, ref_dl, max_dp, dtype, E):
    """dlogits: one rounding of an fp32 expression with an E-term dot (plus
    the format's underflow floor: an fp16 gradient below 2^-14 is stored
    to the nearest multiple of 2^-24)."""
    dl = dl.detach().cpu()
    assert dl.dtype == dtype
    err = (dl.double() - ref_dl).abs()
    bound = RTOL[dtype] * ref_dl.abs() + E * 2.0 ** -23 * max_dp \
        + ATOL[dtype]
    assert bool((err <= bound).all()), float((err - bound).max())
