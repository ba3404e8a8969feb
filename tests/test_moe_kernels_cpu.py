"""MoE routing / layout entry points (hetu_amd.ops.functional.moe_*), CPU
branches, against the brute-force oracle in moe_oracle.py; and the MoEMLP
graph against the op-level torch composition it ran before the entry
points existed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moe_oracle as O  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

# (N, E, K, C, skew, empty_expert)
ROUTE_CASES = [
    (1, 2, 1, 1, 0.0, None),
    (63, 8, 2, 63, 0.0, None),        # C >= N: nothing dropped
    (65, 8, 2, 5, 0.7, 3),            # drops, an empty expert
    (257, 8, 4, 40, 0.7, None),
    (64, 96, 4, 1, 0.0, None),        # C = 1
]


@pytest.mark.parametrize("N,E,K,C,skew,empty", ROUTE_CASES)
def test_route_cpu_matches_oracle(N, E, K, C, skew, empty):
    probs = O.make_probs(N, E, seed=N * 131 + E, skew=skew,
                         empty_expert=empty)
    pos, slot_of, idx, wk = F.moe_route(probs, C, K)
    rpos, rslot, ridx, rwk = O.route(probs, C, K)
    assert torch.equal(idx, ridx)
    assert torch.equal(pos, rpos)
    assert torch.equal(slot_of, rslot)
    assert torch.equal(wk, rwk)
    assert wk.dtype == torch.float32 and pos.dtype == torch.int64
    if skew:
        assert (rslot < 0).any()
    if empty is not None:
        assert (rpos[empty] < 0).all()


def test_route_bf16_probs_compare_in_fp32():
    probs = O.make_probs(40, 8, seed=5).to(torch.bfloat16)
    got = F.moe_route(probs, 6, 2)
    ref = O.route(probs, 6, 2)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("h", [8, 33])
@pytest.mark.parametrize("K", [1, 2])
def test_rows_cpu_match_oracle(h, K):
    N, E, C = 50, 4, 9
    probs = O.make_probs(N, E, seed=h + K, skew=0.7, empty_expert=2)
    pos, slot_of, idx, wk = O.route(probs, C, K)
    assert (slot_of < 0).any() and (pos[2] < 0).all()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, h, generator=g)
    rows = torch.randn(E * C, h, generator=g)
    gy = torch.randn(N, h, generator=g)
    g_w = torch.randn(N, K, generator=g)
    mx = float(max(x.abs().max(), rows.abs().max(), gy.abs().max()))
    tol = dict(rtol=1e-5, atol=1e-6 * K * mx)

    send = F.moe_dispatch_rows(x, pos)
    assert torch.equal(send.double(), O.dispatch_rows(x, pos))
    dx = F.moe_dispatch_rows_bwd(rows, pos, slot_of)
    assert torch.allclose(dx.double(), O.dispatch_rows_bwd(rows, slot_of),
                          **tol)
    dprobs = F.moe_gate_bwd(g_w, slot_of, probs, C)
    assert dprobs.dtype == probs.dtype
    assert torch.equal(dprobs.double(), O.gate_bwd(g_w, slot_of, E, C))
    y = F.moe_combine_rows(rows, wk, slot_of)
    assert torch.allclose(y.double(), O.combine_rows(rows, wk, slot_of),
                          **tol)
    d_recv, dwk = F.moe_combine_rows_bwd(gy, rows, wk, pos, slot_of)
    r_drecv, r_dwk = O.combine_rows_bwd(gy, rows, wk, pos, slot_of)
    assert torch.allclose(d_recv.double(), r_drecv, **tol)
    assert dwk.dtype == torch.float32
    assert torch.allclose(dwk.double(), r_dwk, rtol=1e-4,
                          atol=h * mx * mx * 2.0 ** -23)
    # fully dropped tokens and empty slots are exact zeros
    dead = (slot_of < 0).all(-1)
    assert dead.any()
    assert (y[dead] == 0).all() and (dx[dead] == 0).all()
    assert (send[pos.view(-1) < 0] == 0).all()
    assert (d_recv[pos.view(-1) < 0] == 0).all()


# ---------------------------------------------------------------------------
# The four graph ops' single-rank compute as it stood before the functional
# entry points (torch composition inside the ops), kept here as the recorded
# behaviour the MoEMLP graph must reproduce bit for bit on CPU.
# ---------------------------------------------------------------------------

def _old_route(probs, E, C, K):
    N = probs.shape[0]
    dev = probs.device
    w, idx = probs.topk(K, dim=-1)
    pos_fl = torch.full((E * C + 1,), -1, dtype=torch.int64, device=dev)
    slot_of = torch.full((N, K), -1, dtype=torch.int64, device=dev)
    toks = torch.arange(N, dtype=torch.int64, device=dev)
    base = torch.zeros(E, dtype=torch.int64, device=dev)
    for k in range(K):
        e = idx[:, k]
        onehot = torch.nn.functional.one_hot(e, E)
        order = onehot.cumsum(0) * onehot
        q = (order.gather(1, e.unsqueeze(1)).squeeze(1) - 1) + base[e]
        keep = q < C
        flat = torch.where(keep, e * C + q, torch.full_like(q, E * C))
        pos_fl.scatter_(0, flat, toks)
        slot_of[:, k] = torch.where(keep, flat, torch.full_like(flat, -1))
        base = (pos_fl[:E * C].reshape(E, C) >= 0).sum(-1)
    pos = pos_fl[:E * C].reshape(E, C)
    wk = torch.where(slot_of >= 0, w, torch.zeros_like(w))
    return pos, slot_of, idx, wk


def _old_dispatch(self, op, inputs, ctx):
    x, probs = inputs
    a = op.attrs
    E, C, K = a["experts"], a["capacity"], a["k"]
    pos, slot_of, idx, wk = _old_route(probs.float(), E, C, K)
    pf = pos.view(-1)
    send = x[pf.clamp(min=0)] * (pf >= 0).unsqueeze(-1).to(x.dtype)
    return [send.reshape(E, C, -1), wk, pos, slot_of]


def _old_dispatch_grad(self, op, inputs, ctx):
    g_exp, g_w, pos, slot_of, x, probs = inputs
    a = op.attrs
    E, C, K = a["experts"], a["capacity"], a["k"]
    gsend = g_exp.reshape(E * C, -1)
    dx = torch.zeros_like(x)
    pf = pos.view(-1)
    dx.index_add_(0, pf.clamp(min=0),
                  (gsend * (pf >= 0).unsqueeze(-1)).to(x.dtype))
    dprobs = torch.zeros_like(probs)
    if g_w is not None:
        wmask = (slot_of >= 0).to(probs.dtype)
        _, idx = probs.float().topk(K, dim=-1)
        dprobs.scatter_(1, idx, (g_w.to(probs.dtype) * wmask))
    return [dx, dprobs]


def _old_combine(self, op, inputs, ctx):
    eo, wk, pos, slot_of = inputs
    a = op.attrs
    E, C, K = a["experts"], a["capacity"], a["k"]
    recv = eo.reshape(E * C, -1)
    y = eo.new_zeros(wk.shape[0], eo.shape[-1])
    for k in range(K):
        sl = slot_of[:, k]
        rows = recv[sl.clamp(min=0)]
        y += rows * wk[:, k].unsqueeze(-1).to(rows.dtype)
    return [y]


def _old_combine_grad(self, op, inputs, ctx):
    gy, eo, wk, pos, slot_of = inputs
    a = op.attrs
    E, C, K = a["experts"], a["capacity"], a["k"]
    h = gy.shape[-1]
    d_fl = gy.new_zeros(E * C + 1, h)
    for k in range(K):
        sl = slot_of[:, k]
        tgt = torch.where(sl >= 0, sl, torch.full_like(sl, E * C))
        d_fl.scatter_(0, tgt.unsqueeze(-1).expand(-1, h),
                      gy * wk[:, k].unsqueeze(-1).to(gy.dtype))
    d_recv = d_fl[:E * C]
    recv = eo.reshape(E * C, -1)
    dwk = torch.zeros_like(wk)
    for k in range(K):
        sl = slot_of[:, k]
        dot = (gy.float() * recv[sl.clamp(min=0)].float()).sum(-1)
        dwk[:, k] = dot * (sl >= 0).to(dot.dtype)
    return [d_recv.reshape(E, C, -1), dwk]


def test_moemlp_cpu_matches_previous_composition(monkeypatch):
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.ops import moe_ops as M
    N, H, Fh, E, K = 30, 16, 24, 4, 2
    g, x, tgt, fetches = O.build_moe_graph(N, H, Fh, E, K, cap=0.75)
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    gen = torch.Generator().manual_seed(11)
    feed = {x: torch.randn(N, H, generator=gen) * 4,
            tgt: torch.randn(N, H, generator=gen)}
    new = [t.clone() for t in g.run(fetches, feed, ctx=ctx)]
    assert (new[7] < 0).any(), "capacity 0.75 must drop something"
    monkeypatch.setattr(M.MoEDispatchOp, "compute", _old_dispatch)
    monkeypatch.setattr(M.MoEDispatchGradOp, "compute", _old_dispatch_grad)
    monkeypatch.setattr(M.MoECombineOp, "compute", _old_combine)
    monkeypatch.setattr(M.MoECombineGradOp, "compute", _old_combine_grad)
    old = g.run(fetches, feed, ctx=ctx)
    names = ["y", "loss", "dx", "dgate", "dw1", "dw2", "pos", "slot_of", "wk",
             "probs"]
    for n, a, b in zip(names, new, old):
        assert torch.equal(a, b), n
    assert float(new[3].abs().max()) > 0 and float(new[2].abs().max()) > 0


def test_kernel_limits_mirrored():
    assert F.MOE_MAX_K == 8 and F.MOE_MAX_E == 2048
    assert "moe" not in F._TORCH_FB or os.environ.get(
        "HETU_AMD_TORCH_FALLBACK")
    # beyond the limits the torch branch serves (K = 9 on CPU here)
    probs = O.make_probs(12, 16, seed=1)
    got = F.moe_route(probs, 3, 9)
    ref = O.route(probs, 3, 9)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
