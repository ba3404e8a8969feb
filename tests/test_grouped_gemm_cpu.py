"""Grouped expert GEMM, torch branch and graph layer (CPU): the semantics
the HIP kernels are held to in test_grouped_gemm_gpu.py."""
import os
import subprocess
import sys

import pytest
import torch

from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
from hetu_amd.graph.ops import api as ht
from hetu_amd.ops import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, P, SEG, K, N = 3, 2, 4, 8, 5
COUNTS = torch.tensor([[4, 0], [1, 3], [0, 0]], dtype=torch.int32)


def _mask():
    return (torch.arange(SEG).view(1, 1, SEG)
            < COUNTS.view(G, P, 1)).reshape(G, P * SEG, 1)


@pytest.mark.parametrize("trans_b", [False, True])
def test_torch_branch_zeroes_invalid_rows(trans_b):
    torch.manual_seed(0)
    a = torch.randn(G, P * SEG, K)
    b = torch.randn(G, N, K) if trans_b else torch.randn(G, K, N)
    ref = (a @ (b.transpose(1, 2) if trans_b else b)) * _mask()
    a = torch.where(_mask(), a, torch.full_like(a, float("nan")))
    out = F.grouped_gemm(a, b, COUNTS, SEG, trans_b=trans_b)
    assert torch.equal(out[~_mask().expand_as(out)],
                       torch.zeros(int((~_mask()).sum()) * N))
    torch.testing.assert_close(out, ref)
    full = F.grouped_gemm(torch.nan_to_num(a), b, trans_b=trans_b)
    torch.testing.assert_close(full * _mask(), ref)
    with pytest.raises(RuntimeError, match="counts"):
        F.grouped_gemm(a, b, COUNTS, SEG + 1, trans_b=trans_b)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        F.grouped_gemm(a, b, COUNTS, SEG, trans_b=trans_b, impl="hip")


def test_torch_branch_tn_and_slot_counts():
    torch.manual_seed(1)
    a, b = torch.randn(G, 6, K), torch.randn(G, 6, N)
    torch.testing.assert_close(F.grouped_gemm_tn(a, b),
                               torch.einsum("gmk,gmn->gkn", a, b))
    pos = torch.tensor([[3, 0, -1, -1], [-1, -1, -1, -1], [1, 2, 4, 5]])
    got = F.moe_slot_counts(pos)
    assert got.dtype == torch.int32 and got.tolist() == [2, 0, 4]


def test_graph_gradients_match_autograd():
    torch.manual_seed(2)
    # a's empty slots hold zeros, as dispatch leaves them: the weight
    # gradient runs over all rows and relies on it
    av, bv, cv = (torch.randn(G, P * SEG, K) * _mask(), torch.randn(G, K, N),
                  torch.randn(G, P * SEG, N))
    g = DefineAndRunGraph("gmm")
    push_graph(g)
    try:
        a = ht.placeholder((G, P * SEG, K), name="a")
        c = ht.placeholder((G, P * SEG, N), name="c")
        cnt = ht.placeholder((G, P), dtype=torch.int32, name="cnt")
        b = ht.variable(bv.clone(), name="b")
        y = ht.grouped_matmul(a, b, cnt, SEG)
        loss = ht.reduce_sum(ht.mul(y, c))
        grads = ht.gradients(loss, [a, b])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    yv, da, db = g.run([y] + list(grads), {a: av, c: cv, cnt: COUNTS},
                       ctx=ctx)
    ar, br = av.clone().requires_grad_(True), bv.clone().requires_grad_(True)
    yr = (ar @ br) * _mask()
    (yr * cv).sum().backward()
    torch.testing.assert_close(yv, yr.detach())
    torch.testing.assert_close(da, ar.grad)
    torch.testing.assert_close(db, br.grad)


def run_layer(mode, dtype, device, N, H, Fh, E, cap=1.0):
    """[y, dx, dw1, dw2] of one MoEMLP forward + backward on the same bf16
    valued weights and inputs for every (mode, dtype).  The gate reads
    x[:, :E], which holds multiples of 1/4, through a unit weight: logits
    are exact and either equal or 1/4 apart in every dtype, so all runs
    route alike."""
    from hetu_amd.nn.moe import MoEMLP
    gen = torch.Generator().manual_seed(3)

    def rnd(*shape, std=1.0):
        v = (torch.randn(*shape, generator=gen) * std).to(torch.bfloat16)
        return v.to(dtype)
    g = DefineAndRunGraph(f"layer_{mode}")
    push_graph(g)
    try:
        x = ht.placeholder((N, H), dtype=dtype, name="x")
        c = ht.placeholder((N, H), dtype=dtype, name="c")
        moe = MoEMLP(H, Fh, E, k=2, capacity_factor=cap, dtype=dtype,
                     expert_gemm=mode)
        moe.gate.set_data(torch.eye(E, H, dtype=dtype))
        moe.w1.set_data(rnd(E, H, Fh, std=0.05))
        moe.w2.set_data(rnd(E, Fh, H, std=0.05))
        y = moe(x)
        grads = ht.gradients(ht.reduce_sum(ht.mul(y, c)),
                             [x, moe.w1, moe.w2])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, device, use_comm=False)
    xv, cv = rnd(N, H), rnd(N, H)
    xv[:, :E] = (xv[:, :E] * 4).round() / 4
    return g.run([y] + list(grads), {x: xv.to(device), c: cv.to(device)},
                 ctx=ctx)


def test_layer_grouped_equals_bmm_fp32():
    # capacity 1.0: some slots fill up and some experts stay partly empty
    outs = [run_layer(m, torch.float32, torch.device("cpu"), 24, 16, 24, 4)
            for m in ("grouped", "bmm")]
    for got, ref in zip(*outs):
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)


WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["HETU_REPO"])
import torch
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
from hetu_amd.graph.ops import api as ht
from hetu_amd.graph.ops.basics import _make
from hetu_amd.graph.ops.moe_ops import MoEDispatchOp, MoESlotCountsOp
from hetu_amd.nn.parallel import ParallelSpec

rank, P, N, H, E, C = int(os.environ["RANK"]), 2, 8, 4, 4, 3
spec = ParallelSpec(dp=P)
g = DefineAndRunGraph("counts")
push_graph(g)
try:
    x = ht.placeholder((N, H), name="x", ds=spec.ds_tokens(0),
                       device_group=spec.device_group)
    probs = ht.placeholder((N, E), name="probs", ds=spec.ds_tokens(0),
                           device_group=spec.device_group)
    attrs = {"experts": E, "capacity": C, "k": 2,
             "ep_ranks": list(spec.device_group)}
    disp = _make(g, MoEDispatchOp(), [x, probs], dict(attrs))
    counts = _make(g, MoESlotCountsOp(), [disp.outputs[2]],
                   dict(attrs)).output()
finally:
    pop_graph()
ctx = prepare_run_context(g, torch.device("cpu"))
gen = torch.Generator().manual_seed(11 + rank)
# skewed: most tokens want expert 0, so its segments fill and others do not
pv = torch.softmax(torch.randn(N, E, generator=gen)
                   + torch.tensor([2.0, 0.0, 0.5, -1.0]), -1)
ein, cnt = g.run([disp.outputs[0], counts],
                 {x: torch.randn(N, H, generator=gen) + 3.0, probs: pv},
                 ctx=ctx)
filled = (ein.abs().sum(-1) > 0).reshape(E // P, P, C)
want = torch.arange(C).view(1, 1, C) < cnt.view(E // P, P, 1)
assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (E // P, P), cnt
assert torch.equal(filled, want), (filled, cnt)
assert 0 < int(cnt.sum()) < E // P * P * C, cnt
print("COUNTS_OK")
"""


def test_slot_counts_ep2_layout_matches_expert_in():
    env0 = {**os.environ, "HETU_REPO": REPO, "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": "29583", "GLOO_SOCKET_IFNAME": "lo",
            "WORLD_SIZE": "2"}
    procs = [subprocess.Popen([sys.executable, "-c", WORKER],
                              env=dict(env0, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True) for r in range(2)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        # gloo teardown may SIGABRT (-6) after a clean run
        assert p.returncode in (0, -6) and "COUNTS_OK" in out, \
            f"rank {r} failed:\n{out}\n{err}"
