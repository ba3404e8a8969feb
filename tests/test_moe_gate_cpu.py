"""Fused MoE gate (load-balance + router z-loss): the torch branch of
F.moe_gate / F.moe_gate_grad against the fp64 oracle, the graph op, the
MoEMLP / GPT-MoE wiring.  Bounds are the derived ones of moe_gate_oracle."""
import json
import os
import subprocess
import sys

import pytest
import torch

import moe_gate_oracle as GO

from hetu_amd.ops import functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# functional level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E", [2, 8, 96])
@pytest.mark.parametrize("N", [1, 5, 64, 257])
def test_gate_torch_branch_matches_oracle(N, E, dtype):
    gen = torch.Generator().manual_seed(N * 131 + E)
    for K in (1, 2, 4):
        if K > E:
            continue
        logits = GO.gate_inputs(N, E, dtype, seed=N * 1000 + E * 10 + K)
        out = F.moe_gate(logits, K)
        ref = GO.gate_forward(logits, K)
        GO.check_forward(out, ref, logits, K)
        g_probs = torch.randn(N, E, generator=gen).to(dtype)
        g_aux = torch.tensor(0.7)
        g_z = torch.tensor(-0.3)
        lse, cnt = out[3], out[5]
        for gp, ga, gz in ((g_probs, g_aux, g_z), (None, g_aux, g_z),
                           (g_probs, None, g_z), (g_probs, g_aux, None)):
            dl = F.moe_gate_grad(gp, ga, gz, logits, lse, cnt)
            rdl, mdp = GO.gate_backward(logits, ref["cnt"], gp, ga, gz)
            GO.check_backward(dl, rdl, mdp, dtype, E)


def test_gate_tie_rule():
    # a constant row: every prob ties, the lower indices win in order
    for K in (1, 2, 4):
        out = F.moe_gate(torch.full((3, 8), 1.5), K)
        assert torch.equal(out[1], torch.arange(K).expand(3, K))
    # bf16: logits 2.0 and 2.0078125 (one bf16 ulp apart) give probs that
    # round to the same bf16 value; the lower index must be picked first
    row = torch.tensor([[0.0, 2.0078125, 1.0, 2.0]], dtype=torch.bfloat16)
    probs, idx = F.moe_gate(row, 2)[:2]
    assert probs[0, 1] == probs[0, 3], probs
    assert idx.tolist() == [[1, 3]]
    row = torch.tensor([[0.0, 2.0, 1.0, 2.0078125]], dtype=torch.bfloat16)
    probs, idx = F.moe_gate(row, 2)[:2]
    assert probs[0, 1] == probs[0, 3], probs
    assert idx.tolist() == [[1, 3]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_routing_is_what_dispatch_routes(dtype):
    for N, E, K in ((64, 8, 2), (257, 96, 4), (5, 2, 1)):
        logits = GO.gate_inputs(N, E, dtype, seed=N + E + K)
        probs, idx, w, _, _, cnt = F.moe_gate(logits, K)[:6]
        _, _, ridx, rwk = F.moe_route(probs, N, K)
        assert torch.equal(idx, ridx)
        assert torch.equal(w, rwk)
        assert torch.equal(cnt.long(),
                           torch.bincount(ridx.reshape(-1), minlength=E))


def test_gate_limits():
    with pytest.raises(ValueError):
        F.moe_gate(torch.zeros(4, 2), 3)
    assert F.MOE_GATE_MAX_BLOCKS >= 1


# ---------------------------------------------------------------------------
# graph op
# ---------------------------------------------------------------------------

def _graph():
    from hetu_amd.graph.graph import DefineAndRunGraph, push_graph, pop_graph
    return DefineAndRunGraph("gate"), push_graph, pop_graph


@pytest.mark.parametrize("a,b,use_r", [(0.7, -0.3, True), (0.5, 0.0, False),
                                       (0.0, 2.0, True), (0.0, 0.0, True)])
def test_gate_op_gradient_matches_autograd(a, b, use_r):
    """loss = sum(probs * R) + a * aux + b * z through ht.moe_gate against
    torch.autograd in fp64 on the dense formula with cnt held constant."""
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.ops import api as ht
    N, E, K = 37, 8, 2
    logits_v = GO.gate_inputs(N, E, torch.float32, seed=3)
    R = torch.randn(N, E, generator=torch.Generator().manual_seed(4))
    g, push_graph, pop_graph = _graph()
    push_graph(g)
    try:
        lg = ht.variable(logits_v.clone(), name="logits")
        Rt = ht.variable(R, name="R", requires_grad=False)
        probs, aux, z = ht.moe_gate(lg, K)
        terms = []
        if use_r:
            terms.append(ht.reduce_sum(ht.mul(probs, Rt)))
        if a:
            terms.append(ht.mul(aux, a))
        if b:
            terms.append(ht.mul(z, b))
        if not terms:                       # only probs carries a gradient
            terms.append(ht.reduce_sum(ht.mul(probs, Rt)))
        loss = terms[0] if len(terms) == 1 else ht.add_n(terms)
        (dlg,) = ht.gradients(loss, [lg])
    finally:
        pop_graph()
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    lv, dv, av, zv = g.run([loss, dlg, aux, z], {}, ctx=ctx)
    assert av.dtype == zv.dtype == torch.float32 and av.ndim == 0

    x = logits_v.double().requires_grad_(True)
    p = torch.softmax(x, -1)
    cnt = GO.gate_forward(logits_v, K)["cnt"].double()
    raux = E / N ** 2 * (p.sum(0) * cnt).sum()
    rz = (torch.logsumexp(x, -1) ** 2).mean()
    rl = a * raux + b * rz
    if use_r or not (a or b):
        rl = rl + (p * R.double()).sum()
    rl.backward()
    assert abs(float(lv) - rl.item()) <= 1e-5 * abs(rl.item()) + 1e-6
    mdp = float(R.abs().max()) + abs(a) * E / N ** 2 * float(cnt.max())
    GO.check_backward(dv, x.grad, mdp, torch.float32, E)


# ---------------------------------------------------------------------------
# MoEMLP
# ---------------------------------------------------------------------------

def _build_layer(N=32, H=16, Fh=24, E=4, K=2, cap=100.0, seed=0, **kw):
    from hetu_amd.graph.ops import api as ht
    from hetu_amd.nn.moe import MoEMLP
    torch.manual_seed(seed)
    g, push_graph, pop_graph = _graph()
    push_graph(g)
    try:
        x = ht.placeholder((N, H), name="x")
        tgt = ht.placeholder((N, H), name="tgt")
        moe = MoEMLP(H, Fh, E, k=K, capacity_factor=cap, **kw)
        y = moe(x)
        loss = ht.mse_loss(y, tgt)
        grads = ht.gradients(loss, [x, moe.gate, moe.w1, moe.w2])
    finally:
        pop_graph()
    return g, x, tgt, moe, [y, loss] + list(grads)


def _run_layer(built, N=32, H=16):
    from hetu_amd.engine.runner import prepare_run_context
    g, x, tgt, moe, fetches = built
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    gen = torch.Generator().manual_seed(21)
    feed = {x: torch.randn(N, H, generator=gen) * 3,
            tgt: torch.randn(N, H, generator=gen)}
    return [t.clone() for t in g.run(fetches, feed, ctx=ctx)]


def test_moemlp_default_graph_unchanged():
    default = _build_layer()
    plain = _build_layer(fused_gate=False)
    types_d = [op.type for op in default[0].ops]
    types_p = [op.type for op in plain[0].ops]
    assert types_d == types_p
    assert "MoEGate" not in types_d and "Softmax" in types_d
    assert default[3].aux_loss is None and default[3].z_loss is None
    for a, b in zip(_run_layer(default), _run_layer(plain)):
        assert torch.equal(a, b)


def test_moemlp_fused_gate_same_output():
    plain = _build_layer(fused_gate=False)
    fused = _build_layer(aux_loss_coef=0.01, fused_gate=True)
    types = [op.type for op in fused[0].ops]
    assert "MoEGate" in types and "Softmax" not in types
    assert fused[3].aux_loss is not None and fused[3].z_loss is not None
    a, b = _run_layer(plain), _run_layer(fused)
    assert torch.equal(a[0], b[0])          # y, bit for bit
    # a coefficient alone switches the fused gate on
    auto = _build_layer(z_loss_coef=0.001)
    assert "MoEGate" in [op.type for op in auto[0].ops]


@pytest.mark.parametrize("gate_type", ["hash", "random"])
def test_moemlp_static_gates_reject_coefficients(gate_type):
    from hetu_amd.nn.moe import MoEMLP
    g, push_graph, pop_graph = _graph()
    push_graph(g)
    try:
        with pytest.raises(ValueError):
            MoEMLP(16, 24, 4, gate_type=gate_type, aux_loss_coef=0.01)
        with pytest.raises(ValueError):
            MoEMLP(16, 24, 4, gate_type=gate_type, z_loss_coef=0.01)
        MoEMLP(16, 24, 4, gate_type=gate_type)
    finally:
        pop_graph()


def test_aux_loss_balances_a_collapsing_gate():
    """Tokens share a direction d and gate rows 0 and 1 lean towards it, so
    two experts take almost every choice.  Training the gate on aux alone
    (Adam, lr 1e-2, 40 steps) must spread the load.  Plain torch on the
    same setup: aux 2.640 -> 2.005, largest count 255 -> 82 of 512."""
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.ops import api as ht
    from hetu_amd.graph.ops.optim import Adam
    from hetu_amd.nn.moe import MoEMLP
    N, H, E, K = 256, 32, 8, 2
    torch.manual_seed(0)
    d = torch.randn(H)
    xd = torch.randn(N, H) + d
    dh = d / d.norm()
    gate = 0.02 * torch.randn(E, H)
    gate[0] += 0.05 * dh
    gate[1] += 0.03 * dh
    g, push_graph, pop_graph = _graph()
    push_graph(g)
    try:
        x = ht.placeholder((N, H), name="x")
        moe = MoEMLP(H, 16, E, k=K, capacity_factor=100.0,
                     aux_loss_coef=1.0)
        moe.gate.set_data(gate.clone())
        moe(x)
        step = Adam(lr=1e-2).minimize(moe.aux_loss, params=[moe.gate])
    finally:
        pop_graph()
    cnt = moe.gate_counts
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    hist = []
    for _ in range(41):
        av, cv, _ = g.run([moe.aux_loss, cnt, step], {x: xd}, ctx=ctx)
        hist.append((float(av), int(cv.max())))
    (aux0, max0), (aux40, max40) = hist[0], hist[40]
    print("aux", aux0, "->", aux40, "max count", max0, "->", max40)
    assert aux40 < aux0 - 0.1, hist
    assert max40 < max0 / 2, hist


# ---------------------------------------------------------------------------
# GPT-MoE
# ---------------------------------------------------------------------------

def _gpt(recompute=False, **cfg_kw):
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.models.gpt import GPTConfig, build_gpt_train_graph
    cfg = GPTConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=64,
                    ffn_hidden=128, vocab=312, max_seq=16, moe_experts=4,
                    moe_k=2, **cfg_kw)
    g, h = build_gpt_train_graph(cfg, micro_batch=2, seq_len=16,
                                 dtype=torch.float32, lr=1e-3,
                                 recompute=recompute)
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    torch.manual_seed(0)
    ids = torch.randint(0, 312, (2, 16))
    lab = torch.randint(0, 312, (32,))
    return g, h, ctx, {h["input_ids"]: ids, h["labels"]: lab}


def test_gpt_moe_loss_composition_and_training():
    g, h, ctx, feed = _gpt(moe_aux_coef=0.01, moe_z_coef=0.001)
    assert h["aux_loss"] is not None and h["z_loss"] is not None
    losses = []
    for _ in range(6):
        lv, lm, av, zv, _ = g.run([h["loss"], h["lm_loss"], h["aux_loss"],
                                   h["z_loss"], h["train_op"]], feed,
                                  ctx=ctx)
        assert av.dtype == zv.dtype == torch.float32
        want = float(lm) + 0.01 * float(av) + 0.001 * float(zv)
        # three fp32 roundings of values of the size of the loss
        assert abs(float(lv) - want) <= 4 * 2.0 ** -24 * abs(want), \
            (float(lv), want)
        assert float(av) > 0.0 and float(zv) > 0.0
        losses.append(float(lv))
    assert losses[-1] < losses[0] - 0.5, losses


def test_gpt_moe_gate_grads_same_with_recompute():
    """The gradients the optimizer applies to the two gate weights, with
    and without recompute scopes around the blocks."""
    outs = []
    for rc in (False, True):
        g, h, ctx, feed = _gpt(recompute=rc, moe_aux_coef=0.01,
                               moe_z_coef=0.001)
        ups = [u.producer for u in h["optimizer"].update_ops]
        grads = [u.inputs[1] for u in ups if "gate" in u.inputs[0].name]
        assert len(grads) == 2
        if rc:
            assert any(op.type == "MoEGate" and op.name.endswith("_rc")
                       for op in g.ops)
        outs.append([t.clone() for t in g.run(grads, feed, ctx=ctx)])
    for a, b in zip(*outs):
        assert float(a.abs().max()) > 0
        assert torch.equal(a, b)


def test_gpt_moe_zero_coefficients_change_nothing():
    runs = []
    for kw in ({}, {"moe_aux_coef": 0.0, "moe_z_coef": 0.0}):
        g, h, ctx, feed = _gpt(**kw)
        assert "MoEGate" not in [op.type for op in g.ops]
        assert h["aux_loss"] is None and h["z_loss"] is None
        assert h["lm_loss"] is h["loss"]
        vals = []
        for _ in range(3):
            lv, _ = g.run([h["loss"], h["train_op"]], feed, ctx=ctx)
            vals.append(lv.clone())
        runs.append(vals)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_gpt_pipeline_stage_rejects_gate_losses():
    from hetu_amd.models.gpt import GPTConfig, build_gpt_pipeline_stage
    cfg = GPTConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=64,
                    ffn_hidden=128, vocab=312, max_seq=16, moe_experts=4,
                    moe_k=2, moe_aux_coef=0.01)
    with pytest.raises(NotImplementedError, match="pipeline"):
        build_gpt_pipeline_stage(cfg, None, 2, 16)


# ---------------------------------------------------------------------------
# expert parallelism: statistics are per rank over the rank's own tokens
# ---------------------------------------------------------------------------

WORKER = r"""
import json, os, sys
sys.path.insert(0, os.environ["HETU_REPO"])
import torch
import hetu_amd
from hetu_amd.nn.parallel import ParallelSpec
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import DefineAndRunGraph, push_graph, pop_graph
from hetu_amd.graph.ops import api as ht
from hetu_amd.nn.moe import MoEMLP

ws = int(os.environ.get("WORLD_SIZE", "1"))
rank = int(os.environ.get("RANK", "0"))
sl = int(os.environ.get("TOKEN_SLICE", str(rank)))
N = 8   # tokens per rank
torch.manual_seed(7)
spec = ParallelSpec(dp=ws) if ws > 1 else None
g = DefineAndRunGraph("moe")
push_graph(g)
try:
    x = ht.placeholder((N, 16), name="x",
                       ds=spec.ds_tokens(0) if spec else None,
                       device_group=spec.device_group if spec else None)
    moe = MoEMLP(16, 24, 4, spec=spec, k=2, capacity_factor=100.0,
                 aux_loss_coef=0.01, z_loss_coef=0.001)
    y = moe(x)
finally:
    pop_graph()
ctx = prepare_run_context(g, torch.device("cpu"))
gen = torch.Generator().manual_seed(55)
xd_all = torch.randn(N * 2, 16, generator=gen) * 4
xd = xd_all[sl * N:(sl + 1) * N]
yv, av, zv = g.run([y, moe.aux_loss, moe.z_loss], {x: xd}, ctx=ctx)
print("GOUT:" + json.dumps([rank, float(av), float(zv)]))
"""


def _gout(out):
    for line in out.splitlines():
        if line.startswith("GOUT:"):
            return json.loads(line[5:])
    return None


def test_gate_losses_ep2_are_per_rank():
    env0 = {**os.environ, "HETU_REPO": REPO, "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": "29653", "GLOO_SOCKET_IFNAME": "lo"}
    procs = []
    for r in range(2):
        env = dict(env0, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER],
                                      env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    singles = [subprocess.Popen(
        [sys.executable, "-c", WORKER],
        env={**os.environ, "HETU_REPO": REPO, "WORLD_SIZE": "1",
             "TOKEN_SLICE": str(r)},
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for r in range(2)]
    got = {}
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        # gloo teardown may SIGABRT (-6) after a clean run
        assert p.returncode in (0, -6), f"rank {r} failed:\n{out}\n{err}"
        res = _gout(out)
        assert res is not None, f"rank {r}:\n{out}\n{err}"
        got[res[0]] = res[1:]
    for r, p in enumerate(singles):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err
        res = _gout(out)
        assert res is not None and got[r] == res[1:], (r, got[r], res)
    assert got[0] != got[1]


STEP_WORKER = r"""
import json, os, sys
sys.path.insert(0, os.environ["HETU_REPO"])
import torch
import hetu_amd
from hetu_amd.nn.parallel import ParallelSpec
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import DefineAndRunGraph, push_graph, pop_graph
from hetu_amd.graph.ops import api as ht
from hetu_amd.graph.ops.optim import Adam
from hetu_amd.nn.moe import MoEMLP

ws = int(os.environ.get("WORLD_SIZE", "1"))
rank = int(os.environ.get("RANK", "0"))
sl = int(os.environ.get("TOKEN_SLICE", str(rank)))
N = 8   # tokens per rank
torch.manual_seed(7)
spec = ParallelSpec(dp=ws) if ws > 1 else None
g = DefineAndRunGraph("moe")
push_graph(g)
try:
    kw = dict(ds=spec.ds_tokens(0),
              device_group=spec.device_group) if spec else {}
    x = ht.placeholder((N, 16), name="x", **kw)
    tgt = ht.placeholder((N, 16), name="tgt", **kw)
    moe = MoEMLP(16, 24, 4, spec=spec, k=2, capacity_factor=100.0,
                 aux_loss_coef=0.01, z_loss_coef=0.001)
    loss = ht.add_n([ht.mse_loss(moe(x), tgt), ht.mul(moe.aux_loss, 0.01),
                     ht.mul(moe.z_loss, 0.001)])
    opt = Adam(lr=1e-3)
    step = opt.minimize(loss, params=[moe.gate])
finally:
    pop_graph()
grad = opt.update_ops[0].producer.inputs[1]    # what the optimizer applies
ctx = prepare_run_context(g, torch.device("cpu"))
gen = torch.Generator().manual_seed(55)
xa = torch.randn(N * 2, 16, generator=gen) * 4
ta = torch.randn(N * 2, 16, generator=gen)
feed = {x: xa[sl * N:(sl + 1) * N], tgt: ta[sl * N:(sl + 1) * N]}
gv, lv, _ = g.run([grad, loss, step], feed, ctx=ctx)
print("GOUT:" + json.dumps([rank, float(lv), gv.flatten().tolist()]))
"""


def test_gate_losses_ep2_train_step_gate_gradient():
    """Two ranks, tokens split, experts sharded: mse + 0.01 aux + 0.001 z
    builds (the per-rank scalars are partial sums), a gate step runs, each
    rank's loss is the single-process loss on its token slice and the gate
    gradient the optimizer applies is the same on both ranks: the existing
    gate-gradient all-reduce of the two single-process gradients."""
    env0 = {**os.environ, "HETU_REPO": REPO, "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": "29655", "GLOO_SOCKET_IFNAME": "lo"}
    procs = [subprocess.Popen(
        [sys.executable, "-c", STEP_WORKER],
        env=dict(env0, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r)),
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for r in range(2)]
    singles = [subprocess.Popen(
        [sys.executable, "-c", STEP_WORKER],
        env={**os.environ, "HETU_REPO": REPO, "WORLD_SIZE": "1",
             "TOKEN_SLICE": str(r)},
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for r in range(2)]
    got, ref = {}, {}
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        # gloo teardown may SIGABRT (-6) after a clean run
        assert p.returncode in (0, -6), f"rank {r} failed:\n{out}\n{err}"
        res = _gout(out)
        assert res is not None, f"rank {r}:\n{out}\n{err}"
        got[res[0]] = (res[1], torch.tensor(res[2], dtype=torch.float64))
    for r, p in enumerate(singles):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err
        res = _gout(out)
        ref[r] = (res[1], torch.tensor(res[2], dtype=torch.float64))
    for r in range(2):
        assert got[r][0] == ref[r][0], (r, got[r][0], ref[r][0])
    assert torch.equal(got[0][1], got[1][1])
    want = ref[0][1] + ref[1][1]
    assert float(want.abs().max()) > 0
    # one fp32 addition per element
    err = (got[0][1] - want).abs()
    assert bool((err <= 2.0 ** -23 * want.abs() + 1e-30).all()), \
        float(err.max())


def test_gpt_moe_gate_losses_build_with_split_tokens():
    """dp = 2 (build only): the LM loss and the gate losses are partial
    sums over the two ranks; their sum is too and is all-reduced for the
    report like the LM loss alone."""
    from hetu_amd.models.gpt import GPTConfig, build_gpt_train_graph
    cfg = GPTConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=64,
                    ffn_hidden=128, vocab=312, max_seq=16, moe_experts=4,
                    moe_k=2, moe_aux_coef=0.01, moe_z_coef=0.001)
    g, h = build_gpt_train_graph(cfg, micro_batch=2, seq_len=16,
                                 dtype=torch.float32, dp=2)
    m = h["model"]
    for t in (m.lm_loss, m.aux_loss, m.z_loss):
        assert t.ds.partial == 2, t.ds
    for key in ("loss", "lm_loss", "aux_loss", "z_loss"):
        assert h[key].ds.partial == 1 and h[key].ds.dup == 2, (key, h[key].ds)
    # the reported gate losses are means over the ranks: 1 / split applied
    assert any(op.type == "MulScalar" and op.attrs["value"] == 0.5
               for op in g.ops)
