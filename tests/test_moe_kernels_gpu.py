"""HIP MoE routing / layout kernels (hetu_amd/ops/hip/moe.hip) against the
brute-force fp64 oracle in moe_oracle.py, plus layer-level and hipGraph
capture checks.

Routing inputs are permutations of (j+1)/2048: no ties, and exact in every
tested dtype, so routing must equal the oracle exactly.  Row tolerances are
derived, not tuned: every row output is ONE rounding of an fp32 sum of at
most K terms, so |got - ref| <= eps_out*|ref| + K*2^-24*max|term| with
eps_out = 2^-9 (bf16), 2^-12 (fp16), 2^-25 (fp32); the asserted bounds are
rtol = 2^-8 / 2^-11 / 1e-5 and atol = 1e-6 * K * max|input|.  dwk is an
fp32 dot over h terms: rtol 1e-4, atol = h * max|gy| * max|recv| * 2^-23.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moe_oracle as O  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = ["moe_topk", "moe_assign_slots", "moe_dispatch_rows",
           "moe_dispatch_rows_bwd", "moe_gate_bwd", "moe_combine_rows",
           "moe_combine_rows_bwd"]


def test_extension_has_moe_kernels():
    for name in KERNELS:
        assert hasattr(F.ext(), name), name
    assert "moe" not in F._TORCH_FB


def dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------

NS = [1, 63, 64, 65, 257, 1000]
ES = [2, 8, 96, 256]
KS = [1, 2, 4]
ROUTE_SHAPES = [(N, E, K) for N in NS for E in ES for K in KS if K <= E]


@functools.lru_cache(maxsize=None)
def _probs(N, E, skew, empty, second=None):
    return O.make_probs(N, E, seed=1000 * N + E, skew=skew,
                        empty_expert=empty, second_to=second)


@functools.lru_cache(maxsize=None)
def _oracle(N, E, skew, empty, second, C, K):
    return O.route(_probs(N, E, skew, empty, second), C, K)


def routing_variants(N, E, K):
    """Yield (name, probs, C, oracle outputs).  Which variant covers which
    condition, each asserted on the oracle's own output so no case passes
    vacuously:
      nodrop    C = N: nothing dropped
      exact     C = the fullest expert's queue: filled exactly to C, no drop
      c1        C = 1
      drop_r0   (N >= 63) skewed probs, C = N // 4: drops already in round 0;
                with K < E expert E-1 receives no token (pos row all -1)
      drop_late (N >= 63, K >= 2) second choices crowd expert 0, C = the
                fullest round-0 queue: round 0 drops nothing, later rounds
                drop against the count carried from earlier rounds
    """
    uni = (N, E, 0.0, None, None)
    pos, slot_of, idx_uni, wk = ref = _oracle(*uni, N, K)
    assert (slot_of >= 0).all()
    yield "nodrop", _probs(*uni), N, ref

    C = int(torch.bincount(idx_uni.reshape(-1), minlength=E).max())
    pos, slot_of, idx, wk = ref = _oracle(*uni, C, K)
    assert (slot_of >= 0).all() and (pos >= 0).all(-1).any()
    yield "exact", _probs(*uni), C, ref

    pos, slot_of, idx, wk = ref = _oracle(*uni, 1, K)
    assert pos.shape == (E, 1)
    yield "c1", _probs(*uni), 1, ref

    if N >= 63:
        empty = E - 1 if K < E else None
        sk = (N, E, 0.7, empty, None)
        C = N // 4
        pos, slot_of, idx, wk = ref = _oracle(*sk, C, K)
        assert (slot_of[:, 0] < 0).any()
        if empty is not None:
            assert (pos[empty] < 0).all()
        yield "drop_r0", _probs(*sk), C, ref

    if N >= 63 and K >= 2:
        late = (N, E, 0.0, None, 0)
        C = int(torch.bincount(idx_uni[:, 0], minlength=E).max())
        pos, slot_of, idx, wk = ref = _oracle(*late, C, K)
        assert torch.equal(idx[:, 0], idx_uni[:, 0])
        assert (slot_of[:, 0] >= 0).all() and (slot_of[:, 1:] < 0).any()
        yield "drop_late", _probs(*late), C, ref


@pytest.mark.parametrize("N,E,K", ROUTE_SHAPES)
def test_route_matches_oracle(N, E, K):
    dtypes = [torch.float32]
    if E <= 96:
        dtypes += [torch.bfloat16, torch.float16]
    seen = set()
    for name, probs, C, ref in routing_variants(N, E, K):
        seen.add(name)
        for dt in dtypes:
            p = probs.to(dt)
            assert torch.equal(p.float(), probs), "values must be exact"
            assert all(len(set(r)) == E for r in p.float().tolist()[:64])
            got = F.moe_route(p.to(dev()), C, K)
            for what, a, b in zip(("pos", "slot_of", "idx", "wk"), got, ref):
                assert a.dtype == b.dtype, (name, dt, what)
                assert torch.equal(a.cpu(), b), (name, dt, what)
    assert {"nodrop", "exact", "c1"} <= seen
    if N >= 63:
        assert "drop_r0" in seen
        if K >= 2:
            assert "drop_late" in seen


def test_probs_rows_are_distinct():
    for N, E in ((1000, 256), (257, 96), (65, 2)):
        p = _probs(N, E, 0.7, None, 0)
        assert (p.sort(-1).values.diff(dim=-1) > 0).all()


def test_tie_goes_to_lower_expert_index():
    """fp32, E = 8: experts 2 and 5 hold the same, largest probability for
    every token; 2 must be selected first, then 5."""
    N, E, K, C = 100, 8, 3, 100
    probs = O.make_probs(N, E, seed=9)
    probs[:, 2] = 0.5
    probs[:, 5] = 0.5
    got = F.moe_route(probs.to(dev()), C, K)
    assert (got[2][:, 0].cpu() == 2).all() and (got[2][:, 1].cpu() == 5).all()
    for a, b in zip(got, O.route(probs, C, K)):
        assert torch.equal(a.cpu(), b)


# ---------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------

ROW_N, ROW_E, ROW_C = 130, 8, 12
RTOL = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8,
        torch.float16: 2.0 ** -11}


@functools.lru_cache(maxsize=None)
def _row_routing(K):
    """Skewed routing with drops, fully dropped tokens and an empty expert."""
    probs = O.make_probs(ROW_N, ROW_E, seed=77, skew=0.7, empty_expert=5)
    pos, slot_of, idx, wk = O.route(probs, ROW_C, K)
    assert (slot_of < 0).all(-1).any(), "need a fully dropped token"
    assert (pos[5] < 0).all(), "need an empty expert"
    assert (pos.view(-1) < 0).any() and (pos.view(-1) >= 0).any()
    g = torch.Generator().manual_seed(K)
    w = torch.rand(ROW_N, K, generator=g) * 0.9 + 0.1
    w = torch.where(slot_of >= 0, w, torch.zeros_like(w))
    g_w = torch.randn(ROW_N, K, generator=g)
    return probs, pos, slot_of, w, g_w


@functools.lru_cache(maxsize=None)
def _row_case(h, dt, K):
    """Inputs (as stored in dtype dt) and the fp64 oracle outputs."""
    probs, pos, slot_of, wk, g_w = _row_routing(K)
    g = torch.Generator().manual_seed(h)
    x = torch.randn(ROW_N, h, generator=g).to(dt)
    rows = torch.randn(ROW_E * ROW_C, h, generator=g).to(dt)
    gy = torch.randn(ROW_N, h, generator=g).to(dt)
    ref = dict(send=O.dispatch_rows(x, pos),
               dx=O.dispatch_rows_bwd(rows, slot_of),
               y=O.combine_rows(rows, wk, slot_of),
               dprobs=O.gate_bwd(g_w, slot_of, ROW_E, ROW_C))
    ref["d_recv"], ref["dwk"] = O.combine_rows_bwd(gy, rows, wk, pos, slot_of)
    return x, rows, gy, ref


def _run_rows(h, dt, K):
    probs, pos, slot_of, wk, g_w = _row_routing(K)
    x, rows, gy, _ = _row_case(h, dt, K)
    d = dev()
    pos_d, sl_d, wk_d = pos.to(d), slot_of.to(d), wk.to(d)
    S = ROW_E * ROW_C
    send = torch.full((S, h), float("nan"), dtype=dt, device=d)
    F.moe_dispatch_rows(x.to(d), pos_d, out=send)
    d_recv = torch.full((S, h), float("nan"), dtype=dt, device=d)
    d_recv2, dwk = F.moe_combine_rows_bwd(gy.to(d), rows.to(d), wk_d, pos_d,
                                          sl_d, out=d_recv)
    assert d_recv2.data_ptr() == d_recv.data_ptr()
    return dict(
        send=send, d_recv=d_recv, dwk=dwk,
        send_alloc=F.moe_dispatch_rows(x.to(d), pos_d),
        dx=F.moe_dispatch_rows_bwd(rows.to(d), pos_d, sl_d),
        y=F.moe_combine_rows(rows.to(d), wk_d, sl_d),
        dprobs=F.moe_gate_bwd(g_w.to(d), sl_d, probs.to(dt).to(d), ROW_C))


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16],
                         ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("h", [8, 64, 1000, 1001, 4096])
def test_rows_match_oracle(h, dt, K):
    probs, pos, slot_of, wk, g_w = _row_routing(K)
    x, rows, gy, ref = _row_case(h, dt, K)
    got = {k: v.cpu() for k, v in _run_rows(h, dt, K).items()}
    mx = float(max(x.abs().max(), rows.abs().max(), gy.abs().max()))
    tol = dict(rtol=RTOL[dt], atol=1e-6 * K * mx)
    for k in ("send", "send_alloc", "d_recv", "dx", "y"):
        assert got[k].dtype == dt and not got[k].isnan().any(), k
    assert got["dwk"].dtype == torch.float32

    # pure copies are exact
    assert torch.equal(got["send"].double(), ref["send"])
    assert torch.equal(got["send_alloc"].double(), ref["send"])
    if K == 1:
        assert torch.equal(got["dx"].double(), ref["dx"])
    assert torch.equal(got["dprobs"], ref["dprobs"].to(dt))
    # one rounding of an fp32 sum of <= K terms
    for k in ("dx", "y", "d_recv"):
        err = (got[k].double() - ref[k]).abs()
        bound = tol["atol"] + tol["rtol"] * ref[k].abs()
        assert (err <= bound).all(), (k, float((err - bound).max()))
    err = (got["dwk"].double() - ref["dwk"]).abs()
    gmax, rmax = float(gy.abs().max()), float(rows.abs().max())
    bound = h * gmax * rmax * 2.0 ** -23 + 1e-4 * ref["dwk"].abs()
    assert (err <= bound).all(), float((err - bound).max())

    # empty slots and fully dropped tokens: exact zeros
    pad = pos.view(-1) < 0
    dead = (slot_of < 0).all(-1)
    assert (got["send"][pad] == 0).all() and (got["d_recv"][pad] == 0).all()
    assert (got["y"][dead] == 0).all() and (got["dx"][dead] == 0).all()
    assert (got["dwk"][slot_of < 0] == 0).all()


def test_kernels_are_deterministic():
    """Two calls on the same inputs: bit-equal outputs, every kernel."""
    probs = _probs(1000, 96, 0.7, 95, None).to(dev())
    a, b = F.moe_route(probs, 30, 4), F.moe_route(probs, 30, 4)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for dt in (torch.float32, torch.bfloat16):
        r1, r2 = _run_rows(1000, dt, 2), _run_rows(1000, dt, 2)
        for k in r1:
            assert torch.equal(r1[k], r2[k]), (dt, k)


# ---------------------------------------------------------------------------
# layer level: MoEMLP graph, HIP family live vs forced to the torch branch
# ---------------------------------------------------------------------------

LN, LH, LF, LE, LK, LCAP = 130, 64, 128, 8, 2, 0.75
NAMES = ["y", "loss", "dx", "dgate", "dw1", "dw2", "pos", "slot_of", "wk",
         "probs"]


def _layer_inputs():
    """x, tgt and the gate weight.  The gate is drawn wide (std 0.5) so the
    probabilities of a token are well apart, and everything is stored with
    bf16-exact values so the fp32 and bf16 graphs see the same numbers.
    Seed 29 is the one of 0..299 whose closest pair among a token's top
    three logits is furthest apart (1.2 % of the largest), so bf16 rounding
    of the logits cannot reorder them; the tests assert that no ties and
    no routing difference occur."""
    g = torch.Generator().manual_seed(29)
    x = torch.randn(LN, LH, generator=g).bfloat16().float()
    tgt = torch.randn(LN, LH, generator=g).bfloat16().float()
    gate = (torch.randn(LE, LH, generator=g) * 0.5).bfloat16().float()
    return x, tgt, gate


def _layer_run(dtype, fallback, monkeypatch, params=None):
    from hetu_amd.engine.runner import prepare_run_context
    g, x, tgt, fetches = O.build_moe_graph(LN, LH, LF, LE, LK, LCAP,
                                           dtype=dtype, seed=3)
    xd, td, gate = _layer_inputs()
    for p in g.parameters:
        name = p.name.split(":")[0]
        if params is not None:
            p.set_data(params[name].to(dtype))
        elif name == "moe.gate.weight":
            p.set_data(gate.to(dtype))
    ctx = prepare_run_context(g, dev(), use_comm=False)
    feed = {x: xd.to(dtype).to(dev()), tgt: td.to(dtype).to(dev())}
    outs = {}
    for side in ("hip", "torch") if fallback == "both" else (fallback,):
        with monkeypatch.context() as m:
            if side == "torch":
                m.setattr(F, "_TORCH_FB", F._TORCH_FB | {"moe"})
            outs[side] = dict(zip(NAMES, [t.clone() for t in
                                          g.run(fetches, feed, ctx=ctx)]))
    weights = {p.name.split(":")[0]: p.get_data().float().cpu()
               for p in g.parameters}
    return outs, weights


def _no_ties(probs, K):
    top = probs.float().topk(K + 1, dim=-1).values
    return bool((top[:, :-1] > top[:, 1:]).all())


def test_layer_fp32_hip_matches_torch_branch(monkeypatch):
    outs, _ = _layer_run(torch.float32, "both", monkeypatch)
    hip, ref = outs["hip"], outs["torch"]
    assert _no_ties(ref["probs"], LK)
    assert (ref["slot_of"] < 0).any(), "capacity factor 0.75 must drop"
    for k in ("pos", "slot_of", "wk"):
        assert torch.equal(hip[k], ref[k]), k
    for k in ("y", "loss", "dx", "dgate", "dw1", "dw2"):
        r = ref[k].double()
        err = (hip[k].double() - r).abs()
        bound = 1e-5 * r.abs() + 1e-6 * LK * float(r.abs().max())
        assert float(r.abs().max()) > 0, k
        assert (err <= bound).all(), (k, float((err - bound).max()))


def test_layer_bf16_both_sides_match_fp32_torch_branch(monkeypatch):
    """bf16: the torch branch rounds y K times, so the two bf16 sides are
    each held to the fp32 torch-branch run on the same (bf16-exact) weights
    and inputs instead of to each other.  Bound, normwise: a bf16 value
    carries 2^-9 relative error, a path from x to y crosses <= 6 roundings
    (gate probability, expert_in, h1, gelu, expert_out, y) and the backward
    as many again, errors adding linearly at worst: 12 * 2^-9 < 2^-5 of the
    largest reference magnitude."""
    outs, weights = _layer_run(torch.bfloat16, "both", monkeypatch)
    ref, _ = _layer_run(torch.float32, "torch", monkeypatch, params=weights)
    ref = ref["torch"]
    assert _no_ties(outs["torch"]["probs"], LK)
    assert (ref["slot_of"] < 0).any()
    for side in ("hip", "torch"):
        o = outs[side]
        for k in ("pos", "slot_of"):
            assert torch.equal(o[k], ref[k]), (side, k)
        for k in ("y", "loss", "dx", "dgate", "dw1", "dw2", "wk"):
            r = ref[k].double()
            err = float((o[k].double() - r).abs().max())
            assert err <= 2.0 ** -5 * float(r.abs().max()), (side, k, err)
    for k in ("pos", "slot_of", "wk"):
        assert torch.equal(outs["hip"][k], outs["torch"][k]), k


# ---------------------------------------------------------------------------
# hipGraph capture: one chain, replayed on new inputs
# ---------------------------------------------------------------------------

def _chain(probs, x, gy, C, K):
    pos, slot_of, idx, wk = F.moe_route(probs, C, K)
    send = F.moe_dispatch_rows(x, pos)
    y = F.moe_combine_rows(send, wk, slot_of)
    d_recv, dwk = F.moe_combine_rows_bwd(gy, send, wk, pos, slot_of)
    dx = F.moe_dispatch_rows_bwd(d_recv, pos, slot_of)
    dprobs = F.moe_gate_bwd(dwk, slot_of, probs, C)
    return [pos, slot_of, idx, wk, send, y, d_recv, dwk, dx, dprobs]


def test_capture_and_replay_on_new_inputs():
    N, E, K, h, C = 257, 8, 2, 64, 40
    d = dev()
    g = torch.Generator().manual_seed(12)
    p1 = O.make_probs(N, E, seed=1, skew=0.7).to(torch.bfloat16)
    p2 = O.make_probs(N, E, seed=2, skew=0.7).to(torch.bfloat16)
    x1, x2 = (torch.randn(N, h, generator=g).bfloat16() for _ in range(2))
    gy = torch.randn(N, h, generator=g).bfloat16().to(d)
    r1, r2 = O.route(p1, C, K), O.route(p2, C, K)
    assert not torch.equal(r1[1], r2[1]), "the two routings must differ"
    assert (r1[1] < 0).any() and (r2[1] < 0).any()

    probs, x = p1.to(d), x1.to(d)
    eager1 = [t.clone() for t in _chain(probs, x, gy, C, K)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _chain(probs, x, gy, C, K)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager1):
        assert torch.equal(a, b)
    probs.copy_(p2.to(d))
    x.copy_(x2.to(d))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    eager2 = _chain(p2.to(d), x2.to(d), gy, C, K)
    for a, b in zip(replayed, eager2):
        assert torch.equal(a, b)
    assert torch.equal(replayed[1].cpu(), r2[1])
