"""Fused MoE gate kernels (moe.hip: moe_gate_fwd / moe_gate_grad) against the
brute-force fp64 oracle in moe_gate_oracle.py, plus determinism, hipGraph
replay and a layer-level check against the torch branch.

Exact-routing inputs are row permutations of {0.25 * j} (exact in every
tested dtype; neighbouring probabilities differ by e^0.25, far above any
rounding), so idx and cnt must equal the oracle's; on arbitrary inputs they
must equal the tie rule applied to the kernel's own stored probs, and always
what F.moe_route selects from those probs.

Tolerances are derived, not tuned (asserted in moe_gate_oracle.check_*):
  probs    one rounding of an fp32 value that is good to a few ulp:
           rtol 2^-8 (bf16), 2^-11 (fp16), 1e-5 (fp32); atol 2^-126 where
           fp32 arithmetic may flush (fp32, bf16), half an fp16 subnormal
           step (2^-25) for fp16
  lse      rtol 1e-6 + atol E * 2^-24 (an E-term fp32 sum under the log)
  psum     fp32 sum of N terms in [0, 1], each good to a few ulp:
           rtol (N + 8) * 2^-24
  aux      the psum bounds weighted by cnt: (N + 8) * 2^-24 relative (aux
           itself is summed in fp64 and rounded once)
  z        rtol 1e-5
  dlogits  one rounding of an fp32 expression with an E-term dot: the
           output dtype's rtol + atol E * 2^-23 * max|dp| (+ the same
           underflow floor: small fp16 gradients are stored as subnormals)
"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moe_gate_oracle as GO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def dev():
    return torch.device("cuda", 0)


def test_extension_has_gate_kernels():
    for name in ("moe_gate_fwd", "moe_gate_grad", "moe_gate_bwd",
                 "moe_gate_max_blocks", "moe_gate_tokens_per_block"):
        assert hasattr(F.ext(), name), name
    assert "moe" not in F._TORCH_FB
    assert F.ext().moe_gate_max_blocks() == F.MOE_GATE_MAX_BLOCKS


def _case(N, E, K, dtype, step=0.25):
    """(logits, fp64 reference, upstream grads with their fp64 dlogits)."""
    logits = GO.gate_inputs(N, E, dtype, seed=1000 * N + 10 * E + K,
                            step=step)
    ref = GO.gate_forward(logits, K)
    gen = torch.Generator().manual_seed(N + E + K)
    g_probs = torch.randn(N, E, generator=gen).to(dtype)
    g_aux, g_z = torch.tensor(0.7), torch.tensor(-0.3)
    variants = []
    for gp, ga, gz in ((g_probs, g_aux, g_z), (None, g_aux, g_z),
                       (g_probs, None, g_z), (g_probs, g_aux, None)):
        variants.append((gp, ga, gz) + GO.gate_backward(logits, ref["cnt"],
                                                        gp, ga, gz))
    return logits, ref, variants


def _to(t):
    return None if t is None else t.to(dev())


def _check_case(N, E, K, dtype, step=0.25, logits_dev=None):
    logits, ref, variants = _case(N, E, K, dtype, step)
    ld = logits.to(dev()) if logits_dev is None else logits_dev
    out = F.moe_gate(ld, K)
    GO.check_forward(out, ref, logits, K)
    probs, idx, w, lse, _, cnt = out[:6]
    _, _, ridx, rwk = F.moe_route(probs, N, K)
    assert torch.equal(idx, ridx) and torch.equal(w, rwk)
    for gp, ga, gz, rdl, mdp in variants:
        dl = F.moe_gate_grad(_to(gp), _to(ga), _to(gz), ld, lse, cnt)
        GO.check_backward(dl, rdl, mdp, dtype, E)


NS = [1, 3, 4, 5, 63, 64, 65, 257, 1000]
ES = [2, 8, 63, 64, 65, 96, 256]
KS = [1, 2, 4, 8]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("E", ES)
def test_gate_matches_oracle(E, dtype):
    for N in NS:
        for K in KS:
            if K <= E:
                _check_case(N, E, K, dtype)


def test_gate_e2048_fp32():
    _check_case(65, 2048, 8, torch.float32, step=1.0 / 32)
    _check_case(65, 2048, 1, torch.float32, step=1.0 / 32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_gate_kernel_thresholds(dtype):
    # 64 | 65 (in ES above), 128 | 129 and 256 | 257 switch the forward
    # between 1, 2 and 4 register elements per lane and the looping kernel;
    # 130 leaves the last register element of most lanes empty
    for E in (128, 129, 130, 257):
        for N, K in ((5, 1), (65, 8)):
            _check_case(N, E, K, dtype)


@pytest.mark.parametrize("E,dtype", [(8, torch.bfloat16), (96, torch.bfloat16),
                                     (300, torch.float32)],
                         ids=["8-bf16", "96-bf16", "300-fp32"])
def test_gate_every_block_loops(E, dtype):
    # a block takes tokens_per_block(E) tokens per pass (lane groups for
    # E <= 32, else one wave each): above 2 * that * cap every block of the
    # capped grid loops at least twice
    ext = F.ext()
    N = 2 * ext.moe_gate_tokens_per_block(E) * ext.moe_gate_max_blocks() + 3
    _check_case(N, E, 2, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_gate_element_path(dtype):
    # E % 8 != 0 (and % 4 != 0): no 16 B vector IO in the backward
    _check_case(65, 13, 2, dtype)
    # contiguous rows on a base that is not 16 B aligned
    N, E, K = 65, 64, 2
    logits, _, _ = _case(N, E, K, dtype)
    buf = torch.zeros(N * E + 1, dtype=dtype, device=dev())
    view = buf[1:].view(N, E)
    view.copy_(logits)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    _check_case(N, E, K, dtype, logits_dev=view)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_gate_ties_in_stored_probs(dtype):
    """Arbitrary logits: stored probs tie, the oracle's own top-K no longer
    applies; the tie rule on the kernel's stored probs does."""
    N, E, K = 257, 96, 4
    gen = torch.Generator().manual_seed(5)
    logits = (torch.randn(N, E, generator=gen) * 0.3).to(dtype)
    out = F.moe_gate(logits.to(dev()), K)
    probs = out[0].cpu()
    srt = probs.float().sort(-1, descending=True).values
    assert bool((srt[:, :K] == srt[:, 1:K + 1]).any()), "no tie in the top"
    ref = GO.gate_forward(logits, K, probs=probs)
    GO.check_forward(out, ref, logits, K, exact_routing=False)
    _, _, ridx, rwk = F.moe_route(out[0], N, K)
    assert torch.equal(out[1], ridx) and torch.equal(out[2], rwk)
    dl = F.moe_gate_grad(None, torch.tensor(1.0, device=dev()), None,
                         logits.to(dev()), out[3], out[5])
    rdl, mdp = GO.gate_backward(logits, ref["cnt"], None, 1.0, None)
    GO.check_backward(dl, rdl, mdp, dtype, E)


def _finite(ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


def test_gate_extremes_stay_finite():
    d = dev()
    N, E, K = 65, 64, 2
    gen = torch.Generator().manual_seed(9)
    base = torch.randn(N, E, generator=gen)
    peak = base.clone()
    peak[torch.arange(N), torch.arange(N) % E] += 60.0     # p = 1 exactly
    rows = {"peak": peak, "hi": torch.full((N, E), 80.0) + base,
            "lo": torch.full((N, E), -80.0) + base,
            "const": torch.full((N, E), 3.0)}
    gp = torch.randn(N, E, generator=gen).to(d)
    one = torch.tensor(1.0, device=d)
    for name, lg in rows.items():
        out = F.moe_gate(lg.to(d), K)
        assert _finite(out), name
        ref = GO.gate_forward(lg, K, probs=out[0].cpu())
        GO.check_forward(out, ref, lg, K, exact_routing=False)
        if name == "peak":
            hot = out[0].cpu()[torch.arange(N), torch.arange(N) % E]
            assert bool((hot == 1.0).all())
        if name == "const":
            assert torch.equal(out[1].cpu(), torch.arange(K).expand(N, K))
        for g3 in ((gp, one, one), (None, one, one), (gp, None, one),
                   (gp, one, None), (None, None, None)):
            dl = F.moe_gate_grad(*g3, lg.to(d), out[3], out[5])
            assert _finite([dl]), name
            if g3[0] is None and g3[1] is None and g3[2] is None:
                assert not bool(dl.any())


def test_gate_is_deterministic():
    d = dev()
    N, E, K = 4099, 96, 4
    gen = torch.Generator().manual_seed(2)
    lg = torch.randn(N, E, generator=gen).bfloat16().to(d)
    gp = torch.randn(N, E, generator=gen).bfloat16().to(d)
    ga, gz = torch.tensor(0.5, device=d), torch.tensor(0.25, device=d)
    a = F.moe_gate(lg, K)
    b = F.moe_gate(lg, K)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    da = F.moe_gate_grad(gp, ga, gz, lg, a[3], a[5])
    db = F.moe_gate_grad(gp, ga, gz, lg, b[3], b[5])
    assert torch.equal(da, db)


def _fwd_bwd(lg, gp, ga, gz, K):
    out = F.moe_gate(lg, K)
    return list(out) + [F.moe_gate_grad(gp, ga, gz, lg, out[3], out[5])]


def test_gate_capture_and_three_replays():
    """Capture forward + backward once; rewrite logits in place three times
    (column reduces composed from at::native ops go wrong from the second
    replay) and replay: each replay is bit-equal to an eager call."""
    d = dev()
    N, E, K = 1000, 64, 2
    gen = torch.Generator().manual_seed(31)
    ins = [torch.randn(N, E, generator=gen).bfloat16() for _ in range(4)]
    gp = torch.randn(N, E, generator=gen).bfloat16().to(d)
    ga, gz = torch.tensor(0.01, device=d), torch.tensor(0.001, device=d)
    lg = ins[0].to(d)
    eager = [t.clone() for t in _fwd_bwd(lg, gp, ga, gz, K)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fwd_bwd(lg, gp, ga, gz, K)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    prev_cnt = eager[5].clone()
    for new in ins[1:]:
        lg.copy_(new.to(d))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        want = _fwd_bwd(new.to(d), gp, ga, gz, K)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert not torch.equal(got[5], prev_cnt), "inputs must differ"
        prev_cnt = got[5]


# ---------------------------------------------------------------------------
# layer level: HIP branch here, torch branch in a fresh child process
# ---------------------------------------------------------------------------

LN, LH, LF, LE, LK = 64, 32, 48, 8, 2


def layer_run(out_path=None):
    """MoEMLP(aux_loss_coef=0.01, z_loss_coef=0.001) in bf16 on the GPU with
    loss = mse + 0.01 aux + 0.001 z.  The gate weight is 0.25 on the
    diagonal and the first E columns of x are a row permutation of 0..E-1,
    so the logits are tie-free multiples of 0.25 and both branches route
    alike."""
    from hetu_amd.engine.runner import prepare_run_context
    from hetu_amd.graph.graph import DefineAndRunGraph, push_graph, pop_graph
    from hetu_amd.graph.ops import api as ht
    from hetu_amd.nn.moe import MoEMLP
    dt = torch.bfloat16
    torch.manual_seed(3)
    g = DefineAndRunGraph("gate_layer")
    push_graph(g)
    try:
        x = ht.placeholder((LN, LH), dtype=dt, name="x")
        tgt = ht.placeholder((LN, LH), dtype=dt, name="tgt")
        moe = MoEMLP(LH, LF, LE, k=LK, capacity_factor=100.0, dtype=dt,
                     aux_loss_coef=0.01, z_loss_coef=0.001)
        gate = torch.zeros(LE, LH)
        gate[torch.arange(LE), torch.arange(LE)] = 0.25
        moe.gate.set_data(gate.to(dt))
        y = moe(x)
        loss = ht.add_n([ht.mse_loss(y, tgt), ht.mul(moe.aux_loss, 0.01),
                         ht.mul(moe.z_loss, 0.001)])
        (dgate,) = ht.gradients(loss, [moe.gate])
    finally:
        pop_graph()
    eo = y.producer.inputs[0]
    gen = torch.Generator().manual_seed(8)
    xd = torch.randn(LN, LH, generator=gen)
    xd[:, :LE] = GO.gate_inputs(LN, LE, torch.float32, seed=4, step=1.0)
    td = torch.randn(LN, LH, generator=gen)
    ctx = prepare_run_context(g, dev(), use_comm=False)
    feed = {x: xd.to(dt).to(dev()), tgt: td.to(dt).to(dev())}
    names = ["y", "aux", "z", "dgate", "eo", "cnt"]
    cnt = moe.gate_counts
    vals = g.run([y, moe.aux_loss, moe.z_loss, dgate, eo, cnt], feed,
                 ctx=ctx)
    res = {n: v.detach().float().cpu() for n, v in zip(names, vals)}
    if out_path is not None:
        torch.save(res, out_path)
    return res


def test_layer_bf16_hip_matches_torch_branch(tmp_path):
    """y: both branches combine the same bf16 expert rows r_k with weights
    that differ by at most one bf16 ulp (2 * 2^-8 relative); the kernel
    rounds y once (2^-8), the torch branch rounds K products and K sums
    (2K * 2^-8): |dy| <= (3 + 2K) * 2^-8 * max|r|.  aux and z: both sides
    meet the oracle bounds on identical logits, so they differ by at most
    twice those.  The gate gradient crosses the whole bf16 layer forward
    and backward (<= 12 roundings of 2^-9, as in test_moe_kernels_gpu):
    2^-5 of its largest magnitude."""
    assert "moe" not in F._TORCH_FB
    hip = layer_run()
    out = str(tmp_path / "torch_branch.pt")
    env = {**os.environ, "HETU_AMD_TORCH_FALLBACK": "moe",
           "PYTHONPATH": REPO + os.pathsep + os.environ.get("PYTHONPATH", "")}
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); "
            "import hetu_amd.ops.functional as F; "
            "assert 'moe' in F._TORCH_FB; "
            "import test_moe_gate_gpu as T; T.layer_run(%r)"
            % (REPO, os.path.join(REPO, "tests"), out))
    p = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout + p.stderr
    ref = torch.load(out)
    assert torch.equal(hip["cnt"], ref["cnt"])
    assert float(ref["cnt"].sum()) == LN * LK
    err = float((hip["y"] - ref["y"]).abs().max())
    assert err <= (3 + 2 * LK) * 2.0 ** -8 * float(ref["eo"].abs().max()), err
    ptol = (LN + 8) * 2.0 ** -24
    assert abs(float(hip["aux"]) - float(ref["aux"])) \
        <= 2 * ptol * float(ref["aux"])
    assert abs(float(hip["z"]) - float(ref["z"])) \
        <= 2e-5 * float(ref["z"])
    gmax = float(ref["dgate"].abs().max())
    assert gmax > 0
    err = float((hip["dgate"] - ref["dgate"]).abs().max())
    assert err <= 2.0 ** -5 * gmax, (err, gmax)
