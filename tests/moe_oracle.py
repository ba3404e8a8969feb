"""Brute-force MoE routing / row-movement oracle shared by the MoE kernel
tests.  Plain Python loops over tokens and rounds, fp64 rows; the oracle
functions use no hetu_amd code, no top-k and no prefix sums.  build_moe_graph (at the end)
is the MoEMLP test graph both files run.

Policy (the one hetu_amd.ops.functional.moe_route documents): per token the
K largest probabilities in descending order, ties to the lower expert index;
rounds k = 0..K-1 in order; inside a round tokens queue at their expert in
increasing token index behind everything earlier rounds queued there; a
choice is kept iff its queue position is < C and then owns slot e*C + q.
"""
import torch


def make_probs(N, E, seed, skew=0.0, empty_expert=None, second_to=None):
    """Rows are random permutations of the E distinct values (j+1)/2048
    (exact in fp32; exact in bf16/fp16 for E <= 128).  `skew`: that share
    of the tokens gets the top value moved to expert 0.  `empty_expert`:
    this expert always holds the smallest value, so with K < E no token
    ever selects it.  `second_to`: every token whose top value is elsewhere
    gets its second largest value moved to this expert, so round 1 crowds
    it."""
    g = torch.Generator().manual_seed(seed)
    vals = (torch.arange(E, dtype=torch.float64) + 1) / 2048
    probs = torch.empty(N, E, dtype=torch.float64)
    for t in range(N):
        probs[t] = vals[torch.randperm(E, generator=g)]
    if skew > 0:
        pick = torch.rand(N, generator=g) < skew
        for t in range(N):
            if pick[t]:
                j = int(probs[t].argmax())
                probs[t, j], probs[t, 0] = probs[t, 0].item(), \
                    probs[t, j].item()
    if empty_expert is not None:
        for t in range(N):
            j = int(probs[t].argmin())
            probs[t, j], probs[t, empty_expert] = \
                probs[t, empty_expert].item(), probs[t, j].item()
    if second_to is not None:
        for t in range(N):
            first, j = probs[t].topk(2).indices.tolist()
            if first != second_to:
                probs[t, j], probs[t, second_to] = \
                    probs[t, second_to].item(), probs[t, j].item()
    return probs.float()


def route(probs, C, K):
    """-> pos [E, C] int64, slot_of [N, K] int64, idx [N, K] int64,
    wk [N, K] fp32 (the stored value of the selected probability)."""
    N, E = probs.shape
    pf = probs.float()
    rows = pf.tolist()
    idx = torch.empty(N, K, dtype=torch.int64)
    for t in range(N):
        order = sorted(range(E), key=lambda e: (-rows[t][e], e))
        for k in range(K):
            idx[t, k] = order[k]
    pos = torch.full((E, C), -1, dtype=torch.int64)
    slot_of = torch.full((N, K), -1, dtype=torch.int64)
    wk = torch.zeros(N, K, dtype=torch.float32)
    queued = [0] * E
    for k in range(K):
        for t in range(N):
            e = int(idx[t, k])
            q = queued[e]
            queued[e] += 1
            if q < C:
                pos[e, q] = t
                slot_of[t, k] = e * C + q
                wk[t, k] = pf[t, e]
    return pos, slot_of, idx, wk


def dispatch_rows(x, pos):
    S = pos.numel()
    out = torch.zeros(S, x.shape[1], dtype=torch.float64)
    pf = pos.reshape(-1).tolist()
    for s in range(S):
        if pf[s] >= 0:
            out[s] = x[pf[s]].double()
    return out


def dispatch_rows_bwd(gsend, slot_of):
    N, K = slot_of.shape
    out = torch.zeros(N, gsend.shape[1], dtype=torch.float64)
    sl = slot_of.tolist()
    for t in range(N):
        for k in range(K):
            if sl[t][k] >= 0:
                out[t] += gsend[sl[t][k]].double()
    return out


def gate_bwd(g_w, slot_of, E, C):
    N, K = slot_of.shape
    out = torch.zeros(N, E, dtype=torch.float64)
    sl = slot_of.tolist()
    for t in range(N):
        for k in range(K):
            if sl[t][k] >= 0:
                out[t, sl[t][k] // C] = float(g_w[t, k])
    return out


def combine_rows(recv, wk, slot_of):
    N, K = slot_of.shape
    out = torch.zeros(N, recv.shape[1], dtype=torch.float64)
    sl = slot_of.tolist()
    for t in range(N):
        for k in range(K):
            if sl[t][k] >= 0:
                out[t] += float(wk[t, k]) * recv[sl[t][k]].double()
    return out


def combine_rows_bwd(gy, recv, wk, pos, slot_of):
    N, K = slot_of.shape
    d_recv = torch.zeros(recv.shape, dtype=torch.float64)
    dwk = torch.zeros(N, K, dtype=torch.float64)
    sl = slot_of.tolist()
    for t in range(N):
        for k in range(K):
            s = sl[t][k]
            if s >= 0:
                d_recv[s] = gy[t].double() * float(wk[t, k])
                dwk[t, k] = float((gy[t].double() * recv[s].double()).sum())
    return d_recv, dwk


def build_moe_graph(N, H, Fh, E, K, cap, dtype=torch.float32, seed=0):
    """MoEMLP + mse loss with gradients wrt x, gate, w1, w2.  Returns
    (graph, x, tgt, fetches) with fetches = [y, loss, dx, dgate, dw1, dw2,
    pos, slot_of, wk, probs]."""
    from hetu_amd.graph.graph import DefineAndRunGraph, push_graph, pop_graph
    from hetu_amd.graph.ops import api as ht
    from hetu_amd.nn.moe import MoEMLP
    torch.manual_seed(seed)
    g = DefineAndRunGraph("moe_kernels")
    push_graph(g)
    try:
        x = ht.placeholder((N, H), dtype=dtype, name="x")
        tgt = ht.placeholder((N, H), dtype=dtype, name="tgt")
        moe = MoEMLP(H, Fh, E, k=K, capacity_factor=cap, dtype=dtype)
        y = moe(x)
        loss = ht.mse_loss(y, tgt)
        grads = ht.gradients(loss, [x, moe.gate, moe.w1, moe.w2])
    finally:
        pop_graph()
    _, wk, pos, slot_of = y.producer.inputs
    probs = pos.producer.inputs[1]
    return g, x, tgt, [y, loss] + list(grads) + [pos, slot_of, wk, probs]
