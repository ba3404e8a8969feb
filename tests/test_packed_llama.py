"""Packed-varlen Llama training (build_llama_train_graph(packed=True)) on
CPU in fp32: equivalence to training each sequence alone, isolation between
segments, and the data helper that produces the packed feed."""
import torch
import torch.nn.functional as TF

from hetu_amd.data.bucket import Bucket, packed_feed
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import pop_graph, push_graph
from hetu_amd.models.llama import LlamaConfig, build_llama_train_graph

CFG = LlamaConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=128,
                  ffn_hidden=256, vocab=211, max_seq=64)
SEGS = [24, 40]
T = 64
MAX_SEGMENTS = 4


def _build(micro_batch, seq_len, **kw):
    """Graph + handles + per-parameter gradient tensors; same seed, so
    every build starts from the same weights."""
    torch.manual_seed(0)
    g, h = build_llama_train_graph(CFG, micro_batch=micro_batch,
                                   seq_len=seq_len, dtype=torch.float32,
                                   lr=1e-3, **kw)
    push_graph(g)
    try:
        grads = g.gradients([h["loss"]], list(g.parameters))
    finally:
        pop_graph()
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    return g, h, grads, ctx


def _tokens():
    gen = torch.Generator().manual_seed(11)
    return torch.randint(1, CFG.vocab, (T,), generator=gen)


def _packed_feed(h, tokens):
    cu = torch.tensor([0, SEGS[0], T], dtype=torch.int32)
    f = packed_feed(tokens, cu, MAX_SEGMENTS, seq_lens=SEGS)
    return f, {h["input_ids"]: f["input_ids"].reshape(2, 32),
               h["labels"]: f["labels"],
               h["cu_seqlens"]: f["cu_seqlens"],
               h["position_ids"]: f["position_ids"]}


def _per_token(logits, labels):
    return TF.cross_entropy(logits.float(), labels, ignore_index=-100,
                            reduction="none")


def test_packed_matches_unpacked_training():
    tokens = _tokens()
    # packed: [2, 32] input = one row of 64 tokens, segments 24 | 40
    g, h, grads, ctx = _build(2, 32, packed=True, max_segments=MAX_SEGMENTS)
    assert h["cu_seqlens"].shape == (MAX_SEGMENTS + 1,)
    assert h["position_ids"].shape == (T,)
    f, feed = _packed_feed(h, tokens)
    assert f["cu_seqlens"].tolist() == [0, 24, 64, 64, 64]
    names = [p.name for p in g.parameters]
    p0 = [p.get_data().clone() for p in g.parameters]
    out = g.run([h["loss"]] + grads, feed, ctx=ctx)
    packed_loss, packed_grads = float(out[0]), out[1:]

    # unpacked: each sequence alone through a (1, len) graph
    loss_sum = 0.0
    want = [torch.zeros_like(x) for x in packed_grads]
    off = 0
    for n in SEGS:
        gu, hu, gradu, ctxu = _build(1, n)
        assert [p.name for p in gu.parameters] == names
        for a, b in zip(gu.parameters, p0):
            assert torch.equal(a.get_data(), b), a.name
        seq = tokens[off:off + n]
        labels = torch.cat([seq[1:], torch.tensor([-100])])
        assert torch.equal(labels, f["labels"][off:off + n])
        o = gu.run([hu["loss"]] + gradu,
                   {hu["input_ids"]: seq.reshape(1, n), hu["labels"]: labels},
                   ctx=ctxu)
        # mean over n tokens -> per-token loss sum is loss * n; the packed
        # mean is over T, so the unpacked gradient weighs n / T
        loss_sum += float(o[0]) * n
        for w, gg in zip(want, o[1:]):
            w += gg * (n / T)
        off += n

    print(f"packed_loss*T={packed_loss * T:.6f} unpacked sum={loss_sum:.6f}")
    assert abs(packed_loss * T - loss_sum) <= 1e-4 * abs(loss_sum)
    # fp32 round-off is ~1e-6 of a tensor's scale; 1e-4 of the largest
    # reference entry is the issue's bound
    for name, a, b in zip(names, packed_grads, want):
        err = (a - b).abs().max().item()
        ref = b.abs().max().item()
        print(f"{name}: max abs err {err:.3e} (ref max {ref:.3e})")
        assert ref > 0, name
        assert err <= 1e-4 * ref, (name, err, ref)


def test_segments_are_isolated():
    tokens = _tokens()
    g, h, _, ctx = _build(2, 32, packed=True, max_segments=MAX_SEGMENTS)
    f, feed = _packed_feed(h, tokens)
    (logits,) = g.run([h["logits"]], feed, ctx=ctx)
    base = _per_token(logits, f["labels"])
    changed = tokens.clone()
    changed[:SEGS[0]] = (changed[:SEGS[0]] + 17) % (CFG.vocab - 1) + 1
    feed2 = dict(feed)
    feed2[h["input_ids"]] = changed.reshape(2, 32)      # labels unchanged
    (logits2,) = g.run([h["logits"]], feed2, ctx=ctx)
    other = _per_token(logits2, f["labels"])
    s = SEGS[0]
    assert (base[:s] - other[:s]).abs().max().item() > 1e-3   # it did change
    assert (base[s:] - other[s:]).abs().max().item() <= 1e-6, \
        "segment 1 saw the tokens of segment 0"


def test_packed_feed_from_bucket():
    bucket = Bucket(max_seqlen=64, alignment=16)
    gen = torch.Generator().manual_seed(3)
    lens = [10, 20, 7]
    for n in lens:
        bucket.add(torch.randint(1, 200, (n,), generator=gen))
    tokens, cus = bucket.pack_data()
    assert tokens.shape == (1, 64)
    row = tokens[0]
    f = packed_feed(row, cus[0], MAX_SEGMENTS)
    cu = f["cu_seqlens"]
    assert cu.dtype == torch.int32 and cu.shape == (MAX_SEGMENTS + 1,)
    cu = cu.tolist()
    assert cu[0] == 0 and cu[-1] == 64
    assert all(a <= b for a, b in zip(cu[:-1], cu[1:]))
    pos = f["position_ids"]
    assert pos.dtype == torch.int64 and pos.shape == (64,)
    labels = f["labels"]
    assert labels.dtype == torch.int64 and labels.shape == (64,)
    assert torch.equal(f["input_ids"], row)
    real = sorted(lens, reverse=True)        # pack_data places longest first
    covered = 0
    for i, (s0, s1) in enumerate(zip(cu[:-1], cu[1:])):
        assert pos[s0:s1].tolist() == list(range(s1 - s0))
        n = real[i] if i < len(real) else 0
        for t in range(s0, s1):
            if t - s0 < n - 1:
                assert labels[t] == row[t + 1]
            else:       # the segment's last token, or padding
                assert labels[t] == -100
        covered += s1 - s0
    assert covered == 64
    # the real lengths, when known, give the same feed
    f2 = packed_feed(row, cus[0], MAX_SEGMENTS, seq_lens=real)
    for k in f:
        assert torch.equal(f[k], f2[k]), k


def test_packed_feed_closes_uncovered_tail():
    bucket = Bucket(max_seqlen=64, alignment=16)
    bucket.add(torch.arange(1, 21))          # 20 tokens -> aligned 32
    tokens, cus = bucket.pack_data()
    assert cus[0].tolist() == [0, 32]
    f = packed_feed(tokens[0], cus[0], MAX_SEGMENTS)
    assert f["cu_seqlens"].tolist() == [0, 32, 64, 64, 64]
    assert f["position_ids"][32:].tolist() == list(range(32))
    assert (f["labels"][19:] == -100).all()
    assert torch.equal(f["labels"][:19], tokens[0][1:20])
