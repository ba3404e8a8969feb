"""Packed-varlen Llama on the GPU: head_dim 128 in bf16, so the step runs the
HIP path end to end (table-row gather for the per-token RoPE tables, packed
rope, single-kernel varlen attention forward and backward)."""
import pytest
import torch
import torch.nn.functional as TF

import hetu_amd.ops.functional as F
from hetu_amd.data.bucket import packed_feed
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.models.llama import LlamaConfig, build_llama_train_graph

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(n_layer=2, n_head=2, n_kv_head=2, hidden=256,
                  ffn_hidden=512, vocab=256, max_seq=128)
B, S, MAX_SEGMENTS = 2, 64, 4
T = B * S


def _build(dtype, device):
    torch.manual_seed(0)
    g, h = build_llama_train_graph(CFG, micro_batch=B, seq_len=S,
                                   dtype=dtype, lr=1e-3, packed=True,
                                   max_segments=MAX_SEGMENTS)
    return g, h, prepare_run_context(g, device, use_comm=False)


def _feed(h, f, device, tokens=None):
    ids = f["input_ids"] if tokens is None else tokens
    return {h["input_ids"]: ids.reshape(B, S).to(device),
            h["labels"]: f["labels"].to(device),
            h["cu_seqlens"]: f["cu_seqlens"].to(device),
            h["position_ids"]: f["position_ids"].to(device)}


def test_packed_llama_step_on_gpu():
    assert hasattr(F.ext(), "flash_attn_varlen_bwd")
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(5)
    tokens = torch.randint(1, CFG.vocab, (T,), generator=gen)
    # segments 40 | 60 and an uncovered tail of 28 that packed_feed closes
    f = packed_feed(tokens, torch.tensor([0, 40, 100], dtype=torch.int32),
                    MAX_SEGMENTS, seq_lens=[40, 60])
    assert f["cu_seqlens"].tolist() == [0, 40, 100, 128, 128]

    gc, hc, ctxc = _build(torch.float32, torch.device("cpu"))
    (ref,) = gc.run([hc["loss"]], _feed(hc, f, torch.device("cpu")),
                    ctx=ctxc)

    g, h, ctx = _build(torch.bfloat16, dev)
    loss, logits = g.run([h["loss"], h["logits"]], _feed(h, f, dev), ctx=ctx)
    print(f"packed loss: gpu bf16 {float(loss):.5f} cpu fp32 {float(ref):.5f}")
    # freshly initialised logits are |x| < 1, so their bf16 rounding is
    # <= 2^-9 and moves a token's CE by <= 2 * 2^-9 = 4e-3; allow a few such
    # roundings through the two layers
    assert abs(float(loss) - float(ref)) < 3e-2

    # isolation: other tokens in segment 0 leave segments 1.. untouched.
    # Same inputs through deterministic row-wise kernels give the same
    # numbers; a leak would move these losses by ~1e-1.
    lab = f["labels"].to(dev)
    base = TF.cross_entropy(logits.float(), lab, ignore_index=-100,
                            reduction="none")
    changed = tokens.clone()
    changed[:40] = (changed[:40] + 17) % (CFG.vocab - 1) + 1
    (logits2,) = g.run([h["logits"]], _feed(h, f, dev, changed), ctx=ctx)
    other = TF.cross_entropy(logits2.float(), lab, ignore_index=-100,
                             reduction="none")
    assert (base[:40] - other[:40]).abs().max().item() > 1e-2
    assert (base[40:] - other[40:]).abs().max().item() <= 1e-3

    # one optimizer step through the varlen backward: everything finite
    g.run([h["loss"], h["train_op"]], _feed(h, f, dev), ctx=ctx)
    (loss2,) = g.run([h["loss"]], _feed(h, f, dev), ctx=ctx)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.get_data().float()).all()
               for p in g.parameters)
    assert float(loss2) == float(loss2) and float(loss2) < float(loss)
