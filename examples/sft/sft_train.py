#!/usr/bin/env python3
"""SFT driver (reference examples/sft): prompt/answer pairs with
prompt-masked loss, byte tokenizer, greedy packing stats, Llama graph.

Run: python examples/sft/sft_train.py          (1 rank, tiny model, CPU ok)
     python examples/sft/sft_train.py --packed (packed-varlen training)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))
import torch  # noqa: E402

from hetu_amd.data.bucket import Bucket, packed_feed  # noqa: E402
from hetu_amd.data.tokenizers import ByteTokenizer  # noqa: E402
from hetu_amd.engine.sft_trainer import SFTTrainer, build_sft_example  # noqa
from hetu_amd.models.llama import LlamaConfig, build_llama_train_graph  # noqa
from hetu_amd.parallel.comm import comm_backend  # noqa: E402

PAIRS = [
    ("What is 2+2? ", "4."),
    ("Capital of France? ", "Paris."),
    ("Color of the sky? ", "Blue."),
    ("Opposite of hot? ", "Cold."),
] * 4


def train_packed(cfg, tok, S, dtype, device, comm, max_segments=8):
    """Packed path: every bin of Bucket.pack_data() is one [1, S] row of
    several sequences; packed_feed turns it into the four feed tensors of
    the packed graph (ht.varlen_attention, per-segment RoPE positions).
    Labels are plain next-token here (no prompt masking)."""
    g, h = build_llama_train_graph(cfg, 1, S, dtype=dtype, lr=5e-4,
                                   packed=True, max_segments=max_segments)
    trainer = SFTTrainer(g, h, device)
    bucket = Bucket(max_seqlen=S, alignment=16)
    for p, a in PAIRS:
        bucket.add(torch.tensor(tok.encode(p + a, bos=True, eos=True)))
    rows, cus = bucket.pack_data()
    print(f"packing: {len(PAIRS)} seqs -> {rows.shape[0]} bins "
          f"({sum(len(c) - 1 for c in cus)} segments)")
    feeds = [packed_feed(rows[b], cus[b], max_segments)
             for b in range(rows.shape[0])]
    for step in range(12):
        f = feeds[step % len(feeds)]
        loss = trainer.step({
            h["input_ids"]: f["input_ids"].reshape(1, S).to(device),
            h["labels"]: f["labels"].to(device),
            h["cu_seqlens"]: f["cu_seqlens"].to(device),
            h["position_ids"]: f["position_ids"].to(device)})
        if comm.rank == 0 and step % 3 == 0:
            print(f"step {step} loss {float(loss):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packed", action="store_true",
                    help="train on packed bins (varlen attention)")
    args = ap.parse_args()
    comm = comm_backend()
    device = comm.device
    tok = ByteTokenizer()
    S = 64
    cfg = LlamaConfig(n_layer=2, n_head=4, n_kv_head=4, hidden=128,
                      ffn_hidden=256, vocab=tok.vocab_size, max_seq=S)
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    if args.packed:
        return train_packed(cfg, tok, S, dtype, device, comm)
    B = 4
    g, h = build_llama_train_graph(cfg, B, S, dtype=dtype, lr=5e-4)
    trainer = SFTTrainer(g, h, device)

    # packing stats for the curious (the padded path below is the simple
    # default; --packed trains on these bins through ht.varlen_attention)
    bucket = Bucket(max_seqlen=S, alignment=16)
    for p, a in PAIRS:
        bucket.add(torch.tensor(tok.encode(p + a, bos=True, eos=True)))
    packed, cus = bucket.pack_data()
    print(f"packing: {len(PAIRS)} seqs -> {packed.shape[0]} bins "
          f"({sum(len(c) - 1 for c in cus)} segments)")

    exs = [build_sft_example(tok.encode(p, bos=True), tok.encode(a, eos=True),
                             S) for p, a in PAIRS]
    for step in range(12):
        batch = [exs[(step * B + i) % len(exs)] for i in range(B)]
        x = torch.stack([b[0] for b in batch]).to(device)
        y = torch.stack([b[1] for b in batch]).to(device)
        loss = trainer.sft_step(x, y)
        if comm.rank == 0 and step % 3 == 0:
            print(f"step {step} loss {float(loss):.4f}")


if __name__ == "__main__":
    main()
