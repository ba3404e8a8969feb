#!/usr/bin/env python3
"""LlamaGenerator.generate() end to end: milliseconds per decode step with
decode_impl="hip" (ops/hip/attention_decode.hip) against decode_impl="torch"
(the slice / repeat / fp32 composition), same random weights, bf16.

Both generators run in this process, alternating; a decode step's time is
(generate(new) - generate(1)) / (new - 1) with a host clock around device
synchronises, so prefill and the first sample drop out; the first of
`--rounds` rounds is warm-up and not reported.  Prints one JSON line per
(batch, prompt) row: min / median / max over the rounds.  Needs a GPU.

    python scripts/bench_generate.py [--layers 4] [--new 64] [--rounds 4]
                                     [--rows 1x2048,16x2048,16x3900]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402

from hetu_amd.engine.generator import LlamaGenerator  # noqa: E402
from hetu_amd.models.llama import LlamaConfig  # noqa: E402


def llama_state(cfg, ffn, seed=0):
    g = torch.Generator().manual_seed(seed)
    hid, dh = cfg.hidden, cfg.hidden // cfg.n_head

    def w(*shape):
        return torch.randn(*shape, generator=g) * 0.05
    state = {"wte.weight": w(cfg.vocab, hid), "lnf.weight": torch.ones(hid),
             "lm_head.weight": w(cfg.vocab, hid)}
    for i in range(cfg.n_layer):
        state[f"l{i}.ln1.weight"] = torch.ones(hid)
        state[f"l{i}.ln2.weight"] = torch.ones(hid)
        state[f"l{i}.attn.wqkv.weight"] = \
            w((cfg.n_head + 2 * cfg.n_kv_head) * dh, hid)
        state[f"l{i}.attn.wo.weight"] = w(hid, hid)
        state[f"l{i}.mlp.w_in.weight"] = w(2 * ffn, hid)
        state[f"l{i}.mlp.w_out.weight"] = w(hid, ffn)
    return state


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--rows", default="1x2048,16x2048,16x3900",
                    help="batch x prompt length")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_generate: needs a GPU")
    dev = torch.device("cuda", 0)
    # Llama-7B width with 8 KV heads
    cfg = LlamaConfig(n_layer=args.layers, n_head=32, n_kv_head=8,
                      hidden=4096, ffn_hidden=11008, vocab=32000,
                      max_seq=4096)
    state = llama_state(cfg, 11008)
    gens = {impl: LlamaGenerator(cfg, state, device=dev,
                                 dtype=torch.bfloat16, decode_impl=impl)
            for impl in ("hip", "torch")}
    for row in args.rows.split(","):
        B, S = (int(x) for x in row.split("x"))
        ids = torch.randint(0, cfg.vocab, (B, S),
                            generator=torch.Generator().manual_seed(0))
        times = {impl: [] for impl in gens}
        outs = {}
        for r in range(args.rounds):
            for impl, g in gens.items():
                t1, _ = timed(lambda: g.generate(ids, max_new_tokens=1))
                tn, outs[impl] = timed(
                    lambda: g.generate(ids, max_new_tokens=args.new))
                if r:
                    times[impl].append((tn - t1) / (args.new - 1) * 1e3)
        res = {"bench": "generate", "layers": cfg.n_layer, "H": 32, "Hkv": 8,
               "D": 128, "B": B, "prompt": S, "new": args.new,
               "tokens_equal_frac": round(
                   (outs["hip"] == outs["torch"]).float().mean().item(), 4)}
        for impl, ts in times.items():
            res[impl + "_ms_per_decode_step"] = {
                "median": round(statistics.median(ts), 3),
                "min": round(min(ts), 3), "max": round(max(ts), 3)}
        res["torch_over_hip"] = round(
            statistics.median(times["torch"])
            / statistics.median(times["hip"]), 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
