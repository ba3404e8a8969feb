"""CPU tests of the speculative-decoding path: the argument errors of
F.flash_attn_prefill_paged(impl="split") and generate(speculative=k), and
speculative generation against plain greedy decoding (fp32, torch branches).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_attn_oracle as DO  # noqa: E402
import prefill_paged_oracle as PO  # noqa: E402

import hetu_amd.ops.functional as F  # noqa: E402
from hetu_amd.engine.generator import LlamaGenerator  # noqa: E402
from hetu_amd.models.llama import LlamaConfig  # noqa: E402

CFG = LlamaConfig(n_layer=2, n_head=4, n_kv_head=2, hidden=64, ffn_hidden=64,
                  vocab=97, max_seq=128)
NEW = 12


def generator(monkeypatch=None, **kw):
    kw.setdefault("kv_layout", "paged")
    gen = LlamaGenerator(CFG, DO.llama_state(CFG, 64),
                         device=torch.device("cpu"), dtype=torch.float32,
                         page_size=32, **kw)
    gen.steps = 0
    if monkeypatch is not None:          # count the forwards
        real = gen._hidden

        def counted(*a, **k):
            gen.steps += 1
            return real(*a, **k)
        monkeypatch.setattr(gen, "_hidden", counted)
    return gen


def test_argument_errors():
    c = PO.build(4, 2, 32)
    args = (c["q"], c["k_pool"], c["v_pool"], c["table"], c["cu_q"],
            c["kv_len"])
    with pytest.raises(ValueError, match="q is not on the GPU"):
        F.flash_attn_prefill_paged(*args, impl="split")
    with pytest.raises(ValueError, match="num_splits"):
        F.flash_attn_prefill_paged(*args, impl="torch", num_splits=2)
    ids = torch.zeros(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="kv_layout"):
        generator(kv_layout="dense").generate(ids, 4, speculative=4)
    with pytest.raises(ValueError, match="temperature"):
        generator().generate(ids, 4, speculative=4, temperature=0.7)


def test_speculative_equals_greedy(monkeypatch):
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, CFG.vocab, (n,), generator=g)
               for n in (3, 40, 70)]
    gen = generator(monkeypatch)
    plain = gen.generate(prompts, NEW)
    plain_steps, gen.steps = gen.steps, 0

    def draft(tokens, k):
        """The known continuation: exact for sequence 0, wrong at the second
        proposed token for sequence 1, nothing for sequence 2."""
        n = tokens.numel()
        b = [p.numel() <= n + NEW and torch.equal(p[:n], tokens)
             for p in plain].index(True)
        d = plain[b][n:n + k].clone()
        if b == 1 and d.numel() > 1:
            d[1] = (d[1] + 1) % CFG.vocab
        return d if b < 2 else []
    spec = gen.generate(prompts, NEW, speculative=4, draft=draft)
    assert all(torch.equal(a, b) for a, b in zip(plain, spec))
    # three prefills, then 11 single-token steps for the draftless sequence
    assert gen.steps - len(prompts) < NEW and gen.steps < plain_steps


def test_prompt_lookup_draft_equals_greedy(monkeypatch):
    gen = generator(monkeypatch)
    prompt = [torch.tensor([5, 9, 2, 7, 1, 3] * 5)]
    plain = gen.generate(prompt, NEW)
    gen.steps = 0
    spec = gen.generate(prompt, NEW, speculative=4)
    assert torch.equal(plain[0], spec[0])
    assert gen.steps <= NEW              # the prefill and at most 11 steps
