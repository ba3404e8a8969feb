"""Inference/serving path: KV-cached autoregressive generation.

Reference context: Hetu's user-facing model stack is training-first; for
serving parity this engine runs the same Llama/GPT weights with a
fixed-capacity KV cache.  MI355X-native: prefill goes through the
hand-written flash-attention kernel (one pass over the prompt).  A decode
step (one new token) appends its K/V row to the cache and then calls
F.flash_attn_decode on the whole layer cache and the current length: on
the GPU (bf16, head dim 64 or 128) that is the split-KV HIP kernel, which
reads each cached K and V row once per KV head, in place, with the length
taken from an int32 device tensor that generate() advances in place; on
the CPU, and for other dtypes or head dims, it is fp32 torch math on the
visible slice of the cache.  All norms / RoPE / SwiGLU hit the same HIP
kernels as training via ops.functional.

With kv_layout="paged" the cache is a page pool behind a block table and
generate() takes ragged prompts.  prefill="sequence" prefills them one at a
time through the dense path; prefill="packed" runs them as one packed forward
over the pages (F.flash_attn_prefill_paged: on the GPU, for bf16 and head dim
64 or 128, the HIP prefill kernel), optionally in rounds of prefill_chunk
tokens that attend the context already cached.  kv_dtype="fp8"
makes the pages e4m3 codes with one fp32 scale per cached row (prefill=
"sequence" only: the prefill attends the bf16 rows it just computed).

generate(speculative=k) on the paged cache decodes greedily with up to k
drafted tokens per sequence and step: the chunk [last accepted token] + drafts
of every live sequence goes through one packed forward (the split-KV
verification kernel, F.flash_attn_prefill_paged(impl="split"), where it is
eligible), the longest draft prefix that equals the model's own argmax chain
is accepted and one more token comes for free.  The output is plain greedy
decoding's; a step that accepts drafts reads the cache once for several tokens.

Weights load from a hetu_amd checkpoint dir (utils/checkpoint format,
incl. checkpoints converted from HF with utils/hf_convert) or from an
in-memory state dict.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from ..models.llama import LlamaConfig, rope_tables
from ..ops import functional as F


def sample_next(logits: torch.Tensor, temperature: float = 0.0,
                top_k: int = 0, top_p: float = 0.0,
                gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """Next-token sampling: greedy (temperature<=0), temperature,
    top-k, and nucleus (top-p) filters compose.  CPU multinomial with an
    explicit generator keeps runs reproducible across devices."""
    if temperature <= 0:
        return logits.argmax(-1)
    lg = logits.float() / temperature
    if top_k:
        kth = lg.topk(top_k, dim=-1).values[:, -1:]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    if top_p and 0.0 < top_p < 1.0:
        srt, idx = lg.sort(dim=-1, descending=True)
        cum = torch.softmax(srt, dim=-1).cumsum(dim=-1)
        # keep the smallest prefix with cumulative prob >= top_p (the
        # first token always survives)
        drop_sorted = cum - torch.softmax(srt, dim=-1) >= top_p
        drop = drop_sorted.scatter(-1, idx, drop_sorted)
        lg = lg.masked_fill(drop, float("-inf"))
    probs = torch.softmax(lg, dim=-1).cpu()
    return torch.multinomial(probs, 1, generator=gen).squeeze(-1) \
        .to(logits.device)


def prompt_lookup_draft(tokens: torch.Tensor, k: int) -> torch.Tensor:
    """Drafts without a draft model: up to k tokens that followed the most
    recent earlier occurrence of the sequence's last two tokens; nothing if
    they never occurred before."""
    n = tokens.numel()
    if n < 3:
        return tokens[:0]
    at = ((tokens[:-2] == tokens[-2]) & (tokens[1:-1] == tokens[-1])) \
        .nonzero()
    if not at.numel():
        return tokens[:0]
    i = int(at[-1]) + 2
    return tokens[i:i + k]


class LlamaKVCache:
    def __init__(self, cfg: LlamaConfig, batch: int, max_len: int,
                 device, dtype, kv_dtype: Optional[str] = None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', got "
                             f"{kv_dtype!r}")
        dh = cfg.hidden // cfg.n_head
        shape = (cfg.n_layer, batch, cfg.n_kv_head, max_len, dh)
        self.kv_dtype = kv_dtype
        if kv_dtype == "fp8":
            # e4m3 codes and one fp32 scale per cached row (token x KV
            # head): value = float(code) * scale[row]
            self.k = torch.zeros(shape, device=device,
                                 dtype=torch.float8_e4m3fn)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.zeros(shape[:-1], device=device,
                                       dtype=torch.float32)
            self.v_scale = torch.zeros_like(self.k_scale)
        else:
            self.k = torch.zeros(shape, device=device, dtype=dtype)
            self.v = torch.zeros(shape, device=device, dtype=dtype)
        self.len = 0
        # rows of the cache a decode step attends, the new token's included
        # (pos0 + 1), for the GPU decode kernel.  generate() advances it in
        # place; whoever steps _forward by hand keeps it in step
        # (kv_len.fill_(pos0 + 1)).
        self.kv_len = torch.zeros(batch, device=device, dtype=torch.int32)


class PagedKVCache:
    """A page pool per layer behind one block table.

    k, v [n_layer, P, Hkv, PS, dh]; block_table int32 [B, MP]: key j of
    sequence b is row j % PS of page block_table[b, j // PS]; kv_len int32
    [B].  Sequence b owns ceil(capacity[b] / PS) pages, so P is the sum of
    the sequences' own needs, not B x the longest.  Pages are handed out
    round-robin over the sequences (physical order differs from logical
    order); table entries a sequence does not own hold P, which the kernels
    treat as a page of masked keys.  kv_dtype="fp8": k, v hold e4m3 codes and
    k_scale, v_scale [n_layer, P, Hkv, PS] one fp32 scale per cached row."""

    def __init__(self, cfg: LlamaConfig, capacity, page_size: int, device,
                 dtype, kv_dtype: Optional[str] = None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', got "
                             f"{kv_dtype!r}")
        if page_size not in F._PAGE_SIZES:
            raise ValueError(f"page_size must be one of {F._PAGE_SIZES}, "
                             f"got {page_size}")
        dh = cfg.hidden // cfg.n_head
        need = [-(-int(n) // page_size) for n in capacity]
        self.page_size = page_size
        self.num_pages = sum(need)
        mp = max(need, default=0)
        table = [[self.num_pages] * mp for _ in need]
        nxt = 0
        for j in range(mp):
            for b, n in enumerate(need):
                if j < n:
                    table[b][j] = nxt
                    nxt += 1
        self.block_table = torch.tensor(table, dtype=torch.int32) \
            .view(len(need), mp).to(device)
        shape = (cfg.n_layer, self.num_pages, cfg.n_kv_head, page_size, dh)
        self.kv_dtype = kv_dtype
        self.k_scale = self.v_scale = None
        if kv_dtype == "fp8":
            self.k = torch.zeros(shape, device=device,
                                 dtype=torch.float8_e4m3fn)
            self.v = torch.zeros_like(self.k)
            self.k_scale = torch.zeros(shape[:-1], device=device,
                                       dtype=torch.float32)
            self.v_scale = torch.zeros_like(self.k_scale)
        else:
            self.k = torch.zeros(shape, device=device, dtype=dtype)
            self.v = torch.zeros(shape, device=device, dtype=dtype)
        self.kv_len = torch.zeros(len(need), device=device, dtype=torch.int32)
        self.cu_q = None               # set by packed(): a packed forward

    def packed(self, cu_q, max_q: int, pos,
               split: bool = False) -> "PagedKVCache":
        """The same cache for one packed forward of ragged chunks: cu_q int32
        [B + 1] bounds the chunks in the packed rows, max_q is the longest,
        pos [T] each row's position; kv_len already holds the lengths after
        the chunks.  split: short chunks behind long contexts, for the
        split-KV verification kernel."""
        one = object.__new__(PagedKVCache)
        one.__dict__.update(self.__dict__)
        one.cu_q, one.max_q, one.pos, one.split = cu_q, max_q, pos, split
        return one

    def row(self, b: int) -> "PagedKVCache":
        """Sequence b alone (B = 1) on the same pools, for its prefill."""
        one = object.__new__(PagedKVCache)
        one.__dict__.update(self.__dict__)
        one.block_table = self.block_table[b:b + 1]
        one.kv_len = self.kv_len[b:b + 1]
        return one


class LlamaGenerator:
    """KV-cached Llama generation.  With kv_layout="paged", prefill="packed"
    and bf16 weights on the GPU every attention call at head dim 64 or 128 is
    a HIP kernel: the packed append, the prefill kernel over the pages, the
    split-KV verification kernel of generate(speculative=k) and the paged
    decode kernels."""

    def __init__(self, cfg: LlamaConfig, state: Dict[str, torch.Tensor],
                 device: Optional[torch.device] = None,
                 dtype: torch.dtype = torch.float32,
                 decode_impl: Optional[str] = None,
                 kv_dtype: Optional[str] = None,
                 kv_layout: str = "dense", page_size: int = 64,
                 prefill: str = "sequence",
                 prefill_chunk: Optional[int] = None):
        if kv_layout not in ("dense", "paged"):
            raise ValueError(f"kv_layout must be 'dense' or 'paged', got "
                             f"{kv_layout!r}")
        if prefill not in ("sequence", "packed"):
            raise ValueError(f"prefill must be 'sequence' or 'packed', got "
                             f"{prefill!r}")
        if prefill != "sequence" and kv_layout != "paged":
            raise ValueError("prefill='packed' needs kv_layout='paged'")
        if prefill_chunk is not None and (prefill != "packed"
                                          or prefill_chunk < 1):
            raise ValueError("prefill_chunk needs prefill='packed' and a "
                             f"positive size, got {prefill_chunk!r}")
        # "packed": all prompts in one forward over the paged cache
        # (F.flash_attn_prefill_paged), in rounds of at most prefill_chunk
        # tokens per sequence
        self.prefill = prefill
        self.prefill_chunk = prefill_chunk
        if prefill == "packed" and kv_dtype == "fp8":
            raise ValueError("prefill='packed' with kv_dtype='fp8': an fp8 "
                             "prefill kernel over the pages does not exist "
                             "yet; use prefill='sequence'")
        # "paged": generate() keeps the cache in a PagedKVCache of page_size
        # rows per page and also takes ragged prompts
        self.kv_layout = kv_layout
        self.page_size = page_size
        self.cfg = cfg
        # forwarded to F.flash_attn_decode: None (auto), "torch" or "hip"
        self.decode_impl = decode_impl
        # None: the cache holds `dtype`; "fp8": e4m3 with per-row scales
        self.kv_dtype = kv_dtype
        self.device = device or torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.dtype = dtype
        self.w = {k: v.to(self.device, dtype) for k, v in state.items()}
        dh = cfg.hidden // cfg.n_head
        cos, sin = rope_tables(cfg, cfg.max_seq, torch.float32)
        self.cos = cos.to(self.device)
        self.sin = sin.to(self.device)
        self.scale = 1.0 / math.sqrt(dh)

    @classmethod
    def from_checkpoint(cls, cfg: LlamaConfig, path: str, **kw
                        ) -> "LlamaGenerator":
        import json
        import os

        from safetensors import safe_open
        idx = os.path.join(path, "model.safetensors.index.json")
        if os.path.exists(idx):
            with open(idx) as fh:
                index = json.load(fh)["weight_map"]
        else:
            # single-shard HF convention: plain model.safetensors, no index
            index = {"": "model.safetensors"}
        state = {}
        for fn in sorted(set(index.values())):
            with safe_open(os.path.join(path, fn), framework="pt") as f:
                for k in f.keys():
                    state[k] = f.get_tensor(k)
        return cls(cfg, state, **kw)

    # ---- building blocks -------------------------------------------------
    def _attn_paged(self, x, layer, cache: PagedKVCache):
        """S > 1: the prefill of one sequence (cache = its row(), still
        empty) on the rows it just computed; S == 1: a decode step of all
        sequences; a cache from packed(): ragged chunks of all sequences in
        one row of x, over the pages.  cache.kv_len is the length after the
        append in all three, and append and attention read it on the
        device."""
        cfg = self.cfg
        B, S, _ = x.shape
        H, Hkv = cfg.n_head, cfg.n_kv_head
        dh = cfg.hidden // H
        qkv = x @ self.w[f"l{layer}.attn.wqkv.weight"].t()
        q, k, v = qkv.split([H * dh, Hkv * dh, Hkv * dh], dim=-1)
        q = q.view(B, S, H, dh)
        k = k.view(B, S, Hkv, dh)
        v = v.view(B, S, Hkv, dh)
        kp, vp = cache.k[layer], cache.v[layer]
        wo = self.w[f"l{layer}.attn.wo.weight"]
        # fp8 pools: the scale pools go with the append (`app`) and the decode
        # call (`fp8`); rows that are not bf16 take the torch append
        fp8, app = {}, {}
        if cache.kv_dtype == "fp8":
            fp8 = dict(k_scale=cache.k_scale[layer],
                       v_scale=cache.v_scale[layer])
            app = dict(fp8, impl=None if k.dtype == torch.bfloat16
                       else "torch")
        if cache.cu_q is not None:
            # packed chunks (B == 1, S = all rows): one RoPE row per token
            # from its own position, then append and attention over the
            # pages, the cached context included
            cos, sin = self.cos[cache.pos], self.sin[cache.pos]
            q = F.rope_fwd(q[0], cos, sin)
            k = F.rope_fwd(k[0], cos, sin)
            F.kv_cache_append_paged(k, v[0], kp, vp, cache.block_table,
                                    cache.kv_len, cu_q=cache.cu_q,
                                    max_q=cache.max_q)
            # verification chunks take the split-KV kernel where it is
            # eligible (and HETU_AMD_TORCH_FALLBACK=fa does not ask for torch:
            # an explicit impl would bypass that switch), else today's path
            split = cache.split and "fa" not in F._TORCH_FB and \
                F._prefill_paged_ineligible(q, kp, vp, cache.block_table,
                                            cache.cu_q, cache.kv_len) is None
            o, _ = F.flash_attn_prefill_paged(
                q, kp, vp, cache.block_table, cache.cu_q, cache.kv_len,
                self.scale, max_q=cache.max_q,
                impl="split" if split else None)
            return o.reshape(1, S, H * dh) @ wo.t()
        if S == 1:
            # one RoPE row per sequence, gathered from its own position; the
            # batch takes the place of the packed form's sequence dim
            pos = (cache.kv_len - 1).long()
            cos, sin = self.cos[pos], self.sin[pos]
            q = F.rope_fwd(q[:, 0], cos, sin)
            k = F.rope_fwd(k[:, 0], cos, sin).unsqueeze(1)
            F.kv_cache_append_paged(k, v, kp, vp, cache.block_table,
                                    cache.kv_len, **app)
            o, _ = F.flash_attn_decode(
                q, kp, vp, cache.kv_len, self.scale, impl=self.decode_impl,
                block_table=cache.block_table, **fp8)
            return o.reshape(B, 1, H * dh) @ wo.t()
        q = F.rope_fwd(q, self.cos[:S], self.sin[:S])
        k = F.rope_fwd(k, self.cos[:S], self.sin[:S])
        F.kv_cache_append_paged(k, v, kp, vp, cache.block_table,
                                cache.kv_len, **app)
        return self._prefill_attn(q, k.permute(0, 2, 1, 3),
                                  v.permute(0, 2, 1, 3), 0) @ wo.t()

    def _attn(self, x, layer, cache: LlamaKVCache, pos0: int):
        if isinstance(cache, PagedKVCache):
            return self._attn_paged(x, layer, cache)
        cfg = self.cfg
        B, S, _ = x.shape
        H, Hkv = cfg.n_head, cfg.n_kv_head
        dh = cfg.hidden // H
        qkv = x @ self.w[f"l{layer}.attn.wqkv.weight"].t()
        q, k, v = qkv.split([H * dh, Hkv * dh, Hkv * dh], dim=-1)
        q = q.view(B, S, H, dh)
        k = k.view(B, S, Hkv, dh)
        cos = self.cos[pos0:pos0 + S]
        sin = self.sin[pos0:pos0 + S]
        q = F.rope_fwd(q, cos, sin)
        k = F.rope_fwd(k, cos, sin)
        v = v.view(B, S, Hkv, dh)
        ks = vs = None
        if cache.kv_dtype == "fp8":
            # quantize into rows cache.kv_len - S + s: the device-side
            # length, so append + decode attention hold no Python position
            ks, vs = cache.k_scale[layer], cache.v_scale[layer]
            F.kv_cache_append_fp8(
                k, v, cache.k[layer], cache.v[layer], ks, vs, cache.kv_len,
                impl=None if k.dtype == torch.bfloat16 else "torch")
            if S == 1:
                kk = vv = None
            elif pos0 == 0:
                # prefill attends the rows it just computed
                kk, vv = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
            else:
                # cold path: the visible slice, dequantized with torch
                n = pos0 + S
                kk = (cache.k[layer][:, :, :n].float()
                      * ks[:, :, :n, None]).to(x.dtype)
                vv = (cache.v[layer][:, :, :n].float()
                      * vs[:, :, :n, None]).to(x.dtype)
        else:
            # append to cache
            cache.k[layer][:, :, pos0:pos0 + S] = k.permute(0, 2, 1, 3)
            cache.v[layer][:, :, pos0:pos0 + S] = v.permute(0, 2, 1, 3)
            kk = cache.k[layer][:, :, :pos0 + S]
            vv = cache.v[layer][:, :, :pos0 + S]
        if S == 1:
            # the whole layer cache and the length: nothing is sliced, cast
            # or repeated here
            kc, vc = cache.k[layer], cache.v[layer]
            on_hip = F.flash_attn_decode_on_hip(q[:, 0], kc, vc,
                                                impl=self.decode_impl,
                                                k_scale=ks, v_scale=vs)
            o, _ = F.flash_attn_decode(
                q[:, 0], kc, vc, cache.kv_len if on_hip else pos0 + 1,
                self.scale, impl=self.decode_impl, k_scale=ks, v_scale=vs)
            return o.reshape(B, 1, H * dh) \
                @ self.w[f"l{layer}.attn.wo.weight"].t()
        return self._prefill_attn(q, kk, vv, pos0) \
            @ self.w[f"l{layer}.attn.wo.weight"].t()

    def _prefill_attn(self, q, kk, vv, pos0):
        """Causal attention of q [B, S, H, dh] at positions pos0 .. over kk,
        vv [B, Hkv, pos0 + S, dh] -> [B, S, H * dh]."""
        B, S, H, dh = q.shape
        Hkv = kk.shape[1]
        qt = q.permute(0, 2, 1, 3)
        if qt.is_cuda and dh == 128 and qt.dtype == torch.bfloat16:
            o, _ = F.flash_attn_fwd(qt.contiguous(), kk.contiguous(),
                                    vv.contiguous(), True, self.scale)
        else:
            rep = H // Hkv
            kr = kk.repeat_interleave(rep, dim=1) if rep > 1 else kk
            vr = vv.repeat_interleave(rep, dim=1) if rep > 1 else vv
            mask = None
            if S > 1:
                Skv = pos0 + S
                mask = torch.ones(S, Skv, dtype=torch.bool,
                                  device=q.device).tril(diagonal=Skv - S)
            scores = (qt.float() @ kr.float().transpose(-1, -2)) \
                * self.scale
            if mask is not None:
                scores = scores.masked_fill(~mask, float("-inf"))
            p = torch.softmax(scores, dim=-1)
            o = (p @ vr.float()).to(q.dtype)
        return o.permute(0, 2, 1, 3).reshape(B, S, H * dh)

    def _block(self, x, layer, cache, pos0):
        cfg = self.cfg
        h = F.rmsnorm_fwd(x, self.w[f"l{layer}.ln1.weight"],
                          cfg.rms_eps)[0]
        x = x + self._attn(h, layer, cache, pos0)
        h = F.rmsnorm_fwd(x, self.w[f"l{layer}.ln2.weight"],
                          cfg.rms_eps)[0]
        h = h @ self.w[f"l{layer}.mlp.w_in.weight"].t()
        h = F.swiglu_fwd(h)
        x = x + h @ self.w[f"l{layer}.mlp.w_out.weight"].t()
        return x

    def _hidden(self, ids, cache, pos0):
        x = self.w["wte.weight"][ids]
        for layer in range(self.cfg.n_layer):
            x = self._block(x, layer, cache, pos0)
        return F.rmsnorm_fwd(x, self.w["lnf.weight"], self.cfg.rms_eps)[0]

    def _forward(self, ids, cache, pos0):
        x = self._hidden(ids, cache, pos0)
        return x[:, -1] @ self.w["lm_head.weight"].t()   # last-token logits

    def _packed_hidden(self, chunks, starts, cache: PagedKVCache,
                       split: bool = False):
        """One packed forward over the paged cache: chunks[b] (1-D ids, may be
        empty) stands at positions starts[b] .. of sequence b, behind the
        context already cached; kv_len is set to the lengths after the
        chunks.  -> (the final-norm rows [T, hidden], cu: chunk b is rows
        cu[b] .. cu[b + 1])."""
        ns = [int(c.numel()) for c in chunks]
        cu = [0]
        for n in ns:
            cu.append(cu[-1] + n)
        cache.kv_len.copy_(torch.tensor([s + n for s, n in zip(starts, ns)],
                                        dtype=torch.int32))
        pos = torch.cat([torch.arange(s, s + n) for s, n in zip(starts, ns)])
        view = cache.packed(
            torch.tensor(cu, dtype=torch.int32).to(self.device), max(ns),
            pos.to(self.device), split)
        return self._hidden(torch.cat(chunks).unsqueeze(0), view, None)[0], cu

    def _prefill_packed(self, prompts, lens, cache: PagedKVCache):
        """All prompts through packed forwards over the paged cache, in
        rounds of at most prefill_chunk tokens per sequence (one round
        without it) -> last-token logits [B, vocab].  A finished sequence
        contributes zero rows to later rounds."""
        B = len(prompts)
        step = self.prefill_chunk or max(lens, default=0)
        logits = [None] * B
        for done in range(0, max(lens, default=0), max(step, 1)):
            lo = [min(done, n) for n in lens]
            hi = [min(done + step, n) for n in lens]
            x, cu = self._packed_hidden(
                [p[a:e] for p, a, e in zip(prompts, lo, hi)], lo, cache)
            for b in range(B):
                if lo[b] < hi[b] == lens[b]:       # held its last token
                    logits[b] = x[cu[b + 1] - 1]
        return torch.stack(logits) @ self.w["lm_head.weight"].t()

    # ---- public API ------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 32,
                 temperature: float = 0.0, top_k: int = 0,
                 top_p: float = 0.0, eos_id: Optional[int] = None,
                 seed: int = 0, speculative: Optional[int] = None,
                 draft=None) -> torch.Tensor:
        """input_ids [B, S] -> [B, S + new]; temperature 0 = greedy.  With
        kv_layout="paged" also a list of 1-D prompts of unequal length -> a
        list of 1-D outputs, each cut after its first eos_id.

        speculative=k: greedy decoding that verifies up to k drafted tokens
        per sequence and step (kv_layout="paged", temperature 0, bf16 / fp32
        pages); the tokens are those of speculative=None.  draft(tokens, k)
        -> up to k proposed next tokens of the 1-D sequence so far (tensor or
        list, may be empty); default: prompt lookup (prompt_lookup_draft)."""
        if speculative is not None:
            if int(speculative) < 1:
                raise ValueError("speculative must be None or a positive "
                                 f"draft length, got {speculative!r}")
            if self.kv_layout != "paged":
                raise ValueError("speculative decoding needs kv_layout="
                                 f"'paged', got {self.kv_layout!r}")
            if temperature > 0:
                raise ValueError("speculative decoding is greedy: "
                                 f"temperature must be 0, got {temperature}")
            if self.kv_dtype is not None:
                raise ValueError("speculative decoding needs bf16 / fp32 "
                                 f"pages, got kv_dtype={self.kv_dtype!r}")
            return self._generate_speculative(
                input_ids, max_new_tokens, eos_id, int(speculative),
                draft or prompt_lookup_draft)
        if draft is not None:
            raise ValueError("draft needs speculative=k")
        if self.kv_layout == "paged":
            return self._generate_paged(input_ids, max_new_tokens,
                                        temperature, top_k, top_p, eos_id,
                                        seed)
        ids = input_ids.to(self.device)
        B, S = ids.shape
        cache = LlamaKVCache(self.cfg, B, S + max_new_tokens, self.device,
                             self.dtype, kv_dtype=self.kv_dtype)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        cache.kv_len.fill_(S)
        logits = self._forward(ids, cache, 0)
        pos = S
        out = [ids]
        alive = torch.ones(B, dtype=torch.bool)
        for _ in range(max_new_tokens):
            nxt = sample_next(logits, temperature, top_k, top_p, gen)
            out.append(nxt.unsqueeze(1))
            if eos_id is not None:
                alive &= (nxt.cpu() != eos_id)
                if not alive.any():
                    break
            cache.kv_len.add_(1)
            logits = self._forward(nxt.unsqueeze(1), cache, pos)
            pos += 1
        return torch.cat(out, dim=1)


    def _prefill_paged(self, input_ids, extra):
        """The prompts into a fresh paged cache with room for `extra` more
        tokens each -> (prompts, lens, cache, last-token logits)."""
        prompts = [p.to(self.device).view(-1) for p in input_ids]
        lens = [int(p.numel()) for p in prompts]
        cache = PagedKVCache(self.cfg, [n + extra for n in lens],
                             self.page_size, self.device, self.dtype,
                             kv_dtype=self.kv_dtype)
        cache.kv_len.copy_(torch.tensor(lens, dtype=torch.int32))
        if self.prefill == "packed":
            logits = self._prefill_packed(prompts, lens, cache)
        else:
            # one sequence at a time through the dense prefill path
            logits = torch.cat([self._forward(p.unsqueeze(0), cache.row(b), 0)
                                for b, p in enumerate(prompts)])
        return prompts, lens, cache, logits

    def _generate_speculative(self, input_ids, max_new_tokens, eos_id, k,
                              draft):
        ragged = not isinstance(input_ids, torch.Tensor)
        # a chunk may write k rejected rows past the last token that counts
        prompts, lens, cache, logits = self._prefill_paged(
            input_ids, max_new_tokens + k)
        B = len(prompts)
        if max_new_tokens < 1:
            return prompts if ragged else torch.stack(prompts)
        # new[b]: the tokens generated so far; all but the last are cached
        new = [[t] for t in logits.argmax(-1).tolist()]
        lm_head = self.w["lm_head.weight"]

        def want():
            # as _generate_paged: a ragged sequence ends at its eos, a
            # rectangular batch runs until every row has met one
            end = [n.index(eos_id) + 1 if eos_id is not None and eos_id in n
                   else max_new_tokens for n in new]
            return end if ragged else [max(end)] * B
        while any(alive := [len(n) < w for n, w in zip(new, want())]):
            chunks = []
            for b in range(B):
                d = []
                room = min(k, max_new_tokens - len(new[b]) - 1)
                if alive[b] and room > 0:
                    seq = torch.cat([prompts[b], torch.tensor(
                        new[b], device=self.device)])
                    d = torch.as_tensor(draft(seq, room)).view(-1)[:room] \
                        .tolist()
                chunks.append(torch.tensor(
                    (new[b][-1:] + d) if alive[b] else [], dtype=torch.long,
                    device=self.device))
            starts = [n + len(t) - 1 for n, t in zip(lens, new)]
            x, cu = self._packed_hidden(chunks, starts, cache, split=True)
            pred = (x @ lm_head.t()).argmax(-1).tolist()
            for b in range(B):
                if not alive[b]:
                    continue
                d, p = chunks[b].tolist()[1:], pred[cu[b]:cu[b + 1]]
                a = 0                  # the accepted drafts, then p[a] free
                while a < len(d) and d[a] == p[a]:
                    a += 1
                new[b] += d[:a] + [p[a]]
        out = [torch.cat([p, torch.tensor(n[:w], device=self.device)])
               for p, n, w in zip(prompts, new, want())]
        return out if ragged else torch.stack(out)

    def _generate_paged(self, input_ids, max_new_tokens, temperature, top_k,
                        top_p, eos_id, seed):
        ragged = not isinstance(input_ids, torch.Tensor)
        prompts, lens, cache, logits = self._prefill_paged(input_ids,
                                                           max_new_tokens)
        B = len(prompts)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        new = []
        alive = torch.ones(B, dtype=torch.bool)
        for _ in range(max_new_tokens):
            nxt = sample_next(logits, temperature, top_k, top_p, gen)
            new.append(nxt.unsqueeze(1))
            if eos_id is not None:
                alive &= (nxt.cpu() != eos_id)
                if not alive.any():
                    break
            # a finished sequence keeps stepping (the batch stays whole);
            # its tokens past the eos are cut below
            cache.kv_len.add_(1)
            logits = self._forward(nxt.unsqueeze(1), cache, None)
        new = torch.cat(new, dim=1) if new else \
            torch.empty(B, 0, dtype=torch.long, device=self.device)
        if not ragged:
            return torch.cat([torch.stack(prompts), new], dim=1)
        out = []
        for b, p in enumerate(prompts):
            row = new[b]
            if eos_id is not None:
                hit = (row == eos_id).nonzero()
                if hit.numel():
                    row = row[:int(hit[0]) + 1]
            out.append(torch.cat([p, row]))
        return out


class GPTGenerator:
    """KV-cached generation for the GPT family (learned positions,
    LayerNorm, biased linears, gelu MLP)."""

    def __init__(self, cfg, state: Dict[str, torch.Tensor],
                 device: Optional[torch.device] = None,
                 dtype: torch.dtype = torch.float32,
                 decode_impl: Optional[str] = None):
        self.cfg = cfg
        # forwarded to F.flash_attn_decode: None (auto), "torch" or "hip"
        self.decode_impl = decode_impl
        self.device = device or torch.device(
            "cuda" if torch.cuda.is_available() else "cpu")
        self.dtype = dtype
        self.w = {k: v.to(self.device, dtype) for k, v in state.items()}
        self.scale = 1.0 / math.sqrt(cfg.hidden // cfg.n_head)

    def _lin(self, x, name):
        y = x @ self.w[f"{name}.weight"].t()
        b = self.w.get(f"{name}.bias")
        return y + b if b is not None else y

    def _attn(self, x, layer, kcache, vcache, pos0, kv_len=None):
        cfg = self.cfg
        B, S, _ = x.shape
        H = cfg.n_head
        dh = cfg.hidden // H
        qkv = self._lin(x, f"h{layer}.attn.wqkv")
        q, k, v = qkv.chunk(3, -1)
        q1 = q.view(B, S, H, dh)[:, 0]          # decode: a view into qkv
        q = q.view(B, S, H, dh).permute(0, 2, 1, 3)
        kcache[layer][:, :, pos0:pos0 + S] = \
            k.view(B, S, H, dh).permute(0, 2, 1, 3)
        vcache[layer][:, :, pos0:pos0 + S] = \
            v.view(B, S, H, dh).permute(0, 2, 1, 3)
        if S == 1:
            on_hip = kv_len is not None and F.flash_attn_decode_on_hip(
                q1, kcache[layer], vcache[layer], impl=self.decode_impl)
            o, _ = F.flash_attn_decode(
                q1, kcache[layer], vcache[layer],
                kv_len if on_hip else pos0 + 1, self.scale,
                impl=self.decode_impl)
            return self._lin(o.reshape(B, 1, H * dh), f"h{layer}.attn.wo")
        kk = kcache[layer][:, :, :pos0 + S]
        vv = vcache[layer][:, :, :pos0 + S]
        if q.is_cuda and dh == 128 and q.dtype == torch.bfloat16:
            o, _ = F.flash_attn_fwd(q.contiguous(), kk.contiguous(),
                                    vv.contiguous(), True, self.scale)
        else:
            scores = (q.float() @ kk.float().transpose(-1, -2)) * self.scale
            if S > 1:
                Skv = pos0 + S
                mask = torch.ones(S, Skv, dtype=torch.bool,
                                  device=x.device).tril(diagonal=Skv - S)
                scores = scores.masked_fill(~mask, float("-inf"))
            o = (torch.softmax(scores, -1) @ vv.float()).to(x.dtype)
        o = o.permute(0, 2, 1, 3).reshape(B, S, H * dh)
        return self._lin(o, f"h{layer}.attn.wo")

    def _forward(self, ids, kcache, vcache, pos0, kv_len=None):
        """kv_len: int32 device tensor [B] holding pos0 + 1 for a decode
        step on the GPU (generate() advances one in place); without it the
        length is the Python int."""
        cfg = self.cfg
        S = ids.shape[1]
        pos = torch.arange(pos0, pos0 + S, device=self.device)
        x = self.w["wte.weight"][ids] + self.w["wpe.weight"][pos]
        for i in range(cfg.n_layer):
            h = F.layernorm_fwd(x, self.w[f"h{i}.ln1.weight"],
                                self.w[f"h{i}.ln1.bias"], 1e-5)[0]
            x = x + self._attn(h, i, kcache, vcache, pos0, kv_len)
            h = F.layernorm_fwd(x, self.w[f"h{i}.ln2.weight"],
                                self.w[f"h{i}.ln2.bias"], 1e-5)[0]
            h = F.gelu_fwd(self._lin(h, f"h{i}.mlp.wfc"))
            x = x + self._lin(h, f"h{i}.mlp.wproj")
        x = F.layernorm_fwd(x, self.w["lnf.weight"], self.w["lnf.bias"],
                            1e-5)[0]
        return x[:, -1] @ self.w["lm_head.weight"].t()

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, max_new_tokens: int = 32,
                 temperature: float = 0.0, top_k: int = 0,
                 top_p: float = 0.0, seed: int = 0) -> torch.Tensor:
        cfg = self.cfg
        ids = input_ids.to(self.device)
        B, S = ids.shape
        dh = cfg.hidden // cfg.n_head
        L = S + max_new_tokens
        kc = torch.zeros(cfg.n_layer, B, cfg.n_head, L, dh,
                         device=self.device, dtype=self.dtype)
        vc = torch.zeros_like(kc)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        kv_len = torch.full((B,), S, dtype=torch.int32, device=self.device)
        logits = self._forward(ids, kc, vc, 0, kv_len)
        out = [ids]
        pos = S
        for _ in range(max_new_tokens):
            nxt = sample_next(logits, temperature, top_k, top_p, gen)
            out.append(nxt.unsqueeze(1))
            kv_len.add_(1)
            logits = self._forward(nxt.unsqueeze(1), kc, vc, pos, kv_len)
            pos += 1
        return torch.cat(out, dim=1)
