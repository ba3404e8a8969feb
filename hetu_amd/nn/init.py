"""Initializers (reference hetu/graph/init/initializer.h: constant/uniform/
normal/xavier/he/lecun).  Deterministic per-parameter: the seed is derived
from a global seed and the parameter name, so every rank materializes the
same global weight and slices its own shard."""
from __future__ import annotations

import hashlib
import math

import torch

_GLOBAL_SEED = [1234]


def set_seed(seed: int):
    _GLOBAL_SEED[0] = seed


def _gen(name: str) -> torch.Generator:
    h = hashlib.sha256(f"{_GLOBAL_SEED[0]}:{name}".encode()).digest()
    g = torch.Generator()
    g.manual_seed(int.from_bytes(h[:8], "little") & 0x7FFFFFFFFFFFFFFF)
    return g


def normal(shape, std=0.02, mean=0.0, dtype=torch.float32, name="w"):
    return (torch.randn(*shape, generator=_gen(name)) * std + mean).to(dtype)


def build_with_pooled_draws(build, workers=None, device=None):
    """Return `build()` with its normal() draws computed on a thread pool
    (and, if `device` is given, moved there as each one completes, so the
    host-to-device copies overlap the remaining draws).

    Every draw has its own generator (seeded by global seed + parameter
    name), so draws are independent of each other, but a single generator
    stream is serial: building a 7B model spends ~90% of its time inside
    torch.randn.  A dry run of `build` records the requested draws (handing
    out uninitialized tensors), the pool computes them with the unmodified
    normal(), and the real run of `build` receives those tensors — bit-
    identical to drawing them one by one.  `build` must be repeatable; a
    draw the dry run did not see is computed in place as usual."""
    global normal
    from concurrent.futures import ThreadPoolExecutor
    real = normal
    wanted = []

    def key_of(shape, std, mean, dtype, name):
        return (tuple(shape), std, mean, dtype, name, _GLOBAL_SEED[0])

    def record(shape, std=0.02, mean=0.0, dtype=torch.float32, name="w"):
        wanted.append(key_of(shape, std, mean, dtype, name))
        return torch.empty(*shape, dtype=dtype)

    normal = record
    try:
        build()
    finally:
        normal = real
    workers = workers or max(1, min(16, torch.get_num_threads()))

    def draw(key):
        t = real(*key[:5])
        return t if device is None else t.to(device)

    # one intra-op thread per worker (the setting is per calling thread):
    # the pool already fills the cores, nested teams only fight over them;
    # largest draws first so no long one is left to run alone at the end
    todo = sorted(dict.fromkeys(wanted), key=lambda k: -math.prod(k[0]))
    with ThreadPoolExecutor(workers, initializer=torch.set_num_threads,
                            initargs=(1,)) as pool:
        drawn = {k: pool.submit(draw, k) for k in todo}
    drawn = {k: f.result() for k, f in drawn.items()}

    def replay(shape, std=0.02, mean=0.0, dtype=torch.float32, name="w"):
        t = drawn.pop(key_of(shape, std, mean, dtype, name), None)
        return t if t is not None else real(shape, std, mean, dtype, name)

    normal = replay
    try:
        return build()
    finally:
        normal = real


def uniform(shape, a=-0.1, b=0.1, dtype=torch.float32, name="w"):
    return (torch.rand(*shape, generator=_gen(name)) * (b - a) + a).to(dtype)


def constant(shape, value=0.0, dtype=torch.float32):
    return torch.full(shape, float(value)).to(dtype)


def zeros(shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def ones(shape, dtype=torch.float32):
    return torch.ones(*shape, dtype=dtype)


def xavier_uniform(shape, gain=1.0, dtype=torch.float32, name="w"):
    fan_out, fan_in = shape[0], shape[-1]
    a = gain * math.sqrt(6.0 / (fan_in + fan_out))
    return uniform(shape, -a, a, dtype, name)


def xavier_normal(shape, gain=1.0, dtype=torch.float32, name="w"):
    fan_out, fan_in = shape[0], shape[-1]
    std = gain * math.sqrt(2.0 / (fan_in + fan_out))
    return normal(shape, std, 0.0, dtype, name)


def he_normal(shape, dtype=torch.float32, name="w"):
    fan_in = shape[-1]
    return normal(shape, math.sqrt(2.0 / fan_in), 0.0, dtype, name)


def lecun_normal(shape, dtype=torch.float32, name="w"):
    fan_in = shape[-1]
    return normal(shape, math.sqrt(1.0 / fan_in), 0.0, dtype, name)
