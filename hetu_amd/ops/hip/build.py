"""Build the _hetu_hip extension with hipcc for gfx950 (in-tree .so).

Direct hipcc invocation (no hipify, no CUDA shims): every source is native
HIP/CDNA4. Cross-compiles without a GPU; the built .so travels with the
repo snapshot to the GPU box.
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))

SOURCES = [
    "norms.hip",
    "reduce.hip",
    "activations.hip",
    "swiglu.hip",
    "rope.hip",
    "softmax.hip",
    "ce.hip",
    "dropout.hip",
    "embedding.hip",
    "adam.hip",
    "gemm.hip",
    "gemm_wgrad.hip",
    "transpose.hip",
    "attention.hip",
    "attention_v2.hip",
    "attention_bwd_v3.hip",
    "attention_bwd_v2.hip",
    "attention_decode.hip",
    "quant.hip",
    "moe.hip",
    "ltgemm.cpp",
    "galvatron_dp.cpp",
    "embed_cache.cpp",
    "dataloader.cpp",
    "bindings.cpp",
]


def _torch_paths():
    import torch
    troot = os.path.dirname(torch.__file__)
    inc = [
        os.path.join(troot, "include"),
        os.path.join(troot, "include", "torch", "csrc", "api", "include"),
    ]
    lib = os.path.join(troot, "lib")
    abi = "1" if torch._C._GLIBCXX_USE_CXX11_ABI else "0"
    return inc, lib, abi


def _usable_cpus() -> int:
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def build(verbose: bool = True) -> str:
    inc, libdir, abi = _torch_paths()
    py_inc = sysconfig.get_paths()["include"]
    out = os.path.join(HERE, "_hetu_hip.so")
    srcs = [os.path.join(HERE, s) for s in SOURCES
            if os.path.exists(os.path.join(HERE, s))]
    objs = []
    os.makedirs(os.path.join(HERE, ".build"), exist_ok=True)
    common_flags = [
        "-O3", "-std=c++17", "-fPIC",
        "--offload-arch=gfx950",
        "-DTORCH_EXTENSION_NAME=_hetu_hip",
        "-DTORCH_API_INCLUDE_EXTENSION_H",
        f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
        "-D__HIP_PLATFORM_AMD__=1",
        "-DUSE_ROCM=1",
        "-fno-gpu-rdc",
        "-Wno-deprecated-declarations",
        "-Wno-unused-result",
        # a non-void function falling off its end produced a silent
        # GPU-side hang (see profiles/r02_capture_replay_bug.md era):
        # make it a hard error
        "-Werror=return-type",
    ] + [f"-I{p}" for p in inc] + [f"-I{py_inc}", f"-I{HERE}"]
    # every source may include any header of this directory
    newest_h = max(os.path.getmtime(os.path.join(HERE, f))
                   for f in os.listdir(HERE) if f.endswith(".h"))
    stale = []
    for src in srcs:
        base = os.path.basename(src).rsplit(".", 1)[0]
        obj = os.path.join(HERE, ".build", base + ".o")
        objs.append(obj)
        # skip if up to date
        if (os.path.exists(obj)
                and os.path.getmtime(obj) > os.path.getmtime(src)
                and os.path.getmtime(obj) > newest_h):
            continue
        stale.append((src, obj))

    def compile_one(job):
        src, obj = job
        if verbose:
            print("[hetu_amd build]", os.path.basename(src), flush=True)
        subprocess.run(["hipcc", "-c", src, "-o", obj] + common_flags,
                       check=True)

    # the translation units are independent; one hipcc per core (MAX_JOBS
    # overrides, as for torch extensions) instead of 22 in a row
    jobs = int(os.environ.get("MAX_JOBS", 0)) or min(16, _usable_cpus())
    with ThreadPoolExecutor(max(1, jobs)) as pool:
        list(pool.map(compile_one, stale))
    link = ["hipcc", "-shared", "-fPIC", "-o", out] + objs + [
        f"-L{libdir}", "-ltorch", "-ltorch_cpu", "-lc10",
        "-ltorch_python", "-lamdhip64", "-lhipblaslt",
        f"-Wl,-rpath,{libdir}",
    ]
    hiplibs = [l for l in ("torch_hip", "c10_hip")
               if os.path.exists(os.path.join(libdir, f"lib{l}.so"))]
    for l in hiplibs:
        link.insert(-1, f"-l{l}")
    if verbose:
        print("[hetu_amd build] linking _hetu_hip.so")
    subprocess.run(link, check=True)
    return out


if __name__ == "__main__":
    build()
