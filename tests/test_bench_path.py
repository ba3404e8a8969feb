"""Multi-process CPU smoke of the DRIVER'S bench contract (bench.py):
the exact code path the round-end scaling run takes, at world_size 2 over
gloo — auto strategy broadcast, dp branch, pipeline branch."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run_ws2(extra, port):
    procs = []
    env0 = {**os.environ, "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": str(port), "GLOO_SOCKET_IFNAME": "lo"}
    for r in range(2):
        env = dict(env0, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(
            [sys.executable, BENCH, "--allow-cpu", "--model", "gpt-tiny",
             "--gpus", "2", "--steps", "2", "--warmup", "1",
             "--seq-len", "32", "--global-batch", "8"] + extra,
            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
            text=True))
    line = None
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=600)
        ok = p.returncode in (0, -6)
        assert ok, f"rank {r}: rc={p.returncode}\n{out}\n{err}"
        for ln in out.splitlines():
            if ln.startswith("{"):
                line = json.loads(ln)
    return line


def test_bench_ws2_auto():
    out = _run_ws2([], 29661)
    assert out is not None
    assert out["n_gpus"] == 2
    assert out["value"] > 0
    assert out["config"]["parallelism"].startswith("dp")
    assert out["loss"] is not None


def test_bench_ws2_pp2():
    out = _run_ws2(["--parallel", "pp2_dp1", "--micro-batch", "1"], 29671)
    assert out is not None
    assert out["config"]["parallelism"] == "dp1_pp2"
    assert out["value"] > 0


def _run_ws1(extra):
    p = subprocess.run(
        [sys.executable, BENCH, "--allow-cpu", "--model", "gpt-tiny",
         "--gpus", "1", "--steps", "3", "--warmup", "2",
         "--seq-len", "32", "--global-batch", "4"] + extra,
        capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"{p.stdout}\n{p.stderr}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed step's loss and parameter
    sample as float32 .npy, identical from run to run; --steps sets the
    timed step count and --full keeps the result line's schema."""
    import numpy as np
    outs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        line = _run_ws1(["--dump-outputs", str(d)] + extra)
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert k in line
        files = sorted(f.name for f in d.iterdir())
        assert files == ["loss.npy", "params_sample.npy"]
        arrs = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert np.float32(line["loss"]) == arrs["loss.npy"][0]
        assert np.isfinite(arrs["params_sample.npy"]).all()
        outs.append(arrs)
    for f in outs[0]:
        np.testing.assert_array_equal(outs[0][f], outs[1][f])


def test_pooled_draws_match_serial_build():
    """bench.py builds the model through init.build_with_pooled_draws:
    every weight must be bit-identical to the plain serial build."""
    import torch
    from hetu_amd.models.gpt import GPT_CONFIGS, build_gpt_train_graph
    from hetu_amd.nn import init

    def build():
        return build_gpt_train_graph(GPT_CONFIGS["gpt-tiny"], micro_batch=2,
                                     seq_len=32, dtype=torch.bfloat16)

    serial_normal = init.normal
    _, h_ref = build()
    g, h = init.build_with_pooled_draws(build, workers=3,
                                        device=torch.device("cpu"))
    assert init.normal is serial_normal
    ref, got = h_ref["model"].state_dict(), h["model"].state_dict()
    assert list(ref) == list(got) and len(ref) > 4
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


def test_bench_ws8_auto():
    """8-rank gloo smoke of the exact round-end N=8 invocation shape:
    auto search at ws=8, strategy broadcast to all ranks, whole-job
    aggregation."""
    procs = []
    env0 = {**os.environ, "MASTER_ADDR": "127.0.0.1",
            "MASTER_PORT": "29671", "GLOO_SOCKET_IFNAME": "lo"}
    for r in range(8):
        env = dict(env0, RANK=str(r), WORLD_SIZE="8", LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(
            [sys.executable, BENCH, "--allow-cpu", "--model", "gpt-tiny",
             "--gpus", "8", "--steps", "2", "--warmup", "1",
             "--seq-len", "32", "--global-batch", "16"],
            env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
            text=True))
    line = None
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=900)
        ok = p.returncode in (0, -6)
        assert ok, f"rank {r}: rc={p.returncode}\n{out}\n{err}"
        for ln in out.splitlines():
            if ln.startswith("{"):
                line = json.loads(ln)
    assert line is not None and line["n_gpus"] == 8
    assert line["value"] > 0
