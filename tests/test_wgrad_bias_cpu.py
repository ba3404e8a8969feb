"""F.linear_wgrad_bias on CPU, the two-output grad op a biased Linear
builds, and RowParallelLinear's bias placement."""
import pytest
import torch

import hetu_amd.ops.functional as F
from hetu_amd.engine.runner import prepare_run_context
from hetu_amd.graph.graph import DefineAndRunGraph, pop_graph, push_graph
from hetu_amd.graph.ops import api as ht
from hetu_amd.graph.ops import basics as B
from hetu_amd.nn.parallel import ParallelSpec, RowParallelLinear


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("impl", [None, "auto", "blas"])
def test_equals_matmul_and_column_sum(dtype, impl):
    g = torch.Generator().manual_seed(11)
    gy = torch.randn(96, 40, generator=g).to(dtype)
    x = torch.randn(96, 24, generator=g).to(dtype)
    dw, db = F.linear_wgrad_bias(gy, x, impl=impl)
    assert dw.shape == (40, 24) and db.shape == (40,)
    assert db.dtype == dtype
    assert torch.equal(dw, torch.matmul(gy.t(), x))
    assert torch.equal(db, gy.float().sum(0).to(dtype))


def test_flattens_leading_dims():
    g = torch.Generator().manual_seed(12)
    gy = torch.randn(4, 16, 40, generator=g)
    x = torch.randn(4, 16, 24, generator=g)
    dw, db = F.linear_wgrad_bias(gy, x)
    assert torch.equal(dw, torch.matmul(gy.reshape(64, 40).t(),
                                        x.reshape(64, 24)))
    assert torch.equal(db, gy.reshape(64, 40).sum(0))


def test_hip_on_cpu_raises_and_unknown_impl_rejected():
    gy = torch.randn(64, 256).to(torch.bfloat16)
    x = torch.randn(64, 256).to(torch.bfloat16)
    with pytest.raises(RuntimeError):
        F.linear_wgrad_bias(gy, x, impl="hip")
    with pytest.raises(ValueError):
        F.linear_wgrad_bias(gy, x, impl="fast")
    # a failed call leaves no request behind for the next linear_wgrad
    assert F._wgrad_db_request is None


@pytest.mark.parametrize("T,N,K,switch,want", [
    # the four layer shapes: fused exactly where the wgrad rule admits
    (32768, 12288, 4096, "1", True), (32768, 4096, 4096, "1", True),
    (32768, 16384, 4096, "1", True), (8192, 4096, 16384, "1", True),
    # HETU_AMD_WGRAD_BIAS=0: the unfused pair even there
    (32768, 12288, 4096, "0", False), (8192, 4096, 16384, "0", False),
    # what the wgrad rule sends to the library is never fused
    (1984, 4096, 4096, "1", False), (32768, 4096, 3840, "1", False),
    (32768, 2048, 1024, "1", False),
])
def test_auto_rule_and_switch(T, N, K, switch, want):
    assert F._wgrad_bias_auto_fused(T, N, K, switch) is want
    if switch == "1":
        assert want is F._wgrad_auto_hip(T, N, K)


def _biased_linear_graph():
    torch.manual_seed(5)
    wv, bv = torch.randn(6, 8), torch.randn(6)
    xv, cv = torch.randn(2, 5, 8), torch.randn(2, 5, 6)
    g = DefineAndRunGraph("wgrad_bias_cpu")
    push_graph(g)
    try:
        x = ht.placeholder((2, 5, 8), name="x")
        c = ht.placeholder((2, 5, 6), name="c")
        w = ht.variable(wv.clone(), name="w")
        b = ht.variable(bv.clone(), name="b")
        loss = ht.reduce_sum(ht.mul(ht.linear(x, w, b), c))
        grads = ht.gradients(loss, [x, w, b])
    finally:
        pop_graph()
    return g, (x, c), grads, (wv, bv, xv, cv)


def test_biased_linear_builds_one_two_output_grad_op():
    g, (x, c), grads, (wv, bv, xv, cv) = _biased_linear_graph()
    types = [op.type for op in g.ops]
    assert types.count("LinearGradWB") == 1
    assert "ReduceLeading" not in types and "MatMulGradW" not in types
    (wb,) = [op for op in g.ops if op.type == "LinearGradWB"]
    assert len(wb.outputs) == 2
    assert grads[1].producer is wb and grads[2].producer is wb
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    dx, dw, db = g.run(list(grads), {x: xv, c: cv}, ctx=ctx)
    xt = xv.clone().requires_grad_(True)
    wt = wv.clone().requires_grad_(True)
    bt = bv.clone().requires_grad_(True)
    (torch.nn.functional.linear(xt, wt, bt) * cv).sum().backward()
    torch.testing.assert_close(dx, xt.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dw, wt.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(db, bt.grad, rtol=1e-5, atol=1e-5)


def test_unbiased_linear_keeps_matmul_grad_w():
    g = DefineAndRunGraph("wgrad_nobias_cpu")
    push_graph(g)
    try:
        x = ht.placeholder((2, 5, 8), name="x")
        w = ht.variable(torch.randn(6, 8), name="w")
        ht.gradients(ht.reduce_sum(ht.linear(x, w)), [w])
    finally:
        pop_graph()
    types = [op.type for op in g.ops]
    assert types.count("MatMulGradW") == 1 and "LinearGradWB" not in types


def _same_ds(a, b):
    if a.ds is None or b.ds is None:
        return a.ds is None and b.ds is None
    return a.ds.check_equal(b.ds)


@pytest.mark.parametrize("layout", ["dp2", "tp2_col", "dp2xtp2"])
def test_output_ds_equal_the_two_old_ops(layout):
    spec = {"dp2": ParallelSpec(dp=2), "tp2_col": ParallelSpec(tp=2),
            "dp2xtp2": ParallelSpec(dp=2, tp=2)}[layout]
    B_, S, N, K = 4, 6, 8, 10
    g = DefineAndRunGraph(f"wgrad_bias_ds_{layout}")
    push_graph(g)
    try:
        # a column-parallel Linear's backward: gy split on batch over dp and
        # on features over tp, x dup over tp, bias split over tp
        gy = ht.placeholder((B_, S, N // spec.tp), name="gy",
                            ds=spec._ds({0: spec.dp, 2: spec.tp}, [0, 2]),
                            device_group=spec.device_group)
        x = ht.placeholder((B_, S, K), name="x", ds=spec.ds_activation(0),
                           device_group=spec.device_group)
        b = ht.variable(torch.zeros(N // spec.tp), name="b",
                        ds=spec.ds_weight_col(0),
                        device_group=spec.device_group)
        old_dw = g.make_op(B.MatMulGradWOp(), [gy, x], {}).output()
        old_db = g.make_op(B.ReduceLeadingOp(), [gy, b], {}).output()
        wb = g.make_op(B.LinearGradWBOp(), [gy, x, b], {})
    finally:
        pop_graph()
    dw, db = wb.outputs
    assert old_dw.ds is not None and old_db.ds is not None
    assert _same_ds(dw, old_dw) and _same_ds(db, old_db)
    assert dw.device_group == old_dw.device_group
    assert db.device_group == old_db.device_group
    assert (tuple(dw.shape), dw.dtype) == (tuple(old_dw.shape), old_dw.dtype)
    assert (tuple(db.shape), db.dtype) == (tuple(old_db.shape), old_db.dtype)
    if spec.dp > 1:
        assert dw.ds.partial == spec.dp and db.ds.partial == spec.dp
    if spec.tp > 1:
        assert dw.ds.get_dim(0) == spec.tp and db.ds.get_dim(0) == spec.tp


def test_row_parallel_tp1_folds_bias_into_linear():
    torch.manual_seed(6)
    g = DefineAndRunGraph("row_tp1")
    push_graph(g)
    try:
        layer = RowParallelLinear(8, 6, ParallelSpec(), bias=True)
        x = ht.placeholder((2, 5, 8), name="x")
        y = layer(x)
    finally:
        pop_graph()
    types = [op.type for op in g.ops]
    assert "Add" not in types and "Comm" not in types
    assert types.count("Linear") == 1
    assert len(y.producer.inputs) == 3
    bv = torch.randn(6)
    layer.bias.get_data().copy_(bv)      # the layer initialises it to zero
    wv = layer.weight.get_data().clone()
    xv = torch.randn(2, 5, 8)
    ctx = prepare_run_context(g, torch.device("cpu"), use_comm=False)
    (out,) = g.run([y], {x: xv}, ctx=ctx)
    torch.testing.assert_close(out, xv @ wv.t() + bv, rtol=1e-5, atol=1e-5)


def test_row_parallel_tp1_unfused_when_spec_says_so():
    g = DefineAndRunGraph("row_tp1_unfused")
    push_graph(g)
    try:
        layer = RowParallelLinear(8, 6, ParallelSpec(fuse_row_bias=False))
        y = layer(ht.placeholder((2, 5, 8), name="x"))
    finally:
        pop_graph()
    assert [op.type for op in g.ops if op.type in ("Linear", "Add")] == \
        ["Linear", "Add"]
    assert y.producer.type == "Add"


def test_row_parallel_tp2_keeps_linear_comm_add():
    spec = ParallelSpec(tp=2)
    g = DefineAndRunGraph("row_tp2")
    push_graph(g)
    try:
        layer = RowParallelLinear(8, 6, spec, bias=True)
        x = ht.placeholder((2, 5, 4), name="x",
                           ds=spec._ds({2: 2}, [2]),
                           device_group=spec.device_group)
        y = layer(x)
    finally:
        pop_graph()
    chain = [op.type for op in g.ops if op.type in ("Linear", "Comm", "Add")]
    assert chain == ["Linear", "Comm", "Add"]
    lin = [op for op in g.ops if op.type == "Linear"][0]
    assert len(lin.inputs) == 2
    assert y.producer.type == "Add"
