"""2-D transpose kernel (ops/hip/transpose.hip): transpose2d(w [R, C]) must
equal w.t().contiguous() bit for bit and write nothing else.

Shapes are the smallest that reach each path.  The 16-byte path needs
R % 8 == 0, C % 8 == 0 and 16-B aligned bases: (8, 8) is one partial tile,
(64, 64) one full tile, (320, 192) and (520, 264) several tiles with ragged
edges in one or both dimensions (520 = 8 * 64 + 8, 264 = 4 * 64 + 8: the
last tile holds a single 16-B chunk).  Everything else takes the element
path: single rows and columns, sizes one off the 64 tile in either
direction, odd x odd, and an input whose storage offset is not 16-B
aligned although its shape is eligible.

The output is written into the middle of a larger sentinel-filled buffer;
the guard rows before and after it must keep the sentinel.
"""
import pytest
import torch

import hetu_amd.ops.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 300), (300, 1), (8, 8), (63, 65), (64, 64), (65, 63),
          (127, 129), (320, 192), (520, 264), (255, 77)]
DTYPES = [torch.bfloat16, torch.float16]
SENTINEL = 12345
GUARD = 4          # guard rows of the output's width on each side


def dev():
    return torch.device("cuda", 0)


def _input(R, C, dtype, offset=0):
    """every element distinct mod 2^16 as far as the size allows"""
    bits = torch.arange(R * C + offset, dtype=torch.int64) * 40503 + 17
    buf = (bits & 0xFFFF).to(torch.int16).to(dev()).view(dtype)
    return buf[offset:offset + R * C].view(R, C)


def _guarded_out(R, C, dtype):
    """[C, R] output inside a sentinel buffer, GUARD rows on both sides;
    the rows are 8 * k elements long so the view stays 16-B aligned when
    R % 8 == 0"""
    whole = torch.full(((C + 2 * GUARD) * R,), SENTINEL, dtype=torch.int16,
                       device=dev())
    out = whole[GUARD * R:(GUARD + C) * R].view(dtype).view(C, R)
    return whole, out


def _check(w, R, C, dtype):
    whole, out = _guarded_out(R, C, dtype)
    got = F.ext().transpose2d(w, out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    want = w.t().contiguous()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert (whole[:GUARD * R] == SENTINEL).all(), "wrote before the output"
    assert (whole[(GUARD + C) * R:] == SENTINEL).all(), \
        "wrote past the output"
    fresh = F.ext().transpose2d(w)
    assert fresh.shape == (C, R) and fresh.is_contiguous()
    assert torch.equal(fresh.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,C", SHAPES)
def test_equals_torch_transpose(R, C, dtype):
    _check(_input(R, C, dtype), R, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,C", [(64, 64), (320, 192)])
def test_input_with_unaligned_storage_offset(R, C, dtype):
    w = _input(R, C, dtype, offset=3)
    assert w.is_contiguous() and w.data_ptr() % 16 != 0
    _check(w, R, C, dtype)


@pytest.mark.parametrize("R,C", [(320, 192), (127, 129)])
def test_block_orders_agree(R, C):
    w = _input(R, C, torch.bfloat16)
    assert torch.equal(F.ext().transpose2d(w, None, 0).view(torch.int16),
                       w.t().contiguous().view(torch.int16))


def test_rejects_what_it_cannot_move():
    w32 = torch.zeros(8, 8, device=dev())
    with pytest.raises(RuntimeError):
        F.ext().transpose2d(w32)
    nc = _input(16, 16, torch.bfloat16)[:, ::2]
    with pytest.raises(RuntimeError):
        F.ext().transpose2d(nc)
    w = _input(16, 8, torch.bfloat16)
    with pytest.raises(RuntimeError):
        F.ext().transpose2d(w, torch.empty(16, 8, dtype=w.dtype,
                                           device=dev()))
