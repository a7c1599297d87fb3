"""Exact-arithmetic GPU tests of conv2d_nhwc's dilation and channel-slice
input (conv2d.hip: the tap address iy = y0 + r*dh, ix = x0 + s*dw and the
input pixel stride ldx), through ops.conv2d_act and ops.conv2d_mod.

Method: that of test_gpu_conv_exact.py, whose helpers, data ranges,
ACT_FLOOR and FLOOR_MARGIN are imported unchanged.  x in -3..3, w in -2..2,
bias and residual in -8..8, all held in bf16; |sum| <= 6*Kr + 16 with
Kr <= 2952 is far below 2^24, so every partial sum is exact in any order.
none / relu are compared with torch.equal against float64
F.conv2d(..., dilation=) rounded to bf16, the other activations with
2^-7 |ref| + FLOOR_MARGIN * ACT_FLOOR[act].  Every case asserts the tile it
is meant to run through ops._ext.conv2d_tile before running.

Slice cases fill the buffer with SENTINEL outside the read slice, so one
mis-addressed 16-byte segment wrecks the result, and require every channel
outside the written slice to be bit-unchanged afterwards."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_exact import (ACT_FLOOR, ACTS, FLOOR_MARGIN, SENTINEL,
                                 T64, T128, T256, _act64, _compare, _ints,
                                 _ops, _tile)

pytestmark = pytest.mark.gpu

assert set(ACT_FLOOR) == {'leaky_relu', 'quick_gelu', 'gelu'}
assert FLOOR_MARGIN == 4.0

# name -> ((B, C, H, W, K_out, KH, KW, stride, pad, dil), tile)
CASES = {
    # ---- 256x256 tile
    'd01': ((1, 8, 64, 64, 256, 3, 3, 1, 2, 2), T256),    # ragged last K-tile
    # ragged M, stride 2 with dilation 2
    'd02': ((1, 16, 131, 130, 256, 3, 3, 2, 2, 2), T256),
    # C = 24: a tap boundary falls inside a 64-wide K-tile
    'd03': ((1, 24, 64, 64, 256, 3, 3, 1, 4, 4), T256),
    # ---- 256x64 tile
    'd04': ((2, 64, 16, 16, 64, 3, 3, 1, 4, 4), T64),     # full, pure glds
    'd05': ((1, 16, 47, 45, 40, 3, 3, 1, (2, 3), (2, 3)), T64),   # dh != dw
    # ---- 128x128 tile
    'd06': ((1, 64, 16, 16, 128, 3, 3, 1, 8, 8), T128),   # full tile
    'd07': ((1, 24, 13, 11, 100, 3, 3, 1, 2, 2), T128),   # ragged everything
    # dilation larger than the image: only centre taps are in bounds
    'd08': ((1, 8, 9, 7, 32, 3, 3, 1, 16, 16), T128),
    # everything asymmetric
    'd09': ((1, 16, 20, 33, 128, 3, 5, (2, 3), (3, 4), (3, 2)), T128),
    # B > 1 with odd H, W: tile rows cross image boundaries
    'd10': ((3, 16, 9, 7, 64, 3, 3, 1, 2, 2), T64),
    'd11': ((1, 8, 12, 12, 16, 3, 3, 1, 0, 4), T128),     # no pad
    'd12': ((1, 8, 9, 9, 16, 3, 3, 1, 0, 4), T128),       # M = 1
}
MATRIX_CASES = ['d01', 'd05', 'd07']
RES_CASE = 'd07'

# name -> (buffer (B, C, H, W), read [lo, hi), write offset or None for a
# fresh tensor, K_out, pad, dil, tile); all 3x3 stride 1
SLICE_CASES = {
    # 256x256 full tile, Kr 576: pure glds with ldx != cin
    'fresh256': ((1, 136, 64, 64), (72, 136), None, 256, 1, 1, T256),
    # 256x64 full tile, in place
    'inplace64': ((2, 128, 16, 16), (64, 128), 0, 64, 1, 1, T64),
    # 128x128 full tile, in place
    'inplace128': ((1, 192, 16, 16), (128, 192), 0, 128, 1, 1, T128),
    # M = 240, C = 40: the guarded path
    'guarded': ((2, 72, 10, 12), (32, 72), 0, 32, 1, 1, T64),
    'dil2': ((1, 56, 13, 11), (16, 56), 0, 16, 2, 2, T64),
}


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _geom(shape):
    b, c, h, w, k, kh, kw, stride, pad, dil = shape
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(pad), _pair(dil)
    oh = (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    ow = (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    return (sh, sw), (ph, pw), (dh, dw), oh, ow


def _assert_tile(ops, name, m, kout, want):
    got = _tile(ops, m, kout)
    print(f'{name}: M={m} K_out={kout} tile={got[0]}x{got[1]}')
    assert got == want, (
        f'{name} is meant to run the {want[0]}x{want[1]} tile but routes '
        f'to {got[0]}x{got[1]}: change the SHAPE so it reaches its tile')
    return got


@functools.lru_cache(maxsize=4)
def _problem_cpu(shape):
    """Integer-valued bf16 inputs and the float64 dilated conv of them (no
    bias, no residual): built once per shape, shared read-only."""
    b, c, h, w, k, kh, kw = shape[:7]
    stride, pad, dil, oh, ow = _geom(shape)
    gen = torch.Generator().manual_seed(
        1 + sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19), shape[:7])))
    x = _ints(gen, (b, c, h, w), -3, 3)
    wgt = _ints(gen, (k, c, kh, kw), -2, 2)
    bias = _ints(gen, (k,), -8, 8)
    res = _ints(gen, (b, k, oh, ow), -8, 8)
    y = F.conv2d(x.double(), wgt.double(), None, stride, pad, dil)
    assert y.shape == (b, k, oh, ow)
    return x, wgt, bias, res, y


def _cl(t):
    return t.to('cuda:0').contiguous(memory_format=torch.channels_last)


def _run(name, act, use_res=False):
    ops = _ops()
    shape, want = CASES[name]
    stride, pad, dil, oh, ow = _geom(shape)
    tile = _assert_tile(ops, name, shape[0] * oh * ow, shape[4], want)
    x, wgt, bias, res, y = _problem_cpu(shape)
    out = ops.conv2d_act(_cl(x), _cl(wgt), bias.to('cuda:0'), shape[7],
                         shape[8], act, _cl(res) if use_res else None,
                         dilation=shape[9])
    assert out.is_contiguous(memory_format=torch.channels_last)
    pre = y + bias.double().view(1, -1, 1, 1)
    if use_res:
        pre = pre + res.double()
    _compare(out, _act64(pre, act), act, tile,
             f'{name} act={act} res={use_res} dil={dil}')


@pytest.mark.parametrize('name,act', [
    (n, a) for n in CASES
    for a in (ACTS if n in MATRIX_CASES else ('none', 'relu'))])
def test_dilated(name, act):
    """Bias + activation.  none / relu bit-exact; leaky_relu, quick_gelu
    and gelu (on d01, d05, d07: one case per tile) within
    2^-7 |ref| + 4 * ACT_FLOOR[act]."""
    _run(name, act)


@pytest.mark.parametrize('act', ACTS)
def test_dilated_residual(act):
    _run(RES_CASE, act, use_res=True)


def _sentinel_bits():
    return torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)


def _slice_problem(bshape, lo, hi, kout, seed):
    """Buffer of SENTINEL with integer data in channels [lo, hi), integer
    weights / bias for a 3x3 conv of that slice."""
    gen = torch.Generator().manual_seed(seed)
    buf = torch.full(bshape, SENTINEL, dtype=torch.bfloat16)
    b, _, h, w = bshape
    buf[:, lo:hi] = _ints(gen, (b, hi - lo, h, w), -3, 3)
    wgt = _ints(gen, (kout, hi - lo, 3, 3), -2, 2)
    bias = _ints(gen, (kout,), -8, 8)
    return buf, wgt, bias


@pytest.mark.parametrize('name,act', [(n, a) for n in SLICE_CASES
                                      for a in ('none', 'relu')])
def test_slice_input(name, act):
    ops = _ops()
    bshape, (lo, hi), woff, kout, pad, dil, want = SLICE_CASES[name]
    b, ctot, h, w = bshape
    tile = _assert_tile(ops, name, b * h * w, kout, want)   # 'same' convs
    buf, wgt, bias = _slice_problem(bshape, lo, hi, kout, 11 + ctot)
    ref = _act64(F.conv2d(buf[:, lo:hi].double(), wgt.double(),
                          bias.double(), 1, pad, dil), act)
    dbuf = _cl(buf)
    ret = ops.conv2d_act(dbuf, _cl(wgt), bias.to('cuda:0'), 1, pad, act,
                         out=None if woff is None else dbuf,
                         out_off=0 if woff is None else woff,
                         dilation=dil, in_off=lo, in_ch=hi - lo)
    after = dbuf.cpu()
    before_bits, after_bits = buf.view(torch.int16), after.view(torch.int16)
    if woff is None:
        assert ret.shape == ref.shape
        assert ret.is_contiguous(memory_format=torch.channels_last)
        _compare(ret, ref, act, tile, f'{name} act={act}')
        assert torch.equal(after_bits, before_bits), f'{name}: buffer changed'
        return
    assert ret.data_ptr() == dbuf.data_ptr() and ret.shape == dbuf.shape
    _compare(after[:, woff:woff + kout], ref, act, tile, f'{name} act={act}')
    keep = torch.ones(ctot, dtype=torch.bool)
    keep[woff:woff + kout] = False
    nbad = int((after_bits[:, keep] != before_bits[:, keep]).sum())
    assert nbad == 0, (f'{name}: {nbad} elements outside channels '
                       f'[{woff}, {woff + kout}) changed')


def _mod_case(kout, pad, dil):
    """nn.Conv2d(21, kout, 3) on the buffer (2, 40, 10, 12) laid out
    [16 out | 21 in | 3 pad]; the pad channels hold 3.0, not 0."""
    gen = torch.Generator().manual_seed(100 + kout + dil)
    x = _ints(gen, (2, 21, 10, 12), -3, 3)
    wgt = _ints(gen, (kout, 21, 3, 3), -2, 2)
    bias = _ints(gen, (kout,), -8, 8)
    buf = torch.full((2, 40, 10, 12), SENTINEL, dtype=torch.bfloat16)
    buf[:, 16:37] = x
    buf[:, 37:] = 3.0
    conv = torch.nn.Conv2d(21, kout, 3, padding=pad, dilation=dil)
    with torch.no_grad():
        conv.weight.copy_(wgt)
        conv.bias.copy_(bias)
    ref = F.conv2d(x.double(), wgt.double(), bias.double(), 1, pad, dil)
    return buf, conv.to('cuda:0', torch.bfloat16), ref


@pytest.mark.parametrize('kout,pad,dil', [(16, 1, 1), (16, 2, 2), (2, 1, 1)])
def test_conv2d_mod_slice_channel_pad(kout, pad, dil):
    """C % 8 != 0 slice through conv2d_mod: the kernel reads 24 channels,
    the cached weight's 3 extra columns must be zero (the buffer holds 3.0
    there).  K_out = 2 takes the tiny-N route (16 output channels run)."""
    ops = _ops()
    tile = _assert_tile(ops, f'mod k{kout} d{dil}', 2 * 10 * 12, 16, T64)
    buf, conv, ref = _mod_case(kout, pad, dil)
    dbuf = _cl(buf)
    ret = ops.conv2d_mod(conv, dbuf, 'none', out=dbuf, out_off=0, in_off=16)
    assert ret.data_ptr() == dbuf.data_ptr()
    after = dbuf.cpu()
    _compare(after[:, :kout], ref, 'none', tile, f'conv2d_mod k{kout} d{dil}')
    assert torch.equal(after[:, kout:].view(torch.int16),
                       buf[:, kout:].view(torch.int16))
    if kout == 2:
        # no out=: a fresh channels_last (B, 2, OH, OW)
        y = ops.conv2d_mod(conv, dbuf, 'none', in_off=16)
        assert y.shape == ref.shape
        assert y.is_contiguous(memory_format=torch.channels_last)
        _compare(y, ref, 'none', tile, 'conv2d_mod tiny-N fresh')


def test_overlapping_slices_rejected():
    """Read [0, 64), write [32, 96) of one buffer: a host check, raised
    before any launch."""
    ops = _ops()
    buf = torch.zeros(1, 96, 8, 8, dtype=torch.bfloat16, device='cuda:0') \
        .contiguous(memory_format=torch.channels_last)
    wgt = torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16, device='cuda:0') \
        .contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match='overlap'):
        ops.conv2d_act(buf, wgt, None, 1, 1, out=buf, out_off=32, in_off=0,
                       in_ch=64)
    assert not bool(buf.any())


def test_two_chained_dense_steps():
    """x = cat([conv(x), x], 1) twice on one (1, 192, 16, 16) buffer:
    step 1 reads [128, 192) and writes relu into [64, 128), step 2 reads
    [64, 192) and writes [0, 64).  Step 1's outputs are integers of at most
    6*576 + 8 = 3464, rounded once to bf16 on both sides; step 2's sums stay
    below 2*3464*576 + 6*576 + 8 < 2^22 and integral, so they are exact too
    and the final comparison is torch.equal."""
    ops = _ops()
    tile = _assert_tile(ops, 'chain', 256, 64, T64)
    gen = torch.Generator().manual_seed(77)
    x = _ints(gen, (1, 64, 16, 16), -3, 3)
    w1, b1 = _ints(gen, (64, 64, 3, 3), -2, 2), _ints(gen, (64,), -8, 8)
    w2, b2 = _ints(gen, (64, 128, 3, 3), -2, 2), _ints(gen, (64,), -8, 8)
    y1 = F.conv2d(x.double(), w1.double(), b1.double(), 1, 1).relu() \
        .to(torch.bfloat16)
    x2 = torch.cat([y1.double(), x.double()], 1)
    y2 = F.conv2d(x2, w2.double(), b2.double(), 1, 1)
    ref = torch.cat([y2, x2], 1)
    buf = torch.zeros(1, 192, 16, 16, dtype=torch.bfloat16)
    buf[:, 128:] = x
    dbuf = _cl(buf)
    ops.conv2d_act(dbuf, _cl(w1), b1.to('cuda:0'), 1, 1, 'relu', out=dbuf,
                   out_off=64, in_off=128, in_ch=64)
    ops.conv2d_act(dbuf, _cl(w2), b2.to('cuda:0'), 1, 1, 'none', out=dbuf,
                   out_off=0, in_off=64, in_ch=128)
    _compare(dbuf, ref, 'none', tile, 'two chained dense steps')
