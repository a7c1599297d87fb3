"""Exact-arithmetic GPU tests of the implicit-GEMM conv2d (conv2d.hip):
all three tile configurations, both staging paths, the inline zero-pad,
the channel-pad and tiny-N routes of conv2d_mod and the out= slice write.

Method.  Inputs are small integers held in bf16 (x in -3..3, w in -2..2,
bias and residual in -8..8), so every bf16 product and every fp32 partial
sum is an exact integer (|sum| <= 6*Kr + 16 with Kr <= 2952: far below
2^24) and the pre-activation value is exact in ANY accumulation order.  The
reference is F.conv2d in float64 on the CPU (+ float64 bias and residual).
For act none / relu both sides round the same exact number to bf16 once,
so the comparison is torch.equal: one misplaced 16-byte segment, border
tap or K-tail slice fails it.  leaky_relu / quick_gelu / gelu are inexact
in fp32; they get one bf16 ulp of the reference (2^-7 |ref|) plus an
absolute floor measured on the CPU, see ACT_FLOOR.

Every case states the tile it is meant to run and asserts it through
ops._ext.conv2d_tile (the host function launch_conv itself calls) before
running, so routing drift fails loudly instead of emptying the case."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = ['none', 'relu', 'leaky_relu', 'quick_gelu', 'gelu']

T256, T64, T128 = (256, 256), (256, 64), (128, 128)

# name -> ((B, C, H, W, K_out, KH, KW, stride, pad), tile)
CASES = {
    # ---- 256x256 tile (8 waves); needs K_out >= 256 and M >= 4096
    # 16 full tiles, Kr = 72: two K-tiles, the last ragged (glds -> guard
    # hand-over inside the K loop)
    'c01': ((1, 8, 64, 64, 256, 3, 3, 1, 1), T256),
    # Kr = 576, K full: pure glds, inline pad on every border
    'c02': ((1, 64, 64, 64, 256, 3, 3, 1, 1), T256),
    # M = 4290: 17 tiles, ragged M, stride 2
    'c03': ((1, 16, 131, 130, 256, 3, 3, 2, 1), T256),
    # C = 24: a tap boundary falls inside a 64-wide K-tile
    'c04': ((1, 24, 64, 64, 256, 1, 5, 1, (0, 2)), T256),
    'c05': ((1, 8, 64, 64, 256, 7, 7, 1, 3), T256),
    # M = 4290, N = 2296: 17 x 9 = 153 tiles, ragged M and N, XCD remap
    # remainder 153 % 8 = 1
    'c06': ((1, 8, 66, 65, 2296, 3, 3, 1, 1), T256),
    # ---- 256x64 tile
    'c07': ((2, 64, 16, 16, 64, 3, 3, 1, 1), T64),      # 2 full tiles
    'c08': ((1, 8, 32, 32, 192, 3, 3, 1, 1), T64),      # 12 tiles
    'c09': ((1, 16, 47, 45, 40, 3, 3, 1, 1), T64),      # M 2115, N 40
    'c10': ((1, 8, 30, 30, 136, 3, 3, 1, 1), T64),
    # ---- 128x128 tile
    'c11': ((1, 64, 16, 16, 128, 3, 3, 1, 1), T128),    # full
    'c12': ((1, 24, 13, 11, 100, 3, 3, 1, 1), T128),    # ragged everything
    'c13': ((2, 64, 12, 12, 128, 1, 1, 2, 0), T128),    # strided 1x1
    # ---- geometry edges
    'c14': ((1, 16, 16, 16, 128, 3, 3, 2, (0, 1, 0, 1)), T128),  # TF-SAME
    'c15': ((1, 16, 20, 33, 128, 3, 5, (2, 3), (1, 2)), T128),   # sh != sw
    # pad wider than the kernel reach: whole windows lie in the padding
    'c16': ((1, 8, 4, 4, 16, 3, 3, 1, 3), T128),
    'c17': ((1, 8, 3, 3, 16, 3, 3, 1, 0), T128),        # M = 1
    'c18': ((1, 8, 5, 5, 12, 1, 1, 1, 0), T128),        # 1x1, K_out % 8 != 0
    # B > 1 with odd H, W: tile rows cross image boundaries
    'c19': ((3, 16, 9, 7, 64, 3, 3, 1, 1), T64),
}

# one case per tile, two of them ragged
MATRIX_CASES = ['c01', 'c09', 'c12']

# conv2d_mod routes: (B, C, H, W, K_out, KH, KW, stride, pad), tile of the
# conv actually launched (C padded up to 8 / K_out padded up to 16)
CPAD_CASES = {
    'stem3': ((1, 3, 33, 35, 64, 7, 7, 2, 3), T64),
    'stem2': ((1, 2, 20, 22, 32, 7, 7, 1, 3), T64),
    'corr324': ((1, 324, 12, 14, 96, 3, 3, 1, 1), T128),
    'corr324_1x1': ((1, 324, 12, 14, 256, 1, 1, 1, 0), T128),
}
TINY_N_CASES = {
    'flow2': ((2, 128, 10, 12, 2, 3, 3, 1, 1), T64),
    'n9': ((2, 128, 10, 12, 9, 3, 3, 1, 1), T64),
}

# Worst |torch fp32 activation - float64 activation| over the exact
# pre-activation values of every MATRIX_CASES x bias x residual problem,
# as printed by measure_act_floor() below on the CPU:
#   leaky_relu 5.722e-07, quick_gelu 4.058e-07, gelu 2.477e-07
# The comparison allows 4x these, because the kernel evaluates the
# activation with v_exp_f32 / v_rcp_f32 / tanhf (act_f in mfma_tile.h) and
# not with torch's routines.
ACT_FLOOR = {'leaky_relu': 5.722e-07, 'quick_gelu': 4.058e-07,
             'gelu': 2.477e-07}
FLOOR_MARGIN = 4.0
SENTINEL = -12352.0          # exact in bf16; never a legal neighbour value


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    return ops


def _pad4(pad):
    if isinstance(pad, int):
        return (pad,) * 4
    if len(pad) == 2:
        return (pad[0], pad[0], pad[1], pad[1])
    return tuple(pad)


def _geom(shape):
    b, c, h, w, k, kh, kw, stride, pad = shape
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    pt, pb, pl, pr = _pad4(pad)
    oh = (h + pt + pb - kh) // sh + 1
    ow = (w + pl + pr - kw) // sw + 1
    return (sh, sw), (pt, pb, pl, pr), oh, ow


def _act64(y, act):
    """The activation in float64 (the kernel's formulas, act_f)."""
    if act == 'relu':
        return y.relu()
    if act == 'leaky_relu':
        return F.leaky_relu(y, 0.1)
    if act == 'quick_gelu':
        return y * torch.sigmoid(1.702 * y)
    if act == 'gelu':
        return F.gelu(y, approximate='tanh')
    return y


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.bfloat16)


@functools.lru_cache(maxsize=4)
def _problem_cpu(shape):
    """Integer-valued bf16 inputs of one shape and the float64 CPU conv of
    them (no bias, no residual) -- built once, shared read-only."""
    b, c, h, w, k, kh, kw, _, _ = shape
    (sh, sw), (pt, pb, pl, pr), oh, ow = _geom(shape)
    gen = torch.Generator().manual_seed(
        sum(p * v for p, v in zip((3, 5, 7, 11, 13, 17, 19), shape[:7])))
    x = _ints(gen, (b, c, h, w), -3, 3)
    wgt = _ints(gen, (k, c, kh, kw), -2, 2)
    bias = _ints(gen, (k,), -8, 8)
    res = _ints(gen, (b, k, oh, ow), -8, 8)
    y = F.conv2d(F.pad(x.double(), (pl, pr, pt, pb)), wgt.double(), None,
                 (sh, sw), 0)
    assert y.shape == (b, k, oh, ow)
    return x, wgt, bias, res, y


@functools.lru_cache(maxsize=4)
def _problem(shape):
    """_problem_cpu plus the device copies the kernel reads."""
    x, wgt, bias, res, y = _problem_cpu(shape)
    dev = torch.device('cuda:0')
    cl = torch.channels_last
    return (x.to(dev).contiguous(memory_format=cl),
            wgt.to(dev).contiguous(memory_format=cl), bias.to(dev),
            res.to(dev).contiguous(memory_format=cl), bias, res, y)


def _pre64(shape, use_bias, use_res):
    """Exact pre-activation values in float64 (CPU)."""
    _, _, bias, res, y = _problem_cpu(shape)
    if use_bias:
        y = y + bias.double().view(1, -1, 1, 1)
    if use_res:
        y = y + res.double()
    return y


def measure_act_floor():
    """CPU only: worst |fp32 torch activation - float64 activation| over
    the pre-activation values of the epilogue matrix; the source of
    ACT_FLOOR.  Run by hand (python -c 'import ...; measure_act_floor()')
    when MATRIX_CASES or the data ranges change."""
    worst = {a: 0.0 for a in ACT_FLOOR}
    for name in MATRIX_CASES:
        for ub, ur in itertools.product((False, True), repeat=2):
            pre = _pre64(CASES[name][0], ub, ur)
            for a in worst:
                d = (_act64(pre.float(), a).double() - _act64(pre, a)).abs()
                worst[a] = max(worst[a], d.max().item())
    for a, v in worst.items():
        print(f'{a}: {v:.3e}')
    return worst


def _tile(ops, m, kout):
    return tuple(ops._ext.conv2d_tile(m, kout))


def _assert_tile(ops, name, shape, want, kout=None):
    b, k = shape[0], shape[4] if kout is None else kout
    _, _, oh, ow = _geom(shape)
    got = _tile(ops, b * oh * ow, k)
    print(f'{name}: M={b * oh * ow} K_out={k} '
          f'Kr={shape[5] * shape[6] * ((shape[1] + 7) // 8 * 8)} '
          f'tile={got[0]}x{got[1]}')
    assert got == want, (
        f'{name} is meant to run the {want[0]}x{want[1]} tile but routes '
        f'to {got[0]}x{got[1]}: change the SHAPE so it reaches its tile')
    return got


def _compare(out, ref64, act, tile, what):
    """out: bf16 (B, K, OH, OW) from the kernel; ref64: float64 CPU."""
    out = out.detach().cpu()
    assert out.dtype == torch.bfloat16 and out.shape == ref64.shape, \
        (out.dtype, out.shape, ref64.shape)
    if act in ('none', 'relu'):
        bad = out != ref64.to(torch.bfloat16)
    else:
        tol = ref64.abs() * 2.0 ** -7 + FLOOR_MARGIN * ACT_FLOOR[act]
        bad = ~((out.double() - ref64).abs() <= tol)     # NaN is bad
    nbad = int(bad.sum())
    if nbad:
        # first bad element in NHWC (memory / GEMM row-major) order
        idx = bad.permute(0, 2, 3, 1).nonzero()[0].tolist()
        bi, oy, ox, k = idx
        raise AssertionError(
            f'{what}: {nbad} of {bad.numel()} elements wrong, first at '
            f'(b, oy, ox, k) = {(bi, oy, ox, k)}: got '
            f'{out[bi, k, oy, ox].item()} want {ref64[bi, k, oy, ox].item()}'
            f'; tile {tile[0]}x{tile[1]}')


def _run(name, act='none', use_bias=True, use_res=False):
    ops = _ops()
    shape, want = CASES[name]
    tile = _assert_tile(ops, name, shape, want)
    x, wgt, bias, res, _, _, _ = _problem(shape)
    stride, pad = shape[7], shape[8]
    out = ops.conv2d_act(x, wgt, bias if use_bias else None, stride, pad,
                         act, res if use_res else None)
    assert out.is_contiguous(memory_format=torch.channels_last)
    ref = _act64(_pre64(shape, use_bias, use_res), act)
    _compare(out, ref, act, tile,
             f'{name} act={act} bias={use_bias} res={use_res}')
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_exact(name):
    """Bias, no activation: bit-exact against the float64 reference."""
    _run(name)


@pytest.mark.parametrize(
    'name,act,use_bias,use_res',
    [(n, a, b, r) for n in MATRIX_CASES for a in ACTS
     for b in (True, False) for r in (False, True)])
def test_epilogue_matrix(name, act, use_bias, use_res):
    """Every activation x bias / None x residual / none, one case per
    tile.  none and relu are bit-exact; leaky_relu, quick_gelu and gelu
    allow 2^-7 |ref| + 4 * ACT_FLOOR[act] (floors measured on the CPU:
    leaky_relu 5.722e-07, quick_gelu 4.058e-07, gelu 2.477e-07)."""
    _run(name, act, use_bias, use_res)


@pytest.mark.parametrize('name,act,use_res',
                         [(n, a, r) for n in MATRIX_CASES
                          for a, r in (('none', False), ('relu', True))])
def test_slice_write(name, act, use_res):
    """out= a wider channels_last buffer, out_off=8: the slice equals the
    reference and the 8 channels below / 16 above keep the sentinel bit
    for bit."""
    ops = _ops()
    shape, want = CASES[name]
    tile = _assert_tile(ops, name, shape, want)
    x, wgt, bias, res, _, _, _ = _problem(shape)
    b, k = shape[0], shape[4]
    _, _, oh, ow = _geom(shape)
    buf = torch.full((b, k + 24, oh, ow), SENTINEL, dtype=torch.bfloat16,
                     device=x.device).contiguous(
                         memory_format=torch.channels_last)
    ret = ops.conv2d_act(x, wgt, bias, shape[7], shape[8], act,
                         res if use_res else None, out=buf, out_off=8)
    assert ret.data_ptr() == buf.data_ptr() and ret.shape == buf.shape
    assert buf.is_contiguous(memory_format=torch.channels_last)
    ref = _act64(_pre64(shape, True, use_res), act)
    _compare(buf[:, 8:8 + k], ref, act, tile, f'{name} slice act={act}')
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)
    bits = buf.cpu().view(torch.int16)
    for lo, hi in ((0, 8), (8 + k, k + 24)):
        nbad = int((bits[:, lo:hi] != sent).sum())
        assert nbad == 0, (f'{name}: {nbad} elements of channels [{lo}, {hi})'
                           f' overwritten; tile {tile[0]}x{tile[1]}')


def _module(shape, dev):
    """nn.Conv2d holding the integer weights / bias of _problem_cpu."""
    _, c, _, _, k, kh, kw, stride, pad = shape
    _, wgt, bias, _, _ = _problem_cpu(shape)
    conv = torch.nn.Conv2d(c, k, (kh, kw), stride, pad)
    with torch.no_grad():
        conv.weight.copy_(wgt)
        conv.bias.copy_(bias)
    return conv.to(dev, torch.bfloat16)


@pytest.mark.parametrize('name', list(CPAD_CASES))
def test_channel_pad_route(name):
    """C % 8 != 0 through conv2d_mod: pad2d_nhwc widens the channels (the
    straddling 16-byte segment copied element-wise), the cached weight is
    zero-padded to match.  Then the weight changes in place and the result
    must follow it (GPU twin of
    test_conv2d_mod_padded_weight_cache_invalidates)."""
    ops = _ops()
    shape, want = CPAD_CASES[name]
    tile = _assert_tile(ops, name, shape, want)
    x = _problem(shape)[0]
    conv = _module(shape, x.device)
    out = ops.conv2d_mod(conv, x)
    assert out.is_contiguous(memory_format=torch.channels_last)
    _compare(out, _pre64(shape, True, False), 'none', tile, name)

    # new integer weights in place: w -> 1 - w stays in -1..3
    with torch.no_grad():
        conv.weight.neg_().add_(1.0)
    out2 = ops.conv2d_mod(conv, x)
    xc, wc, bias, _, _ = _problem_cpu(shape)
    (sh, sw), (pt, pb, pl, pr), _, _ = _geom(shape)
    ref2 = F.conv2d(F.pad(xc.double(), (pl, pr, pt, pb)), 1.0 - wc.double(),
                    bias.double(), (sh, sw), 0)
    _compare(out2, ref2, 'none', tile, name + ' after weight update')
    assert not torch.equal(out, out2)


@pytest.mark.parametrize('name', list(TINY_N_CASES))
def test_tiny_n_route(name):
    """K_out < 16 through conv2d_mod: output channels padded to 16, run
    in-tree, sliced back to a channels_last (B, K_out, OH, OW)."""
    ops = _ops()
    shape, want = TINY_N_CASES[name]
    tile = _assert_tile(ops, name, shape, want, kout=16)
    x = _problem(shape)[0]
    conv = _module(shape, x.device)
    out = ops.conv2d_mod(conv, x)
    b, k = shape[0], shape[4]
    _, _, oh, ow = _geom(shape)
    assert out.shape == (b, k, oh, ow)
    assert out.is_contiguous(memory_format=torch.channels_last)
    _compare(out, _pre64(shape, True, False), 'none', tile, name)


@pytest.mark.parametrize('name', ['c02', 'c06'])
def test_run_twice_bit_identical(name):
    """A race between the next K-tile's staging and the MFMA reads of the
    current one would show as run-to-run differences."""
    o1 = _run(name, 'relu', True, True)
    o2 = _run(name, 'relu', True, True)
    assert torch.equal(o1, o2)
