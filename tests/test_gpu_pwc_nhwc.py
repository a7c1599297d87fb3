"""GPU tests of the channels_last PWC-Net path: the transposed-conv kernels
(tconv.hip), the NHWC warp and cost-volume kernels, and the whole net.

Method of the "exact" cases, as in test_gpu_conv_exact.py: the inputs are
small integers (or, for the flow, multiples of 0.25) held in bf16, so every
product and every f32 partial sum is exact in ANY accumulation order and
the kernel and the float64 CPU reference round the same exact number to
bf16 once.  The comparison is equality of the bf16 values."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the library routine itself: the references use it while the kernel-path
# tests replace torch.nn.functional.conv_transpose2d by a tripwire
_TCONV_REF = F.conv_transpose2d
SENTINEL = -12352.0          # exact in bf16; never a legal result here
CL = torch.channels_last


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    return ops


def _dev():
    return torch.device('cuda:0')


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.bfloat16)


def _assert_equal(out, ref64, what):
    """out: bf16 from the kernel; ref64: the exact float64 CPU values."""
    out = out.detach().cpu()
    assert out.dtype == torch.bfloat16 and out.shape == ref64.shape, \
        (what, out.dtype, out.shape, ref64.shape)
    bad = out != ref64.to(torch.bfloat16)
    nbad = int(bad.sum())
    if nbad:
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            f'{what}: {nbad} of {bad.numel()} elements wrong, first at '
            f'(b, c, y, x) = {idx}: got {out[idx].item()} want '
            f'{ref64[idx].item()}')


def _assert_sentinel(buf, lo, hi, what):
    """Channels outside [lo, hi) keep the sentinel bit for bit."""
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)
    bits = buf.detach().cpu().view(torch.int16)
    for a, b in ((0, lo), (hi, buf.shape[1])):
        nbad = int((bits[:, a:b] != sent).sum())
        assert nbad == 0, f'{what}: {nbad} elements of channels [{a}, {b}) ' \
                          'overwritten'


def _sentinel_buf(shape):
    return torch.full(shape, SENTINEL, dtype=torch.bfloat16,
                      device=_dev()).contiguous(memory_format=CL)


# ---------------------------------------------------------- transposed conv
@functools.lru_cache(maxsize=None)
def _tconv_problem(b, c, h, w, kout=2):
    """x in -3..3, W in -2..2, integer bias: |sum| <= 4*C*6 + 8 < 2^24 for
    C <= 568.  Returns the bf16 CPU tensors and the float64 reference."""
    gen = torch.Generator().manual_seed(1000 * c + 100 * b + 10 * h + w)
    x = _ints(gen, (b, c, h, w), -3, 3)
    wgt = _ints(gen, (c, kout, 4, 4), -2, 2)
    bias = _ints(gen, (kout,), -8, 8)
    ref = _TCONV_REF(x.double(), wgt.double(), bias.double(), 2, 1)
    return x, wgt, bias, ref


@pytest.fixture
def no_library_tconv(monkeypatch):
    """The kernel path must not reach F.conv_transpose2d."""
    def boom(*a, **k):
        raise AssertionError('F.conv_transpose2d called on the kernel path')
    monkeypatch.setattr(torch.nn.functional, 'conv_transpose2d', boom)


def test_tconv_slice_in_slice_out(no_library_tconv):
    """(a) channels [16, 40) of a (2, 40, 5, 7) buffer, out into channels
    [5, 7) of an 8-wide sentinel buffer (odd out_off: 2-byte stores)."""
    ops = _ops()
    x, wgt, bias, ref = _tconv_problem(2, 24, 5, 7)
    gen = torch.Generator().manual_seed(1)
    buf = _ints(gen, (2, 40, 5, 7), -3, 3)
    buf[:, 16:40] = x
    buf = buf.to(_dev()).contiguous(memory_format=CL)
    out = _sentinel_buf((2, 8, 10, 14))
    ret = ops.conv_transpose2d_act(buf, wgt.to(_dev()), bias.to(_dev()),
                                   out=out, out_off=5, in_off=16, in_ch=24)
    assert ret.data_ptr() == out.data_ptr() and ret.shape == out.shape
    _assert_equal(out[:, 5:7], ref, 'tconv (a)')
    _assert_sentinel(out, 5, 7, 'tconv (a)')
    # the same slice without out=: a new channels_last tensor
    y = ops.conv_transpose2d_act(buf, wgt.to(_dev()), bias.to(_dev()),
                                 in_off=16, in_ch=24)
    assert y.is_contiguous(memory_format=CL)
    _assert_equal(y, ref, 'tconv (a) no out')


def test_tconv_mod_rounded_slice(no_library_tconv):
    """(b) conv_transpose2d_mod, in_channels=21 at in_off=16 of a 40-wide
    buffer: the kernel reads 24 channels, the packed weight's zero rows
    cancel the finite non-zero channels 37..39.  Then the weight changes in
    place and the cached packing must follow."""
    ops = _ops()
    x, wgt, bias, ref = _tconv_problem(2, 21, 5, 7)
    gen = torch.Generator().manual_seed(2)
    buf = _ints(gen, (2, 40, 5, 7), 1, 3)            # non-zero everywhere
    buf[:, 16:37] = x
    buf = buf.to(_dev()).contiguous(memory_format=CL)
    m = torch.nn.ConvTranspose2d(21, 2, 4, 2, 1)
    with torch.no_grad():
        m.weight.copy_(wgt)
        m.bias.copy_(bias)
    m = m.to(_dev(), torch.bfloat16)
    with torch.no_grad():
        y = ops.conv_transpose2d_mod(m, buf, in_off=16)
        assert y.is_contiguous(memory_format=CL)
        _assert_equal(y, ref, 'tconv (b)')
        assert m._vfa_tconv_wp[1].shape == (32, 24)
        m.weight.neg_().add_(1.0)                    # w -> 1 - w, in -1..3
        y2 = ops.conv_transpose2d_mod(m, buf, in_off=16)
    ref2 = _TCONV_REF(x.double(), 1.0 - wgt.double(), bias.double(), 2, 1)
    _assert_equal(y2, ref2, 'tconv (b) after weight update')
    with pytest.raises(ValueError):                  # rounded slice too wide
        ops.conv_transpose2d_mod(m, buf, in_off=24)


@pytest.mark.parametrize('shape', [
    (1, 568, 9, 8),     # (c) 18 K steps, K tail of 24, M = 72 < one block
    (3, 64, 17, 19),    # (d) M = 969: ragged, 8 blocks, image boundaries
    (2, 24, 1, 1),      # (e) H = W = 1: every output has one input pixel
    (1, 8, 3, 2),       # one K step, masked from 8 on
])
def test_tconv_pform_exact(no_library_tconv, shape):
    ops = _ops()
    x, wgt, bias, ref = _tconv_problem(*shape)
    xg = x.to(_dev()).contiguous(memory_format=CL)
    y = ops.conv_transpose2d_act(xg, wgt.to(_dev()), bias.to(_dev()))
    assert y.is_contiguous(memory_format=CL)
    _assert_equal(y, ref, f'tconv {shape}')
    # K_out = 1 and no bias
    w1 = wgt[:, :1].contiguous()
    y1 = ops.conv_transpose2d_act(xg, w1.to(_dev()))
    _assert_equal(y1, _TCONV_REF(x.double(), w1.double(), None, 2, 1),
                  f'tconv {shape} K_out=1')


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
def test_tconv_direct_small_c(no_library_tconv, layout):
    """(f) C = 2 on the direct kernel (the `upflow` path), from an NCHW and
    from a channels_last tensor; also into an odd-offset slice."""
    ops = _ops()
    x, wgt, bias, ref = _tconv_problem(2, 2, 5, 7)
    xg = x.to(_dev())
    if layout == 'channels_last':
        xg = xg.contiguous(memory_format=CL)
        assert not xg.is_contiguous()
    m = torch.nn.ConvTranspose2d(2, 2, 4, 2, 1)
    with torch.no_grad():
        m.weight.copy_(wgt)
        m.bias.copy_(bias)
    m = m.to(_dev(), torch.bfloat16)
    with torch.no_grad():
        y = ops.conv_transpose2d_mod(m, xg)
    assert y.is_contiguous(memory_format=CL)
    _assert_equal(y, ref, f'tconv direct {layout}')
    out = _sentinel_buf((2, 16, 10, 14))
    ops.conv_transpose2d_act(xg, wgt.to(_dev()), bias.to(_dev()), out=out,
                             out_off=13)
    _assert_equal(out[:, 13:15], ref, f'tconv direct {layout} slice')
    _assert_sentinel(out, 13, 15, f'tconv direct {layout}')


def test_tconv_out_sharing_storage_raises():
    """(g)"""
    ops = _ops()
    buf = torch.zeros(1, 16, 4, 4, dtype=torch.bfloat16,
                      device=_dev()).contiguous(memory_format=CL)
    wgt = torch.zeros(8, 2, 4, 4, dtype=torch.bfloat16, device=_dev())
    with pytest.raises(ValueError):
        ops.conv_transpose2d_act(buf, wgt, None, out=buf, out_off=8,
                                 in_off=0, in_ch=8)
    m = torch.nn.ConvTranspose2d(8, 2, 4, 2, 1).to(_dev(), torch.bfloat16)
    with pytest.raises(ValueError):
        ops.conv_transpose2d_mod(m, buf, out=buf[:, 8:], in_off=0)


def test_tconv_other_geometry_is_the_composition():
    """(h) a 3x3 ConvTranspose2d takes the composition and matches it."""
    ops = _ops()
    torch.manual_seed(3)
    m = torch.nn.ConvTranspose2d(16, 2, 3, 2, 1).to(_dev(), torch.bfloat16)
    x = torch.randn(2, 16, 5, 7, device=_dev(),
                    dtype=torch.bfloat16).contiguous(memory_format=CL)
    with torch.no_grad():
        assert torch.equal(ops.conv_transpose2d_mod(m, x), m(x))
        assert torch.equal(
            ops.conv_transpose2d_act(x, m.weight, m.bias, 2, 1),
            F.conv_transpose2d(x, m.weight, m.bias, 2, 1))


# --------------------------------------------------------------------- warp
@functools.lru_cache(maxsize=None)
def _warp_problem(shape, scale):
    """x integers in -8..8, flow multiples of 0.25 in -3..3 (samples leave
    the image on every side).  With scale 1 or 0.625 the bilinear weights
    are multiples of 2^-10, so every product and sum is exact in f32 and
    the exact result is a multiple of 2^-10.

    The reference is ops.bilinear_warp(x, flow*scale) in float64 on the CPU.
    Its grid normalisation ((y + fy) / (H - 1) * 2 - 1 and back) is not
    exact in float64: it leaves ~4e-15 of noise, which flips a bf16 rounding
    tie now and then.  The reference is therefore snapped to the nearest
    multiple of 2^-10 (asserted to move it by < 1e-12) before it is rounded
    to bf16 -- that IS the exact value."""
    from video_features_amd import ops
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(c * 100 + h * 10 + w)
    x = _ints(gen, shape, -8, 8)
    flow = (torch.randint(-12, 13, (b, 2, h, w), generator=gen).double()
            * 0.25).to(torch.bfloat16)
    # the small image cannot rely on chance: one sample strictly inside
    # (fractional in x and y), one outside
    flow[:, 0, 0, 0], flow[:, 1, 0, 0] = 0.25, 0.5
    flow[:, 0, -1, -1], flow[:, 1, -1, -1] = 3.0, -3.0
    ref =ops.bilinear_warp(x.double(), flow.double() * scale)
    snapped = torch.round(ref * 1024.0) / 1024.0
    assert (snapped - ref).abs().max().item() < 1e-12
    inside = (snapped != 0).any(dim=1)
    assert bool(inside.any()) and not bool(inside.all()), \
        'the case must have samples inside and outside the image'
    return x, flow, snapped


@pytest.mark.parametrize('flow_mode', ['plain', 'slice'])
@pytest.mark.parametrize('scale', [1.0, 0.625])
@pytest.mark.parametrize('shape', [(2, 32, 7, 9), (1, 8, 3, 2)])
def test_warp_nhwc_exact(shape, scale, flow_mode):
    ops = _ops()
    x, flow, ref = _warp_problem(shape, scale)
    b, c, h, w = shape
    xg = x.to(_dev()).contiguous(memory_format=CL)
    assert ops._cl_only(xg)
    if flow_mode == 'plain':
        fg = flow.to(_dev())
    else:
        # channels [13, 15) of a 16-wide channels_last buffer, read in place
        wide = _sentinel_buf((b, 16, h, w))
        wide[:, 13:15] = flow.to(_dev())
        fg = wide[:, 13:15]
        assert fg.data_ptr() == wide.data_ptr() + 13 * 2
    y = ops.bilinear_warp(xg, fg, scale=scale)
    assert y.is_contiguous(memory_format=CL) and y.shape == xg.shape
    _assert_equal(y, ref, f'warp {shape} scale={scale} flow={flow_mode}')


def test_warp_nchw_scale_keeps_the_nchw_kernel():
    """NCHW input: today's kernel and layout, scale multiplies the flow."""
    ops = _ops()
    x, flow, ref = _warp_problem((2, 32, 7, 9), 0.625)
    y = ops.bilinear_warp(x.to(_dev()), flow.to(_dev()), scale=0.625)
    assert y.is_contiguous()
    y0 = ops.bilinear_warp(x.to(_dev()), flow.to(_dev()) * 0.625)
    assert torch.equal(y, y0)


# -------------------------------------------------------------- correlation
@functools.lru_cache(maxsize=None)
def _corr_problem(shape, integers=True):
    from video_features_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    if integers:
        f1 = _ints(gen, shape, -2, 2)
        f2 = _ints(gen, shape, -2, 2)
        ref = ops._pwc_correlation_torch(f1.double(), f2.double(), 4)
    else:
        f1 = (torch.rand(shape, generator=gen) * 4 - 2).to(torch.bfloat16)
        f2 = (torch.rand(shape, generator=gen) * 4 - 2).to(torch.bfloat16)
        ref = ops._pwc_correlation_torch(f1.float(), f2.float(), 4)
    return f1, f2, ref


def _leaky_like_kernel(ref):
    """The kernel's epilogue: one f32 multiply by 0.1f of the negatives."""
    r = ref.float()
    return torch.where(r < 0, r * torch.tensor(0.1, dtype=torch.float32), r)


def _forbid_repack(monkeypatch, ops):
    def boom(*a, **k):
        raise AssertionError('NCHW repack path taken for channels_last input')
    monkeypatch.setattr(ops._ext, 'pwc_correlation', boom)


@pytest.mark.parametrize('mode', ['plain', 'slice'])
@pytest.mark.parametrize('act', ['none', 'leaky_relu'])
@pytest.mark.parametrize('hw', [(30, 37), (3, 5)])
@pytest.mark.parametrize('c', [32, 128])             # corr_tiled / corr_wave
def test_correlation_nhwc_exact(monkeypatch, c, hw, act, mode):
    """Integers in -2..2, 1/C a power of two: sums (|s| <= 4*C) and the mean
    are exact.  (3, 5) is smaller than the 9x9 window."""
    ops = _ops()
    shape = (2 if hw == (30, 37) else 1, c) + hw
    f1, f2, ref = _corr_problem(shape)
    if act == 'leaky_relu':
        ref = _leaky_like_kernel(ref).double()
    g1 = f1.to(_dev()).contiguous(memory_format=CL)
    g2 = f2.to(_dev()).contiguous(memory_format=CL)
    assert ops._cl_only(g1)
    _forbid_repack(monkeypatch, ops)
    b = shape[0]
    if mode == 'plain':
        y = ops.pwc_correlation(g1, g2, act=act)
        assert y.shape == (b, 81) + hw and y.dtype == torch.bfloat16
        assert y.is_contiguous(memory_format=CL)
    else:
        buf = _sentinel_buf((b, 104) + hw)
        ret = ops.pwc_correlation(g1, g2, out=buf, out_off=16, act=act)
        assert ret.data_ptr() == buf.data_ptr() and ret.shape == buf.shape
        _assert_sentinel(buf, 16, 97, f'corr C={c} {hw}')
        y = buf[:, 16:97]
    _assert_equal(y, ref, f'corr C={c} {hw} act={act} {mode}')


@pytest.mark.parametrize('mode', ['plain', 'slice'])
@pytest.mark.parametrize('shape', [(2, 196, 6, 5), (1, 196, 1, 1)])
def test_correlation_nhwc_c196(monkeypatch, shape, mode):
    """C = 196 (no multiple of 8) against the f32 torch composition at the
    3e-2 of test_gpu_ops.test_pwc_correlation.  (1, 196, 1, 1) is both
    channels_last- and NCHW-contiguous and keeps the NCHW kernels."""
    ops = _ops()
    f1, f2, ref = _corr_problem(shape, integers=False)
    ref = F.leaky_relu(ref, 0.1)
    g1 = f1.to(_dev()).contiguous(memory_format=CL)
    g2 = f2.to(_dev()).contiguous(memory_format=CL)
    if ops._cl_only(g1):
        _forbid_repack(monkeypatch, ops)
    b, _, h, w = shape
    if mode == 'plain':
        y = ops.pwc_correlation(g1, g2, act='leaky_relu')
        assert y.shape == (b, 81, h, w) and y.dtype == torch.bfloat16
        assert y.is_contiguous(memory_format=CL)
    else:
        buf = _sentinel_buf((b, 104, h, w))
        ops.pwc_correlation(g1, g2, out=buf, out_off=16, act='leaky_relu')
        _assert_sentinel(buf, 16, 97, f'corr {shape}')
        y = buf[:, 16:97]
    err = (y.float().cpu() - ref).abs().max().item()
    print(f'{shape} {mode}: max |err| {err:.3e}')
    assert err < 3e-2, (shape, err)


# ---------------------------------------------------------------- whole net
def _rel_l2(out, ref):
    return ((out.float().cpu() - ref).norm() / ref.norm()).item()


def test_whole_net_channels_last(monkeypatch):
    """PWCNet bf16 at (2, 3, 128, 192), levels 2x3 .. 32x48, against the CPU
    fp32 forward: relative L2 error at most twice the cat path's.  The
    forward reaches no F.conv2d / F.conv_transpose2d and no Conv2d /
    ConvTranspose2d module forward, and every feature argument and result
    of the warp and the cost volume is channels_last-contiguous.  With
    VFA_NO_PWC_NHWC=1 the earlier dense path runs and meets the same
    bound."""
    ops = _ops()
    from video_features_amd.models.pwc import PWCNet
    dev = _dev()
    torch.manual_seed(0)
    m = PWCNet().eval()
    x1 = (torch.rand(2, 3, 128, 192) * 255).to(torch.bfloat16).float()
    x2 = (torch.rand(2, 3, 128, 192) * 255).to(torch.bfloat16).float()
    with torch.no_grad():
        ref = m(x1, x2)
    mb = copy.deepcopy(m).to(dev, torch.bfloat16)
    g1, g2 = x1.to(dev, torch.bfloat16), x2.to(dev, torch.bfloat16)
    with torch.no_grad():
        mb.dense_buffer = False
        old = mb(g1, g2)
        mb.dense_buffer = None
    e_old = _rel_l2(old, ref)

    calls = {'F.conv2d': 0, 'F.conv_transpose2d': 0, 'Conv2d.forward': 0,
             'ConvTranspose2d.forward': 0}
    seen = {'warp': 0, 'corr': 0}
    not_cl = []

    def count(name, fn):
        def spy(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return spy

    def check(what, *tensors):
        for t in tensors:
            if not t.is_contiguous(memory_format=CL):
                not_cl.append((what, tuple(t.shape), t.stride()))

    warp0, corr0 = ops.bilinear_warp, ops.pwc_correlation

    def warp(x, flow, *a, **k):
        seen['warp'] += 1
        y = warp0(x, flow, *a, **k)
        check('warp', x, y)
        return y

    def corr(f1, f2, *a, **k):
        seen['corr'] += 1
        y = corr0(f1, f2, *a, **k)
        check('corr', f1, f2, y)
        return y

    def hook(name):
        def pre(mod, args):
            calls[name] += 1
        return pre

    def spied_forward():
        for k in calls:
            calls[k] = 0
        seen.update(warp=0, corr=0)
        del not_cl[:]
        with monkeypatch.context() as mp:
            mp.setattr(torch.nn.functional, 'conv2d',
                       count('F.conv2d', F.conv2d))
            mp.setattr(torch.nn.functional, 'conv_transpose2d',
                       count('F.conv_transpose2d', F.conv_transpose2d))
            mp.setattr(ops, 'bilinear_warp', warp)
            mp.setattr(ops, 'pwc_correlation', corr)
            handles = []
            for mod in mb.modules():
                if isinstance(mod, torch.nn.ConvTranspose2d):
                    handles.append(mod.register_forward_pre_hook(
                        hook('ConvTranspose2d.forward')))
                elif isinstance(mod, torch.nn.Conv2d):
                    handles.append(mod.register_forward_pre_hook(
                        hook('Conv2d.forward')))
            try:
                with torch.no_grad():
                    out = mb(g1, g2)
            finally:
                for hd in handles:
                    hd.remove()
        torch.cuda.synchronize()
        return out

    new = spied_forward()
    assert new.shape == ref.shape == (2, 2, 128, 192)
    assert torch.isfinite(new.float()).all()
    e_new = _rel_l2(new, ref)
    print(f'relative L2 error vs CPU fp32: channels_last e_new={e_new:.4e}, '
          f'cat path e_old={e_old:.4e}; calls {calls}; {seen}')
    assert all(v == 0 for v in calls.values()), calls
    assert seen == {'warp': 4, 'corr': 5}, seen
    assert not not_cl, not_cl
    assert e_new <= 2.0 * e_old, (e_new, e_old)

    monkeypatch.setenv('VFA_NO_PWC_NHWC', '1')
    flagged = spied_forward()
    e_flag = _rel_l2(flagged, ref)
    print(f'VFA_NO_PWC_NHWC=1: e={e_flag:.4e}; calls {calls}')
    assert calls['ConvTranspose2d.forward'] == 8, calls   # the earlier path
    assert torch.isfinite(flagged.float()).all()
    assert e_flag <= 2.0 * e_old, (e_flag, e_old)
