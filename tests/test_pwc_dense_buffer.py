"""CPU tests of the PWC dense-buffer path and of conv2d_act's dilation /
slice arguments.

On the CPU the dense-buffer path is a pure-torch re-expression of the cat
path (ops.conv2d_mod and ops.pwc_correlation compose F.conv2d there), so in
float64 the two differ by re-association noise only (~1e-13 relative); a
wrong slice offset or channel order is an O(1) error."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops
from video_features_amd.models.pwc import Decoder, PWCNet


@pytest.fixture(scope='module')
def net_and_input():
    torch.manual_seed(0)
    net = PWCNet().double().eval()
    gen = torch.Generator().manual_seed(1)
    im1 = torch.rand(1, 3, 64, 96, generator=gen, dtype=torch.float64) * 255
    im2 = torch.rand(1, 3, 64, 96, generator=gen, dtype=torch.float64) * 255
    return net, im1, im2


def test_dense_buffer_matches_cat_path_float64(net_and_input):
    net, im1, im2 = net_and_input
    with torch.no_grad():
        net.dense_buffer = False
        ref = net(im1, im2)
        net.dense_buffer = True
        got = net(im1, im2)
    net.dense_buffer = None
    assert got.shape == ref.shape == (1, 2, 64, 96)
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f'max |delta| {err:.3e}, max |ref| {scale:.3e}')
    assert scale > 0
    assert err <= 1e-9 * scale


def test_dense_buffer_selection(net_and_input, monkeypatch):
    """None is automatic (off on the CPU), True / False force, and
    VFA_NO_PWC_CL=1 overrides a forced True."""
    net, im1, _ = net_and_input
    x = im1
    assert PWCNet.__init__.__defaults__ == (None,)
    net.dense_buffer = None
    assert net._dense(x) is False
    net.dense_buffer = True
    assert net._dense(x) is True
    monkeypatch.setenv('VFA_NO_PWC_CL', '1')
    assert net._dense(x) is False
    monkeypatch.setenv('VFA_NO_PWC_CL', '0')
    assert net._dense(x) is True
    net.dense_buffer = None


def test_dense_buffer_layout():
    """Write offsets 0, 32, 96, 192, 320 and corr at 448, every conv
    reading the suffix behind its own slice."""
    dec = Decoder(96)
    assert dec.DENSE_OFF == [320, 192, 96, 32, 0] and dec.CORR_OFF == 448
    for conv, off in zip(dec.convs, dec.DENSE_OFF):
        k, c = conv[0].out_channels, conv[0].in_channels
        assert off % 8 == 0 and off + k + c == dec.out_channels, off


@pytest.mark.parametrize('dilation,stride,padding', [
    (1, 1, 1), (2, 1, 2), ((2, 3), (2, 1), (2, 3)), (4, 1, 0)])
def test_conv2d_act_dilation_and_slices_cpu(dilation, stride, padding):
    gen = torch.Generator().manual_seed(3)
    buf = torch.randn(2, 40, 13, 11, generator=gen, dtype=torch.float64)
    w = torch.randn(16, 24, 3, 3, generator=gen, dtype=torch.float64)
    bias = torch.randn(16, generator=gen, dtype=torch.float64)
    ref = F.leaky_relu(F.conv2d(buf[:, 16:40], w, bias, stride, padding,
                                dilation), 0.1)
    got = ops.conv2d_act(buf, w, bias, stride, padding, 'leaky_relu',
                         dilation=dilation, in_off=16, in_ch=24)
    assert torch.equal(got, ref)
    # out= a wider buffer; only the slice changes
    out = torch.full((2, 32) + tuple(ref.shape[2:]), 7.0, dtype=torch.float64)
    ret = ops.conv2d_act(buf, w, bias, stride, padding, 'leaky_relu',
                         out=out, out_off=8, dilation=dilation, in_off=16,
                         in_ch=24)
    assert ret is out
    assert torch.equal(out[:, 8:24], ref)
    assert bool((out[:, :8] == 7.0).all()) and bool((out[:, 24:] == 7.0).all())
    # no slice: plain dilation
    ref2 = F.conv2d(buf, torch.cat([w, w[:, :16]], 1), bias, stride, padding,
                    dilation)
    got2 = ops.conv2d_act(buf, torch.cat([w, w[:, :16]], 1), bias, stride,
                          padding, dilation=dilation)
    assert torch.equal(got2, ref2)


def test_conv2d_act_in_place_dense_step_cpu():
    """x = cat([conv(x), x], 1) as one in-place call on the buffer."""
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(1, 24, 9, 7, generator=gen, dtype=torch.float64)
    w = torch.randn(16, 24, 3, 3, generator=gen, dtype=torch.float64)
    ref = torch.cat([F.conv2d(x, w, None, 1, 1), x], 1)
    buf = torch.zeros(1, 40, 9, 7, dtype=torch.float64)
    buf[:, 16:] = x
    ops.conv2d_act(buf, w, None, 1, 1, out=buf, out_off=0, in_off=16,
                   in_ch=24)
    assert torch.equal(buf, ref)


def test_conv2d_mod_slice_cpu():
    """conv2d_mod with in_off reads conv.in_channels channels (no rounding
    on the eager path) and honours the module's dilation."""
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(21, 16, 3, padding=2, dilation=2).double()
    buf = torch.full((2, 40, 10, 12), 3.0, dtype=torch.float64)
    x = torch.randn(2, 21, 10, 12, dtype=torch.float64)
    buf[:, 16:37] = x
    with torch.no_grad():
        ref = F.leaky_relu(conv(x), 0.1)
        ops.conv2d_mod(conv, buf, 'leaky_relu', out=buf, out_off=0,
                       in_off=16)
    assert torch.equal(buf[:, :16], ref)
    assert torch.equal(buf[:, 16:37], x) and bool((buf[:, 37:] == 3.0).all())


def test_pwc_correlation_out_slice_cpu():
    gen = torch.Generator().manual_seed(6)
    f1 = torch.randn(2, 8, 9, 10, generator=gen)
    f2 = torch.randn(2, 8, 9, 10, generator=gen)
    ref = F.leaky_relu(ops._pwc_correlation_torch(f1, f2, 4), 0.1)
    assert torch.equal(ops.pwc_correlation(f1, f2, act='leaky_relu'), ref)
    out = torch.full((2, 104, 9, 10), -1.0)
    ret = ops.pwc_correlation(f1, f2, out=out, out_off=16, act='leaky_relu')
    assert ret is out and torch.equal(out[:, 16:97], ref)
    assert bool((out[:, :16] == -1.0).all()) and bool((out[:, 97:] == -1.0).all())
    with pytest.raises(ValueError):
        ops.pwc_correlation(f1, f2, act='relu')
