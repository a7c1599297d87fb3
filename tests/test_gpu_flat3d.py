"""Exact-arithmetic GPU tests of ``conv3d_flat`` (models/_flat3d.py): the
geometries of tests/test_flat3d_conv.py on the kernels the models run, and
the whole-model rule of ``VFA_FORCE_TORCH_OPS``.

Method (that of test_gpu_conv_exact.py, for the two roundings of this
path).  x and w are drawn from {-1, 0, 1} and the bias from -8..8, in bf16,
O = 16, B = 2, channels_last, so the channel pad is active for C = 3, 2, 9.
Each tap's conv sum is an integer of magnitude <= 7*7*3 + 8 = 155 <= 256:
exact in bf16 when the merged conv stores it.  tmerge.hip adds the taps in
f32 (|sum| <= 7*155 < 2^24), so the merged value is exact and rounded to
bf16 once — as the float64 ``F.conv3d`` reference is.  The comparison is
torch.equal: one misplaced tap, pad cell or stride fails it."""
import pytest
import torch

from test_flat3d_conv import GEOMETRIES, conv3d_ref, geometry_pads

pytestmark = pytest.mark.gpu

O, B = 16, 2


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@pytest.mark.parametrize('act', ['none', 'relu'])
@pytest.mark.parametrize('kernel,stride,c,t,hw,same', GEOMETRIES)
def test_conv3d_flat_exact(kernel, stride, c, t, hw, same, act):
    from video_features_amd import ops
    from video_features_amd.models._flat3d import (conv3d_flat, flatten_time,
                                                   unflatten_time)
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(sum(kernel) * 100 + c * 10 + t)
    x = _ints(gen, (B, c, t, hw, hw), -1, 1)
    conv = torch.nn.Conv3d(c, O, kernel, stride)
    with torch.no_grad():
        conv.weight.copy_(_ints(gen, conv.weight.shape, -1, 1))
        conv.bias.copy_(_ints(gen, (O,), -8, 8))
    pads = geometry_pads(kernel, stride, t, hw, same)
    ref = conv3d_ref(x, conv.weight.detach().double(),
                     conv.bias.detach().double(), stride, pads)
    if act == 'relu':
        ref = ref.relu()
    conv = conv.to(dev, torch.bfloat16)
    xf = flatten_time(x.to(dev, torch.bfloat16))
    assert ops.native_ready(xf, channels_last=True)
    with torch.no_grad():
        yf = conv3d_flat(conv, xf, B, pads=pads, act=act)
    assert yf.dtype == torch.bfloat16
    assert yf.is_contiguous(memory_format=torch.channels_last)
    assert conv._vfa_flat[1][0].shape[1] == (c + 7) // 8 * 8    # channel pad
    out = unflatten_time(yf, B).cpu()
    want = ref.to(torch.bfloat16)
    assert out.shape == want.shape
    bad = out != want
    assert not bad.any(), (
        f'{int(bad.sum())} of {bad.numel()} elements wrong, first at '
        f'(b, o, t, y, x) = {bad.nonzero()[0].tolist()}')


def test_r21d_force_torch_ops_takes_the_eager_path(monkeypatch):
    """VFA_FORCE_TORCH_OPS=1: the whole model runs its torch compositions
    (no channel-padded weights, no in-tree kernels) and still meets the
    bound of test_r21d_gpu_bf16 against the CPU fp32 forward."""
    from video_features_amd.models.r21d import R2Plus1D18
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = R2Plus1D18().eval()
    x = torch.randn(1, 3, 4, 32, 32)
    monkeypatch.setenv('VFA_FORCE_TORCH_OPS', '1')
    with torch.no_grad():
        ref = m.forward_features(x)
        out = m.to(dev, torch.bfloat16) \
            .forward_features(x.to(dev, torch.bfloat16)).float().cpu()
    assert out.shape == (1, 512)
    assert torch.isfinite(out).all()
    # stem conv C = 3 and its 45 mid-planes: not padded to 8 on this path
    assert m.stem[0]._vfa_flat[1][0].shape[1] == 3
    assert m.stem[3]._vfa_flat[1][0].shape[1] == 45
    cos = torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(),
                                                dim=0).item()
    print(f'cos {cos:.5f}')
    assert cos > 0.98
