"""CPU tests of the model-layer helpers: ``conv3d_flat`` (the Conv3d →
conv2d + temporal merge decomposition of models/_flat3d.py) against
``F.conv3d``, the derived-parameter cache ``ops.derived`` and the path gate
``ops.native_ready``.

``conv3d_flat`` in float64 against ``conv(F.pad(x, pads))``: the two differ
only in summation order (measured worst 1.6e-15 at |ref| ~ 1.5 over these
cases), a misplaced tap, pad or stride by O(0.1); the bound is 1e-12."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops
from video_features_amd.models._flat3d import (conv3d_flat, flatten_time,
                                               unflatten_time)
from video_features_amd.models.i3d import _same_pad_1d

O, B = 5, 2

# (kernel, stride, C_in, T, H = W, TF-SAME pads instead of symmetric k // 2)
GEOMETRIES = [
    ((7, 7, 7), (2, 2, 2), 3, 4, 9, True),      # the I3D stem
    ((7, 7, 7), (2, 2, 2), 2, 5, 8, True),
    ((7, 7, 7), (2, 2, 2), 3, 2, 8, True),
    ((3, 3, 3), (1, 1, 1), 8, 3, 5, False),
    ((3, 3, 3), (1, 1, 1), 8, 1, 5, False),
    ((3, 1, 1), (2, 1, 1), 9, 5, 4, False),
    ((3, 1, 1), (1, 1, 1), 9, 2, 4, False),
    ((1, 3, 3), (1, 2, 2), 8, 3, 7, False),
    ((1, 7, 7), (1, 2, 2), 3, 3, 9, False),
    ((1, 1, 1), (2, 2, 2), 8, 5, 6, False),
    ((1, 1, 1), (1, 1, 1), 8, 1, 3, False),
]


def geometry_pads(kernel, stride, t, hw, same):
    """((t0, t1), (h0, h1), (w0, w1)) of one GEOMETRIES row."""
    if same:
        return tuple(_same_pad_1d(n, k, s)
                     for n, k, s in zip((t, hw, hw), kernel, stride))
    return tuple((k // 2, k // 2) for k in kernel)


def conv3d_ref(x, weight, bias, stride, pads):
    (t0, t1), (h0, h1), (w0, w1) = pads
    return F.conv3d(F.pad(x, (w0, w1, h0, h1, t0, t1)), weight, bias, stride)


@pytest.mark.parametrize('pad_channels', [False, True])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('kernel,stride,c,t,hw,same', GEOMETRIES)
def test_conv3d_flat_matches_conv3d(kernel, stride, c, t, hw, same, bias,
                                    pad_channels):
    torch.manual_seed(sum(kernel) * 100 + c * 10 + t)
    conv = torch.nn.Conv3d(c, O, kernel, stride, bias=bias).double()
    x = torch.randn(B, c, t, hw, hw, dtype=torch.float64)
    pads = geometry_pads(kernel, stride, t, hw, same)
    with torch.no_grad():
        ref = conv3d_ref(x, conv.weight, conv.bias, stride, pads)
        out = unflatten_time(
            conv3d_flat(conv, flatten_time(x), B, pads=pads,
                        pad_channels=pad_channels), B)
    assert conv._vfa_flat[1][0].shape[1] == \
        ((c + 7) // 8 * 8 if pad_channels else c)
    assert out.shape == ref.shape
    err = (out - ref).abs().max().item()
    print(f'max |diff| {err:.2e} at max |ref| {ref.abs().max().item():.2f}')
    torch.testing.assert_close(out, ref, atol=1e-12, rtol=0)


def test_conv3d_flat_default_pads_and_relu():
    """Without ``pads`` the conv's own padding is used; act='relu' applies
    to the merged (kt > 1) and to the single-conv (kt == 1) result."""
    torch.manual_seed(0)
    for kernel, pad in (((3, 3, 3), (1, 1, 1)), ((1, 3, 3), (0, 1, 1))):
        conv = torch.nn.Conv3d(4, O, kernel, 1, pad).double()
        x = torch.randn(B, 4, 3, 5, 5, dtype=torch.float64)
        with torch.no_grad():
            out = unflatten_time(
                conv3d_flat(conv, flatten_time(x), B, act='relu'), B)
            torch.testing.assert_close(out, conv(x).relu(), atol=1e-12,
                                       rtol=0)


def test_conv3d_flat_rejects_invalid_bias_tap():
    """The bias rides tap kt // 2; where that tap reads temporal padding at
    some output position the decomposition would drop the bias there."""
    conv = torch.nn.Conv3d(4, O, (3, 1, 1))
    xf = flatten_time(torch.randn(B, 4, 4, 3, 3))
    with pytest.raises(ValueError, match='tap'):
        conv3d_flat(conv, xf, B, pads=((2, 0), (0, 0), (0, 0)))
    with pytest.raises(ValueError, match='tap'):
        conv3d_flat(conv, xf, B, pads=((0, 2), (0, 0), (0, 0)))
    conv3d_flat(conv, xf, B, pads=((1, 1), (0, 0), (0, 0)))


def _params():
    return [torch.nn.Parameter(torch.randn(3)) for _ in range(3)]


def test_derived_rebuilds_on_any_param_dtype_and_extra():
    mod, ps = torch.nn.Module(), _params()
    calls = []

    def get(params, extra=None):
        def make():
            calls.append(extra)
            return sum(p.detach().double() for p in params)
        return ops.derived(mod, '_vfa_sum', params, make, extra)

    first = get(ps)
    assert get(ps) is first and len(calls) == 1          # cached
    for p in ps:                       # an in-place write to any one param
        with torch.no_grad():
            p.mul_(2.0)
        n = len(calls)
        v = get(ps)
        assert len(calls) == n + 1
        torch.testing.assert_close(v, sum(q.detach().double() for q in ps))
        assert get(ps) is v
    n = len(calls)
    ps16 = [ps[0].to(torch.float16)] + ps[1:]             # .to(dtype)
    get(ps16)
    assert len(calls) == n + 1
    get(ps16, extra=8)                                    # extra changes
    assert len(calls) == n + 2
    assert get(ps16, extra=8) is mod._vfa_sum[1] and len(calls) == n + 2
    # None entries are skipped, not an error
    assert ops.derived(mod, '_vfa_none', (ps[0], None), lambda: 7) == 7


def test_derived_value_is_detached_with_autograd_on():
    """make() runs under no_grad even when the caller does not: the cached
    tensor must not hang on a graph.  conv2d_mod's padded weight is the
    cache that was built with autograd on."""
    conv = torch.nn.Conv2d(3, 16, 3, 1, 1)
    assert conv.weight.requires_grad and torch.is_grad_enabled()
    v = ops.derived(conv, '_vfa_twice', (conv.weight,),
                    lambda: conv.weight * 2.0)
    assert not v.requires_grad and v.grad_fn is None
    ps = _params()
    fold = ops.derived(conv, '_vfa_cat', ps, lambda: torch.cat(ps))
    assert not fold.requires_grad


def test_native_ready_false_off_the_bf16_gpu_path(monkeypatch):
    for x in (torch.zeros(1, 8, 2, 2), torch.zeros(4, dtype=torch.bfloat16),
              torch.zeros(1, 8, 2, 2, dtype=torch.bfloat16)):
        assert ops.native_ready(x) is False
        # never raises, whatever the rank, also when asked about the layout
        assert ops.native_ready(x, knob='VFA_NO_CONV',
                                channels_last=True) is False
    monkeypatch.setenv('VFA_FORCE_TORCH_OPS', '1')
    assert ops.native_ready(torch.zeros(1, 8, 2, 2)) is False
    assert ops.env_flag('VFA_FORCE_TORCH_OPS')
    monkeypatch.setenv('VFA_FORCE_TORCH_OPS', '0')
    assert not ops.env_flag('VFA_FORCE_TORCH_OPS')
