"""GPU tests of the PWC dense-buffer decoder: the correlation kernels'
slice-write mode and the whole net in bf16 against the cat path."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = -12352.0          # exact in bf16


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    return ops


@pytest.mark.parametrize('c', [32, 196])      # corr_tiled / corr_wave
def test_correlation_slice_write(c):
    """leaky_relu(0.1) of the cost volume as bf16 into channels [16, 97) of
    a (2, 104, 30, 37) channels_last buffer, at the bf16 tolerance of
    test_gpu_ops.test_pwc_correlation (3e-2); the other channels keep the
    sentinel bit for bit."""
    ops = _ops()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    f1 = torch.randn(2, c, 30, 37, device=dev, dtype=torch.bfloat16)
    f2 = torch.randn(2, c, 30, 37, device=dev, dtype=torch.bfloat16)
    buf = torch.full((2, 104, 30, 37), SENTINEL, dtype=torch.bfloat16,
                     device=dev).contiguous(memory_format=torch.channels_last)
    ret = ops.pwc_correlation(f1, f2, out=buf, out_off=16, act='leaky_relu')
    assert ret.data_ptr() == buf.data_ptr() and ret.shape == buf.shape
    assert buf.is_contiguous(memory_format=torch.channels_last)
    ref = F.leaky_relu(
        ops._pwc_correlation_torch(f1.float(), f2.float(), 4), 0.1)
    err = (buf[:, 16:97].float() - ref).abs().max().item()
    print(f'C={c}: max |err| {err:.3e}')
    assert err < 3e-2, (c, err)
    sent = torch.tensor(SENTINEL, dtype=torch.bfloat16).view(torch.int16)
    bits = buf.cpu().view(torch.int16)
    for lo, hi in ((0, 16), (97, 104)):
        nbad = int((bits[:, lo:hi] != sent).sum())
        assert nbad == 0, f'{nbad} elements of channels [{lo}, {hi}) changed'
    # act='none' without out= still returns the (B, 81, H, W) tensor
    plain = ops.pwc_correlation(f1, f2)
    assert plain.shape == (2, 81, 30, 37) and plain.dtype == torch.bfloat16
    got = buf[:, 16:97].float()
    want = F.leaky_relu(plain.float(), 0.1)
    assert (got - want).abs().max().item() < 3e-2


def _rel_l2(out, ref):
    return ((out.float().cpu() - ref).norm() / ref.norm()).item()


def test_whole_net_dense_buffer_vs_cat_path(monkeypatch):
    """PWCNet bf16 at (2, 3, 128, 192) against the CPU fp32 forward: the
    dense-buffer path's relative L2 error e_new must not exceed twice the
    cat path's e_old (both round to bf16 once per layer with f32
    accumulation, so they should be level; the factor 2 covers
    single-sample noise).  The dense-buffer forward must reach neither
    F.conv2d nor nn.Conv2d.forward."""
    _ops()
    from video_features_amd.models.pwc import PWCNet
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    m = PWCNet().eval()
    # pixel values exact in bf16, so all three forwards see the same input
    x1 = (torch.rand(2, 3, 128, 192) * 255).to(torch.bfloat16).float()
    x2 = (torch.rand(2, 3, 128, 192) * 255).to(torch.bfloat16).float()
    with torch.no_grad():
        ref = m(x1, x2)
    mb = copy.deepcopy(m).to(dev, torch.bfloat16)
    g1, g2 = x1.to(dev, torch.bfloat16), x2.to(dev, torch.bfloat16)
    assert mb.dense_buffer is None

    with torch.no_grad():
        mb.dense_buffer = False
        old = mb(g1, g2)

    calls = {'F.conv2d': 0, 'Conv2d.forward': 0}
    orig = F.conv2d

    def spy(*a, **k):
        calls['F.conv2d'] += 1
        return orig(*a, **k)

    def hook(mod, args):
        calls['Conv2d.forward'] += 1

    monkeypatch.setattr(torch.nn.functional, 'conv2d', spy)
    handles = [mod.register_forward_pre_hook(hook) for mod in mb.modules()
               if isinstance(mod, torch.nn.Conv2d)]
    try:
        with torch.no_grad():
            mb.dense_buffer = True
            new = mb(g1, g2)
    finally:
        for hd in handles:
            hd.remove()
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert new.shape == old.shape == ref.shape == (2, 2, 128, 192)
    assert torch.isfinite(new.float()).all()
    e_old, e_new = _rel_l2(old, ref), _rel_l2(new, ref)
    print(f'relative L2 error vs CPU fp32: dense-buffer e_new={e_new:.4e}, '
          f'cat path e_old={e_old:.4e}; conv calls {calls}')
    assert calls == {'F.conv2d': 0, 'Conv2d.forward': 0}, calls
    assert e_new <= 2.0 * e_old, (e_new, e_old)
