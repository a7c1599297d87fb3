"""GPU numerics: the implicit-GEMM conv2d HIP kernel (conv2d.hip) vs plain
fp32 PyTorch conv2d, over the hot shapes of the ResNet / RAFT / I3D /
VGGish conv stacks."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops

pytestmark = pytest.mark.gpu


def _hip():
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    return ops


def _run(b, c, h, w, k, kh, kw, stride, pad, act='none', use_res=False,
         tol=0.08):
    """max|err| / max(max|ref|, 1) < tol and, as in test_gpu_gemm.py (same
    arithmetic: bf16 I/O, fp32 accumulation), mean|err| / mean|ref| < 5e-3.
    The fp32 reference merely rounded to bf16 sits at 1.40e-3 .. 1.41e-3
    on this data (CPU, ten of the shapes below, every activation and the
    residual), so the mean bound leaves a 3.5x margin over output
    rounding."""
    _hip()
    torch.manual_seed(0)
    dev = 'cuda:0'
    x = (torch.randn(b, c, h, w, device=dev) * 0.5).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    wgt = (torch.randn(k, c, kh, kw, device=dev) *
           (2.0 / (c * kh * kw)) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(k, device=dev).to(torch.bfloat16)
    oh = (h + 2 * pad[0] - kh) // stride + 1
    ow = (w + 2 * pad[1] - kw) // stride + 1
    res = (torch.randn(b, k, oh, ow, device=dev) * 0.5).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last) if use_res else None

    out = ops.conv2d_act(x, wgt, bias, stride, pad, act, res)
    assert out.is_contiguous(memory_format=torch.channels_last)

    ref = F.conv2d(x.float(), wgt.float(), bias.float(), stride, pad)
    if res is not None:
        ref = ref + res.float()
    if act == 'relu':
        ref = F.relu(ref)
    elif act == 'leaky_relu':
        ref = F.leaky_relu(ref, 0.1)
    assert out.shape == ref.shape
    diff = (out.float() - ref).abs()
    scale = ref.abs().max().clamp(min=1.0)
    mean = (diff.mean() / ref.abs().mean().clamp_min(1e-6)).item()
    print(f'{(b, c, h, w, k, kh, kw, stride, pad)} {act} res={use_res}: '
          f'max-rel {(diff / scale).max().item():.3e} mean-rel {mean:.3e}')
    assert (diff / scale).max().item() < tol, \
        (diff.max().item(), scale.item())
    assert mean < 5e-3, mean


# ---- ResNet-50 bottleneck 3x3 shapes (stride 1 and the stride-2 stage
# transitions), reference torchvision geometry
@pytest.mark.parametrize('c,hw,k,stride', [
    (64, 56, 64, 1), (128, 28, 128, 1), (256, 14, 256, 1),
    (512, 7, 512, 1), (128, 56, 128, 2), (256, 28, 256, 2),
    (512, 14, 512, 2),
])
def test_conv3x3_resnet_shapes(c, hw, k, stride):
    _run(4, c, hw, hw, k, 3, 3, stride, (1, 1))


# ---- RAFT encoder (instance-norm net: 64/96/128 channels at 1/2..1/8) —
# includes the C=96 ragged-K case (Kr = 864, not a multiple of 64)
@pytest.mark.parametrize('c,hw,k,stride', [
    (64, 56, 64, 1), (64, 56, 96, 2), (96, 28, 96, 1), (96, 28, 128, 2),
    (128, 28, 128, 1),
])
def test_conv3x3_raft_shapes(c, hw, k, stride):
    _run(2, c, hw, hw, k, 3, 3, stride, (1, 1))


# ---- RAFT SepConvGRU 1x5 / 5x1 merged convs
def test_conv1x5_gru():
    _run(2, 384, 28, 28, 256, 1, 5, 1, (0, 2))


def test_conv5x1_gru():
    _run(2, 384, 28, 28, 256, 5, 1, 1, (2, 0))


# ---- I3D merged-tap convs on the flattened-time path: 3x3 with
# K_out = 3*O (temporal taps concatenated)
def test_conv3x3_i3d_merged_taps():
    _run(8, 192, 28, 28, 288, 3, 3, 1, (1, 1))


# ---- VGGish audio conv stack (96x64 mel input downscales)
@pytest.mark.parametrize('c,h,w,k', [
    (64, 48, 32, 128), (128, 24, 16, 256), (256, 24, 16, 256),
    (512, 12, 8, 512),
])
def test_conv3x3_vggish_shapes(c, h, w, k):
    _run(4, c, h, w, k, 3, 3, 1, (1, 1))


# ---- fused epilogues
def test_conv_relu_epilogue():
    _run(4, 64, 28, 28, 64, 3, 3, 1, (1, 1), act='relu')


def test_conv_leaky_relu_epilogue():
    _run(2, 64, 28, 28, 96, 3, 3, 1, (1, 1), act='leaky_relu')


def test_conv_residual_relu_epilogue():
    """BasicBlock tail: conv + residual add + ReLU in ONE kernel."""
    _run(4, 64, 28, 28, 64, 3, 3, 1, (1, 1), act='relu', use_res=True)


# ---- no padding (VALID) and 7x7
def test_conv3x3_no_pad():
    _run(2, 64, 30, 30, 64, 3, 3, 1, (0, 0))


def test_conv7x7_stride2():
    _run(2, 64, 56, 56, 128, 7, 7, 2, (3, 3))


# ---- odd M edges (B*OH*OW far from a tile multiple)
def test_conv_ragged_m():
    _run(1, 64, 13, 11, 64, 3, 3, 1, (1, 1))


def test_conv_big_tile_path():
    """M = 6272, N = 256: large, but the cost model gives this shape to
    the 128x128 tile (49 x 2 tiles beat 25 padded 256x256 ones)."""
    _hip()
    assert tuple(ops._ext.conv2d_tile(8 * 28 * 28, 256)) == (128, 128)
    _run(8, 256, 28, 28, 256, 3, 3, 1, (1, 1))


def test_conv_256x256_tile():
    """M = 4096, N = 256: 16 full tiles of the 256x256 (8-wave) kernel."""
    _hip()
    assert tuple(ops._ext.conv2d_tile(64 * 64, 256)) == (256, 256)
    _run(1, 64, 64, 64, 256, 3, 3, 1, (1, 1))


def test_pad_matches_torch():
    _hip()
    x = torch.randn(2, 16, 9, 11, device='cuda:0').to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    # exercised through conv2d_act pad path vs F.conv2d's implicit pad
    _run(2, 16, 9, 11, 24, 3, 3, 1, (1, 1))


# ---- ResNet bottleneck DOWNSAMPLE 1x1 convs (stride 2 at the stage
# transitions, stride 1 at layer1.0) — routed in-tree by
# models/resnet.py via conv2d_mod (reference pulls these from
# torchvision, models/resnet/extract_resnet.py:54-67)
@pytest.mark.parametrize('c,hw,k,stride', [
    (64, 56, 256, 1), (256, 56, 512, 2), (512, 28, 1024, 2),
    (1024, 14, 2048, 2),
])
def test_conv1x1_downsample_shapes(c, hw, k, stride):
    _run(4, c, hw, hw, k, 1, 1, stride, (0, 0))


def test_conv2d_mod_downsample_route():
    """conv2d_mod on a folded downsample [conv, Identity] matches the
    eager nn.Sequential on GPU (the Bottleneck fused path's idt)."""
    _hip()
    torch.manual_seed(0)
    dev = 'cuda:0'
    conv = torch.nn.Conv2d(256, 512, 1, 2, 0).to(dev, torch.bfloat16)
    x = (torch.randn(2, 256, 56, 56, device=dev) * 0.5) \
        .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    out = ops.conv2d_act(x, conv.weight, conv.bias, 2, 0, 'none')
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), 2, 0)
    assert ((out.float() - ref).abs() / ref.abs().max()).max().item() < 0.08


@pytest.mark.parametrize('padding', [1, 0])
def test_conv2d_mod_1x1_padding(padding, monkeypatch):
    """A 1x1 module conv with padding keeps its border (the implicit-GEMM
    kernel; the 1x1 -> GEMM shortcut is for unpadded convs only), and
    without padding still takes the GEMM.  Small-integer operands: every
    product and sum is exact, so the result equals the float64 conv."""
    _hip()
    dev = 'cuda:0'
    gen = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(8, 16, 1, padding=padding)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-3, 4, (16, 8, 1, 1), generator=gen))
        conv.bias.copy_(torch.randint(-3, 4, (16,), generator=gen))
    x = torch.randint(-4, 5, (1, 8, 4, 4), generator=gen).double()
    ref = F.conv2d(x, conv.weight.double(), conv.bias.double(),
                   padding=padding).to(torch.bfloat16)
    gemm_calls = []
    real = ops.conv1x1_act
    monkeypatch.setattr(ops, 'conv1x1_act', lambda *a, **k: (
        gemm_calls.append(1), real(*a, **k))[1])
    conv = conv.to(dev, torch.bfloat16)
    xg = x.to(dev, torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    out = ops.conv2d_mod(conv, xg)
    assert out.shape == (1, 16, 4 + 2 * padding, 4 + 2 * padding)
    assert len(gemm_calls) == (0 if padding else 1)
    assert torch.equal(out.cpu(), ref)
