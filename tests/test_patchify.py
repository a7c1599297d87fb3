"""ops.patchify: the patch gather in front of a ViT's patch-embedding GEMM.
Pure data movement, so every check is bit-exact against the reshape /
permute composition it replaces."""
import pytest
import torch

from video_features_amd import ops

SHAPES = [(2, 3, 64, 96, 32), (3, 3, 32, 48, 16), (1, 1, 32, 32, 32)]


def compose(x, p):
    t, c, h, w = x.shape
    gy, gx = h // p, w // p
    xp = x.reshape(t, c, gy, p, gx, p).permute(0, 2, 4, 1, 3, 5)
    return xp.reshape(t, gy * gx, c * p * p)


def make(shape, dtype, device):
    """Every element distinct (up to the dtype's range), so a misplaced
    element cannot hide behind an equal neighbour."""
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.bfloat16:
        # bit patterns 0 .. n-1 folded into the finite positive bf16 range
        bits = torch.arange(n, dtype=torch.int32, device=device) % 0x7F00
        return bits.to(torch.int16).view(torch.bfloat16).reshape(shape)
    return torch.arange(n, dtype=dtype, device=device).reshape(shape)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('shape', SHAPES)
def test_patchify_cpu(shape, dtype):
    *dims, p = shape
    x = make(dims, dtype, 'cpu')
    y = ops.patchify(x, p)
    t, c, h, w = dims
    assert y.shape == (t, (h // p) * (w // p), c * p * p)
    assert torch.equal(y, compose(x, p))


def test_patchify_rejects_ragged():
    with pytest.raises(ValueError):
        ops.patchify(torch.zeros(1, 3, 30, 32), 16)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('shape', SHAPES)
def test_patchify_gpu(shape, dtype):
    *dims, p = shape
    x = make(dims, dtype, 'cuda:0')
    y = ops.patchify(x, p)
    assert y.is_contiguous()
    assert torch.equal(y, compose(x, p))


@pytest.mark.gpu
def test_patchify_gpu_many_frames():
    """The launch has about 4096 blocks, so a 1024 x 1024 frame (1536 blocks)
    gets 3 frame rows: 14 frames run the 4-frame batches and the tail loop.
    A 224 x 224 frame ends in a partly filled block."""
    x = make((14, 3, 1024, 1024), torch.bfloat16, 'cuda:0')
    assert torch.equal(ops.patchify(x, 16), compose(x, 16))
    x = make((9, 3, 224, 224), torch.bfloat16, 'cuda:0')
    assert torch.equal(ops.patchify(x, 32), compose(x, 32))


@pytest.mark.gpu
def test_patchify_gpu_refused_shape_takes_composition():
    """p = 4 in bf16 is an 8-B run: not a HIP shape, same result."""
    x = make((2, 3, 16, 24), torch.bfloat16, 'cuda:0')
    assert torch.equal(ops.patchify(x, 4), compose(x, 4))


def test_patchify_cpu_refused_shape():
    x = make((2, 3, 16, 24), torch.bfloat16, 'cpu')
    assert torch.equal(ops.patchify(x, 4), compose(x, 4))


@pytest.mark.gpu
def test_patch_embed_bit_identical(monkeypatch):
    from video_features_amd.models.clip_vit import VisionTransformer
    torch.manual_seed(0)
    dev = torch.device('cuda:0')
    model = VisionTransformer().to(dev, torch.bfloat16).eval()
    x = torch.randn(2, 3, 224, 224, device=dev).to(torch.bfloat16)
    with torch.no_grad():
        a = model._patch_embed(x)
        monkeypatch.setenv('VFA_FORCE_TORCH_OPS', '1')
        b = model._patch_embed(x)
    assert a.shape == (2, 49, 768)
    assert torch.equal(a, b)
