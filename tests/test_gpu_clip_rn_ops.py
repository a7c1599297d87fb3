"""GPU tests for the three kernels behind the CLIP ModifiedResNet path:
avgpool2d_nhwc, attnpool_tokens, attention_pool."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _one_rounding(out, ref, what):
    """f32 arithmetic, one rounding to bf16: |out - ref| <= 2^-8 |ref| + 1e-6
    elementwise."""
    out, ref = out.float().cpu(), ref.float().cpu()
    excess = ((out - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-6)).max().item()
    print(what, 'max |err|', (out - ref).abs().max().item(),
          'max excess over bound', excess)
    assert excess <= 0, (what, excess)


# ------------------------------------------------------------ avgpool2d_nhwc
@pytest.mark.parametrize('shape', [(2, 8, 4, 4), (1, 40, 6, 10),
                                   (3, 136, 7, 9), (1, 1280, 2, 2)])
def test_avgpool2d_nhwc(dev, shape):
    from video_features_amd import ops
    torch.manual_seed(0)
    x = torch.randn(*shape).to(BF16)
    ref = F.avg_pool2d(x.float(), 2)
    xg = x.to(dev).contiguous(memory_format=torch.channels_last)
    out = ops.avgpool2d_nhwc(xg, 2)
    assert out.dtype == BF16
    assert out.shape == ref.shape == (shape[0], shape[1], shape[2] // 2,
                                      shape[3] // 2)
    assert out.is_contiguous(memory_format=torch.channels_last)
    _one_rounding(out, ref, f'avgpool {shape}')


def test_avgpool2d_nhwc_many_blocks_and_nchw_input(dev):
    """More work items than one grid pass (grid-stride loop) and an input
    that arrives NCHW-contiguous."""
    from video_features_amd import ops
    torch.manual_seed(1)
    # 4*65*65*(256/8) = 540800 work items > the 2048 x 256 thread grid cap
    x = torch.randn(4, 256, 130, 130).to(BF16)
    ref = F.avg_pool2d(x.float(), 2)
    out = ops.avgpool2d_nhwc(x.to(dev), 2)
    assert out.is_contiguous(memory_format=torch.channels_last)
    _one_rounding(out, ref, 'avgpool big')


def test_avgpool2d_nhwc_k3_and_bad_channels(dev):
    from video_features_amd import ops
    torch.manual_seed(2)
    x = torch.randn(1, 16, 7, 10).to(BF16)
    out = ops.avgpool2d_nhwc(x.to(dev), 3)
    ref = F.avg_pool2d(x.float(), 3)
    assert out.shape == ref.shape == (1, 16, 2, 3)
    # 1/9 is not a power of two: sum * (1/9) and sum / 9 differ by an f32 ulp,
    # far inside the bf16 rounding bound
    _one_rounding(out, ref, 'avgpool k=3')
    with pytest.raises(ValueError):
        ops.avgpool2d_nhwc(torch.zeros(1, 12, 4, 4, device=dev, dtype=BF16))


# ----------------------------------------------------------- attnpool_tokens
@pytest.mark.parametrize('b,hw,c', [(2, 4, 64), (1, 49, 2048), (3, 9, 1024)])
def test_attnpool_tokens(dev, b, hw, c):
    from video_features_amd import ops
    torch.manual_seed(0)
    x = torch.randn(b, hw, c).to(BF16)
    pos = (torch.randn(hw + 1, c) / c ** 0.5).to(BF16)
    xf, pf = x.float(), pos.float()
    ref = torch.cat([xf.mean(dim=1, keepdim=True), xf], dim=1) + pf
    out = ops.attnpool_tokens(x.to(dev), pos.to(dev))
    assert out.dtype == BF16 and out.shape == (b, hw + 1, c)
    assert out.is_contiguous()
    _one_rounding(out, ref, f'tokens {(b, hw, c)}')


def test_attnpool_tokens_from_channels_last_view(dev):
    """The (B, HW, C) input as the tower passes it: a permuted view of a
    channels_last map."""
    from video_features_amd import ops
    torch.manual_seed(3)
    m = torch.randn(2, 64, 3, 3).to(BF16)
    pos = torch.randn(10, 64).to(BF16)
    mg = m.to(dev).contiguous(memory_format=torch.channels_last)
    out = ops.attnpool_tokens(mg.permute(0, 2, 3, 1).reshape(2, 9, 64),
                              pos.to(dev))
    xf = m.float().flatten(2).permute(0, 2, 1)
    ref = torch.cat([xf.mean(dim=1, keepdim=True), xf], dim=1) + pos.float()
    _one_rounding(out, ref, 'tokens CL view')


# ------------------------------------------------------------ attention_pool
def _sdpa_ref(q, kv, heads):
    b, c = q.shape
    l, d = kv.shape[1], c // heads
    qh = q.float().view(b, heads, 1, d)
    kh = kv[..., :c].float().reshape(b, l, heads, d).transpose(1, 2)
    vh = kv[..., c:].float().reshape(b, l, heads, d).transpose(1, 2)
    return F.scaled_dot_product_attention(
        qh, kh, vh, scale=1.0 / d ** 0.5).reshape(b, c)


@pytest.mark.parametrize('heads', [2, 16])
@pytest.mark.parametrize('l', [1, 5, 50, 64, 65, 82, 145, 200])
def test_attention_pool_vs_fp32(dev, heads, l):
    from video_features_amd import ops
    torch.manual_seed(0)
    b, d = 3, 64
    c = heads * d
    q = torch.randn(b, c).to(BF16)
    kv = torch.randn(b, l, 2 * c).to(BF16)
    out = ops.attention_pool(q.to(dev), kv.to(dev), heads)
    assert out.dtype == BF16 and out.shape == (b, c)
    out = out.float().cpu()
    ref = _sdpa_ref(q, kv, heads)
    err = (out - ref).abs().max().item()
    print('attention_pool', heads, l, 'max |err|', err)
    assert err < 3e-2, (heads, l, err)
    if l == 1:
        # softmax over one key is exactly 1: v's bf16 values come back
        assert torch.equal(out, kv[:, 0, c:].float())


@pytest.mark.parametrize('l', [50, 145])
def test_attention_pool_softmax_stability(dev, l):
    # x8 inputs: scores of magnitude ~500 overflow exp() without the max
    # subtraction, and exercise the cross-chunk rescale
    from video_features_amd import ops
    torch.manual_seed(1)
    b, heads, d = 3, 4, 64
    c = heads * d
    q = (torch.randn(b, c) * 8).to(BF16)
    kv = (torch.randn(b, l, 2 * c) * 8).to(BF16)
    out = ops.attention_pool(q.to(dev), kv.to(dev), heads).float().cpu()
    assert torch.isfinite(out).all()
    ref = _sdpa_ref(q, kv, heads)
    err = ((out - ref).abs() / ref.abs().clamp(min=1.0)).max().item()
    print('attention_pool x8', l, 'max rel err', err)
    assert err < 2e-2, err


def test_attention_pool_other_head_dim_takes_torch(dev):
    """d != 64 is outside the kernel: documented torch composition, same
    contract."""
    from video_features_amd import ops
    torch.manual_seed(2)
    b, heads, d, l = 2, 4, 32, 10
    c = heads * d
    q = torch.randn(b, c).to(BF16)
    kv = torch.randn(b, l, 2 * c).to(BF16)
    out = ops.attention_pool(q.to(dev), kv.to(dev), heads).float().cpu()
    err = (out - _sdpa_ref(q, kv, heads)).abs().max().item()
    assert err < 3e-2, err
