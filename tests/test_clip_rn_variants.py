"""CLIP-RN50x4 / CLIP-RN50x16 feature types and the CPU contracts of the
three ops behind the ModifiedResNet GPU path (no GPU needed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops
from video_features_amd.config import Config
from video_features_amd.models.clip_resnet import build_clip_resnet

# feature_type: (conv1.weight, positional_embedding, c_proj.weight, params,
#                input resolution, output dim)
VARIANTS = {
    'CLIP-RN50x4': ((40, 3, 3, 3), (82, 2560), (640, 2560), 87_137_080,
                    288, 640),
    'CLIP-RN50x16': ((48, 3, 3, 3), (145, 3072), (768, 3072), 167_328_912,
                     384, 768),
}


@pytest.fixture(scope='module')
def towers():
    torch.manual_seed(0)
    return {ft: build_clip_resnet(ft).eval() for ft in VARIANTS}


@pytest.mark.parametrize('ft', sorted(VARIANTS))
def test_config_and_registry_accept(ft):
    from video_features_amd.extractors.clip import ExtractCLIP
    from video_features_amd.models.registry import get_extractor_class
    assert Config(feature_type=ft).feature_type == ft
    assert get_extractor_class(ft) is ExtractCLIP


def test_cli_accepts_new_types():
    from video_features_amd.config import FEATURE_TYPES
    for ft in VARIANTS:
        assert ft in FEATURE_TYPES


@pytest.mark.parametrize('ft', sorted(VARIANTS))
def test_tower_shapes_and_param_count(towers, ft):
    conv1, pos, cproj, nparams, res, out_dim = VARIANTS[ft]
    m = towers[ft]
    assert tuple(m.conv1.weight.shape) == conv1
    assert tuple(m.attnpool.positional_embedding.shape) == pos
    assert tuple(m.attnpool.c_proj.weight.shape) == cproj
    assert m.input_resolution == res and m.output_dim == out_dim
    # head dim 64 in every tower
    assert m.attnpool.k_proj.weight.shape[0] // m.attnpool.num_heads == 64
    assert sum(p.numel() for p in m.parameters()) == nparams


@pytest.mark.parametrize('ft', sorted(VARIANTS))
def test_cpu_forward(towers, ft):
    res, out_dim = VARIANTS[ft][4:]
    torch.manual_seed(1)
    with torch.no_grad():
        y = towers[ft].encode_image(torch.randn(1, 3, res, res))
    assert y.shape == (1, out_dim)
    assert torch.isfinite(y).all()


def test_rn50x4_openai_scheme_roundtrip(towers):
    from video_features_amd.utils.convert_checkpoints import convert_auto
    sd = towers['CLIP-RN50x4'].state_dict()
    assert 'layer1.0.downsample.-1' not in sd       # the pool has no state
    assert 'layer1.0.downsample.0.weight' in sd
    assert 'layer1.0.downsample.1.running_mean' in sd
    legacy = {'visual.' + k: v.clone() for k, v in sd.items()}
    legacy['logit_scale'] = torch.zeros(())
    m2 = build_clip_resnet('CLIP-RN50x4')
    m2.load_state_dict(convert_auto(legacy))
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_unknown_variant_still_rejected():
    with pytest.raises(ValueError):
        Config(feature_type='CLIP-RN50x64')
    with pytest.raises(ValueError):
        build_clip_resnet('CLIP-RN50x64')


# ------------------------------------------------------------ op contracts
@pytest.mark.parametrize('shape', [(2, 8, 4, 4), (3, 136, 7, 9)])
def test_avgpool2d_nhwc_cpu_reference(shape):
    torch.manual_seed(0)
    x = torch.randn(*shape)
    assert torch.equal(ops.avgpool2d_nhwc(x, 2), F.avg_pool2d(x, 2))
    xcl = x.contiguous(memory_format=torch.channels_last)
    y = ops.avgpool2d_nhwc(xcl, 2)
    assert y.shape == (shape[0], shape[1], shape[2] // 2, shape[3] // 2)
    assert torch.allclose(y, F.avg_pool2d(x, 2), atol=1e-6)


def test_attnpool_tokens_cpu_reference():
    torch.manual_seed(0)
    b, hw, c = 3, 9, 64
    x = torch.randn(b, hw, c)
    pos = torch.randn(hw + 1, c)
    t = ops.attnpool_tokens(x, pos)
    assert t.shape == (b, hw + 1, c)
    ref = torch.empty(b, hw + 1, c)
    for i in range(b):
        ref[i, 0] = x[i].sum(dim=0) / hw + pos[0]
        for j in range(hw):
            ref[i, 1 + j] = x[i, j] + pos[1 + j]
    assert torch.allclose(t, ref, atol=1e-6)
    with pytest.raises(ValueError):
        ops.attnpool_tokens(x, pos[:-1])


@pytest.mark.parametrize('heads,d', [(2, 64), (4, 16)])
@pytest.mark.parametrize('l', [1, 5, 82])
def test_attention_pool_cpu_reference(heads, d, l):
    torch.manual_seed(0)
    b, c = 3, heads * d
    q = torch.randn(b, c)
    kv = torch.randn(b, l, 2 * c)
    out = ops.attention_pool(q, kv, heads)
    assert out.shape == (b, c)
    qh = q.view(b, heads, 1, d)
    kh = kv[..., :c].view(b, l, heads, d).transpose(1, 2)
    vh = kv[..., c:].view(b, l, heads, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qh, kh, vh).reshape(b, c)
    assert torch.allclose(out, ref, atol=1e-5)
    if l == 1:      # softmax over one key is exactly 1
        assert torch.equal(out, kv[:, 0, c:])


def test_attention_pool_matches_module_attention():
    """ops.attnpool_tokens + packed k/v projection + ops.attention_pool
    reproduce AttentionPool2d.forward."""
    from video_features_amd.models.clip_resnet import AttentionPool2d
    torch.manual_seed(0)
    pool = AttentionPool2d(3, 128, 2, 32).eval()
    x = torch.randn(2, 128, 3, 3)
    with torch.no_grad():
        ref = pool(x)
        t = ops.attnpool_tokens(x.flatten(2).permute(0, 2, 1),
                                pool.positional_embedding)
        wkv, bkv = pool._kv_packed()
        kv = F.linear(t, wkv, bkv)
        q = pool.q_proj(t[:, 0])
        out = pool.c_proj(ops.attention_pool(q, kv, pool.num_heads))
    assert torch.allclose(out, ref, atol=1e-5)


def test_kv_cache_follows_load_state_dict():
    from video_features_amd.models.clip_resnet import AttentionPool2d
    torch.manual_seed(0)
    pool = AttentionPool2d(2, 64, 1, 16)
    w0, _ = pool._kv_packed()
    assert pool._kv_packed()[0] is w0               # cached
    sd = {k: v.clone() for k, v in pool.state_dict().items()}
    sd['k_proj.weight'] = sd['k_proj.weight'] + 1.0
    pool.load_state_dict(sd)
    w1, _ = pool._kv_packed()
    assert torch.equal(w1[:64], sd['k_proj.weight'])
    assert torch.equal(w1[64:], sd['v_proj.weight'])


@pytest.mark.parametrize('layers,res', [([1, 1, 1, 1], 64),
                                        ([1, 2, 1, 1], 96)])
def test_fused_wiring_equals_eager_on_cpu(monkeypatch, layers, res):
    """The fused branch's composition (its ops fall to their torch
    references on the CPU) computes what the eager branch computes."""
    from video_features_amd.models import clip_resnet
    from video_features_amd.utils.fold_bn import fold_batchnorms
    torch.manual_seed(0)
    m = clip_resnet.ModifiedResNet(layers, output_dim=64, heads=16,
                                   input_resolution=res, width=32).eval()
    for mod in m.modules():                 # non-trivial BN statistics
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 3, res, res)
    with torch.no_grad():
        ref = m(x)
        fold_batchnorms(m)
        monkeypatch.setattr(clip_resnet, '_fused_ready',
                            lambda mod, t: isinstance(mod.bn1,
                                                      torch.nn.Identity))
        out = m(x)
    assert torch.allclose(out, ref, atol=1e-4, rtol=1e-4)


def test_rn50x4_extractor_cpu(y4m_video):
    from video_features_amd.extractors.clip import ExtractCLIP
    cfg = Config(feature_type='CLIP-RN50x4', video_paths=[y4m_video],
                 cpu=True, extract_method='uni_2')
    out = ExtractCLIP(cfg, external_call=True)(torch.arange(1))[0]
    assert out['CLIP-RN50x4'].shape == (2, 640)
    assert np.isfinite(out['CLIP-RN50x4']).all()
