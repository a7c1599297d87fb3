"""GPU tests for the fused CLIP ModifiedResNet tower: numerics against the
fp32 eager reference, no eager conv/pool dispatch, k/v weight-cache
invalidation, and an end-to-end CLIP-RN50x4 extraction."""
import numpy as np
import pytest
import torch

from tests.conftest import synthetic_frames
from video_features_amd.config import Config
from video_features_amd.io.y4m import write_y4m
from video_features_amd.models.clip_resnet import ModifiedResNet
from video_features_amd.utils.fold_bn import fold_batchnorms

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
# (layers, input resolution): final maps 2x2 (L=5) and 3x3 (L=10); every
# pooled map is even-sized and the head dim is (32 * 32) / 16 = 64
TOWERS = {'l5': ([1, 1, 1, 1], 64), 'l10': ([1, 2, 1, 1], 96)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _tower(name):
    layers, res = TOWERS[name]
    return ModifiedResNet(layers, output_dim=64, heads=16,
                          input_resolution=res, width=32).eval()


@pytest.fixture(scope='module')
def cases(dev):
    """name -> (folded bf16 GPU tower, bf16 GPU input, fp32 CPU eager
    reference taken before folding).  Built once, left unchanged."""
    out = {}
    for name, (_, res) in TOWERS.items():
        torch.manual_seed(0)
        m = _tower(name)
        x = torch.randn(2, 3, res, res)
        with torch.no_grad():
            ref = m(x)
        fold_batchnorms(m)
        out[name] = (m.to(dev, BF16), x.to(dev, BF16), ref)
    return out


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(
        a.float().cpu().flatten(), b.float().cpu().flatten(), dim=0).item()


@pytest.mark.parametrize('name', sorted(TOWERS))
def test_fused_tower_cosine_vs_fp32_eager(cases, name):
    m, x, ref = cases[name]
    with torch.no_grad():
        out = m.encode_image(x)
    assert out.shape == ref.shape == (2, 64) and out.dtype == BF16
    assert torch.isfinite(out.float()).all()
    cos = _cos(out, ref)
    print(f'fused CLIP-RN tower {name}: cosine vs fp32 eager = {cos:.6f}')
    assert cos > 0.99, (name, cos)


def _count_eager(monkeypatch):
    import torch.nn.functional as F
    calls = {'conv2d': 0, 'avg_pool2d': 0}
    real_conv, real_pool = F.conv2d, F.avg_pool2d

    def conv2d(*a, **k):
        calls['conv2d'] += 1
        return real_conv(*a, **k)

    def avg_pool2d(*a, **k):
        calls['avg_pool2d'] += 1
        return real_pool(*a, **k)

    monkeypatch.setattr(F, 'conv2d', conv2d)
    monkeypatch.setattr(F, 'avg_pool2d', avg_pool2d)
    return calls


def test_fused_tower_dispatches_no_eager_conv_or_pool(cases, monkeypatch):
    m, x, _ = cases['l10']
    monkeypatch.delenv('VFA_NO_CLIPRN', raising=False)
    calls = _count_eager(monkeypatch)
    with torch.no_grad():
        fused = m.encode_image(x)
    assert calls == {'conv2d': 0, 'avg_pool2d': 0}, calls
    # the switch restores the eager composition (read per call, not cached)
    monkeypatch.setenv('VFA_NO_CLIPRN', '1')
    with torch.no_grad():
        eager = m.encode_image(x)
    assert calls['conv2d'] > 0 and calls['avg_pool2d'] > 0, calls
    # both paths compute the same tower
    assert _cos(fused, eager) > 0.99


def test_kv_weight_cache_invalidated_by_load_state_dict(dev):
    torch.manual_seed(0)
    m = _tower('l5')
    fold_batchnorms(m)
    # unit-scale positional embedding: with the 1/sqrt(C) init the five
    # tokens of a random tower are nearly equal, every attention pattern
    # then pools the same vector and a stale k weight would not show
    # (fp32 on the CPU: the two outputs differ by 0.87 at scale 0.70 with
    # it, by a third of a bf16 ulp without it)
    with torch.no_grad():
        m.attnpool.positional_embedding.normal_(
            0, 1, generator=torch.Generator().manual_seed(4))
    m = m.to(dev, BF16)
    x = torch.randn(2, 3, 64, 64).to(dev, BF16)
    with torch.no_grad():
        out1 = m.encode_image(x)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    sd['attnpool.k_proj.weight'] = (
        torch.randn(sd['attnpool.k_proj.weight'].shape, generator=g) * 0.5
    ).to(dev, BF16)
    m.load_state_dict(sd)
    with torch.no_grad():
        out2 = m.encode_image(x)
    fresh = _tower('l5')
    fold_batchnorms(fresh)          # same module structure as ``sd``
    fresh = fresh.to(dev, BF16)
    fresh.load_state_dict(sd)
    with torch.no_grad():
        want = fresh.encode_image(x)
    scale = want.float().abs().max().item()
    stale = (out1.float() - want.float()).abs().max().item()
    diff = (out2.float() - want.float()).abs().max().item()
    print('kv cache: |second - fresh| =', diff, ' |first - fresh| =', stale,
          ' max |fresh| =', scale)
    # same weights, same kernels: at most one bf16 ulp apart; a stale
    # concatenated weight would leave the first forward's output
    assert diff <= 2.0 ** -7 * scale
    assert stale > 8 * 2.0 ** -7 * scale


def test_clip_rn50x4_e2e(dev, tmp_path):
    from video_features_amd.models.registry import get_extractor_class
    p = str(tmp_path / 'v.y4m')
    write_y4m(p, synthetic_frames(t=10, h=64, w=64), fps=25.0)
    cfg = Config(feature_type='CLIP-RN50x4', video_paths=[p],
                 extract_method='uni_2', tmp_path=str(tmp_path / 'tmp'))
    ex = get_extractor_class(cfg.feature_type)(cfg, external_call=True)
    out = ex(torch.arange(1, device=dev))
    assert len(out) == 1, 'extraction failed (error swallowed per-video)'
    f = out[0]['CLIP-RN50x4']
    assert f.shape == (2, 640) and np.isfinite(f).all()
