"""CLIP ViT: the CLS-only last block and the fused token embedding compute
what the full forward computes (CPU, fp32)."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops
from video_features_amd.models.clip_vit import ViTConfig, VisionTransformer


def _model(layers):
    torch.manual_seed(layers)
    return VisionTransformer(ViTConfig(64, 16, 128, layers, 2, 64)).eval()


@pytest.mark.parametrize('layers', [1, 3])
@pytest.mark.parametrize('batch', [3, 5])
def test_pruned_tail_matches_full_tail(layers, batch, monkeypatch):
    model = _model(layers)
    x = torch.randn(batch, 3, 64, 64,
                    generator=torch.Generator().manual_seed(batch))
    with torch.no_grad():
        monkeypatch.delenv('VFA_CLIP_FULL_TAIL', raising=False)
        pruned = model(x)
        monkeypatch.setenv('VFA_CLIP_FULL_TAIL', '1')
        full = model(x)
    assert pruned.shape == full.shape == (batch, 64)
    diff = (pruned - full).abs().max().item()
    print(f'layers={layers} batch={batch} max abs diff {diff:.3g} '
          f'(output max {full.abs().max().item():.3g})')
    assert diff <= 1e-5


def test_full_tail_switch_changes_the_path(monkeypatch):
    """The switch is read per forward: with it set, the single-query
    attention of the pruned tail is not called."""
    model = _model(2)
    x = torch.randn(2, 3, 64, 64)
    calls = []
    real = ops.attention_pool
    monkeypatch.setattr(ops, 'attention_pool',
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        monkeypatch.delenv('VFA_CLIP_FULL_TAIL', raising=False)
        model(x)
        assert len(calls) == 1
        monkeypatch.setenv('VFA_CLIP_FULL_TAIL', '1')
        model(x)
        assert len(calls) == 1
        monkeypatch.setenv('VFA_CLIP_FULL_TAIL', '0')
        model(x)
        assert len(calls) == 2


@pytest.mark.parametrize('t,p,w', [(3, 4, 128), (2, 49, 36), (1, 1, 8)])
def test_clip_embed_ln_cpu_matches_composition(t, p, w):
    g = torch.Generator().manual_seed(t * 100 + p)
    pe = torch.randn(t, p, w, generator=g)
    cls = torch.randn(w, generator=g)
    pos = torch.randn(p + 1, w, generator=g)
    weight = torch.randn(w, generator=g)
    bias = torch.randn(w, generator=g)
    out = ops.clip_embed_ln(pe, cls, pos, weight, bias, 1e-5)
    ref = torch.cat([cls.expand(t, 1, w), pe], dim=1) + pos
    ref = F.layer_norm(ref, (w,), weight, bias, 1e-5)
    assert out.shape == (t, p + 1, w)
    assert (out - ref).abs().max().item() <= 1e-6


def test_state_dict_keys_unchanged():
    keys = list(VisionTransformer(ViTConfig(64, 16, 128, 3, 2, 64))
                .state_dict().keys())
    assert len(keys) == 44                  # 8 + 12 per block
    assert len(VisionTransformer().state_dict()) == 152
    for name in ('class_embedding', 'positional_embedding', 'proj',
                 'conv1.weight', 'ln_pre.weight', 'ln_post.bias',
                 'blocks.2.attn.qkv.weight', 'blocks.2.attn.qkv.bias',
                 'blocks.2.attn.proj.weight', 'blocks.2.mlp.c_fc.weight',
                 'blocks.2.mlp.c_proj.bias', 'blocks.0.ln_1.weight',
                 'blocks.2.ln_2.bias'):
        assert name in keys, name
    # the weight slices of the pruned tail are views, not parameters: the
    # last block has exactly the keys of every other block
    last = sorted(k.split('.', 2)[2] for k in keys
                  if k.startswith('blocks.2.'))
    first = sorted(k.split('.', 2)[2] for k in keys
                   if k.startswith('blocks.0.'))
    assert last == first and len(last) == 12
