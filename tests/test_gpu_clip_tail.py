"""GPU checks of the CLIP ViT token-embedding kernel and the CLS-only last
block (bf16, HIP path)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# Slack of the clip_embed_ln bound beyond one bf16 rounding of the reference.
# The existing HIP ops.layer_norm, given the same summed tokens (rounded to
# bf16, as the eager cat/add hands them over), exceeds 2^-8 |ref| by at most
# EMBED_LN_EXCESS over the three shapes below (measured on MI355X: 0.00600,
# 0.01098, 0.01175 - the rounding of the sums, scaled by rstd and weight);
# eps is twice that.  clip_embed_ln itself measured <= 1e-8 over 2^-8 |ref|.
EMBED_LN_EXCESS = 0.01175
EMBED_EPS = 2 * EMBED_LN_EXCESS


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _embed_case(t, p, w):
    """bf16 inputs and the fp32 reference built from those same bf16 values."""
    g = torch.Generator().manual_seed(1000 * t + p)
    pe = torch.randn(t, p, w, generator=g).to(BF16)
    cls = torch.randn(w, generator=g).to(BF16)
    pos = torch.randn(p + 1, w, generator=g).to(BF16)
    weight = (1 + 0.25 * torch.randn(w, generator=g)).to(BF16)
    bias = (0.25 * torch.randn(w, generator=g)).to(BF16)
    tokens = torch.cat([cls.float().expand(t, 1, w), pe.float()], dim=1) \
        + pos.float()
    ref = F.layer_norm(tokens, (w,), weight.float(), bias.float(), 1e-5)
    return (pe, cls, pos, weight, bias), tokens, ref


def _excess(out, ref):
    return ((out - ref).abs() - 2.0 ** -8 * ref.abs()).max().item()


@pytest.mark.parametrize('t,p,w', [(3, 4, 128), (2, 49, 768), (1, 196, 768)])
def test_clip_embed_ln_vs_fp32(dev, t, p, w):
    from video_features_amd import ops
    args, tokens, ref = _embed_case(t, p, w)
    dargs = [a.to(dev) for a in args]
    out = ops.clip_embed_ln(*dargs, 1e-5)
    assert out.dtype == BF16 and out.shape == (t, p + 1, w)
    assert out.is_contiguous()
    out = out.float().cpu()
    # what the existing LayerNorm kernel makes of the same summed tokens
    ln = ops.layer_norm(tokens.to(BF16).to(dev), dargs[3], dargs[4], 1e-5)
    print(f'clip_embed_ln ({t},{p},{w}): excess over 2^-8|ref| '
          f'{_excess(out, ref):.4g}; ops.layer_norm on the bf16 sums '
          f'{_excess(ln.float().cpu(), ref):.4g}')
    bad = (out - ref).abs() > 2.0 ** -8 * ref.abs() + EMBED_EPS
    assert not bad.any(), (int(bad.sum()), _excess(out, ref))
    # row 0 of every frame is cls + pos[0], whatever the patches hold
    pe2 = (args[0].float() * -3.0 + 1.0).to(BF16).to(dev)
    out2 = ops.clip_embed_ln(pe2, *dargs[1:], 1e-5).float().cpu()
    assert torch.equal(out2[:, 0], out[:, 0])
    assert not torch.equal(out2[:, 1:], out[:, 1:])
    assert torch.equal(out[:, 0], out[:1, 0].expand(t, w))


def _tail_model(dev):
    from video_features_amd.models.clip_vit import ViTConfig, VisionTransformer
    torch.manual_seed(0)
    m32 = VisionTransformer(ViTConfig(64, 32, 128, 2, 2, 64)).eval()
    mgpu = VisionTransformer(ViTConfig(64, 32, 128, 2, 2, 64))
    mgpu.load_state_dict(m32.state_dict())
    return m32, mgpu.to(dev, BF16).eval()


def _inputs(seed, batch=6):
    return torch.randn(batch, 3, 64, 64,
                       generator=torch.Generator().manual_seed(seed))


def test_pruned_tail_vs_full_tail_bf16(dev, monkeypatch):
    m32, mgpu = _tail_model(dev)
    x = _inputs(0)
    with torch.no_grad():
        monkeypatch.setenv('VFA_CLIP_FULL_TAIL', '1')
        ref = m32(x)
        full = mgpu(x.to(dev, BF16)).float().cpu()
        monkeypatch.delenv('VFA_CLIP_FULL_TAIL')
        pruned = mgpu(x.to(dev, BF16)).float().cpu()
    assert pruned.shape == (6, 64)
    cos = F.cosine_similarity(pruned, full, dim=1).min().item()
    d_pf = (pruned - full).abs().max().item()
    d_fr = (full - ref).abs().max().item()
    print(f'pruned vs full tail: min cos {cos:.6f}, max abs {d_pf:.4g}; '
          f'full tail vs CPU fp32: max abs {d_fr:.4g}')
    assert cos >= 0.999
    assert d_pf <= d_fr


@pytest.mark.parametrize('full_tail', [False, True])
def test_tail_graph_replay_equals_eager(dev, monkeypatch, full_tail):
    _, mgpu = _tail_model(dev)
    if full_tail:
        monkeypatch.setenv('VFA_CLIP_FULL_TAIL', '1')
    else:
        monkeypatch.delenv('VFA_CLIP_FULL_TAIL', raising=False)
    xs = [_inputs(s).to(dev, BF16) for s in (1, 2)]
    with torch.no_grad():
        eager = [mgpu(x).clone() for x in xs]
        static_in = torch.zeros_like(xs[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mgpu(static_in)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = mgpu(static_in)
        for x, e in zip(xs, eager):
            static_in.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, e)
    assert not torch.equal(eager[0], eager[1])
