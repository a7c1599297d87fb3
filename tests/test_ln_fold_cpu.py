"""LayerNorm folded into the linear layer that follows it (ops.fold_ln_linear,
ops.linear_res_stats, ops.linear_ln_act) and its routing in the CLIP ViT
blocks — the algebra and the torch compositions, no GPU."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops
from video_features_amd.models.clip_vit import ViTConfig, VisionTransformer

EPS = 1e-5


def _folded(s, fold, act='none'):
    """The folded formula on un-normalised rows, in the rows' dtype."""
    wf, c, bf = fold
    mean = s.mean(1, keepdim=True)
    rstd = (s.var(1, unbiased=False, keepdim=True) + EPS).rsqrt()
    return ops._apply_act(rstd * (s @ wf.t() - mean * c) + bf, act)


@pytest.mark.parametrize('gamma', ['random', 'negative', 'zeros'])
def test_fold_matches_layer_norm_linear_fp64(gamma):
    torch.manual_seed(0)
    m, n, k = 37, 24, 40
    s = torch.randn(m, k, dtype=torch.float64) * 3 + 5
    w = torch.randn(n, k, dtype=torch.float64)
    b = torch.randn(n, dtype=torch.float64)
    g = torch.randn(k, dtype=torch.float64)      # both signs
    if gamma == 'negative':
        g = -g.abs()
    elif gamma == 'zeros':
        g[::3] = 0.0
    be = torch.randn(k, dtype=torch.float64)
    fold = ops.fold_ln_linear(w, b, g, be)
    assert fold[0].dtype == torch.float64 and fold[0].shape == (n, k)
    assert fold[1].shape == (n,) and fold[2].shape == (n,)
    ref = F.linear(F.layer_norm(s, (k,), g, be, EPS), w, b)
    assert (_folded(s, fold) - ref).abs().max().item() < 1e-10


def test_fold_fp32_and_no_bias():
    torch.manual_seed(1)
    m, n, k = 20, 16, 32
    s, w = torch.randn(m, k), torch.randn(n, k)
    g, be = torch.randn(k), torch.randn(k)
    fold = ops.fold_ln_linear(w, None, g, be)
    assert fold[1].dtype == torch.float32 and fold[2].dtype == torch.float32
    ref = F.linear(F.layer_norm(s, (k,), g, be, EPS), w)
    err = (_folded(s, fold) - ref).abs().max().item()
    assert err < 1e-5 * max(ref.abs().max().item(), 1.0), err


def test_fold_c_is_summed_from_the_rounded_weight():
    """bf16 layer: W' is bf16 and c is the f32 row sum of that bf16 W', not
    of the unrounded product — with it acc - mean * c cancels a large row
    mean exactly."""
    torch.manual_seed(2)
    w = torch.randn(16, 64).to(torch.bfloat16)
    g, be = torch.randn(64).to(torch.bfloat16), torch.randn(64)
    wf, c, bf = ops.fold_ln_linear(w, None, g, be.to(torch.bfloat16))
    assert wf.dtype == torch.bfloat16
    assert c.dtype == torch.float32 and bf.dtype == torch.float32
    assert torch.equal(c, wf.double().sum(1).float())
    unrounded = (w.double() * g.double()).sum(1).float()
    assert not torch.equal(c, unrounded)


def test_ops_compositions_cpu():
    """Off the GPU both ops are their torch compositions, with and without
    the unfolded parameters."""
    torch.manual_seed(3)
    m, n, k = 12, 24, 16
    x, res = torch.randn(m, 8), torch.randn(m, k)
    w1, b1 = torch.randn(k, 8), torch.randn(k)
    w2, b2 = torch.randn(n, k), torch.randn(n)
    g, be = torch.randn(k), torch.randn(k)
    assert not ops.fused_ln_tiles(x, w1)
    s, st = ops.linear_res_stats(x, w1, b1, res)
    assert torch.equal(s, F.linear(x, w1, b1) + res)
    assert st.shape == (m, 1, 2) and st.dtype == torch.float32
    mr = ops.ln_stats(st, k, EPS)
    assert torch.allclose(mr[:, 0], s.mean(1), atol=1e-6)
    assert torch.allclose(mr[:, 1],
                          (s.var(1, unbiased=False) + EPS).rsqrt(), rtol=1e-5)
    fold = ops.fold_ln_linear(w2, b2, g, be)
    ref = ops._apply_act(
        F.linear(F.layer_norm(s, (k,), g, be, EPS), w2, b2), 'quick_gelu')
    a = ops.linear_ln_act(s, st, *fold, act='quick_gelu', eps=EPS,
                          unfolded=(w2, b2, g, be))
    assert torch.equal(a, ref)
    bnd = 1e-5 * max(ref.abs().max().item(), 1.0)
    assert (ops.linear_ln_act(s, st, *fold, act='quick_gelu', eps=EPS)
            - ref).abs().max().item() < bnd
    with pytest.raises(ValueError):
        ops.linear_ln_act(s, st, *fold, act='swish')


def test_ln_stats_merges_groups():
    """Partials of T equal-width groups merge to the statistics of the whole
    row, also when the row mean dwarfs the spread."""
    torch.manual_seed(5)
    s = torch.randn(9, 4, 16, dtype=torch.float64) + 100.0
    gm = s.mean(2)
    st = torch.stack([gm, ((s - gm[..., None]) ** 2).sum(2)], dim=2)
    mr = ops.ln_stats(st, 64, EPS)
    row = s.reshape(9, 64)
    assert torch.allclose(mr[:, 0], row.mean(1), rtol=1e-13)
    assert torch.allclose(mr[:, 1],
                          (row.var(1, unbiased=False) + EPS).rsqrt(),
                          rtol=1e-12)


def _tiny_vit():
    torch.manual_seed(4)
    cfg = ViTConfig(input_resolution=32, patch_size=16, width=64, layers=3,
                    heads=4, output_dim=32)
    model = VisionTransformer(cfg).eval()
    with torch.no_grad():                 # LN affines off their defaults
        for blk in model.blocks:
            blk.ln_2.weight.normal_()
            blk.ln_2.bias.normal_()
    return model, torch.randn(3, 3, 32, 32)


def test_block_forward_fold_on_off(monkeypatch):
    model, x = _tiny_vit()
    monkeypatch.delenv('VFA_NO_LNFOLD', raising=False)
    with torch.no_grad():
        assert model.blocks[0].fold_routed(x)
        on = model(x)
        assert model.blocks[0]._fold is not None     # the route was taken
        assert model.blocks[-1]._fold is None        # not the [CLS] tail
        monkeypatch.setenv('VFA_NO_LNFOLD', '1')
        assert not model.blocks[0].fold_routed(x)
        off = model(x)
    assert (on - off).abs().max().item() < 1e-5 * off.abs().max().item()
    assert not any('_fold' in k for k in model.state_dict())
    assert sorted(model.state_dict()) == sorted(
        VisionTransformer(model.cfg).state_dict())


def test_fold_cache_rebuilt(monkeypatch):
    monkeypatch.delenv('VFA_NO_LNFOLD', raising=False)
    model, x = _tiny_vit()
    blk = model.blocks[0]
    with torch.no_grad():
        model(x)
        first = blk._ln2_fold()
        assert blk._ln2_fold() is first              # cached between calls

        # in-place write of one source parameter
        blk.ln_2.weight.copy_(torch.randn(64))
        second = blk._ln2_fold()
        assert second is not first
        assert torch.equal(second[0], ops.fold_ln_linear(
            blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.ln_2.weight,
            blk.ln_2.bias)[0])

        # load_state_dict: every block's fold follows the new weights
        other, _ = _tiny_vit()
        for p in other.parameters():
            p.mul_(0.5)
        model.load_state_dict(other.state_dict())
        third = blk._ln2_fold()
        assert third is not second
        assert torch.allclose(model(x), other(x), atol=1e-6)

        # .to(): the parameters are replaced
        model.double()
        assert blk._ln2_fold()[0].dtype == torch.float64
