"""GPU numerics of the LayerNorm-fold GEMM epilogues: ops.linear_res_stats
(residual + per-row LN statistics out of the persistent 256^2 kernel),
ops.linear_ln_act (LN folded into the next linear layer) and their route in
the CLIP ViT blocks.  Every case prints its error figures before asserting.

Tolerances: the outputs use test_gpu_gemm.py's (fp32 torch reference,
max-rel < 3e-2, mean-rel < 5e-3).  The statistics — the partials the
kernel returns, merged by ops.ln_stats — are compared with fp64 statistics
of the returned bf16 rows: |d mean| <= 1e-3 std and |d rstd| / rstd <= 1e-3,
half a bf16 ulp (2^-9) with margin."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ops():
    from video_features_amd import ops
    assert ops.hip_available()
    return ops


def _rel(out, ref):
    """(max-rel, mean-rel) as test_gpu_gemm.py defines them."""
    err = (out.float() - ref).abs()
    return (err.max().item() / max(ref.abs().max().item(), 1e-6),
            (err.mean() / ref.abs().mean().clamp_min(1e-6)).item())


def _residual(kind, m, n, dev):
    r = torch.randn(m, n, device=dev)
    if kind == 'mean100':          # rows of mean ~100, std ~1
        r = r + 100.0
    elif kind == 'outlier':        # one channel 200x the rest
        r[:, n // 3] *= 200.0
    return r.to(BF16)


# (M, N, K): 30 tiles / 3 tile columns = 12 strips, 3 partials per row, one
# K-tile; three K-tiles; 272 tiles on 256 CUs (some blocks walk two tiles,
# N = 256 so one tile holds the whole row); 270 tiles (XCD-remap
# remainder); ragged -> the torch composition
RES_SHAPES = [(2560, 768, 64), (2560, 768, 192), (69632, 256, 64),
              (23040, 768, 128), (2560, 776, 72)]


@pytest.mark.parametrize('kind', ['randn', 'mean100', 'outlier'])
@pytest.mark.parametrize('m,n,k', RES_SHAPES)
def test_linear_res_stats(dev, m, n, k, kind):
    ops = _ops()
    torch.manual_seed(0)
    x = (torch.randn(m, k, device=dev) / (k ** 0.25)).to(BF16)
    w = (torch.randn(n, k, device=dev) / (k ** 0.25)).to(BF16)
    b = torch.randn(n, device=dev).to(BF16)
    r = _residual(kind, m, n, dev)
    fused = ops.fused_ln_tiles(x, w)
    assert fused == (m % 256 == 0 and n % 256 == 0 and k % 64 == 0)
    s, part = ops.linear_res_stats(x, w, b, r)
    assert s.shape == (m, n) and s.dtype == BF16
    assert part.shape == (m, n // 256 if fused else 1, 2)
    assert part.dtype == torch.float32
    st = ops.ln_stats(part, n, EPS)

    ref = F.linear(x.float(), w.float(), b.float()) + r.float()
    mx, mn = _rel(s, ref)
    del ref
    # statistics of the rows the consumer will read: the rounded s
    s64 = s.double()
    var64, mean64 = torch.var_mean(s64, dim=1, unbiased=False)
    del s64
    rstd64 = (var64 + EPS).rsqrt()
    dmean = ((st[:, 0].double() - mean64).abs() / var64.sqrt()).max().item()
    drstd = ((st[:, 1].double() - rstd64).abs() / rstd64).max().item()
    print(f'\nlinear_res_stats {m}x{n}x{k} {kind} fused={fused}: s max-rel '
          f'{mx:.3e} mean-rel {mn:.3e}; |d mean|/std {dmean:.3e} '
          f'|d rstd|/rstd {drstd:.3e}')
    assert mx < 3e-2 and mn < 5e-3
    assert dmean <= 1e-3 and drstd <= 1e-3

    s2, part2 = ops.linear_res_stats(x, w, b, r)
    assert torch.equal(s, s2) and torch.equal(part, part2)  # bit-identical


def _ln_case(ops, dev, m, n, k, act, mean100, groups):
    torch.manual_seed(1)
    s = torch.randn(m, k, device=dev)
    if mean100:
        s = s + 100.0
    s = s.to(BF16)
    w = (torch.randn(n, k, device=dev) / (k ** 0.25)).to(BF16)
    b = torch.randn(n, device=dev).to(BF16)
    g = (1.0 + 0.5 * torch.randn(k, device=dev)).to(BF16)
    be = (0.5 * torch.randn(k, device=dev)).to(BF16)
    # exact partials of `groups` column groups, rounded to f32
    s64 = s.double().reshape(m, groups, k // groups)
    gm = s64.mean(2)
    st = torch.stack([gm, ((s64 - gm[..., None]) ** 2).sum(2)], 2).float()
    del s64
    fold = ops.fold_ln_linear(w, b, g, be)
    out = ops.linear_ln_act(s, st.contiguous(), *fold, act=act, eps=EPS,
                            unfolded=(w, b, g, be))
    today = ops.linear_act(ops.layer_norm(s, g, be, EPS), w, b, act)
    ref = ops._apply_act(
        F.linear(F.layer_norm(s.float(), (k,), g.float(), be.float(), EPS),
                 w.float(), b.float()), act)
    assert out.shape == (m, n) and out.dtype == BF16
    return _rel(out, ref), _rel(today, ref)


def _check_ln(ops, dev, m, n, k, act, mean100, groups):
    (mx, mn), (tmx, tmn) = _ln_case(ops, dev, m, n, k, act, mean100, groups)
    print(f'\nlinear_ln_act {m}x{n}x{k} {act} mean100={mean100} '
          f'groups={groups}: max-rel '
          f'{mx:.3e} (layer_norm + linear_act {tmx:.3e}), mean-rel {mn:.3e} '
          f'({tmn:.3e})')
    assert mx < 3e-2 and mn < 5e-3
    # one bf16 rounding of the weights for one of the activations: no more
    # than 1.5x the error of today's composition
    assert mx <= 1.5 * tmx and mn <= 1.5 * tmn


# 150 tiles, K = the LN width, the 3 partials per row a 768-wide producer
# writes; one tile column, one partial; 272 tiles for every activation of
# the table; ragged -> layer_norm + linear_act
LN_CASES = ([(2560, 3840, 768, 'quick_gelu', 3), (2560, 256, 768, 'none', 1)]
            + [(4352, 4096, 256, a, 1 if a == 'relu' else 4)
               for a in ('none', 'relu', 'quick_gelu', 'gelu', 'leaky_relu')]
            + [(2560, 776, 72, 'quick_gelu', 1)])


@pytest.mark.parametrize('mean100', [False, True])
@pytest.mark.parametrize('m,n,k,act,groups', LN_CASES)
def test_linear_ln_act(dev, m, n, k, act, groups, mean100):
    ops = _ops()
    assert ops.fused_ln_tiles(torch.empty(m, k, device=dev, dtype=BF16),
                              torch.empty(n, k, device=dev, dtype=BF16)) \
        == (n % 256 == 0 and k % 64 == 0)
    _check_ln(ops, dev, m, n, k, act, mean100, groups)


def test_pair_matches_layer_norm_residual(dev):
    """The two ops chained, as the ViT block chains them, against today's
    F.linear + layer_norm_residual + linear_act on the same inputs."""
    ops = _ops()
    torch.manual_seed(2)
    m, wd, n2 = 2560, 768, 1024
    x = (torch.randn(m, wd, device=dev) / (wd ** 0.25)).to(BF16)
    r = _residual('outlier', m, wd, dev)
    w1 = (torch.randn(wd, wd, device=dev) / (wd ** 0.25)).to(BF16)
    b1 = torch.randn(wd, device=dev).to(BF16)
    w2 = (torch.randn(n2, wd, device=dev) / (wd ** 0.25)).to(BF16)
    b2 = torch.randn(n2, device=dev).to(BF16)
    g = (1.0 + 0.5 * torch.randn(wd, device=dev)).to(BF16)
    be = (0.5 * torch.randn(wd, device=dev)).to(BF16)
    s, st = ops.linear_res_stats(x, w1, b1, r)
    assert st.shape == (m, 3, 2)
    out = ops.linear_ln_act(s, st, *ops.fold_ln_linear(w2, b2, g, be),
                            act='quick_gelu', eps=EPS)
    y, s0 = ops.layer_norm_residual(F.linear(x, w1, b1), r, g, be, EPS)
    today = ops.linear_act(y, w2, b2, 'quick_gelu')
    ref = ops._apply_act(
        F.linear(F.layer_norm(s.float(), (wd,), g.float(), be.float(), EPS),
                 w2.float(), b2.float()), 'quick_gelu')
    mx, mn = _rel(out, ref)
    print(f'\npair: max-rel {mx:.3e} mean-rel {mn:.3e}; today vs the same '
          f'reference {_rel(today, ref)}')
    assert mx < 3e-2 and mn < 5e-3


def test_vit_block_fold_on_off(dev, monkeypatch):
    """One full block (plus the [CLS] tail) of a width-256, 4-head ViT on
    256 frames x 5 tokens = 1280 rows, so both GEMMs of the block take the
    fused kernels.  Fold on against VFA_NO_LNFOLD=1: within the off path's
    own distance from an fp32 forward."""
    ops = _ops()
    from video_features_amd.models.clip_vit import (ViTConfig,
                                                    VisionTransformer)
    torch.manual_seed(3)
    cfg = ViTConfig(input_resolution=32, patch_size=16, width=256, layers=2,
                    heads=4, output_dim=64)
    m32 = VisionTransformer(cfg).eval()
    with torch.no_grad():
        m32.blocks[0].ln_2.weight.normal_(1.0, 0.3)
        m32.blocks[0].ln_2.bias.normal_(0.0, 0.3)
    mgpu = VisionTransformer(cfg)
    mgpu.load_state_dict(m32.state_dict())
    mgpu = mgpu.to(dev, BF16).eval()
    x = torch.randn(256, 3, 32, 32)
    xg = x.to(dev, BF16)
    monkeypatch.delenv('VFA_NO_LNFOLD', raising=False)
    with torch.no_grad():
        ref = m32(xg.float().cpu())
        assert mgpu.blocks[0].fold_routed(
            torch.empty(256, 5, 256, device=dev, dtype=BF16))
        on = mgpu(xg).float().cpu()
        assert mgpu.blocks[0]._fold is not None
        monkeypatch.setenv('VFA_NO_LNFOLD', '1')
        off = mgpu(xg).float().cpu()
    d_on_off = (on - off).abs().max().item()
    d_off_ref = (off - ref).abs().max().item()
    d_on_ref = (on - ref).abs().max().item()
    print(f'\nViT block: |on - off| {d_on_off:.3e}, |off - fp32| '
          f'{d_off_ref:.3e}, |on - fp32| {d_on_ref:.3e}')
    assert d_on_off <= d_off_ref
