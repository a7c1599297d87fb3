"""RAFT on-the-fly correlation lookup (``ops.corr_lookup_otf``,
``CorrOnTheFly``, ``RAFT(corr=...)``, ``--raft_corr``) on the CPU.

The yardstick is written here and uses nothing of the package: the float64
all-pairs volume ``einsum / sqrt(D)``, its ``avg_pool2d`` pyramid and an
explicit four-tap gather in pixel units with zero outside the level.

Exact cases: features from {-1, 0, 1}, D = 256 and coordinates that are
multiples of 1/2 make every product, pooled value and blend exact in f32 in
any summation order (worst case 22 significant bits at level 3), so the f32
result must be BIT-EQUAL to the float64 yardstick, and the bf16 result equal
to the yardstick rounded once.  Random cases: tol = 4 x the error of the
yardstick's own f32 evaluation (the factor allows for another summation
order of a 256-term f32 dot).
"""
import math

import pytest
import torch
import torch.nn.functional as F

# (B, H8, W8): 17x27 pools to 8x13, 4x6, 2x3 (odd-size floors at every
# step); 8x12 ends in a 1x1 level
SHAPES = [(2, 17, 27), (1, 16, 16)]
SHAPE_1x1 = (1, 8, 12)


# ---------------------------------------------------------------- yardstick
def _taps(planes, cx, cy):
    """planes (N, hl, wl), cx / cy (N,) in the planes' pixel units ->
    (N, 81): tap t = i*9+j is the bilinear sample at (cx + i - 4,
    cy + j - 4), zero outside the plane."""
    n, hl, wl = planes.shape
    d = torch.arange(-4, 5, dtype=planes.dtype)
    sx = (cx[:, None] + d)[:, :, None].expand(n, 9, 9)   # X moves with i
    sy = (cy[:, None] + d)[:, None, :].expand(n, 9, 9)   # Y moves with j
    x0, y0 = torch.floor(sx), torch.floor(sy)
    ax, ay = sx - x0, sy - y0
    x0, y0 = x0.long(), y0.long()
    ni = torch.arange(n)[:, None, None]

    def at(y, x):
        ok = (x >= 0) & (x < wl) & (y >= 0) & (y < hl)
        v = planes[ni, y.clamp(0, hl - 1), x.clamp(0, wl - 1)]
        return v * ok.to(planes.dtype)

    out = ((1 - ax) * (1 - ay) * at(y0, x0) + ax * (1 - ay) * at(y0, x0 + 1)
           + (1 - ax) * ay * at(y0 + 1, x0) + ax * ay * at(y0 + 1, x0 + 1))
    return out.reshape(n, 81)


def yardstick(fmap1, fmap2, coords, levels=4, dtype=torch.float64):
    """fmap1 / fmap2 (B, D, H, W), coords (B, 2, H, W) -> (B, levels*81,
    H, W) in ``dtype``: all-pairs volume, pooled pyramid, four-tap gather."""
    b, d, h, w = fmap1.shape
    corr = torch.einsum('bdhw,bdyx->bhwyx', fmap1.to(dtype),
                        fmap2.to(dtype)) / math.sqrt(d)
    corr = corr.reshape(b * h * w, 1, h, w)
    cx = coords[:, 0].reshape(-1).to(dtype)
    cy = coords[:, 1].reshape(-1).to(dtype)
    out = []
    for lvl in range(levels):
        if lvl:
            corr = F.avg_pool2d(corr, 2, 2)
        out.append(_taps(corr[:, 0], cx / 2 ** lvl, cy / 2 ** lvl))
    return torch.cat(out, dim=1).reshape(b, h, w, -1).permute(0, 3, 1, 2) \
        .contiguous()


# ------------------------------------------------------------------- inputs
def exact_case(b, h, w, d=256, seed=0):
    """Features from {-1, 0, 1}; coords multiples of 1/2 spread over
    [-0.3, 1.3] x size."""
    g = torch.Generator().manual_seed(seed)
    fmap1 = torch.randint(-1, 2, (b, d, h, w), generator=g).float()
    fmap2 = torch.randint(-1, 2, (b, d, h, w), generator=g).float()
    u = torch.rand(b, 2, h, w, generator=g) * 1.6 - 0.3
    size = torch.tensor([w, h], dtype=torch.float32).view(1, 2, 1, 1)
    coords = torch.round(u * size * 2) / 2
    return fmap1, fmap2, coords


def random_case(b, h, w, d=256, seed=1):
    g = torch.Generator().manual_seed(seed)
    fmap1 = torch.randn(b, d, h, w, generator=g)
    fmap2 = torch.randn(b, d, h, w, generator=g)
    u = torch.rand(b, 2, h, w, generator=g) * 1.6 - 0.3
    size = torch.tensor([w, h], dtype=torch.float32).view(1, 2, 1, 1)
    return fmap1, fmap2, u * size


def pixel_major(fmap1, fmap2, levels=4):
    """(f1, f2_levels) as ``ops.corr_lookup_otf`` takes them: f32,
    (B, h, w, D), f2 avg-pooled in f32."""
    f1 = fmap1.permute(0, 2, 3, 1).contiguous()
    lv, f2 = [], fmap2
    for lvl in range(levels):
        if lvl:
            f2 = F.avg_pool2d(f2, 2, 2)
        lv.append(f2.permute(0, 2, 3, 1).contiguous())
    return f1, lv


def random_tol(fmap1, fmap2, coords, ref64):
    """4 x max|f32 evaluation of the yardstick - float64 yardstick|."""
    ref32 = yardstick(fmap1, fmap2, coords, dtype=torch.float32)
    return 4 * (ref32.double() - ref64).abs().max().item()


_CACHE = {}


def cached(kind, shape, d=256):
    """(fmap1, fmap2, coords, float64 yardstick) — computed once per case
    and shared, never modified."""
    key = (kind, shape, d)
    if key not in _CACHE:
        make = exact_case if kind == 'exact' else random_case
        fmap1, fmap2, coords = make(*shape, d=d)
        _CACHE[key] = (fmap1, fmap2, coords,
                       yardstick(fmap1, fmap2, coords))
    return _CACHE[key]


def assert_not_trivial(ref64, levels=4):
    """The yardstick has a non-zero share of at least 0.1 on every level —
    a test against it cannot pass on zeros."""
    for lvl in range(levels):
        share = (ref64[:, lvl * 81:(lvl + 1) * 81] != 0).double().mean().item()
        assert share >= 0.1, (lvl, share)


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize('shape', SHAPES + [SHAPE_1x1])
def test_exact_f32_bit_equal(shape):
    from video_features_amd import ops
    fmap1, fmap2, coords, ref = cached('exact', shape)
    if shape != SHAPE_1x1:      # its 1x1 level holds too few non-zeros
        assert_not_trivial(ref)
    f1, lv = pixel_major(fmap1, fmap2)
    out = ops.corr_lookup_otf(f1, lv, coords)
    assert out.dtype == torch.float32 and out.shape == ref.shape
    assert out.is_contiguous()
    assert torch.equal(out.double(), ref)


@pytest.mark.parametrize('shape', SHAPES)
def test_exact_bf16_rounded_once(shape):
    from video_features_amd import ops
    fmap1, fmap2, coords, ref = cached('exact', shape)
    f1, lv = pixel_major(fmap1, fmap2)
    out = ops.corr_lookup_otf(f1, lv, coords, 4, True, torch.bfloat16)
    assert out.dtype == torch.bfloat16
    assert out.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out, ref.to(torch.bfloat16))


@pytest.mark.parametrize('shape', SHAPES)
def test_random_within_f32_error(shape):
    from video_features_amd import ops
    fmap1, fmap2, coords, ref = cached('random', shape)
    assert_not_trivial(ref)
    tol = random_tol(fmap1, fmap2, coords, ref)
    f1, lv = pixel_major(fmap1, fmap2)
    out = ops.corr_lookup_otf(f1, lv, coords)
    diff = (out.double() - ref).abs().max().item()
    print(f'{shape}: diff {diff:.3e} tol {tol:.3e}')
    assert diff <= tol, (diff, tol)


def test_on_the_fly_matches_all_pairs_path():
    """CorrOnTheFly against the shipped CorrPyramid + ops.corr_lookup on the
    CPU: the f32 tolerance plus the 5e-4 the all-pairs CPU path loses in its
    round trip through [-1, 1] grid coordinates."""
    from video_features_amd.models.raft import CorrOnTheFly, CorrPyramid
    fmap1, fmap2, coords, ref = cached('random', SHAPES[0])
    tol = random_tol(fmap1, fmap2, coords, ref) + 5e-4
    otf = CorrOnTheFly(fmap1, fmap2)
    out = otf(coords)
    shipped = CorrPyramid(fmap1, fmap2)(coords)
    assert out.shape == shipped.shape == (2, 324, 17, 27)
    diff = (out - shipped).abs().max().item()
    print(f'otf vs all-pairs path: diff {diff:.3e} tol {tol:.3e}')
    assert diff <= tol, (diff, tol)
    assert otf.nbytes == sum(t.numel() * 4 for t in [otf.f1, *otf.f2_levels])
    assert [tuple(t.shape[1:3]) for t in otf.f2_levels] == [
        (17, 27), (8, 13), (4, 6), (2, 3)]


def test_one_by_one_level():
    """(1, 8, 12): level 3 is 1x1.  Compared with the yardstick only — the
    all-pairs CPU path mis-places samples on a level 1 wide or 1 high."""
    from video_features_amd.models.raft import CorrOnTheFly
    fmap1, fmap2, coords, ref = cached('random', SHAPE_1x1)
    tol = random_tol(fmap1, fmap2, coords, ref)
    otf = CorrOnTheFly(fmap1, fmap2)
    assert tuple(otf.f2_levels[3].shape) == (1, 1, 1, 256)
    out = otf(coords)
    assert (ref[:, 243:] != 0).any()
    diff = (out.double() - ref).abs().max().item()
    assert diff <= tol, (diff, tol)


def test_tap_order_one_hot():
    """Tap t = i*9+j offsets X by i-4 and Y by j-4: a one-hot f2 at
    (x + 2, y - 3) of the query pixel lights tap 6*9 + 1 alone."""
    from video_features_amd import ops
    h, w, d = 10, 12, 32
    qy, qx = 5, 4
    f1 = torch.zeros(1, h, w, d)
    f1[..., 0] = 1.0
    f2 = torch.zeros(1, h, w, d)
    f2[0, qy - 3, qx + 2, 0] = math.sqrt(d)
    coords = torch.zeros(1, 2, h, w)
    coords[0, 0], coords[0, 1] = float(qx), float(qy)
    out = ops.corr_lookup_otf(f1, [f2], coords)
    assert out.shape == (1, 81, h, w)
    taps = out[0, :, qy, qx]
    assert taps[6 * 9 + 1].item() == pytest.approx(1.0, abs=1e-6)
    assert taps.abs().sum().item() == pytest.approx(1.0, abs=1e-6)


def test_far_and_non_finite_coords_give_zeros():
    from video_features_amd import ops
    fmap1, fmap2, coords, ref = cached('exact', SHAPES[1])
    f1, lv = pixel_major(fmap1, fmap2)
    bad = coords.clone()
    bad[0, 0, 0, :4] = torch.tensor([3e4, -3e4, float('inf'), float('nan')])
    bad[0, 1, 1, :2] = torch.tensor([float('-inf'), 1e30])
    out = ops.corr_lookup_otf(f1, lv, bad)
    assert torch.isfinite(out).all()
    assert (out[0, :, 0, :4] == 0).all() and (out[0, :, 1, :2] == 0).all()
    keep = torch.ones(16, 16, dtype=torch.bool)
    keep[0, :4] = False
    keep[1, :2] = False
    assert torch.equal(out[0][:, keep].double(), ref[0][:, keep])


def test_corr_mode_for_quarter_of_memory():
    from video_features_amd.models.raft import corr_mode_for
    b, h8, w8 = 2, 46, 80
    need = 5.3125 * b * (h8 * w8) ** 2
    assert corr_mode_for(b, h8, w8, int(4 * need) + 4096) == 'allpairs'
    assert corr_mode_for(b, h8, w8, int(4 * need) - 4096) == 'onthefly'
    total = 288 * 1024 ** 3
    assert corr_mode_for(1, 28, 28, total) == 'allpairs'      # 224^2 crop
    assert corr_mode_for(16, 28, 28, total) == 'allpairs'
    assert corr_mode_for(16, 135, 240, total) == 'onthefly'   # 1080p x 16
    assert corr_mode_for(1, 270, 480, total) == 'onthefly'    # one 4K pair


def test_config_and_cli():
    from video_features_amd.cli import build_parser
    from video_features_amd.config import Config, sanity_check
    assert Config().raft_corr == 'allpairs'
    sanity_check(Config(feature_type='raft', raft_corr='auto'))
    with pytest.raises(ValueError, match='raft_corr'):
        sanity_check(Config(feature_type='raft', raft_corr='bogus'))
    parser = build_parser()
    args = parser.parse_args(['--feature_type', 'raft',
                              '--raft_corr', 'onthefly'])
    assert Config.coerce(args).raft_corr == 'onthefly'
    assert Config.coerce(parser.parse_args(
        ['--feature_type', 'raft'])).raft_corr == 'allpairs'
    with pytest.raises(SystemExit):
        parser.parse_args(['--feature_type', 'raft', '--raft_corr', 'bogus'])


def test_extractors_pass_raft_corr(npz_video):
    from video_features_amd.config import Config
    from video_features_amd.extractors.raft import ExtractRAFT
    cfg = Config(feature_type='raft', cpu=True, raft_corr='onthefly',
                 video_paths=[npz_video])
    model = ExtractRAFT(cfg).build_models(torch.device('cpu'), torch.float32)
    assert model.corr == 'onthefly'


def test_raft_corr_argument():
    from video_features_amd.models.raft import (RAFT, CorrOnTheFly,
                                                CorrPyramid)
    torch.manual_seed(0)
    base = RAFT(iters=2).eval()
    same = RAFT(iters=2, corr='allpairs').eval()
    same.load_state_dict(base.state_dict())
    img1 = torch.randint(0, 256, (1, 3, 64, 64)).float()
    img2 = torch.randint(0, 256, (1, 3, 64, 64)).float()
    with torch.no_grad():
        assert torch.equal(base(img1, img2), same(img1, img2))
    fmap = torch.zeros(1, 256, 8, 8)
    assert base._corr_class(fmap) is CorrPyramid
    assert RAFT(corr='onthefly')._corr_class(fmap) is CorrOnTheFly
    assert RAFT(corr='auto')._corr_class(fmap) is CorrPyramid   # CPU
    with pytest.raises(ValueError, match='corr'):
        RAFT(corr='bogus')
