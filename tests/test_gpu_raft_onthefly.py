"""GPU tests of the on-the-fly RAFT correlation lookup (``corr_otf`` kernel
behind ``ops.corr_lookup_otf``, ``CorrOnTheFly``, ``RAFT(corr='onthefly')``).

The yardstick, the inputs and the tolerance rule are those of
tests/test_raft_corr_onthefly.py: the float64 all-pairs volume evaluated on
the CPU.  Exact cases must be bit-equal to it on the device; random cases
within 4 x the yardstick's own f32 evaluation error.

Run on MI355X with: pytest tests/test_gpu_raft_onthefly.py -m gpu -x -q
"""
import pytest
import torch

from test_raft_corr_onthefly import (SHAPE_1x1, SHAPES, cached, pixel_major,
                                     random_tol)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _hip_loaded():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built in-tree'
    return ops


def _on_device(fmap1, fmap2, coords, dev):
    f1, lv = pixel_major(fmap1, fmap2)
    return f1.to(dev), [t.to(dev) for t in lv], coords.to(dev)


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('shape', SHAPES + [SHAPE_1x1])
def test_exact_bit_equal(dev, shape, dtype, nhwc):
    ops = _hip_loaded()
    fmap1, fmap2, coords, ref = cached('exact', shape)
    f1, lv, cc = _on_device(fmap1, fmap2, coords, dev)
    out = ops.corr_lookup_otf(f1, lv, cc, 4, nhwc, dtype)
    assert out.dtype == dtype and out.shape == ref.shape
    if nhwc:
        assert out.is_contiguous(memory_format=torch.channels_last)
    else:
        assert out.is_contiguous()
    assert (ref != 0).double().mean().item() > 0.1
    assert torch.equal(out.cpu(), ref.to(dtype))


@pytest.mark.parametrize('shape,d', [(SHAPES[0], 256), (SHAPES[1], 256),
                                     (SHAPE_1x1, 256), (SHAPES[1], 128)])
def test_random_within_f32_error(dev, shape, d):
    """D = 128 covers the channel loop bound (4 of the 8 chunks)."""
    ops = _hip_loaded()
    fmap1, fmap2, coords, ref = cached('random', shape, d)
    tol = random_tol(fmap1, fmap2, coords, ref)
    f1, lv, cc = _on_device(fmap1, fmap2, coords, dev)
    out = ops.corr_lookup_otf(f1, lv, cc)
    diff = (out.cpu().double() - ref).abs().max().item()
    print(f'{shape} D={d}: diff {diff:.3e} tol {tol:.3e}')
    assert diff <= tol, (diff, tol)


@pytest.mark.parametrize('nhwc', [False, True])
def test_far_away_coords_are_zero(dev, nhwc):
    """+-3e4 and whole rows beyond every border return exact zeros (the
    kernel clamps floor() before the int conversion); the other pixels stay
    bit-equal."""
    ops = _hip_loaded()
    fmap1, fmap2, coords, ref = cached('exact', SHAPES[0])
    h, w = SHAPES[0][1:]
    bad = coords.clone()
    bad[0, 0, 0, :] = 3e4               # a row far right
    bad[0, 1, 1, :] = -3e4              # a row far above
    bad[1, 0, 2, :] = -3e4
    bad[1, 1, 2, :] = 3e4
    bad[1, 0, 3, :] = w + 5.0           # just beyond: window misses level 0
    bad[1, 1, 4, :] = -6.0              # ... and the coarser levels too:
    bad[1, 0, 5, :] = -48.0             # |x / 8| - 5 > 0
    far = torch.zeros(2, h, w, dtype=torch.bool)
    far[0, 0] = far[0, 1] = far[1, 2] = far[1, 5] = True
    f1, lv, _ = _on_device(fmap1, fmap2, coords, dev)
    out = ops.corr_lookup_otf(f1, lv, bad.to(dev), 4, nhwc).cpu()
    po = out.permute(0, 2, 3, 1)
    assert (po[far] == 0).all()
    assert (po[1, 3][:, :81] == 0).all() and (po[1, 4][:, :81] == 0).all()
    keep = torch.ones(2, h, w, dtype=torch.bool)
    keep[0, :2] = False
    keep[1, 2:6] = False
    assert torch.equal(po[keep].double(), ref.permute(0, 2, 3, 1)[keep])


def test_refusals(dev):
    ops = _hip_loaded()
    fmap1, fmap2, coords, _ = cached('exact', SHAPES[1])
    f1, lv, cc = _on_device(fmap1, fmap2, coords, dev)
    with pytest.raises(RuntimeError, match='unsupported dtype'):
        ops.corr_lookup_otf(f1, lv, cc, 4, False, torch.float64)
    strided = f1.permute(0, 2, 1, 3)            # square map: same shape
    assert not strided.is_contiguous()
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.corr_lookup_otf(strided, lv, cc)
    with pytest.raises(RuntimeError):
        ops.corr_lookup_otf(f1, [lv[0], lv[1][..., :128]], cc)


def test_memory_is_linear(dev):
    """Constructing CorrOnTheFly on (1, 256, 64, 96) maps and one lookup
    peak at no more than 4 x (|f1| + |f2| + |out|), about 82 MB; level 0 of
    the all-pairs volume alone is 151 MB at this shape."""
    from video_features_amd.models.raft import CorrOnTheFly
    _hip_loaded()
    torch.manual_seed(0)
    fmap1 = torch.randn(1, 256, 64, 96, device=dev)
    fmap2 = torch.randn(1, 256, 64, 96, device=dev)
    coords = torch.rand(1, 2, 64, 96, device=dev) * 60
    out_bytes = 324 * 64 * 96 * 4
    bound = 4 * (fmap1.numel() * 4 + fmap2.numel() * 4 + out_bytes)
    assert bound < 4 * (64 * 96) ** 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    otf = CorrOnTheFly(fmap1, fmap2)
    out = otf(coords)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f'peak increase {peak / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB')
    assert out.shape == (1, 324, 64, 96)
    assert peak <= bound, (peak, bound)
    held = [otf.f1, *otf.f2_levels]
    assert otf.nbytes == sum(t.numel() * t.element_size() for t in held)
    assert all(t.dtype == torch.float32 for t in held)


@pytest.fixture(scope='module')
def raft_runs(dev):
    """One set of weights, images 128x136, iters=4: the f32 all-pairs
    forward on the CPU and the f32 / bf16 forwards on the GPU per layout and
    correlation mode."""
    from video_features_amd.models.raft import RAFT
    _hip_loaded()
    torch.manual_seed(0)
    cpu = RAFT(iters=4).eval()
    img1 = torch.randint(0, 256, (1, 3, 128, 136)).float()
    img2 = torch.randint(0, 256, (1, 3, 128, 136)).float()
    runs = {}
    with torch.no_grad():
        runs['cpu'] = cpu(img1, img2)
        for corr in ('allpairs', 'onthefly'):
            for nhwc in (False, True):
                for dtype in (torch.float32, torch.bfloat16):
                    if dtype == torch.bfloat16 and not nhwc:
                        continue
                    m = RAFT(iters=4, corr=corr).eval()
                    m.load_state_dict(cpu.state_dict())
                    m = m.to(dev, dtype)
                    if nhwc:
                        m = m.use_channels_last()
                    runs[corr, nhwc, dtype] = m(
                        img1.to(dev), img2.to(dev)).float().cpu()
    return runs


@pytest.mark.parametrize('nhwc', [False, True])
def test_raft_on_the_fly_within_f32_reordering(raft_runs, nhwc):
    """d_otf = max|onthefly_GPU - allpairs_GPU| is at most d_ref =
    max|allpairs_GPU - allpairs_CPU|: d_ref is what f32 reordering costs on
    this model, and the two modes differ by a reordering only.

    Measured on the MI355X (outputs reach |1.4|), three runs.  Contiguous:
    d_otf 1.013e-6 and 1.073e-6 against d_ref 1.431e-6.  channels_last:
    d_otf 1.907e-6 against d_ref 1.818e-6 in the first run — a MISS by
    5 % — and 1.788e-6 against 1.907e-6 in a later one, which passed, as
    did the run inside the whole suite: the f32 GPU forwards themselves
    differ in the last bits from process to process.  Both sides sit on
    the model's f32 noise floor: on the CPU, changing each correlation
    value by one ulp at random moves this output by 1.2e-6 to 1.8e-6, and
    an exactly rounded (float64) correlation by 1.1e-6.  The lookup itself
    is within 6.1e-7 of the float64 yardstick where 4 x its f32 error
    allows 3.5e-6 to 1.7e-5 (test_random_within_f32_error), so no change
    to the kernel moves d_otf below that floor; the bound stays as set and
    the channels_last case can miss it."""
    ap = raft_runs['allpairs', nhwc, torch.float32]
    otf = raft_runs['onthefly', nhwc, torch.float32]
    assert otf.shape == ap.shape == (1, 2, 128, 136)
    d_ref = (ap - raft_runs['cpu']).abs().max().item()
    d_otf = (otf - ap).abs().max().item()
    print(f'nhwc={nhwc}: d_otf {d_otf:.3e} d_ref {d_ref:.3e}')
    assert d_otf <= d_ref, (d_otf, d_ref)


def test_raft_on_the_fly_bf16(raft_runs):
    """The bf16 channels_last on-the-fly forward tracks the bf16 all-pairs
    forward, and the f32 GPU forward, at least as closely as
    test_raft_bf16_vs_fp32 asks of the all-pairs path (cos > 0.9)."""
    cos = torch.nn.functional.cosine_similarity
    f32 = raft_runs['allpairs', False, torch.float32].flatten()
    ap = raft_runs['allpairs', True, torch.bfloat16].flatten()
    otf = raft_runs['onthefly', True, torch.bfloat16].flatten()
    c_pair = cos(otf, ap, dim=0).item()
    c_f32 = cos(otf, f32, dim=0).item()
    c_ap = cos(ap, f32, dim=0).item()
    print(f'cos otf/ap {c_pair:.4f} otf/f32 {c_f32:.4f} ap/f32 {c_ap:.4f}')
    assert c_pair > 0.9 and c_f32 > 0.9, (c_pair, c_f32, c_ap)
