"""The LayerNorm row kernels (layernorm.hip): ``layer_norm``,
``layer_norm_residual`` and ``clip_embed_ln`` on both reduction paths (wave
per row for d <= 4096, block per row above), f32 / bf16 / f16.

Every case is a handful of rows.  Besides the f64 reference comparison the
file pins what the three ops share: they are one two-pass row loop, so on
data whose sums are exact they agree bit for bit.

Run on MI355X with: pytest tests/test_gpu_layernorm.py -m gpu -q
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# test_gpu_ops.py::test_layer_norm's bounds; f16 rounds finer than bf16, so
# the bf16 bound holds for it a fortiori
TOL = {torch.float32: 1e-4, torch.bfloat16: 6e-2, torch.float16: 6e-2}
# a scalar tail (100), the wave / block boundary from both sides (4096, 4102)
# and a block-path tail for every dtype (4102 % 4 and % 8 != 0)
DIMS = [8, 100, 768, 4096, 4102, 8200]
ROWS = 9  # a partly filled 4-row block on the wave path


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built in-tree'
    return ops


@functools.lru_cache(maxsize=None)
def _randn_case(dtype, d):
    """(x, w, b, res) drawn as in test_gpu_ops.py::test_layer_norm, and the
    f64 references of LN(x) and LN(x + res).  Shared, never written to."""
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = torch.randn(ROWS, d, device=dev, dtype=dtype)
    w = torch.randn(d, device=dev, dtype=dtype)
    b = torch.randn(d, device=dev, dtype=dtype)
    res = torch.randn(ROWS, d, device=dev, dtype=dtype)
    ref = F.layer_norm(x.double(), (d,), w.double(), b.double())
    ref_res = F.layer_norm(x.double() + res.double(), (d,), w.double(),
                           b.double())
    return x, w, b, res, ref, ref_res


def _int_case(dtype, shape, d, seed):
    """Integer-valued rows in [-8, 8] (sums of two are exact in every
    dtype), weight in {0.5, 1, 2}, integer bias."""
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(seed)

    def ints(*s):
        return torch.randint(-8, 9, s, generator=g).to(dev, dtype)
    w = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (d,), generator=g)]
    return ints(*shape, d), ints(*shape, d), w.to(dev, dtype), ints(d)


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_norm_vs_f64(dev, dtype, d):
    ops = _ops()
    x, w, b, _, ref, _ = _randn_case(dtype, d)
    err = (ops.layer_norm(x, w, b).double() - ref).abs().max().item()
    print(f'layer_norm {dtype} d={d}: max err {err:.3e}')
    assert err < TOL[dtype]


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_norm_residual_vs_f64(dev, dtype, d):
    ops = _ops()
    x, w, b, res, _, ref = _randn_case(dtype, d)
    y, s = ops.layer_norm_residual(x, res, w, b)
    err = (y.double() - ref).abs().max().item()
    print(f'layer_norm_residual {dtype} d={d}: max err {err:.3e}')
    assert err < TOL[dtype]
    # s is the f32 sum, rounded once
    assert torch.equal(s, (x.float() + res.float()).to(dtype))


@pytest.mark.parametrize('d', [768, 8200])
@pytest.mark.parametrize('dtype', DTYPES)
def test_residual_is_layer_norm_of_sum(dev, dtype, d):
    ops = _ops()
    x, res, w, b = _int_case(dtype, (5,), d, seed=1)
    y, s = ops.layer_norm_residual(x, res, w, b)
    assert torch.equal(s, x + res)
    assert torch.equal(y, ops.layer_norm(x + res, w, b))


@pytest.mark.parametrize('t,p,width', [(3, 4, 128), (2, 49, 768)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_clip_embed_ln_is_layer_norm_of_sum(dev, dtype, t, p, width):
    ops = _ops()
    pe, _, w, b = _int_case(dtype, (t, p), width, seed=2)
    pos, _, _, cls = _int_case(dtype, (p + 1,), width, seed=3)
    x = torch.cat([cls.expand(t, 1, width), pe], dim=1) + pos
    out = ops.clip_embed_ln(pe, cls, pos, w, b)
    assert out.shape == (t, p + 1, width)
    assert torch.equal(out, ops.layer_norm(x, w, b))


@pytest.mark.parametrize('rows', [1, 3, 5])
@pytest.mark.parametrize('d', [768, 8200])
@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_are_independent(dev, dtype, d, rows):
    """Row r of a batched call is the same row run alone, bit for bit."""
    ops = _ops()
    x, w, b, res, _, _ = _randn_case(dtype, d)
    x, res = x[:rows], res[:rows]
    out = ops.layer_norm(x, w, b)
    y, s = ops.layer_norm_residual(x, res, w, b)
    for r in range(rows):
        assert torch.equal(out[r:r + 1], ops.layer_norm(x[r:r + 1], w, b))
        y1, s1 = ops.layer_norm_residual(x[r:r + 1], res[r:r + 1], w, b)
        assert torch.equal(y[r:r + 1], y1)
        assert torch.equal(s[r:r + 1], s1)


@pytest.mark.parametrize('d', [64, 8192])
@pytest.mark.parametrize('dtype', DTYPES)
def test_constant_rows_give_bias(dev, dtype, d):
    """sum = 3 d and sumsq = 9 d are exact, so sumsq/d - mean^2 is exactly 0,
    every x - mean is 0 and the result is the bias."""
    ops = _ops()
    _, w, b, _, _, _ = _randn_case(dtype, 8200)
    w, b = w[:d], b[:d]
    x = torch.full((5, d), 3.0, device=dev, dtype=dtype)
    assert torch.equal(ops.layer_norm(x, w, b), b.expand(5, d))
    y, s = ops.layer_norm_residual(x - 2, x - 1, w, b)
    assert torch.equal(s, x)
    assert torch.equal(y, b.expand(5, d))


def _gpu_still_works(dev):
    a = torch.ones(4, device=dev) + 1
    torch.cuda.synchronize()
    assert a.sum().item() == 8


def test_zero_rows(dev):
    ops = _ops()
    x = torch.empty(0, 64, device=dev, dtype=torch.bfloat16)
    w = torch.ones(64, device=dev, dtype=torch.bfloat16)
    assert ops.layer_norm(x, w, w).shape == (0, 64)
    y, s = ops.layer_norm_residual(x, x, w, w)
    assert y.shape == (0, 64) and s.shape == (0, 64)
    _gpu_still_works(dev)


def test_clip_embed_ln_zero_frames(dev):
    ops = _ops()
    pe = torch.empty(0, 4, 64, device=dev, dtype=torch.bfloat16)
    w = torch.ones(64, device=dev, dtype=torch.bfloat16)
    pos = torch.ones(5, 64, device=dev, dtype=torch.bfloat16)
    assert ops.clip_embed_ln(pe, w, pos, w, w).shape == (0, 5, 64)
    _gpu_still_works(dev)


def test_residual_checks_affine_size(dev):
    ops = _ops()
    x = torch.ones(3, 64, device=dev, dtype=torch.bfloat16)
    short = torch.ones(32, device=dev, dtype=torch.bfloat16)
    full = torch.ones(64, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='affine shape mismatch'):
        ops.layer_norm_residual(x, x, short, full)
    with pytest.raises(RuntimeError, match='affine shape mismatch'):
        ops.layer_norm_residual(x, x, full, short)
