"""The LayerNorm row kernels (layernorm.hip) and InstanceNorm (instancenorm.hip)
on ill-conditioned rows and planes: large offsets, low spread, constant rows,
outliers, mixed within one call.

The inputs, the float64 yardstick and the tolerance rule are those of
tests/test_norm_conditioning.py: |out - ref64| <= 4 E + u(ref64), E the
error of the yardstick's own f32 two-pass evaluation; constant rows within
|w| D 2^-24 |c| / sqrt(eps) + u(bias) and finite.  Every case is a handful of
rows or planes.

Run on MI355X with: pytest tests/test_gpu_norm_conditioning.py -m gpu -q -s
"""
import functools

import pytest
import torch

from test_norm_conditioning import (DIMS, DTYPES, KINDS, PLANES, ROWS, Case,
                                    in_case, ln_case, ln_res_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built in-tree'
    return ops


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_norm(dev, dtype, kind, d):
    x, w, b, case = ln_case(kind, dtype, d)
    out = _ops().layer_norm(x.to(dev), w.to(dev), b.to(dev))
    case.check(out, f'layer_norm {dtype} {kind} d={d}')


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_layer_norm_residual(dev, dtype, kind, d):
    """x and res carry half of the offset each.  s is the f32 sum rounded
    once, y that s normalised with the statistics of the f32 sums."""
    x, res, w, b, s_ref, case = ln_res_case(kind, dtype, d)
    y, s = _ops().layer_norm_residual(x.to(dev), res.to(dev), w.to(dev),
                                      b.to(dev))
    assert torch.equal(s.cpu(), s_ref)
    case.check(y, f'layer_norm_residual {dtype} {kind} d={d}')


@functools.lru_cache(maxsize=None)
def _embed_case(dtype, t, p, width, via):
    """Token j of every frame gets its own conditioning.  via 'pos': pos[j]
    is the offset c_j throughout and the patch embeddings of token j have
    spread s_j, (c_j, s_j) from (0, 1), (100, 1), (-1000, 1), (30, 0.01) in
    turn.  via 'cls': cls = 100 + randn, pos and pe randn, so token 0 is the
    offset row.  The kernel adds in f32, so 30 + 0.01 randn is a true
    low-spread row in bf16 / f16 as well."""
    g = torch.Generator().manual_seed(11 + p)
    pe = torch.randn(t, p, width, generator=g)
    cls = torch.randn(width, generator=g)
    pos = torch.randn(p + 1, width, generator=g)
    if via == 'pos':
        spec = [(0.0, 1.0), (100.0, 1.0), (-1000.0, 1.0), (30.0, 0.01)]
        for j in range(1, p + 1):
            c, s = spec[j % 4]
            pos[j] = c
            pe[:, j - 1] *= s
    else:
        cls += 100.0
    pe, cls, pos = pe.to(dtype), cls.to(dtype), pos.to(dtype)
    w = torch.randn(width, generator=g).to(dtype)
    b = torch.randn(width, generator=g).to(dtype)
    cat = torch.cat([cls.expand(t, 1, width), pe], dim=1)
    x64 = cat.double() + pos.double()
    none_const = torch.zeros(t, p + 1, dtype=torch.bool)
    return pe, cls, pos, w, b, Case(cat, none_const, 0, w, b, x64=x64)


@pytest.mark.parametrize('via', ['pos', 'cls'])
@pytest.mark.parametrize('t,p,width', [(3, 4, 128), (2, 49, 768)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_clip_embed_ln(dev, dtype, t, p, width, via):
    pe, cls, pos, w, b, case = _embed_case(dtype, t, p, width, via)
    out = _ops().clip_embed_ln(pe.to(dev), cls.to(dev), pos.to(dev),
                               w.to(dev), b.to(dev))
    assert out.shape == (t, p + 1, width)
    case.check(out, f'clip_embed_ln {dtype} ({t}, {p}, {width}) via {via}')


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('shape', PLANES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_instance_norm(dev, dtype, shape, nhwc, relu):
    x, case = in_case(dtype, shape, nhwc)
    mf = torch.channels_last if nhwc else torch.contiguous_format
    out = _ops().instance_norm(x.to(dev).contiguous(memory_format=mf),
                               relu=relu, nhwc=nhwc)
    assert out.shape == x.shape
    assert out.is_contiguous(memory_format=mf)   # layout preserved
    case.check(out.contiguous().reshape(case.ref.shape),
               f'instance_norm {dtype} {shape} nhwc={nhwc} relu={relu}',
               relu=relu)


@pytest.mark.parametrize('kind', ['offset', 'lowspread', 'const'])
@pytest.mark.parametrize('d', [768, 8200])
@pytest.mark.parametrize('dtype', DTYPES)
def test_rows_are_independent_under_mixed_conditioning(dev, dtype, d, kind):
    """Row r of the mixed batch is the same row run alone, bit for bit."""
    ops = _ops()
    x, res, w, b, _, _ = ln_res_case(kind, dtype, d)
    x, res, w, b = x.to(dev), res.to(dev), w.to(dev), b.to(dev)
    out = ops.layer_norm(x, w, b)
    y, s = ops.layer_norm_residual(x, res, w, b)
    for r in range(ROWS):
        assert torch.equal(out[r:r + 1], ops.layer_norm(x[r:r + 1], w, b))
        y1, s1 = ops.layer_norm_residual(x[r:r + 1], res[r:r + 1], w, b)
        assert torch.equal(y[r:r + 1], y1)
        assert torch.equal(s[r:r + 1], s1)


def _gpu_still_works(dev):
    a = torch.ones(4, device=dev) + 1
    torch.cuda.synchronize()
    assert a.sum().item() == 8


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('shape', [(0, 8, 5, 7), (3, 0, 5, 7)])
def test_instance_norm_empty(dev, shape, nhwc):
    """No batch or no channels: the empty result, nothing launched."""
    x = torch.empty(shape, device=dev, dtype=torch.bfloat16)
    out = _ops().instance_norm(x, relu=True, nhwc=nhwc)
    assert out.shape == shape and out.dtype == x.dtype
    _gpu_still_works(dev)
