"""LayerNorm and InstanceNorm on ill-conditioned inputs: the yardstick, the
inputs and the tolerance rule, on the CPU.  tests/test_gpu_norm_conditioning.py
imports them and applies them to the HIP kernels.

Inputs.  Every case is a batch of ROWS rows (or a few planes) that mixes
conditionings, so a row that picked up a neighbour's statistics is far off:
  randn      well-conditioned rows, mean ~ 0: the control
  threshold  c + randn with |c| around 1, both sides of the point (variance
             = mean^2) where the kernels change the way they form the variance
  offset     c + randn for c in {100, -1000}
  lowspread  30 + 0.01 randn (f32); a few adjacent representable values
             around 30 (bf16, f16)
  const      rows that are 30.1, 77.7, 123.456 or 0.1 throughout
  outlier    randn with one element at 1000, first or last in the row: easy
             for sumsq/d - mean^2, bad for a shift by the row's first element

Yardstick.  The float64 evaluation of (x - mean) / sqrt(var + eps) * w + b
on the inputs as the kernel gets them (rounded to the dtype).  Its own f32
two-pass evaluation (mean, then the mean of (x - mean)^2) gives E = max
|two-pass - float64| over the non-constant rows of the case.

Rule.  |out - ref64| <= 4 E + u(ref64) per element; u = 0 for f32 output
(its rounding is inside E), for bf16 / f16 the spacing of the output dtype at
|ref64| (one output rounding with a binade of slack).

Constant rows.  Every x - mean is a rounding error of the mean, E says
nothing and eps dominates: |out - b_i| <= |w_i| D 2^-24 |c| / sqrt(eps) +
u(b_i), D the number of f32 additions between an element and the row sum in
the kernel (ln_depth / in_depth below), and every output finite.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

EPS = 1e-5
ROWS = 9  # leaves the wave path's 4-row block partly filled
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# test_gpu_layernorm.py's DIMS: a scalar tail, the wave / block boundary from
# both sides, a block-path tail for every dtype
DIMS = [8, 100, 768, 4096, 4102, 8200]
KINDS = ['randn', 'threshold', 'offset', 'lowspread', 'const', 'outlier']
ILL = ['offset', 'lowspread']
# hw below the 16 NHWC sub-rows; hw below the 256 NCHW threads and a c tail;
# c tail at full size; c == 64
PLANES = [(1, 8, 1, 5), (3, 72, 5, 7), (2, 96, 37, 53), (1, 64, 64, 96)]
CONSTS = [30.1, 77.7, 123.456, 0.1]
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}


def spacing(v, dtype):
    """Distance between neighbouring ``dtype`` values at |v| (float64)."""
    e = torch.frexp(v.double().abs())[1] - 1          # |v| in [2^e, 2^(e+1))
    e = e.clamp(min=MIN_EXP[dtype]).double()
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def _adjacent(g, shape, c, dtype):
    """Values c + k * spacing(c), k in {-1, 0, 1, 2}: exact in ``dtype``."""
    c = torch.tensor(c).to(dtype).double()
    k = torch.randint(-1, 3, shape, generator=g).double()
    return c + k * spacing(c, dtype)


def _row(g, d, spec, dtype, half):
    """One row (float64) for a spec: ('const', c) | ('low', c) |
    ('out', index) | ('first', value of element 0) | (c, spread).  ``half``
    halves offsets, constants and outliers: two such rows sum to a full
    one."""
    f = 0.5 if half else 1.0
    if spec[0] == 'const':
        return torch.full((d,), float(torch.tensor(spec[1] * f).to(dtype)),
                          dtype=torch.float64)
    if spec[0] == 'low':
        if dtype == torch.float32:
            return spec[1] * f + 0.01 * torch.randn(d, generator=g).double()
        return _adjacent(g, (d,), spec[1] * f, dtype)
    if spec[0] == 'out':
        x = torch.randn(d, generator=g).double()
        x[spec[1]] = 1000.0 * f
        return x
    if spec[0] == 'first':
        x = torch.randn(d, generator=g).double()
        x[0] = spec[1] * f
        return x
    return spec[0] * f + spec[1] * torch.randn(d, generator=g).double()


SPECS = {
    'randn': [(0.0, 1.0)] * ROWS,
    'threshold': [(c, 1.0) for c in
                  (0.8, -0.9, 1.0, -1.1, 1.25, 0.95, -1.05, 2.0, -0.5)],
    'offset': [(100.0, 1.0), (-1000.0, 1.0), (0.0, 1.0)] * 3,
    'lowspread': [('low', 30.0)] * 4 + [(0.0, 1.0)] + [('low', 30.0)] * 4,
    'const': [('const', c) for c in CONSTS] + [(0.0, 1.0)]
             + [('const', c) for c in CONSTS],
    'outlier': [('out', 0), ('out', -1)] * 4 + [('out', 0)],
}


def ln_rows(kind, dtype, d, seed=0, half=False):
    """(x (ROWS, d) in ``dtype``, is_const (ROWS,) bool)."""
    g = torch.Generator().manual_seed(1000 * seed + d)
    specs = SPECS[kind]
    x = torch.stack([_row(g, d, s, dtype, half) for s in specs]).to(dtype)
    return x, torch.tensor([s[0] == 'const' for s in specs])


@functools.lru_cache(maxsize=None)
def ln_affine(dtype, d):
    g = torch.Generator().manual_seed(7 + d)
    return (torch.randn(d, generator=g).to(dtype),
            torch.randn(d, generator=g).to(dtype))


def in_planes(dtype, shape, seed=0):
    """(x (b, c, h, w) in ``dtype``, is_const (b, c) bool): plane (i, j) takes
    offset and spread from kinds (a)-(d) in turn.  The kernels sum about a
    plane's first value and sweep again if that lies more than sqrt(15)
    sigma from the mean, so three planes put it at 1000, 3.5 and 4.5."""
    b, c, h, w = shape
    specs = [(0.0, 1.0), (100.0, 1.0), ('const', 30.1), ('low', 30.0),
             (-1000.0, 1.0), ('first', 1000.0), ('first', 3.5),
             ('first', 4.5), ('const', 123.456), (1.0, 3.0), ('const', 77.7),
             ('const', 0.1)]
    g = torch.Generator().manual_seed(seed + h * w)
    pick = [specs[i % len(specs)] for i in range(b * c)]
    x = torch.stack([_row(g, h * w, s, dtype, False) for s in pick])
    return (x.reshape(b, c, h, w).to(dtype),
            torch.tensor([s[0] == 'const' for s in pick]).reshape(b, c))


# ---------------------------------------------------------------- yardstick
def norm_ref(x, w=None, b=None, dtype=torch.float64, stats_of=None):
    """Two-pass normalisation of the last dim in ``dtype``; mean and variance
    are those of ``stats_of`` where it is given."""
    x = x.to(dtype)
    v = x if stats_of is None else stats_of.to(dtype)
    mean = v.mean(-1, keepdim=True)
    c = v - mean
    y = (x - mean) * torch.rsqrt((c * c).mean(-1, keepdim=True) + EPS)
    return y if w is None else y * w.to(dtype) + b.to(dtype)


class Case:
    """Yardstick and bound for rows ``x`` (..., n) in the kernel's dtype.
    ``x64`` replaces their values where the kernel forms the rows itself
    (clip_embed_ln: the exact sum; its f32 rounding is then part of E).
    ``stats64``: the rows whose mean and variance normalise ``x``
    (layer_norm_residual: the exact sums, x being their rounded copy)."""

    def __init__(self, x, is_const, depth, w=None, b=None, x64=None,
                 stats64=None):
        self.dtype = x.dtype
        x64 = x.double() if x64 is None else x64
        self.ref = norm_ref(x64, w, b, stats_of=stats64)
        ref32 = norm_ref(
            x64.float(), w, b, torch.float32,
            None if stats64 is None else stats64.float()).double()
        live = ~is_const
        self.E = (ref32 - self.ref)[live].abs().max().item() if live.any() \
            else 0.0
        self.u = torch.zeros_like(self.ref) if self.dtype == torch.float32 \
            else spacing(self.ref, self.dtype)
        # constant rows: |w| D 2^-24 |c| / sqrt(eps) + u(bias)
        wabs = torch.ones(x.shape[-1], dtype=torch.float64) if w is None \
            else w.double().abs()
        bias = torch.zeros(x.shape[-1], dtype=torch.float64) if b is None \
            else b.double()
        ub = 0.0 if self.dtype == torch.float32 else spacing(bias, self.dtype)
        cval = x64[..., :1].abs()
        const_bound = wabs * depth * 2.0 ** -24 * cval / math.sqrt(EPS) + ub
        self.is_const = is_const
        self.const_bound = const_bound.expand_as(self.ref)[is_const]

    def bound(self, E=None):
        bound = 4 * (self.E if E is None else E) + self.u
        bound[self.is_const] = self.const_bound
        return bound

    def _errors(self, out, relu, E):
        ref = self.ref.relu() if relu else self.ref
        err = (out.double().cpu() - ref).abs()
        err = torch.where(torch.isfinite(err), err,
                          torch.full_like(err, math.inf))
        bound = self.bound(E)
        return err, bound, err / bound

    def worst(self, out, relu=False, E=None, rows=None):
        """(max error, max error / bound) of ``out`` against the yardstick,
        a non-finite output counting as an infinite error; over the rows
        selected by the bool mask ``rows`` if given."""
        err, _, ratio = self._errors(out, relu, E)
        if rows is not None:
            err, ratio = err[rows], ratio[rows]
        return err.max().item(), ratio.max().item()

    def check(self, out, what, relu=False, E=None):
        """Print the largest error and the element closest to (or furthest
        beyond) its bound, then assert the rule."""
        err, bound, ratio = self._errors(out, relu, E)
        i = ratio.argmax()
        print(f'{what}: E {self.E if E is None else E:.3e}  max err '
              f'{err.max().item():.3e}  worst element: err '
              f'{err.flatten()[i].item():.3e} bound '
              f'{bound.flatten()[i].item():.3e}')
        err, ratio = err.max().item(), ratio.max().item()
        assert torch.isfinite(out.float()).all(), what
        assert ratio <= 1.0, (what, err, ratio)


# D: f32 additions between an element and the row sum, as the kernels are
# built.  layernorm.hip: a lane adds the VEC elements of each of its 16-B
# vectors (every STRIDE-th vector of the row) and its share of the scalar
# tail in sequence, then 6 butterfly steps across the wave; the block path
# (d > 4096, 512 threads) adds the 8 wave sums in sequence.  The largest is
# d = 4096: 64 + 6 = 70.
def ln_depth(d, dtype, wave_only=False):
    vec = 16 // torch.tensor([], dtype=dtype).element_size()
    stride = 64 if (wave_only or d <= 4096) else 512
    dvec = d // vec
    lane = vec * -(-dvec // stride) + -(-(d - dvec * vec) // stride)
    return lane + 6 + (0 if stride == 64 else 8)


# instancenorm.hip.  NCHW: 256 threads stride the plane, 6 butterfly steps in
# the wave, 6 more over the wave sums.  NHWC: a lane's 16 sub-rows stride the
# pixels, then 15 additions in sequence.  The largest here is 64*96 NHWC:
# 384 + 15 = 399.
def in_depth(hw, nhwc):
    return -(-hw // 16) + 15 if nhwc else -(-hw // 256) + 12


@functools.lru_cache(maxsize=None)
def ln_case(kind, dtype, d):
    x, is_const = ln_rows(kind, dtype, d)
    w, b = ln_affine(dtype, d)
    return x, w, b, Case(x, is_const, ln_depth(d, dtype), w, b)


@functools.lru_cache(maxsize=None)
def ln_res_case(kind, dtype, d):
    """x and res carry half the offset each.  The op returns s, the f32 sum
    rounded once, and y, that s normalised with the mean and variance of the
    f32 sums; the yardstick is the same in float64 with the exact sums."""
    x, is_const = ln_rows(kind, dtype, d, seed=1, half=True)
    res, _ = ln_rows(kind, dtype, d, seed=2, half=True)
    w, b = ln_affine(dtype, d)
    s = (x.float() + res.float()).to(dtype)
    return x, res, w, b, s, Case(s, is_const, ln_depth(d, dtype), w, b,
                                 stats64=x.double() + res.double())


@functools.lru_cache(maxsize=None)
def in_case(dtype, shape, nhwc):
    x, is_const = in_planes(dtype, shape)
    b, c, h, w = shape
    case = Case(x.reshape(b, c, h * w), is_const, in_depth(h * w, nhwc))
    return x, case


# ------------------------------------------------- emulation of the kernels
def _lane_sums(vals, lanes, vec):
    """vals (rows, n) f32 -> (rows, lanes): lane l adds, in f32 and in index
    order, the ``vec`` elements of every ``lanes``-th group and its share of
    the tail, as the kernels' strided loops do."""
    rows, n = vals.shape
    nvec = n // vec
    steps = -(-nvec // lanes)
    body = np.zeros((rows, steps * lanes, vec), np.float32)
    body[:, :nvec] = vals[:, :nvec * vec].reshape(rows, nvec, vec)
    body = body.reshape(rows, steps, lanes, vec)
    tail = vals[:, nvec * vec:]
    tsteps = -(-tail.shape[1] // lanes)
    tpad = np.zeros((rows, tsteps * lanes), np.float32)
    tpad[:, :tail.shape[1]] = tail
    acc = np.zeros((rows, lanes), np.float32)
    for s in range(steps):
        for j in range(vec):
            acc = acc + body[:, s, :, j]
    for s in range(tsteps):
        acc = acc + tpad[:, s * lanes:(s + 1) * lanes]
    return acc


def _tree(v):
    """Butterfly over the last axis (a power of two), f32."""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _row_sum(vals, lanes, vec, serial):
    """The kernels' sum of each row: strided lane sums, a butterfly per group
    of 64 lanes (or per lane when ``serial`` covers single lanes), then the
    groups in sequence (``serial``) or in a second butterfly."""
    acc = _lane_sums(vals, lanes, vec)
    if lanes > 16:
        acc = _tree(acc.reshape(acc.shape[0], -1, 64))
    if not serial:
        return _tree(acc)
    tot = acc[:, 0]
    for k in range(1, acc.shape[1]):
        tot = tot + acc[:, k]
    return tot


def emulate(x, layout, centre):
    """(mean, var) in f32 per row of x (rows, n) with the kernels' summation
    structure.  ``layout``: ('ln', dtype) | 'nchw' | 'nhwc'.  ``centre`` False
    is the one-pass formula sumsq/n - mean^2 throughout.  True is what the
    kernels do now: LayerNorm re-forms the variance of a row with var <=
    mean^2 from a sweep about the mean; InstanceNorm sums about the plane's
    first value k and sweeps again if (mean - k)^2 > 15 var."""
    vals = x.float().numpy()
    rows, n = vals.shape
    if layout == 'nchw':
        lanes, vec, serial = 256, 1, False
    elif layout == 'nhwc':
        lanes, vec, serial = 16, 1, True
    else:
        vec = 16 // torch.tensor([], dtype=layout[1]).element_size()
        lanes, serial = (64, False) if n <= 4096 else (512, True)
    nf = np.float32(n)

    def total(v):
        return _row_sum(v.astype(np.float32), lanes, vec, serial)
    with np.errstate(all='ignore'):
        if centre and layout in ('nchw', 'nhwc'):
            k = vals[:, :1]
            m = total(vals - k) / nf
            mean = k[:, 0] + m
            var = total((vals - k) * (vals - k)) / nf - m * m
            redo = ~(m * m <= np.float32(15) * var)
        else:
            mean = total(vals) / nf
            var = total(vals * vals) / nf - mean * mean
            redo = ~(var > mean * mean)
        if centre:
            c = vals - mean[:, None]
            mean = np.where(redo, mean + total(c) / nf, mean)
            var = np.where(redo, total(c * c) / nf, var)
    return mean.astype(np.float32), var.astype(np.float32)


def emulated_out(x, layout, centre, w=None, b=None):
    """f32 output of the emulated kernel, as a torch tensor shaped like x."""
    flat = x.reshape(-1, x.shape[-1])
    mean, var = emulate(flat, layout, centre)
    with np.errstate(all='ignore'):
        rstd = (np.float32(1) / np.sqrt(var + np.float32(EPS))) \
            .astype(np.float32)
        y = (flat.float().numpy() - mean[:, None]) * rstd[:, None]
        if w is not None:
            y = y * w.float().numpy() + b.float().numpy()
    return torch.from_numpy(y.astype(np.float32)).reshape(x.shape)


# -------------------------------------------------------------------- tests
def twin_E(case, f32_case):
    """E for torch's CPU kernels on a bf16 / f16 case.  Rows of 16-bit values
    within a factor 2 of c lie on a grid of at most 2^12 points, so every f32
    sum of d <= 8192 of them is exact, and at d = 8 and 4096 so is the mean:
    E shrinks to the rounding of the last few operations (8e-7 where the f32
    case of the same kind has 1e-4) and the rule asks for an all but exact
    result.  The HIP kernels are held to that, their sums being exact as
    well.  torch's Welford update rounds the running mean at every step and
    is off by a few ulp of c whatever the inputs, so it is held to the E of
    the same kind and size built in f32, where the sums round."""
    return max(case.E, f32_case.E)


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_torch_layer_norm_is_inside_the_rule(dtype, kind, d):
    """An independent f32 implementation stays inside the rule: the inputs
    and the rule are sound.  For bf16 / f16 with E of the f32 case of the
    same kind, see twin_E."""
    x, w, b, case = ln_case(kind, dtype, d)
    out = F.layer_norm(x.float(), (d,), w.float(), b.float(), EPS).to(dtype)
    case.check(out, f'torch layer_norm {dtype} {kind} d={d}',
               E=twin_E(case, ln_case(kind, torch.float32, d)[-1]))
    # for the residual op torch supplies the statistics of the f32 sums
    x, res, w, b, s, case = ln_res_case(kind, dtype, d)
    v = x.float() + res.float()
    var, mean = torch.var_mean(v, -1, unbiased=False, keepdim=True)
    out = ((s.float() - mean) * torch.rsqrt(var + EPS) * w.float()
           + b.float()).to(dtype)
    case.check(out, f'torch residual {dtype} {kind} d={d}',
               E=twin_E(case, ln_res_case(kind, torch.float32, d)[-1]))


@pytest.mark.parametrize('shape', PLANES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_torch_instance_norm_is_inside_the_rule(dtype, shape):
    for nhwc in (False, True):   # the two layouts differ in D only
        x, case = in_case(dtype, shape, nhwc)
        out = F.instance_norm(x.float(), eps=EPS).to(dtype)
        case.check(out.reshape(case.ref.shape),
                   f'torch instance_norm {dtype} {shape} nhwc={nhwc}',
                   E=twin_E(case, in_case(torch.float32, shape, nhwc)[-1]))


def _ratio(case, out):
    err, ratio = case.worst(out)
    return err, (err / case.E if case.E else math.inf), ratio


@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('kind', KINDS)
def test_one_pass_layer_norm_breaks_the_rule(kind, d):
    """sumsq/d - mean^2 with the kernel's summation structure, f32: outside
    the rule on every offset and lowspread case; the centred variance the
    kernel forms now is inside it on every case."""
    dtype = torch.float32
    x, w, b, case = ln_case(kind, dtype, d)
    layout = ('ln', dtype)
    err, per_e, ratio = _ratio(case, emulated_out(x, layout, False, w, b))
    print(f'one-pass layer_norm {kind} d={d}: E {case.E:.3e}  err {err:.3e}  '
          f'err/E {per_e:.1f}  err/bound {ratio:.2f}')
    if kind in ILL:
        assert ratio > 1.0
    new = emulated_out(x, layout, True, w, b)
    case.check(new, f'centred layer_norm {kind} d={d}')


@pytest.mark.parametrize('nhwc', [False, True])
@pytest.mark.parametrize('shape', PLANES)
def test_one_pass_instance_norm_breaks_the_rule(shape, nhwc):
    """Every plane batch holds offset and lowspread planes."""
    x, case = in_case(torch.float32, shape, nhwc)
    layout = 'nhwc' if nhwc else 'nchw'
    flat = x.reshape(case.ref.shape)
    err, per_e, ratio = _ratio(case, emulated_out(flat, layout, False))
    print(f'one-pass instance_norm {shape} nhwc={nhwc}: E {case.E:.3e}  '
          f'err {err:.3e}  err/E {per_e:.1f}  err/bound {ratio:.2f}')
    _, bad = case.worst(emulated_out(flat, layout, False),
                        rows=~case.is_const)
    assert bad > 1.0
    case.check(emulated_out(flat, layout, True),
               f'centred instance_norm {shape} nhwc={nhwc}')


def _const_breaks(case, out):
    return case.worst(out, rows=case.is_const)[1] > 1.0


def test_one_pass_breaks_on_constant_rows():
    """At least one constant case per op where sumsq/n - mean^2 is outside
    the derived bound or not finite."""
    hits = []
    for d in DIMS:
        x, w, b, case = ln_case('const', torch.float32, d)
        out = emulated_out(x, ('ln', torch.float32), False, w, b)
        hits.append(_const_breaks(case, out))
        print(f'one-pass layer_norm const d={d}: '
              f'finite {bool(torch.isfinite(out).all())}  breaks {hits[-1]}')
    assert any(hits)
    hits = []
    for shape in PLANES:
        for nhwc in (False, True):
            x, case = in_case(torch.float32, shape, nhwc)
            out = emulated_out(x.reshape(case.ref.shape),
                               'nhwc' if nhwc else 'nchw', False)
            hits.append(_const_breaks(case, out))
            print(f'one-pass instance_norm const {shape} nhwc={nhwc}: '
                  f'finite {bool(torch.isfinite(out).all())}  '
                  f'breaks {hits[-1]}')
    assert any(hits)


@pytest.mark.parametrize('dtype', DTYPES[1:])
def test_which_16_bit_cases_discriminate(dtype):
    """The output rounding hides most of the effect in bf16 / f16; those
    cases mainly carry finiteness.  Printed, not asserted."""
    for kind in ILL + ['const']:
        for d in DIMS:
            x, w, b, case = ln_case(kind, dtype, d)
            out = emulated_out(x, ('ln', dtype), False, w, b).to(dtype)
            err, ratio = case.worst(out)
            print(f'one-pass layer_norm {dtype} {kind} d={d}: err {err:.3e} '
                  f'err/bound {ratio:.2f} '
                  f'{"discriminates" if ratio > 1 else "-"}')
    for shape in PLANES:
        for nhwc in (False, True):
            x, case = in_case(dtype, shape, nhwc)
            out = emulated_out(x.reshape(case.ref.shape),
                               'nhwc' if nhwc else 'nchw', False).to(dtype)
            err, ratio = case.worst(out)
            print(f'one-pass instance_norm {dtype} {shape} nhwc={nhwc}: '
                  f'err {err:.3e} err/bound {ratio:.2f} '
                  f'{"discriminates" if ratio > 1 else "-"}')


def test_depths():
    assert ln_depth(4096, torch.float32) == 70
    assert ln_depth(4096, torch.bfloat16) == 70
    assert ln_depth(8200, torch.bfloat16) == 24 + 6 + 8
    assert ln_depth(100, torch.float32) == 4 + 6
    assert ln_depth(4102, torch.bfloat16) == 8 + 1 + 6 + 8
    assert in_depth(64 * 96, True) == 399
    assert in_depth(5, False) == 13
