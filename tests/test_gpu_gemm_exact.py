"""Exact-arithmetic GPU tests of the GEMM family (gemm.hip): every route of
ops.linear_act -- the thin streaming kernel, the persistent 256^2 kernel
with and without its guarded edge column, the guarded 256^2 and 128^2
tiles, the 8-phase kernel -- and the two LayerNorm-fold modes of the
persistent kernel's epilogue (ops.linear_res_stats, ops.linear_ln_act).

Method (that of test_gpu_conv_exact.py).  Inputs are small integers held in
bf16, so every bf16 product and every fp32 partial sum is an exact integer
far below 2^24 and the pre-activation value is exact in ANY accumulation
order.  The reference is torch.matmul in float64 (on the GPU for the cases
that run there, on the CPU for the unmarked tests), independent of this
project's kernels.  For act none / relu both sides round the same exact
number to bf16 once, so the comparison is torch.equal: one misplaced
16-byte segment, one wrong row at a strip boundary, one dropped 8-element
K slice or a second rounding fails it.  leaky_relu / quick_gelu / gelu are
inexact in fp32; they get one bf16 ulp of the reference (2^-7 |ref|) plus
an absolute floor measured on the CPU, see ACT_FLOOR.

Two data kinds:
  sym  x in -3..3, w in -2..2: sums stay small (every integer below 256 is
       a bf16), so this kind isolates PLACEMENT;
  pos  x and w in 0..7: |sum| <= 49 K + 16 <= 15696 for K <= 320, typical
       values several hundred to a few thousand, where bf16 spacing is
       2..16, so this kind isolates ROUNDING (an epilogue that rounds the
       accumulator before it adds bias / residual differs from one that
       rounds once; test_pos_kind_has_teeth keeps that true).
Bias and residual are in -8..8 for both.

Every case names its route and asserts it through ops._ext.linear_route
(the host function the launchers themselves call) before running, so
routing drift fails loudly instead of emptying the case.

The unmarked tests at the end run on the CPU and keep the data design
honest: the 2^24 bound, the teeth of the pos kind, and that the tolerance
of the crafted-statistics linear_ln_act test cannot hide swapped rows."""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
ACTS = ['none', 'relu', 'leaky_relu', 'quick_gelu', 'gelu']
ACT_ID = {'none': 0, 'relu': 1, 'quick_gelu': 2, 'gelu': 3, 'leaky_relu': 4}
KINDS = {'sym': ((-3, 3), (-2, 2)), 'pos': ((0, 7), (0, 7))}
BR = 8                       # bias and residual in -BR..BR

# route -> [(M, N, K)]: the smallest shapes that reach each code path
SMALL = [
    (1, 16, 8),              # M = 1 and K below one K-tile
    (129, 256, 128),         # ragged M
    (333, 100, 72),          # ragged everything
    (128, 128, 64),          # exactly one full tile
    (384, 130, 320),         # 5 K-tiles: buffer parity flips; N tail of 2
    (257, 19, 72),           # odd N: 2-byte store alignment
]
P256 = [
    (2560, 3840, 64),        # 150 tiles, one K-tile
    (2560, 3840, 192),
    (4352, 4096, 128),       # 272 tiles: some blocks walk two tiles
    (4608, 3840, 128),       # 270 tiles, 270 % 8 != 0 (XCD remap)
    (2560, 3840, 320),       # odd K-tile count
    (4352, 4096, 192),       # two-tile walk, odd K-tile count: buffer
                             # parity differs at the tile boundary
]
P256_EDGE = [(2560, 3848, 128)]      # tile_base of the guarded column
BIG_GUARD = [
    (2560, 3840, 136),       # ragged K: glds -> guard in the last K-step
    (2560, 3845, 128),       # n % 8 != 0: no persistent kernel
]
P8 = [
    (2048, 2048, 192),       # 64 tiles, minimum K depth
    (4096, 2048, 256),
]
# (M, N, K) -> the N-chunk the launcher picks
THIN = {
    (65536, 16, 64): 16,             # minimum of everything
    (65536 + 37, 24, 72): 32,        # clamped rows, N % 16 = 8, K % 32 = 8
    (65536, 136, 256): 128,          # second N-chunk, of 8 columns
    (65536, 72, 232): 80,            # K % 32 = 8 at KF = 8
    (65536, 64, 144): 64,
    (4096 * 128 + 200, 16, 64): 16,  # the grid-stride loop's second pass,
                                     # ragged end
}
WALK2 = (4352, 4096, 128)            # 256p, two-tile walk
STRIDE2 = (4096 * 128 + 200, 16, 64)  # thin, grid-stride

EXACT_CASES = ([(s, 'small') for s in SMALL] + [(s, '256p') for s in P256]
               + [(s, '256p+edge') for s in P256_EDGE]
               + [(s, 'big_guard') for s in BIG_GUARD])

# one case per route: small ragged, 256p two-tile walk, 256p+edge, thin
MATRIX_CASES = [((333, 100, 72), 'small'), (WALK2, '256p'),
                (P256_EDGE[0], '256p+edge'), ((65536 + 37, 24, 72), 'thin:32')]

# Worst |torch fp32 activation - float64 activation| over the exact
# pre-activation values of every MATRIX_CASES x bias x residual problem of
# the sym kind, as printed by measure_act_floor() below on the CPU:
#   leaky_relu 1.144e-06, quick_gelu 4.058e-07, gelu 2.477e-07
# The comparison allows 4x these, because the kernel evaluates the
# activation with v_exp_f32 / v_rcp_f32 / tanhf (act_f in mfma_tile.h) and
# not with torch's routines.
ACT_FLOOR = {'leaky_relu': 1.144e-06, 'quick_gelu': 4.058e-07,
             'gelu': 2.477e-07}
FLOOR_MARGIN = 4.0

# linear_res_stats: single tile; 3 partials per row; 16 partials per row
# and a two-tile walk
STATS_SHAPES = [(256, 256, 64), (2560, 768, 192), (4352, 4096, 64)]
# f32 roundings a term of M2 passes through, read from epilogue_strips and
# the merge in linear256p_kernel: 8 fma (the strip's squares about its
# mean, 8 elements per lane), 3 DPP adds (sum8), 1 fma (64 d^2 + M2_i in
# the merge), 4 adds (m2 += over the four strips).  Everything else on the
# way -- the 8-element sums, sum8, x 1/64, 0.25 (...) and every d = value -
# mean -- is exact for integer-valued s.
M2_DEPTH = 16
# linear_ln_act
LN_SHAPES = [(256, 256, 64), (2560, 3840, 256)]
LN_ACT_SHAPE = (4352, 4096, 128)


def _ops():
    from video_features_amd import ops
    assert ops.hip_available(), 'HIP extension must be built on a GPU box'
    return ops


def _act64(y, act):
    """The activation in float64 (the kernel's formulas, act_f)."""
    if act == 'relu':
        return y.relu()
    if act == 'leaky_relu':
        return F.leaky_relu(y, 0.1)
    if act == 'quick_gelu':
        return y * torch.sigmoid(1.702 * y)
    if act == 'gelu':
        return F.gelu(y, approximate='tanh')
    return y


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(BF16)


@functools.lru_cache(maxsize=2)
def _inputs(shape, kind):
    """Integer-valued bf16 x (M, K), w (N, K), bias (N), res (M, N) of one
    shape and kind, on the CPU -- built once, shared read-only."""
    m, n, k = shape
    (xl, xh), (wl, wh) = KINDS[kind]
    gen = torch.Generator().manual_seed(m * 7 + n * 3 + k + len(kind))
    return (_ints(gen, (m, k), xl, xh), _ints(gen, (n, k), wl, wh),
            _ints(gen, (n,), -BR, BR), _ints(gen, (m, n), -BR, BR))


@functools.lru_cache(maxsize=2)
def _problem(shape, kind, dev):
    """The inputs on ``dev`` and x @ w^T in float64 there (exact)."""
    x, w, b, r = (t.to(dev) for t in _inputs(shape, kind))
    return x, w, b, r, x.double() @ w.double().t()


def _pre64(shape, kind, dev, use_bias, use_res):
    """Exact pre-activation values in float64."""
    _, _, b, r, y = _problem(shape, kind, dev)
    if use_bias:
        y = y + b.double()
    if use_res:
        y = y + r.double()
    return y


def measure_act_floor():
    """CPU only: worst |fp32 torch activation - float64 activation| over
    the pre-activation values of the epilogue matrix; the source of
    ACT_FLOOR.  Run by hand (python -c 'import ...; measure_act_floor()')
    when MATRIX_CASES or the data ranges change."""
    worst = {a: 0.0 for a in ACT_FLOOR}
    for shape, _ in MATRIX_CASES:
        for ub in (False, True):
            for ur in (False, True):
                pre = _pre64(shape, 'sym', 'cpu', ub, ur)
                for a in worst:
                    d = (_act64(pre.float(), a).double()
                         - _act64(pre, a)).abs()
                    worst[a] = max(worst[a], d.max().item())
    for a, v in worst.items():
        print(f'{a}: {v:.3e}')
    return worst


def _assert_route(ops, shape, act, want):
    m, n, k = shape
    got = ops._ext.linear_route(m, n, k, ACT_ID[act])
    print(f'{shape} act={act}: route {got}')
    assert got == want, (
        f'{shape} act={act} is meant to run the {want} route but goes to '
        f'{got}: change the SHAPE so it reaches its route')
    return got


def _bad_mask(out, ref64, act):
    assert out.dtype == BF16 and out.shape == ref64.shape, \
        (out.dtype, out.shape, ref64.shape)
    if act in ('none', 'relu'):
        return out != ref64.to(BF16)
    tol = ref64.abs() * 2.0 ** -7 + FLOOR_MARGIN * ACT_FLOOR[act]
    return ~((out.double() - ref64).abs() <= tol)        # NaN is bad


def _report(bad, out, ref64, what):
    nbad = int(bad.sum())
    if nbad:
        row, col = bad.nonzero()[0].tolist()
        raise AssertionError(
            f'{what}: {nbad} of {bad.numel()} elements wrong, first at '
            f'(row, col) = {(row, col)}: got {out[row, col].item()} want '
            f'{ref64[row, col].item()}')


def _run(shape, route, kind='sym', act='none', use_bias=True, use_res=False):
    ops = _ops()
    _assert_route(ops, shape, act, route)
    dev = torch.device('cuda:0')
    x, w, b, r, _ = _problem(shape, kind, dev)
    out = ops.linear_act(x, w, b if use_bias else None, act,
                         r if use_res else None)
    ref = _act64(_pre64(shape, kind, dev, use_bias, use_res), act)
    _report(_bad_mask(out, ref, act), out, ref,
            f'{shape} {kind} route={route} act={act} bias={use_bias} '
            f'res={use_res}')
    return out


def _ids(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else None


@gpu
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('shape,route', EXACT_CASES, ids=_ids)
def test_exact(shape, route, kind):
    """Bias, no activation: bit-exact against the float64 reference."""
    _run(shape, route, kind)


@gpu
@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('shape', P8, ids=_ids)
def test_exact_8p(shape, kind, use_res):
    """The 8-phase kernel's default share: act none, 64..149 full tiles."""
    _run(shape, '8p', kind, 'none', True, use_res)


@gpu
@pytest.mark.parametrize('use_bias,use_res',
                         [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize('act', ['none', 'relu'])
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('shape', list(THIN), ids=_ids)
def test_exact_thin(shape, kind, act, use_bias, use_res):
    """The thin streaming kernel, N-chunking pinned.  On the pos kind with
    bias or residual this fails for an epilogue that rounds the
    accumulator to bf16 before adding them."""
    _run(shape, f'thin:{THIN[shape]}', kind, act, use_bias, use_res)


@gpu
@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('use_bias', [True, False])
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape,route', MATRIX_CASES, ids=_ids)
def test_epilogue_matrix(shape, route, act, use_bias, use_res):
    """Every activation x bias / None x residual / none, one case per
    route, sym kind.  none and relu are bit-exact; leaky_relu, quick_gelu
    and gelu allow 2^-7 |ref| + 4 * ACT_FLOOR[act]."""
    _run(shape, route, 'sym', act, use_bias, use_res)


@gpu
@pytest.mark.parametrize('shape,route', [(WALK2, '256p'),
                                         (STRIDE2, 'thin:16')], ids=_ids)
def test_run_twice_bit_identical(shape, route):
    """A race between the next tile's staging and the epilogue's LDS bounce
    (256p), or between two passes of the grid-stride loop over the bounce
    tile (thin), would show as run-to-run differences."""
    o1 = _run(shape, route, 'pos', 'relu', True, True)
    o2 = _run(shape, route, 'pos', 'relu', True, True)
    assert torch.equal(o1, o2)


def _child(switch):
    """Body of the forced-route child process: the 8p shapes, every
    activation with bias and residual, the same exact comparison."""
    sys.path.insert(0, ROOT)
    want = {'VFA_8P': ['8p', '8p'], 'VFA_NO_8P': ['small', 'small']}[switch]
    for shape, route in zip(P8, want):
        for kind in KINDS:
            for act in ACTS:
                if kind == 'pos' and act not in ('none', 'relu'):
                    continue
                _run(shape, route, kind, act, True, True)
    torch.cuda.synchronize()
    print('CHILD-OK')


@gpu
@pytest.mark.parametrize('switch', ['VFA_8P', 'VFA_NO_8P'])
def test_forced_route_child(switch):
    """The route switch is read once into a static, so the forced routes
    run in a fresh process each: the 8-phase kernel with every activation
    (VFA_8P) and the 128^2 tile on the same shapes (VFA_NO_8P).  The child
    asserts linear_route itself."""
    env = {k: v for k, v in os.environ.items()
           if k not in ('VFA_8P', 'VFA_NO_8P')}
    env[switch] = '1'
    p = subprocess.run([sys.executable, os.path.abspath(__file__), 'child',
                        switch], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert 'CHILD-OK' in p.stdout


# ------------------------------------------------------- linear_res_stats
@gpu
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('shape', STATS_SHAPES, ids=_ids)
def test_res_stats_exact(shape, kind):
    """s bit-equal to the float64 value rounded once; the mean partials
    bit-equal to the float64 mean of each 256-column group of the rounded
    s (an integer / 256: every step the kernel takes to it is exact); M2
    within 2 * M2_DEPTH * 2^-24 relative of the float64 M2 of the same
    rounded values (all terms non-negative, no term passes through more
    than M2_DEPTH = 16 f32 roundings, counted at M2_DEPTH above)."""
    ops = _ops()
    m, n, k = shape
    dev = torch.device('cuda:0')
    x, w, b, r, _ = _problem(shape, kind, dev)
    assert ops.fused_ln_tiles(x, w)
    s, part = ops.linear_res_stats(x, w, b, r)
    ref = _pre64(shape, kind, dev, True, True)
    _report(_bad_mask(s, ref, 'none'), s, ref, f'res_stats s {shape} {kind}')
    assert part.shape == (m, n // 256, 2) and part.dtype == torch.float32
    g = ref.to(BF16).double().reshape(m, n // 256, 256)
    mean64 = g.mean(2)
    m2_64 = ((g - mean64[..., None]) ** 2).sum(2)
    assert torch.equal(mean64.float().double(), mean64)
    bad = part[..., 0] != mean64.float()
    _report(bad, part[..., 0], mean64, f'res_stats mean {shape} {kind}')
    err = (part[..., 1].double() - m2_64).abs()
    rel = (err / m2_64.clamp_min(1e-300)).max().item()
    print(f'res_stats {shape} {kind}: M2 max rel err {rel:.3e}')
    bad = ~(err <= 2 * M2_DEPTH * 2.0 ** -24 * m2_64)
    _report(bad, part[..., 1], m2_64, f'res_stats M2 {shape} {kind}')


# ---------------------------------------- linear_ln_act, crafted statistics
def _ln_inputs(shape, groups):
    """Crafted problem for linear_ln_act, on the CPU.

    Row r gets the integer mean mu_r = (37 r) mod 257 - 128 -- distinct
    over any 256 consecutive rows, and different for r and r + 256 -- and
    the variance 4^e_r, e_r = r mod 7 - 3, so rstd = 2^-e_r.  The
    statistics are NOT computed from the rows: s = mu_r + (-3..3), so that
    s W'^T - mu c is small and a row that is handed another row's mean is
    off by (d mu) c, many times its own value.  The pair is split over
    ``groups`` partials with different group means mu_r +- 2^(e_r - 1)
    (and +- 2^(e_r - 2)) -- powers of two scaled with the row's spread,
    integer offsets would exceed the smallest variances -- and different
    group M2, so the epilogue's Chan merge has work to do; with power-of-
    two groups and K every step of that merge is exact in f32.
    -> s (M, K) bf16, stats (M, groups, 2) f32, W' (N, K) bf16, c (N) f32
    (the row sums of W'), b' (N) f32, mu (M) f64, var (M) f64."""
    m, n, k = shape
    gen = torch.Generator().manual_seed(m + n * 5 + k * 11 + groups)
    rows = torch.arange(m)
    mu = ((37 * rows) % 257 - 128).double()
    e = (rows % 7 - 3).double()
    var = 4.0 ** e
    s = (mu[:, None] + torch.randint(-3, 4, (m, k), generator=gen)).to(BF16)
    wf = _ints(gen, (n, k), -2, 2)
    c = wf.double().sum(1).float()
    bf = torch.randint(-BR, BR + 1, (n,), generator=gen).float()
    d1, d2 = 2.0 ** (e - 1), 2.0 ** (e - 2)
    if groups == 1:
        gm = mu[:, None]
        q = (k * var)[:, None]
    elif groups == 2:
        # between-group part K d1^2 = K var / 4; the rest split 1 : 2
        gm = torch.stack([mu + d1, mu - d1], 1)
        q = (k * var / 4)[:, None] * torch.tensor([1.0, 2.0])
    else:
        assert groups == 4
        # between-group part (K/4) 2 (d1^2 + d2^2) = K var 5/32
        gm = torch.stack([mu + d1, mu - d1, mu + d2, mu - d2], 1)
        q = (k * var / 32)[:, None] * torch.tensor([3.0, 6.0, 8.0, 10.0])
    stats = torch.stack([gm, q], 2)
    # the merge the consumer does, in float64: must give (mu, var) back
    gmean = gm.mean(1)
    m2 = (q + (k / groups) * (gm - gmean[:, None]) ** 2).sum(1)
    assert torch.equal(gmean, mu) and torch.equal(m2 / k, var)
    assert torch.equal(stats.float().double(), stats)
    return s, stats.float().contiguous(), wf, c, bf, mu, var


def _ln_ref(acc, mu, var, c, bf, act):
    """act(rstd (acc - mu c) + b') in float64 and its tolerance: 2^-8 |ref|
    for the one bf16 rounding plus 2^-20 (rstd (|acc| + |mu c|) + |b'|)
    for rsqrtf and the three f32 fused operations -- 16 f32 ulps of the
    largest intermediate -- plus the activation's floor."""
    rstd = var.rsqrt()[:, None]
    muc = mu[:, None] * c.double()
    ref = _act64(rstd * (acc - muc) + bf.double(), act)
    tol = ref.abs() * 2.0 ** -8 + 2.0 ** -20 * (
        rstd * (acc.abs() + muc.abs()) + bf.double().abs())
    if act in ACT_FLOOR:
        tol = tol + FLOOR_MARGIN * ACT_FLOOR[act]
    return ref, tol


def _run_ln(shape, groups, act):
    ops = _ops()
    dev = torch.device('cuda:0')
    s, stats, wf, c, bf, mu, var = (t.to(dev)
                                    for t in _ln_inputs(shape, groups))
    assert ops.fused_ln_tiles(s, wf)
    out = ops.linear_ln_act(s, stats, wf, c, bf, act, eps=0.0)
    ref, tol = _ln_ref(s.double() @ wf.double().t(), mu, var, c, bf, act)
    assert out.dtype == BF16 and out.shape == ref.shape
    bad = ~((out.double() - ref).abs() <= tol)
    _report(bad, out, ref, f'linear_ln_act {shape} groups={groups} {act}')


@gpu
@pytest.mark.parametrize('groups', [1, 2, 4])
@pytest.mark.parametrize('shape', LN_SHAPES, ids=_ids)
def test_ln_act_crafted_stats(shape, groups):
    """The row -> (mean, rstd) pairing of EPI_LN: every row of a tile has
    its own mean and rstd, so a lane that fetches a neighbour's pair is
    loudly wrong (test_ln_tolerance_sees_swapped_rows)."""
    _run_ln(shape, groups, 'none')


@gpu
@pytest.mark.parametrize('act', ACTS)
def test_ln_act_crafted_stats_acts(act):
    """Every activation on the two-tile walk, 4 partials per row."""
    _run_ln(LN_ACT_SHAPE, 4, act)


# --------------------------------------------------------------- CPU tests
ALL_SHAPES = (SMALL + P256 + P256_EDGE + BIG_GUARD + P8 + list(THIN)
              + STATS_SHAPES)


@pytest.mark.parametrize('kind', list(KINDS))
def test_sums_stay_below_2_24(kind):
    """Every partial sum of every shape x kind is an integer below 2^24,
    so fp32 accumulation is exact in any order."""
    (xl, xh), (wl, wh) = KINDS[kind]
    big = max(abs(xl), abs(xh)) * max(abs(wl), abs(wh))
    for m, n, k in ALL_SHAPES:
        assert big * k + 2 * BR < 2 ** 24, (m, n, k)
    # linear_ln_act: |s| <= 131, |w| <= 2
    for m, n, k in LN_SHAPES + [LN_ACT_SHAPE]:
        assert 131 * 2 * k + 128 * 2 * k < 2 ** 24


@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('shape', list(THIN), ids=_ids)
def test_pos_kind_has_teeth(shape, use_res):
    """On the pos kind of each thin case with bias (and residual), an
    epilogue that rounds the accumulator to bf16, adds bias / residual in
    f32 and rounds again differs from the single rounding in at least 10 %
    of the elements.  A condition on the data, not a measurement: if a
    case falls below, change the data."""
    x, w, b, r = _inputs(shape, 'pos')
    acc = (x.double() @ w.double().t()).float()          # exact
    add = b.float().expand_as(acc)
    if use_res:
        add = add + r.float()
    once = (acc + add).to(BF16)
    twice = (acc.to(BF16).float() + add).to(BF16)
    frac = (once != twice).float().mean().item()
    print(f'{shape} res={use_res}: round-twice differs in {frac:.1%}')
    assert frac >= 0.10, frac


@pytest.mark.parametrize('shape,groups',
                         [(LN_SHAPES[0], 2), (LN_SHAPES[1], 4),
                          (LN_ACT_SHAPE, 1)], ids=_ids)
def test_ln_tolerance_sees_swapped_rows(shape, groups):
    """Row i of the first tile evaluated with row j's statistics, for every
    pair i != j of the tile (first 256 columns): at least one element of
    the row leaves the tolerance of _ln_ref.  So no exchange of statistics
    between two rows of a tile can pass test_ln_act_crafted_stats.  The
    pattern continues with another phase in the next tiles."""
    s, _, wf, c, bf, mu, var = _ln_inputs(shape, groups)
    s, wf, c, bf = s[:512], wf[:256], c[:256], bf[:256]
    acc = s.double() @ wf.double().t()
    for t0 in (0, 256):
        if t0 >= s.shape[0]:
            break
        a, m_, v_ = acc[t0:t0 + 256], mu[t0:t0 + 256], var[t0:t0 + 256]
        ref, tol = _ln_ref(a, m_, v_, c, bf, 'none')
        seen = torch.zeros(256, 256, dtype=torch.bool)
        for j in range(256):         # every row with row j's statistics
            alt, _ = _ln_ref(a, m_[j].expand(256), v_[j].expand(256), c, bf,
                             'none')
            seen[:, j] = ((alt - ref).abs() > tol).any(1)
        seen |= torch.eye(256, dtype=torch.bool)
        assert bool(seen.all()), (
            f'{int((~seen).sum())} (row, other row) pairs of tile {t0} pass '
            f'with swapped statistics, first {(~seen).nonzero()[0].tolist()}')
    # and the same statistics one tile further are another row's
    if s.shape[0] > 256:
        assert not torch.equal(mu[:256], mu[256:512])


if __name__ == '__main__' and sys.argv[1:2] == ['child']:
    _child(sys.argv[2])
