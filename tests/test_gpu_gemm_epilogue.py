"""The 256x256 GEMM tile boundary: the persistent full-tile kernel
(cross-tile prefetch, XCD remap remainders, ragged end of the tile walk),
the shared vectorised epilogue under both 256^2 kernels (every activation,
with and without bias / residual), the guarded edge column beside it, and
the leaky_relu activation id.

Reference and tolerances are those of test_gpu_gemm.py: fp32 torch,
max|err| / max|ref| < 3e-2 and mean|err| / mean|ref| < 5e-3.  K stays tiny
so every case is milliseconds of GPU work."""
import functools
import os
import subprocess
import sys

import pytest
import torch

gpu = pytest.mark.gpu

ACTS = ['none', 'relu', 'quick_gelu', 'gelu', 'leaky_relu']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from video_features_amd import ops
    assert ops.hip_available()
    return ops


def _act(y, act):
    if act == 'relu':
        return y.relu()
    if act == 'quick_gelu':
        return y * torch.sigmoid(1.702 * y)
    if act == 'gelu':
        return torch.nn.functional.gelu(y, approximate='tanh')
    if act == 'leaky_relu':
        return torch.nn.functional.leaky_relu(y, 0.1)
    return y


@functools.lru_cache(maxsize=3)
def _problem(m, n, k):
    """Inputs and the fp32 pre-activation references of one shape, built
    once and shared (read-only) by every case on that shape."""
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(m * 7 + n * 3 + k)
    x = (torch.randn(m, k, device=dev, generator=g) / (k ** 0.25)) \
        .to(torch.bfloat16)
    w = (torch.randn(n, k, device=dev, generator=g) / (k ** 0.25)) \
        .to(torch.bfloat16)
    b = torch.randn(n, device=dev, generator=g).to(torch.bfloat16)
    r = torch.randn(m, n, device=dev, generator=g).to(torch.bfloat16)
    y = torch.nn.functional.linear(x.float(), w.float())
    return x, w, b, r, y


ACT_ID = {'none': 0, 'relu': 1, 'quick_gelu': 2, 'gelu': 3, 'leaky_relu': 4}


def _check(m, n, k, act, bias=True, res=False, route=None):
    """route: the kernel the case is meant for, asserted through
    ops._ext.linear_route (the host function the launchers call) so that
    routing drift fails instead of silently emptying the case."""
    ops = _ops()
    if route is not None:
        got = ops._ext.linear_route(m, n, k, ACT_ID[act])
        assert got == route, (
            f'{(m, n, k)} act={act} is meant to run the {route} route but '
            f'goes to {got}: change the SHAPE so it reaches its route')
    x, w, b, r, y = _problem(m, n, k)
    out = ops.linear_act(x, w, b if bias else None, act, r if res else None)
    assert out.shape == (m, n) and out.dtype == torch.bfloat16
    ref = y
    if bias:
        ref = ref + b.float()
    if res:
        ref = ref + r.float()
    ref = _act(ref, act)
    err = (out.float() - ref).abs()
    rel = err.max().item() / max(ref.abs().max().item(), 1e-6)
    mean = (err.mean() / ref.abs().mean().clamp_min(1e-6)).item()
    print(f'{(m, n, k)} {act} bias={bias} res={res}: '
          f'max-rel {rel:.3e} mean-rel {mean:.3e}')
    assert rel < 3e-2, rel
    assert mean < 5e-3, mean


# tiles = (M/256) * ceil(N/256); the 256^2 route needs >= 150
PERSISTENT_SHAPES = [
    (2560, 3840, 64),     # 150 tiles, one per block; 1 K-tile
    (2560, 3840, 128),    # 2 K-tiles
    (2560, 3840, 192),    # 3 K-tiles
    (4352, 4096, 128),    # 272 tiles > 256 CUs: some blocks walk 2 tiles
    (4608, 3840, 128),    # 270 tiles, 270 % 8 != 0: XCD remap remainder
    (13056, 2560, 128),   # 510 tiles, ~2 per block, 510 % 8 = 6
    (2560, 3848, 128),    # N tail: persistent interior + guarded column
    (2560, 3840, 136),    # ragged K on the 256^2 route
]


@gpu
@pytest.mark.parametrize('m,n,k', PERSISTENT_SHAPES)
def test_tile_walk(m, n, k):
    route = ('256p+edge' if n % 256 else '256p') if k % 64 == 0 \
        else 'big_guard'
    _check(m, n, k, 'quick_gelu', route=route)


@gpu
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('m,n,k', [(4352, 4096, 128), (2560, 3848, 128)])
def test_epilogue_specialisations(m, n, k, act, bias, res):
    _check(m, n, k, act, bias, res,
           route='256p+edge' if n % 256 else '256p')


@gpu
@pytest.mark.parametrize('m,n,k', [(256, 128, 64), (333, 100, 72)])
def test_leaky_relu_small_tile(m, n, k):
    _check(m, n, k, 'leaky_relu', route='small')


@gpu
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('m,n,k', [(4096, 2048, 768), (4096, 256, 192)])
def test_8phase_shapes(m, n, k, act):
    # by default only act none on the 128-tile shape is the 8-phase
    # kernel's (64..149 full tiles); test_forced_route_child runs the rest
    route = '8p' if (n == 2048 and act == 'none') else 'small'
    _check(m, n, k, act, True, True, route=route)


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
from video_features_amd import ops
assert ops.hip_available()
dev = torch.device('cuda:0')
torch.manual_seed(0)
m, n, k = 4096, 2048, 768
x = (torch.randn(m, k, device=dev) / (k ** 0.25)).to(torch.bfloat16)
w = (torch.randn(n, k, device=dev) / (k ** 0.25)).to(torch.bfloat16)
b = torch.randn(n, device=dev).to(torch.bfloat16)
r = torch.randn(m, n, device=dev).to(torch.bfloat16)
y = torch.nn.functional.linear(x.float(), w.float(), b.float()) + r.float()
F = torch.nn.functional
refs = {'none': y, 'relu': y.relu(),
        'quick_gelu': y * torch.sigmoid(1.702 * y),
        'gelu': F.gelu(y, approximate='tanh'),
        'leaky_relu': F.leaky_relu(y, 0.1)}
for act, ref in refs.items():
    out = ops.linear_act(x, w, b, act, r)
    err = (out.float() - ref).abs()
    rel = err.max().item() / ref.abs().max().item()
    mean = (err.mean() / ref.abs().mean()).item()
    print(act, rel, mean)
    assert rel < 3e-2 and mean < 5e-3, (act, rel, mean)
torch.cuda.synchronize()
print('CHILD-OK')
'''


@gpu
@pytest.mark.parametrize('switch', ['VFA_8P', 'VFA_NO_8P'])
def test_forced_route_child(switch):
    """The route switch is read once into a static, so the kernel the
    default routing does not pick is exercised in a fresh process: every
    activation with bias and residual under the 8-phase kernel (VFA_8P)
    and under the 2-buffer kernels (VFA_NO_8P)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ('VFA_8P', 'VFA_NO_8P')}
    env[switch] = '1'
    p = subprocess.run([sys.executable, '-c', _CHILD, ROOT], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert 'CHILD-OK' in p.stdout


@gpu
def test_run_twice_bit_identical():
    """A race between the next tile's glds and the epilogue's LDS bounce
    would show as run-to-run differences."""
    ops = _ops()
    x, w, b, r, _ = _problem(4352, 4096, 128)
    o1 = ops.linear_act(x, w, b, 'quick_gelu', r)
    o2 = ops.linear_act(x, w, b, 'quick_gelu', r)
    assert torch.equal(o1, o2)


def test_leaky_relu_cpu_fallback():
    from video_features_amd import ops
    torch.manual_seed(0)
    x = torch.randn(37, 24)
    w = torch.randn(19, 24)
    b = torch.randn(19)
    out = ops.linear_act(x, w, b, 'leaky_relu')
    ref = torch.nn.functional.leaky_relu(
        torch.nn.functional.linear(x, w, b), 0.1)
    assert torch.equal(out, ref)
    neg = ref < 0
    assert neg.any() and not torch.equal(out, ref.relu())
