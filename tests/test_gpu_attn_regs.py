"""The ViT-length attention kernels: ``ops.mhsa_fused`` for N <= 64 (the
register-resident kernel, variant 0, against the general flash kernel's
single-tile branch, variant 1) and ``ops.attention_pool``.

The layout tests make the softmax exactly one-hot, so a wrong key order,
transpose or operand map shows as a wrong ROW, not as a tolerance miss: with
K[j] = 32 e_j and Q[i] = 32 e_pi(i) the scaled scores are 128 on the selected
key and 0 elsewhere, exp(-128) underflows to 0 in f32, P is one-hot, l = 1 and
the output is V[pi(i)] bit for bit.  The torch paths give exactly that too, so
the same cases run on the CPU in the plain suite."""
import pytest
import torch

from video_features_amd import ops

D = 64
NS = [1, 17, 32, 33, 50, 64]
POOL_LS = [1, 7, 8, 9, 50, 64, 65, 145]
NEW, OLD = 0, 1          # mhsa_fused variants

DEVICES = ['cpu', pytest.param('cuda:0', marks=pytest.mark.gpu)]


def one_hot_qkv(b, h, n, device, seed):
    """(qkv (b, n, 3*h*64) bf16, expected output (b, n, h*64))."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(b, h, n, D)
    k = torch.zeros(b, h, n, D)
    v = torch.randn(b, h, n, D, generator=g).to(torch.bfloat16).float()
    want = torch.empty(b, h, n, D)
    for bi in range(b):
        for hi in range(h):
            pi = torch.randperm(n, generator=g)
            k[bi, hi, torch.arange(n), torch.arange(n)] = 32.0
            q[bi, hi, torch.arange(n), pi] = 32.0
            want[bi, hi] = v[bi, hi, pi]
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4)   # (b, n, 3, h, d)
    qkv = qkv.reshape(b, n, 3 * h * D).to(torch.bfloat16).to(device)
    want = want.permute(0, 2, 1, 3).reshape(b, n, h * D).to(torch.bfloat16)
    return qkv, want.to(device)


@pytest.mark.parametrize('variant', [NEW, OLD])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('device', DEVICES)
def test_mhsa_one_hot_rows(device, n, variant):
    qkv, want = one_hot_qkv(2, 3, n, device, seed=n)
    out = ops.mhsa_fused(qkv, 3, variant=variant)
    assert torch.equal(out, want)


@pytest.mark.parametrize('l', POOL_LS)
@pytest.mark.parametrize('device', DEVICES)
def test_attention_pool_one_hot(device, l):
    """One selected key per (b, h): q = 32 e_a, the selected key is 32 e_a,
    every other key 32 e_c with c != a."""
    b, h = 2, 3
    g = torch.Generator().manual_seed(l)
    q = torch.zeros(b, h, D)
    k = torch.zeros(b, l, h, D)
    v = torch.randn(b, l, h, D, generator=g).to(torch.bfloat16).float()
    want = torch.empty(b, h, D)
    for bi in range(b):
        for hi in range(h):
            a = int(torch.randint(D, (1,), generator=g))
            sel = int(torch.randint(l, (1,), generator=g))
            other = (a + 1 + torch.randint(D - 1, (l,), generator=g)) % D
            k[bi, torch.arange(l), hi, other] = 32.0
            k[bi, sel, hi] = 0.0
            k[bi, sel, hi, a] = 32.0
            q[bi, hi, a] = 32.0
            want[bi, hi] = v[bi, sel, hi]
    kv = torch.cat([k.reshape(b, l, h * D), v.reshape(b, l, h * D)], -1)
    out = ops.attention_pool(q.reshape(b, h * D).to(torch.bfloat16).to(device),
                             kv.to(torch.bfloat16).to(device), h)
    assert torch.equal(out, want.reshape(b, h * D).to(torch.bfloat16)
                       .to(device))


def sdpa_fp32(qkv, h):
    b, n, _ = qkv.shape
    q, k, v = qkv.float().view(b, n, 3, h, D).permute(2, 0, 3, 1, 4).unbind(0)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q, k, v, scale=1.0 / D ** 0.5)
    return ref.permute(0, 2, 1, 3).reshape(b, n, h * D)


@pytest.mark.gpu
@pytest.mark.parametrize('h', [1, 12])
@pytest.mark.parametrize('n', NS)
def test_regs_vs_fp32_and_old(n, h):
    """3e-2 absolute against fp32 SDPA (the bound of test_gpu_flash.py), and
    no more than 1.25x the old variant's error on the same input: both round
    P to bf16 and differ only in summation order."""
    torch.manual_seed(0)
    qkv = torch.randn(3, n, 3 * h * D, device='cuda:0', dtype=torch.bfloat16)
    ref = sdpa_fp32(qkv, h)
    e_new = (ops.mhsa_fused(qkv, h, variant=NEW).float() - ref).abs().max()
    e_old = (ops.mhsa_fused(qkv, h, variant=OLD).float() - ref).abs().max()
    print(f'n={n} h={h} err new {e_new.item():.3e} old {e_old.item():.3e}')
    assert e_new.item() < 3e-2, (n, h, e_new.item())
    assert e_new.item() <= 1.25 * e_old.item(), (e_new.item(), e_old.item())


@pytest.mark.gpu
def test_regs_persistent_walk():
    """The launch has at most 768 blocks of 4 waves and a unit is one (pair,
    32-query block): 270 x 12 pairs x 2 = 6480 units over 3072 waves is 2
    rounds plus a remainder of 336, so some waves walk 3 units and most 2."""
    torch.manual_seed(2)
    b, n, h = 270, 50, 12
    qkv = torch.randn(b, n, 3 * h * D, device='cuda:0', dtype=torch.bfloat16)
    new = ops.mhsa_fused(qkv, h, variant=NEW).float()
    old = ops.mhsa_fused(qkv, h, variant=OLD).float()
    ref = sdpa_fp32(qkv, h)
    e_new = (new - ref).abs().max().item()
    e_old = (old - ref).abs().max().item()
    print(f'walk: err new {e_new:.3e} old {e_old:.3e} '
          f'new-old {(new - old).abs().max().item():.3e}')
    assert e_new < 3e-2
    assert e_new <= 1.25 * e_old


@pytest.mark.gpu
@pytest.mark.parametrize('n', [33, 50])
def test_regs_softmax_stability(n):
    """The x8-scaled inputs of test_gpu_flash's stability test."""
    torch.manual_seed(1)
    b, h = 2, 4
    qkv = (torch.randn(b, n, 3 * h * D, device='cuda:0',
                       dtype=torch.bfloat16) * 8)
    out = ops.mhsa_fused(qkv, h).float()
    assert torch.isfinite(out).all()
    ref = sdpa_fp32(qkv, h)
    err = ((out - ref).abs() / (ref.abs().clamp(min=1.0))).max().item()
    assert err < 2e-2, err
