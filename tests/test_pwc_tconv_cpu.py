"""CPU tests of the transposed-conv op layer and of bilinear_warp's scale.

The P-form (`ops._conv_transpose2d_pform`: GEMM with the packed weight, then
the col2im gather) is the index arithmetic of the kernels in tconv.hip in
pure torch; in float64 it differs from F.conv_transpose2d by re-association
noise only, and a wrong tap parity or packing order is an O(1) error."""
import pytest
import torch
import torch.nn.functional as F

from video_features_amd import ops


@pytest.mark.parametrize('shape,kout', [
    ((2, 21, 5, 7), 2), ((1, 21, 1, 1), 2), ((2, 2, 5, 7), 2),
    ((1, 2, 1, 1), 2), ((2, 8, 4, 3), 1)])
def test_pform_matches_torch_float64(shape, kout):
    gen = torch.Generator().manual_seed(sum(shape) + kout)
    c = shape[1]
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    w = torch.randn(c, kout, 4, 4, generator=gen, dtype=torch.float64)
    bias = torch.randn(kout, generator=gen, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, bias, 2, 1)
    got = ops._conv_transpose2d_pform(x, w, bias)
    assert got.shape == ref.shape == (shape[0], kout, 2 * shape[2],
                                      2 * shape[3])
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f'{shape}: max |delta| {err:.3e}, max |ref| {scale:.3e}')
    assert scale > 0 and err <= 1e-12 * scale
    nb = ops._conv_transpose2d_pform(x, w)
    ref_nb = F.conv_transpose2d(x, w, None, 2, 1)
    assert (nb - ref_nb).abs().max().item() <= 1e-12 * scale


def test_pack_tconv_weight_layout():
    """Row (ky*4 + kx)*K_out + ko holds W[:, ko, ky, kx]; the columns c8
    adds are zero."""
    c, kout = 21, 2
    w = torch.arange(c * kout * 16, dtype=torch.float64).reshape(c, kout, 4, 4)
    wp = ops._pack_tconv_weight(w, 24)
    assert wp.shape == (32, 24) and wp.is_contiguous()
    for ky, kx, ko in ((0, 0, 0), (1, 2, 1), (3, 3, 0), (2, 1, 1)):
        assert torch.equal(wp[(ky * 4 + kx) * kout + ko, :c], w[:, ko, ky, kx])
    assert bool((wp[:, c:] == 0).all())
    assert torch.equal(ops._pack_tconv_weight(w, c), wp[:, :c])
    with pytest.raises(ValueError):
        ops._pack_tconv_weight(w, 16)
    with pytest.raises(ValueError):
        ops._pack_tconv_weight(w[:, :, :3, :3], 24)


def test_conv_transpose2d_act_slices_cpu():
    gen = torch.Generator().manual_seed(7)
    buf = torch.randn(2, 40, 5, 7, generator=gen, dtype=torch.float64)
    w = torch.randn(24, 2, 4, 4, generator=gen, dtype=torch.float64)
    bias = torch.randn(2, generator=gen, dtype=torch.float64)
    ref = F.conv_transpose2d(buf[:, 16:40], w, bias, 2, 1)
    got = ops.conv_transpose2d_act(buf, w, bias, in_off=16, in_ch=24)
    assert torch.equal(got, ref)
    out = torch.full((2, 8, 10, 14), 7.0, dtype=torch.float64)
    ret = ops.conv_transpose2d_act(buf, w, bias, out=out, out_off=5,
                                   in_off=16, in_ch=24)
    assert ret is out
    assert torch.equal(out[:, 5:7], ref)
    assert bool((out[:, :5] == 7.0).all()) and bool((out[:, 7:] == 7.0).all())
    # unsliced, other geometry: still the composition
    w3 = torch.randn(40, 3, 3, 3, generator=gen, dtype=torch.float64)
    assert torch.equal(ops.conv_transpose2d_act(buf, w3, None, 1, 1),
                       F.conv_transpose2d(buf, w3, None, 1, 1))
    with pytest.raises(ValueError):
        ops.conv_transpose2d_act(buf, w, bias, in_off=16)
    with pytest.raises(ValueError):          # out shares storage with x
        ops.conv_transpose2d_act(buf, w, bias, out=buf[:, :8], in_off=16,
                                 in_ch=24)


def test_conv_transpose2d_mod_slice_cpu():
    """in_off reads m.in_channels channels: no rounding on the eager path,
    so the non-finite channels behind the slice do not matter."""
    torch.manual_seed(8)
    m = torch.nn.ConvTranspose2d(21, 2, 4, 2, 1).double()
    buf = torch.full((2, 40, 5, 7), float('nan'), dtype=torch.float64)
    x = torch.randn(2, 21, 5, 7, dtype=torch.float64)
    buf[:, 16:37] = x
    out = torch.full((2, 8, 10, 14), 7.0, dtype=torch.float64)
    with torch.no_grad():
        ref = m(x)
        ret = ops.conv_transpose2d_mod(m, buf, out=out, out_off=5, in_off=16)
        plain = ops.conv_transpose2d_mod(m, x)
    assert ret is out and torch.equal(out[:, 5:7], ref)
    assert bool((out[:, :5] == 7.0).all()) and bool((out[:, 7:] == 7.0).all())
    assert torch.equal(plain, ref)
    assert not hasattr(m, '_vfa_tconv_wp')


def test_bilinear_warp_scale_cpu():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 7, 9, generator=gen, dtype=torch.float64)
    f = torch.randn(2, 2, 7, 9, generator=gen, dtype=torch.float64) * 3
    assert torch.equal(ops.bilinear_warp(x, f, scale=0.625),
                       ops.bilinear_warp(x, f * 0.625))
    assert torch.equal(ops.bilinear_warp(x, f, scale=1.0),
                       ops.bilinear_warp(x, f))
    assert torch.equal(ops.bilinear_warp(x, f, 1.0), ops.bilinear_warp(x, f))


def test_channels_last_path_is_gpu_only():
    """A forced dense buffer on the CPU keeps the torch composition: the
    channels_last glue is for bf16 on the GPU."""
    from video_features_amd.models.pwc import PWCNet
    net = PWCNet(dense_buffer=True)
    x = torch.zeros(1, 16, 8, 8)
    assert net._dense(x) is True and net._nhwc(x) is False
    assert net._nhwc(x.to(torch.bfloat16)) is False
