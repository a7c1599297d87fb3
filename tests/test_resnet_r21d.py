import numpy as np
import pytest
import torch

from video_features_amd.config import Config


def test_resnet_shapes():
    from video_features_amd.models.resnet import build_resnet
    torch.manual_seed(0)
    for name, dim in [('resnet18', 512), ('resnet50', 2048)]:
        m = build_resnet(name).eval()
        with torch.no_grad():
            f = m.forward_features(torch.randn(2, 3, 224, 224))
            logits = m(torch.randn(1, 3, 224, 224))
        assert f.shape == (2, dim)
        assert logits.shape == (1, 1000)


def test_resnet_param_counts():
    # sanity vs the published architectures (±1% of torchvision counts)
    from video_features_amd.models.resnet import build_resnet
    expected = {'resnet18': 11.69e6, 'resnet34': 21.80e6, 'resnet50': 25.56e6,
                'resnet101': 44.55e6, 'resnet152': 60.19e6}
    for name, exp in expected.items():
        n = sum(p.numel() for p in build_resnet(name).parameters())
        assert abs(n - exp) / exp < 0.01, (name, n, exp)


def test_r21d_shapes_and_params():
    from video_features_amd.models.r21d import R2Plus1D18
    torch.manual_seed(0)
    m = R2Plus1D18().eval()
    n = sum(p.numel() for p in m.parameters())
    # torchvision r2plus1d_18 has 31.51M params
    assert abs(n - 31.51e6) / 31.51e6 < 0.01, n
    with torch.no_grad():
        f = m.forward_features(torch.randn(1, 3, 16, 112, 112))
    assert f.shape == (1, 512)


def test_r21d_34_depth_and_equivalence():
    """R(2+1)D-34 (BASELINE config 5's depth): (3,4,6,3) basic blocks; the
    flattened-time path must match the conv3d composition."""
    from video_features_amd.models.r21d import R2Plus1D34
    torch.manual_seed(1)
    m = R2Plus1D34().eval()
    assert len(m.layer1) == 3 and len(m.layer2) == 4
    assert len(m.layer3) == 6 and len(m.layer4) == 3
    x = torch.randn(1, 3, 8, 32, 32)

    def ref(m, x):
        x = m.stem(x)
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                x = blk.forward(x)
        return m.avgpool(x).flatten(1)

    with torch.no_grad():
        a = m.forward_features(x)
        b = ref(m, x)
    assert a.shape == (1, 512)
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


def test_resnet_extractor_end_to_end(y4m_video):
    from video_features_amd.extractors.resnet import ExtractResNet
    cfg = Config(feature_type='resnet18', video_paths=[y4m_video],
                 batch_size=8, cpu=True)
    ex = ExtractResNet(cfg, external_call=True)
    out = ex(torch.arange(1))[0]
    assert out['resnet18'].shape == (16, 512)
    assert len(out['timestamps_ms']) == 16
    assert np.isfinite(out['resnet18']).all()


def test_r21d_extractor_end_to_end(y4m_video):
    from video_features_amd.extractors.r21d import ExtractR21D
    cfg = Config(feature_type='r21d_rgb', video_paths=[y4m_video], cpu=True)
    ex = ExtractR21D(cfg, external_call=True)
    out = ex(torch.arange(1))[0]
    # 16 frames, stack 16 step 16 → exactly 1 window
    assert out['r21d_rgb'].shape == (1, 512)
    assert np.isfinite(out['r21d_rgb']).all()


def test_show_pred_labels():
    from video_features_amd.utils.labels import class_names
    assert len(class_names('kinetics')) == 400
    assert len(class_names('imagenet')) == 1000


def test_r21d_flat_path_matches_5d_reference():
    """forward_features (flattened-time, no conv3d) must match the plain
    conv3d composition exactly."""
    from video_features_amd.models.r21d import R2Plus1D18

    torch.manual_seed(5)
    model = R2Plus1D18().eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 3, 16, 64, 64)

    def ref(m, x):
        x = m.stem(x)
        for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
            for blk in layer:
                x = blk.forward(x)
        return m.avgpool(x).flatten(1)

    with torch.no_grad():
        out = model.forward_features(x)
        expect = ref(model, x)
    assert out.shape == expect.shape == (2, 512)
    assert torch.allclose(out, expect, atol=2e-4, rtol=1e-4), \
        (out - expect).abs().max().item()


def test_conv2d_act_out_buffer_slice():
    """conv2d_act writes a channel slice of a wider NHWC buffer (the
    cat-elimination path); CPU fallback must match the kernel contract."""
    import torch.nn.functional as F
    from video_features_amd import ops
    torch.manual_seed(0)
    x = torch.randn(2, 16, 8, 8)
    w = torch.randn(24, 16, 3, 3)
    buf = torch.zeros(2, 40, 8, 8)
    out = ops.conv2d_act(x, w, None, 1, 1, 'relu', out=buf, out_off=8)
    assert out is buf
    ref = F.relu(F.conv2d(x, w, None, 1, 1))
    torch.testing.assert_close(buf[:, 8:32], ref)
    assert (buf[:, :8] == 0).all() and (buf[:, 32:] == 0).all()


def test_conv2d_mod_padded_weight_cache_invalidates():
    """The cached channel-padded weight must refresh when new weights are
    loaded into the module (version-keyed by ops.derived)."""
    from video_features_amd.ops import conv2d_mod
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(3, 16, 3, 1, 1)
    x = torch.randn(1, 3, 8, 8)
    y1 = conv2d_mod(conv, x)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    y2 = conv2d_mod(conv, x)
    ref = torch.nn.functional.conv2d(x, conv.weight, conv.bias, 1, 1)
    torch.testing.assert_close(y2, ref)
    assert not torch.allclose(y1, y2)
