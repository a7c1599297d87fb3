"""Cross-implementation numerical parity against the REFERENCE's vendored
nets (pure torch/numpy, CPU).

All other correctness evidence is self-referential (HIP vs our own torch).
These tests load weights laid out in the reference's own state-dict scheme
into our models (utils/convert_checkpoints + the documented load paths) and
assert feature agreement with what the reference's model sources computed
from the same weights and inputs — a TF-SAME, flatten-order, GRU merging,
or mel-frontend bug diverges here.

The reference's side is recorded under ``tests/golden/parity_*.npz`` by
``tools/make_parity_golden.py`` (which needs a reference checkout; the tests
do not).  Each file holds the reference model's state-dict key names and
shapes plus its outputs.  Weights are not stored: ``synth_state_dict``
regenerates them from the names, shapes and a seed, identically in the tool
and here, and the inputs come from the seeded ``*_input`` helpers below.
"""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def synth_state_dict(keys, shapes, seed, gain=6.0):
    """Deterministic weights for a reference-scheme state dict, from key
    names and shapes alone.  Scales follow the default torch inits the
    reference's constructors apply, except that conv/linear weights are
    uniform ±sqrt(gain/fan_in): gain 6 (He) keeps the input's signal alive
    through the deep ReLU stacks, so the compared features depend on the
    input and not only on the last layers' shifts (gain 1 is torch's
    default init).  Norm affines and running stats are non-trivial so
    BatchNorm folding/ordering bugs cannot hide behind identity stats."""
    sd = {}
    for i, (key, shape) in enumerate(zip(keys, shapes)):
        g = torch.Generator().manual_seed(seed * 100003 + i)
        shape = tuple(shape)
        if key.endswith('num_batches_tracked'):
            t = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith('running_mean'):
            t = torch.randn(shape, generator=g) * 0.3
        elif key.endswith('running_var'):
            t = torch.rand(shape, generator=g) + 0.5
        elif len(shape) >= 2:
            bound = (gain / float(np.prod(shape[1:]))) ** 0.5
            t = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif key.endswith('weight'):          # norm scale
            t = torch.rand(shape, generator=g) * 0.5 + 0.75
        else:                                 # bias / norm shift
            t = (torch.rand(shape, generator=g) * 2 - 1) * 0.05
        sd[key] = t
    return sd


def load_golden(name):
    """→ (reference-scheme state dict, {array name: recorded ndarray})."""
    with np.load(os.path.join(GOLDEN, f'parity_{name}.npz'),
                 allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k != 'meta'}
        meta = json.loads(str(z['meta']))
    sd = synth_state_dict(meta['keys'], meta['shapes'], meta['seed'],
                          meta['gain'])
    return sd, arrays


def i3d_input(modality, seed):
    c = 3 if modality == 'rgb' else 2
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, c, 16, 224, 224, generator=g) * 2 - 1


def image_pair_input(seed):
    g = torch.Generator().manual_seed(seed)
    im1 = torch.rand(1, 3, 128, 128, generator=g) * 255
    im2 = torch.rand(1, 3, 128, 128, generator=g) * 255
    return im1, im2


def wav_input():
    rng = np.random.default_rng(9)
    return (rng.random(int(16000 * 2.5)) * 2 - 1).astype(np.float64)


def vggish_examples_input():
    g = torch.Generator().manual_seed(11)
    return torch.randn(3, 96, 64, generator=g)


# ------------------------------------------------------------------- I3D
@pytest.mark.parametrize('modality', ['rgb', 'flow'])
def test_i3d_feature_parity(modality):
    """Our flattened-time I3D must reproduce the reference's conv3d I3D
    (reference models/i3d/i3d_src/i3d_net.py:160-264) bit-for-bit up to
    fp32 accumulation order, weights mapped via convert_auto."""
    from video_features_amd.models.i3d import I3D as OurI3D
    from video_features_amd.utils.convert_checkpoints import convert_auto

    sd, gold = load_golden(f'i3d_{modality}')
    ours = OurI3D(modality=modality).eval()
    ours.load_state_dict(convert_auto(sd))

    x = i3d_input(modality, seed=2)
    with torch.no_grad():
        f_ours = ours.forward_features(x)
    f_ref = torch.from_numpy(gold['features'])
    assert f_ref.shape == f_ours.shape == (1, 1024)
    torch.testing.assert_close(f_ours, f_ref, rtol=1e-4, atol=1e-4)


def test_i3d_logits_parity():
    """--show_pred path: the classifier logits must also agree
    (reference i3d_net.py:265-275 softmax head)."""
    from video_features_amd.models.i3d import I3D as OurI3D
    from video_features_amd.utils.convert_checkpoints import convert_auto

    sd, gold = load_golden('i3d_logits')
    ours = OurI3D(modality='rgb').eval()
    ours.load_state_dict(convert_auto(sd))
    x = i3d_input('rgb', seed=5)
    with torch.no_grad():
        logits_ours = ours(x)
    # the second element of the reference forward's (softmax, logits)
    logits_ref = torch.from_numpy(gold['logits'])
    torch.testing.assert_close(logits_ours, logits_ref,
                               rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------- RAFT
def test_raft_flow_parity():
    """Our RAFT (merged convzr GRU, persistent buffers, fused-op calls)
    must match the reference RAFT (models/raft/raft_src/raft.py:113-174)
    given its state dict — same iters, same uint8-range inputs."""
    from video_features_amd.models.raft import RAFT as OurRAFT

    sd, gold = load_golden('raft')
    # the reference aliases each downsample norm twice (norm3 AND
    # downsample.1 are the same module, extractor.py:44-45); keep the
    # downsample.1 naming ours uses
    sd = {k: v for k, v in sd.items() if '.norm3.' not in k}
    ours = OurRAFT().eval()
    missing, unexpected = ours.load_state_dict(sd, strict=False)
    # the SepConvGRU hook merges convz/convr into convzr; nothing else may
    # be missing or unexpected
    assert not missing, missing
    assert not unexpected, unexpected

    # NOTE ≥128 px: below that, the reference's 4-level corr pyramid
    # bottoms out at 1x1 and its bilinear_sampler divides by W-1 = 0
    # (models/raft/raft_src/utils/utils.py:64-65) → NaN.  A reference
    # input-domain limit, not a divergence.
    im1, im2 = image_pair_input(seed=8)
    with torch.no_grad():
        f_ours = ours(im1, im2, iters=6, test_mode=True)
    f_ref = torch.from_numpy(gold['flow'])
    assert f_ref.shape == f_ours.shape == (1, 2, 128, 128)
    torch.testing.assert_close(f_ours, f_ref, rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------ VGGish
def test_vggish_mel_frontend_parity():
    """Our torch-native log-mel frontend vs the reference's numpy STFT
    pipeline (models/vggish_torch/vggish_src/mel_features.py:192-223 +
    vggish_input.py example framing, 16 kHz path — no resample)."""
    from video_features_amd.models.vggish import waveform_to_examples

    _, gold = load_golden('vggish_mel')
    ref_examples = gold['examples']
    ours = waveform_to_examples(torch.from_numpy(wav_input()).float())
    assert ours.shape == ref_examples.shape == (2, 96, 64)
    np.testing.assert_allclose(ours.numpy(), ref_examples,
                               rtol=1e-4, atol=1e-4)


def test_vggish_net_parity():
    """Our VGGish net (conv stack + TF-order flatten + FC head) vs the
    reference's VGG (models/vggish_torch/vggish_src/vggish.py:9-31),
    weights mapped via convert_auto."""
    from video_features_amd.models.vggish import VGGish
    from video_features_amd.utils.convert_checkpoints import convert_auto

    sd, gold = load_golden('vggish_net')
    ours = VGGish().eval()
    ours.load_state_dict(convert_auto(sd),
                         strict=False)   # pproc tensors stay ours
    with torch.no_grad():
        f_ours = ours(vggish_examples_input())
    f_ref = torch.from_numpy(gold['features'])
    assert f_ref.shape == f_ours.shape == (3, 128)
    torch.testing.assert_close(f_ours, f_ref, rtol=1e-4, atol=1e-4)


# -------------------------------------------------------------------- PWC
def test_pwc_net_parity():
    """Our PWC pyramid/warp/decoder vs the reference's vendored net
    (models/pwc/pwc_src/pwc_net.py:212-263) with mapped weights.  The
    reference's correlation is CUDA-only (CuPy); when the golden output was
    recorded its call site was patched to our torch correlation — itself
    GPU-tested against the HIP kernel — so this validates everything around
    it.  The reference's warp was recorded in the corner-aligned
    grid_sample convention its grid arithmetic is written for (the tool
    says why)."""
    from video_features_amd.models.pwc import PWCNet
    from video_features_amd.utils.convert_checkpoints import convert_pwc

    sd, gold = load_golden('pwc')
    ours = PWCNet().eval()
    ours.load_state_dict(convert_pwc(sd))
    im1, im2 = image_pair_input(seed=13)
    with torch.no_grad():
        f_ours = ours(im1, im2)
    f_ref = torch.from_numpy(gold['flow'])
    assert f_ref.shape == f_ours.shape
    torch.testing.assert_close(f_ours, f_ref, rtol=1e-3, atol=1e-3)
