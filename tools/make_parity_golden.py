#!/usr/bin/env python3
"""Record the reference side of tests/test_reference_parity.py.

Usage:  python tools/make_parity_golden.py --reference PATH_TO_REFERENCE

Imports the reference checkout's own model sources, gives each model the
deterministic weights ``synth_state_dict`` derives from its state-dict key
names and shapes, runs it on the tests' seeded inputs (CPU, fp32) and writes
``tests/golden/parity_<case>.npz``: the key names, shapes and seed (``meta``,
JSON) plus the reference's outputs.  The tests rebuild the same weights and
inputs and need no reference checkout.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import test_reference_parity as tp  # noqa: E402


def _seeded(ref, seed, aliased=(), gain=6.0):
    """Load synthetic weights into the reference model; → meta dict."""
    ref_sd = ref.state_dict()
    keys = list(ref_sd.keys())
    shapes = [list(v.shape) for v in ref_sd.values()]
    sd = tp.synth_state_dict(keys, shapes, seed, gain)
    ref.load_state_dict(sd)
    # what the tests feed our models must be what the reference now holds
    for k, v in ref.state_dict().items():
        if not any(a in k for a in aliased):
            assert torch.equal(v, sd[k]), k
    return {'keys': keys, 'shapes': shapes, 'seed': seed, 'gain': gain}


def _save(name, meta, **arrays):
    os.makedirs(tp.GOLDEN, exist_ok=True)
    path = os.path.join(tp.GOLDEN, f'parity_{name}.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    mags = {k: float(np.abs(v).mean()) for k, v in arrays.items()}
    print(f'{path}: {os.path.getsize(path)} bytes, mean |x| {mags}')


def make_i3d():
    from models.i3d.i3d_src.i3d_net import I3D as RefI3D
    for modality in ('rgb', 'flow'):
        ref = RefI3D(num_classes=400, modality=modality).eval()
        meta = _seeded(ref, seed=1)
        with torch.no_grad():
            f = ref(tp.i3d_input(modality, seed=2), features=True)
        _save(f'i3d_{modality}', meta, features=f.numpy())
    ref = RefI3D(num_classes=400, modality='rgb').eval()
    meta = _seeded(ref, seed=4)
    with torch.no_grad():
        _, logits = ref(tp.i3d_input('rgb', seed=5))
    _save('i3d_logits', meta, logits=logits.numpy())


def make_raft():
    from models.raft.raft_src.raft import RAFT as RefRAFT
    ref = RefRAFT().eval()
    # norm3 and downsample.1 are one module under two names; the later key
    # (downsample.1, the one the test keeps) wins the load
    meta = _seeded(ref, seed=7, aliased=('.norm3.',))
    im1, im2 = tp.image_pair_input(seed=8)
    with torch.no_grad():
        flow = ref(im1, im2, iters=6, test_mode=True)
    _save('raft', meta, flow=flow.numpy())


def make_vggish():
    from models.vggish_torch.vggish_src import mel_features
    log_mel = mel_features.log_mel_spectrogram(
        tp.wav_input(), audio_sample_rate=16000, log_offset=0.01,
        window_length_secs=0.025, hop_length_secs=0.010,
        num_mel_bins=64, lower_edge_hertz=125, upper_edge_hertz=7500)
    examples = mel_features.frame(log_mel, window_length=96, hop_length=96)
    _save('vggish_mel', {'keys': [], 'shapes': [], 'seed': 0, 'gain': 0.0},
          examples=np.asarray(examples))

    # vggish.py pulls in vggish_input → resampy/soundfile (audio IO); stub
    # them — VGG itself never touches audio IO
    for name in ('resampy', 'soundfile'):
        sys.modules.setdefault(name, types.ModuleType(name))
    from models.vggish_torch.vggish_src.vggish import VGG, make_layers
    ref = VGG(make_layers()).eval()
    meta = _seeded(ref, seed=10)
    with torch.no_grad():
        f = ref(tp.vggish_examples_input()[:, None, :, :])
    _save('vggish_net', meta, features=f.numpy())


def make_pwc():
    from video_features_amd.ops import _pwc_correlation_torch
    # import the reference PWC net around its CuPy JIT machinery: stub cupy
    # (never called on CPU) and its torch<1 version assert
    cupy = types.ModuleType('cupy')
    cupy.util = types.SimpleNamespace(
        memoize=lambda for_each_device=False: (lambda f: f))
    sys.modules['cupy'] = cupy
    ver = torch.__version__
    torch.__version__ = '1.6.0'
    try:
        m = importlib.import_module('models.pwc.pwc_src.pwc_net')
    finally:
        torch.__version__ = ver
    m.correlation.FunctionCorrelation = \
        lambda tensorFirst, tensorSecond, device=None: \
        _pwc_correlation_torch(tensorFirst, tensorSecond, 4)
    ref = m.PWCNet().eval()
    meta = _seeded(ref, seed=12)
    im1, im2 = tp.image_pair_input(seed=13)
    # the reference's Backward() warp builds its grid in the corner-aligned
    # convention (linspace(-1, 1), flow / ((W-1)/2)) of the torch 0.4 it was
    # written for and passes no align_corners; newer torch defaults that to
    # False, so run the reference under the convention its arithmetic assumes
    grid_sample = torch.nn.functional.grid_sample
    torch.nn.functional.grid_sample = \
        lambda *a, **kw: grid_sample(*a, **{'align_corners': True, **kw})
    try:
        with torch.no_grad():
            flow = ref(im1, im2)
    finally:
        torch.nn.functional.grid_sample = grid_sample
    _save('pwc', meta, flow=flow.numpy())


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--reference', required=True,
                   help='path to a checkout of the reference project')
    args = p.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    make_i3d()
    make_raft()
    make_vggish()
    make_pwc()


if __name__ == '__main__':
    main()
