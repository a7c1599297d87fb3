"""CPU checks of the op dispatch layer's plumbing: the extension build's
dependency rule and the activation-name validation."""
import os

import pytest
import torch

from video_features_amd import ops
from video_features_amd.ops.build import _newer


def test_newer_tracks_every_header(tmp_path):
    """An object is stale when ANY header beside its source is newer, and
    up to date when source and headers are all older."""
    src, hdr, obj = (tmp_path / n for n in ('k.hip', 'tile.h', 'k.o'))
    for f in (src, hdr, obj):
        f.write_text('')
    os.utime(src, (1000, 1000))
    os.utime(obj, (2000, 2000))
    os.utime(hdr, (3000, 3000))
    assert _newer(src, obj)
    os.utime(hdr, (1500, 1500))
    assert not _newer(src, obj)
    obj.unlink()
    assert _newer(src, obj)


def test_unknown_activation_raises():
    x = torch.randn(4, 8)
    with pytest.raises(ValueError, match='bogus'):
        ops.linear_act(x, torch.randn(16, 8), act='bogus')
    with pytest.raises(ValueError, match='bogus'):
        ops.conv2d_act(x.reshape(1, 8, 2, 2), torch.randn(16, 8, 1, 1),
                       act='bogus')
