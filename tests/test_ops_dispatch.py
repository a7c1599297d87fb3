"""CPU checks of the op dispatch layer's plumbing: the extension build's
dependency rule, the activation-name validation, the one declaration of the
launcher ABI and the slice arguments on the torch compositions."""
import os
import re
from pathlib import Path

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


CSRC = Path(ops.__file__).parent / 'csrc'


def test_c_abi_declared_once():
    """vfa_api.h is the only declaration of the launcher ABI: bindings.cpp
    has no prototypes of its own, every .hip sees the header through
    vfa_common.h, and what the .hip files define is what it declares."""
    assert 'extern "C"' not in (CSRC / 'bindings.cpp').read_text()
    assert '#include "vfa_api.h"' in (CSRC / 'vfa_common.h').read_text()
    name = re.compile(r'\b(vfa_\w+)\s*\(')
    api = (CSRC / 'vfa_api.h').read_text()
    declared = set(name.findall(api[api.index('extern "C"'):]))
    defined = set()
    for hip in CSRC.glob('*.hip'):
        text = hip.read_text()
        if '#include "mfma_tile.h"' not in text:
            assert '#include "vfa_common.h"' in text, hip.name
        # a definition: the name at the start of a declarator, a body after
        defined |= set(re.findall(
            r'^(?:extern "C" )?[\w ]+?\b(vfa_\w+)\([^;{]*\)\s*\{', text,
            re.M))
    assert defined == declared, defined ^ declared


def test_conv2d_act_slice_out_composition():
    """out= / out_off= on the torch composition: F.conv2d plus a slice
    assignment, the rest of ``out`` untouched."""
    torch.manual_seed(0)
    x, w, b = torch.randn(1, 16, 4, 4), torch.randn(5, 16, 3, 3), \
        torch.randn(5)
    out = torch.full((1, 8, 4, 4), 7.0)
    ret = ops.conv2d_act(x, w, b, 1, 1, 'relu', out=out, out_off=3)
    assert ret is out
    want = torch.full((1, 8, 4, 4), 7.0)
    want[:, 3:8] = torch.relu(torch.nn.functional.conv2d(x, w, b, 1, 1))
    assert torch.equal(out, want)


def test_conv_transpose2d_act_slices_composition():
    """in_off= / in_ch= / out= / out_off= on the torch composition:
    F.conv_transpose2d of the input slice plus a slice assignment."""
    torch.manual_seed(0)
    x, w, b = torch.randn(1, 16, 4, 4), torch.randn(8, 2, 4, 4), \
        torch.randn(2)
    out = torch.full((1, 8, 8, 8), 7.0)
    ret = ops.conv_transpose2d_act(x, w, b, in_off=8, in_ch=8, out=out,
                                   out_off=3)
    assert ret is out
    want = torch.full((1, 8, 8, 8), 7.0)
    want[:, 3:5] = torch.nn.functional.conv_transpose2d(x[:, 8:16], w, b, 2,
                                                        1)
    assert torch.equal(out, want)
