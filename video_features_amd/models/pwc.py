"""Native PWC-Net optical flow (Sun et al., CVPR'18 architecture).

Re-implementation of the network the reference vendors
(reference models/pwc/pwc_src/pwc_net.py): 6-level feature pyramid,
per-level cost volume over a 9×9 displacement window, DenseNet-style
decoders with backward warping, dilated-conv context refiner, ×20 flow
scaling with pad-to-/64 bilinear resizing.

MI355X mapping: the 81-channel cost volume — which the reference JIT-compiles
from CUDA strings via CuPy (reference models/pwc/pwc_src/correlation.py) —
dispatches through ``ops.pwc_correlation``: ONE fused hand-written CDNA4 HIP
kernel on GPU (no rearrange pass, LDS-staged center features, wave64
channel reduction), and a vectorized torch fallback on CPU.  Warping goes
through ``ops.bilinear_warp``.

Dense-buffer path (``PWCNet.dense_buffer``): each decoder level owns ONE
zero-initialised channels_last buffer

    [conv5 32 | conv4 64 | conv3 96 | conv2 128 | conv1 128 | corr 81 | f1 |
     upflow 2 | upfeat 2 | zero pad to a multiple of 8]

which is the channel order the reference's ``cat([new, x], 1)`` chain ends
with, so the weights need no permutation.  Every dense conv reads the
suffix behind its own slice and writes its slice in place (fused
LeakyReLU), the correlation kernel writes its slice directly, and the
dilated refiner convs run on the same implicit-GEMM kernel: no cat, no
NCHW conv.  The path is plain ``ops.conv2d_mod`` / ``ops.pwc_correlation``
calls, so on CPU it is a pure-torch re-expression of the cat path.
``VFA_NO_PWC_CL=1`` forces the cat path.

On the GPU in bf16 the dense-buffer path is channels_last end to end
(``PWCNet._nhwc``): a level's buffer is allocated BEFORE the previous
level's upsamplers run, ``upflow`` / ``upfeat`` write their two channels
each straight into it through ``ops.conv_transpose2d_mod`` (``upfeat``
reading the previous buffer in place), the warp reads the channels_last
``f2`` and the ``upflow`` slice view with the warp scale folded in, and the
cost volume reads the channels_last ``f1`` and warped ``f2``: no NCHW
feature tensor and no library convolution.  ``VFA_NO_PWC_NHWC=1`` restores
the earlier dense path (NCHW warp / correlation inputs, eager upsamplers).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops


class _ConvLeaky(nn.Sequential):
    """conv + LeakyReLU(0.1) with the Sequential key scheme (``0.weight``)
    preserved; on GPU the pair runs as ONE fused implicit-GEMM kernel
    (act=leaky_relu) via conv2d_mod when the input is channels_last bf16."""

    def forward(self, x):
        return ops.conv2d_mod(self[0], x, 'leaky_relu')


def _conv(in_ch: int, out_ch: int, stride: int = 1, dilation: int = 1):
    return _ConvLeaky(
        nn.Conv2d(in_ch, out_ch, 3, stride, padding=dilation, dilation=dilation),
        nn.LeakyReLU(0.1, inplace=True))


class PyramidExtractor(nn.Module):
    """6-level siamese feature pyramid, channels 16/32/64/96/128/196
    (reference pwc_net.py:44-110)."""

    CHANNELS = [16, 32, 64, 96, 128, 196]

    def __init__(self):
        super().__init__()
        levels = []
        in_ch = 3
        for out_ch in self.CHANNELS:
            levels.append(nn.Sequential(_conv(in_ch, out_ch, 2),
                                        _conv(out_ch, out_ch),
                                        _conv(out_ch, out_ch)))
            in_ch = out_ch
        self.levels = nn.ModuleList(levels)

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        if x.is_cuda and x.dtype == torch.bfloat16:
            # channels_last through the pyramid so the fused conv kernel
            # runs; warp and correlation read it as it is
            x = x.contiguous(memory_format=torch.channels_last)
        feats = []
        for level in self.levels:
            x = level(x)
            feats.append(x)
        return feats   # [1/2 .. 1/64]


class Decoder(nn.Module):
    """Per-level flow decoder with dense connections
    (reference pwc_net.py:113-186)."""

    DENSE = [128, 128, 96, 64, 32]

    def __init__(self, feat_ch: int, top: bool = False, last: bool = False):
        super().__init__()
        self.top = top
        in_ch = 81 if top else 81 + feat_ch + 2 + 2   # corr + f1 + upflow + upfeat
        convs = []
        c = in_ch
        for out_ch in self.DENSE:
            convs.append(_conv(c, out_ch))
            c += out_ch
        self.convs = nn.ModuleList(convs)
        self.predict = nn.Conv2d(c, 2, 3, 1, 1)
        self.out_channels = c
        # upflow/upfeat feed the NEXT (finer) level; the bottom decoder
        # (level 2) has no consumer, so the parameter set matches the
        # reference's exactly (its Decoder(l) holds the upsamplers the
        # consumer side, pwc_net.py:119-120 — same tensors, shifted owner)
        if not last:
            self.upflow = nn.ConvTranspose2d(2, 2, 4, 2, 1)
            self.upfeat = nn.ConvTranspose2d(c, 2, 4, 2, 1)

    def forward(self, f1: torch.Tensor, f2: torch.Tensor,
                upflow: Optional[torch.Tensor],
                upfeat: Optional[torch.Tensor],
                warp_scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
        # NCHW copies of the (on the GPU channels_last) pyramid features:
        # this path keeps the NCHW warp and cost-volume kernels
        f1n, f2n = f1.contiguous(), f2.contiguous()
        if self.top:
            corr = F.leaky_relu(ops.pwc_correlation(f1n, f2n), 0.1)
            x = corr
        else:
            warped = ops.bilinear_warp(f2n, upflow * warp_scale)
            corr = F.leaky_relu(ops.pwc_correlation(f1n, warped), 0.1)
            x = torch.cat([corr, f1, upflow, upfeat], dim=1)
        for conv in self.convs:
            x = torch.cat([conv(x), x], dim=1)
        flow = self.predict(x)
        return flow, x

    # dense-buffer layout: write offsets of convs[0..4] and of the cost
    # volume; conv i reads everything behind its own slice
    DENSE_OFF = [320, 192, 96, 32, 0]
    CORR_OFF = 448

    def forward_dense(self, f1: torch.Tensor, f2: torch.Tensor,
                      upflow: Optional[torch.Tensor],
                      upfeat: Optional[torch.Tensor],
                      warp_scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """Same result as ``forward``; the second return value is the
        level's buffer, of which channels [0, out_channels) are ``x``."""
        fc = f1.shape[1]
        buf = self.new_buffer(f1)
        # the NCHW warp and cost-volume kernels, as in ``forward``
        f1n, f2n = f1.contiguous(), f2.contiguous()
        if not self.top:
            f2n = ops.bilinear_warp(f2n, upflow * warp_scale)
        ops.pwc_correlation(f1n, f2n, out=buf, out_off=self.CORR_OFF,
                            act='leaky_relu')
        if not self.top:
            o = self.CORR_OFF + 81
            buf[:, o:o + fc] = f1
            buf[:, o + fc:o + fc + 2] = upflow
            buf[:, o + fc + 2:o + fc + 4] = upfeat
        return self._dense_convs(buf)

    def new_buffer(self, f1: torch.Tensor) -> torch.Tensor:
        """The level's zero-initialised channels_last buffer; allocated per
        forward (a captured graph replays the allocation)."""
        b, _, h, w = f1.shape
        width = (self.out_channels + 7) // 8 * 8
        return torch.zeros((b, h, w, width), dtype=f1.dtype,
                           device=f1.device).permute(0, 3, 1, 2)

    def up_off(self, fc: int) -> int:
        """First channel of ``upflow`` in the buffer (``upfeat`` follows)."""
        return self.CORR_OFF + 81 + fc

    def forward_nhwc(self, f1: torch.Tensor, f2: torch.Tensor,
                     buf: torch.Tensor, warp_scale: float
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``forward_dense`` on channels_last features.  ``buf`` is
        ``new_buffer(f1)``; below the top level the caller has already let
        the previous level's upsamplers write its ``upflow`` / ``upfeat``
        channels."""
        fc = f1.shape[1]
        if not self.top:
            o = self.up_off(fc)
            f2 = ops.bilinear_warp(f2, buf[:, o:o + 2], scale=warp_scale)
        ops.pwc_correlation(f1, f2, out=buf, out_off=self.CORR_OFF,
                            act='leaky_relu')
        if not self.top:
            o = self.CORR_OFF + 81
            buf[:, o:o + fc] = f1
        return self._dense_convs(buf)

    def _dense_convs(self, buf: torch.Tensor
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The five dense convs and the flow head on a filled buffer."""
        for conv, off in zip(self.convs, self.DENSE_OFF):
            ops.conv2d_mod(conv[0], buf, 'leaky_relu', out=buf, out_off=off,
                           in_off=off + conv[0].out_channels)
        flow = ops.conv2d_mod(self.predict, buf, in_off=0)
        return flow, buf


class Refiner(nn.Module):
    """Dilated-conv context network (reference pwc_net.py:189-210)."""

    def __init__(self, in_ch: int):
        super().__init__()
        self.net = nn.Sequential(
            _conv(in_ch, 128, dilation=1), _conv(128, 128, dilation=2),
            _conv(128, 128, dilation=4), _conv(128, 96, dilation=8),
            _conv(96, 64, dilation=16), _conv(64, 32, dilation=1),
            nn.Conv2d(32, 2, 3, 1, 1))

    def forward(self, x):
        return self.net(x)

    def forward_dense(self, buf: torch.Tensor) -> torch.Tensor:
        """``buf``: the level-2 decoder buffer, read in place."""
        x = ops.conv2d_mod(self.net[0][0], buf, 'leaky_relu', in_off=0)
        for layer in list(self.net)[1:-1]:
            x = ops.conv2d_mod(layer[0], x, 'leaky_relu')
        return ops.conv2d_mod(self.net[-1], x)


class PWCNet(nn.Module):
    # flow at level l is in level-l pixel units; upsampled flow must be scaled
    # before warping the next level's features (reference pwc_net.py:250-254)
    WARP_SCALES = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}

    def __init__(self, dense_buffer: Optional[bool] = None):
        super().__init__()
        # None: automatic (bf16 on GPU with the extension loaded);
        # True / False force the dense-buffer / the cat path
        self.dense_buffer = dense_buffer
        self.extractor = PyramidExtractor()
        ch = PyramidExtractor.CHANNELS       # [16, 32, 64, 96, 128, 196]
        self.decoder6 = Decoder(ch[5], top=True)
        self.decoder5 = Decoder(ch[4])
        self.decoder4 = Decoder(ch[3])
        self.decoder3 = Decoder(ch[2])
        self.decoder2 = Decoder(ch[1], last=True)
        self.refiner = Refiner(self.decoder2.out_channels)

    def _nhwc(self, x: torch.Tensor) -> bool:
        """Channels_last end to end: the dense-buffer path on the GPU in
        bf16 with the extension loaded, unless VFA_NO_PWC_NHWC=1."""
        return self._dense(x) and ops.native_ready(x, knob='VFA_NO_PWC_NHWC')

    def _dense(self, x: torch.Tensor) -> bool:
        if ops.env_flag('VFA_NO_PWC_CL'):
            return False
        if self.dense_buffer is not None:
            return bool(self.dense_buffer)
        return ops.native_ready(x)

    def forward(self, im1: torch.Tensor, im2: torch.Tensor) -> torch.Tensor:
        """uint8-range RGB (B, 3, H, W) pairs → (B, 2, H, W) flow in input
        pixel units (reference pwc_net.py:213-261: BGR/255 input, /64
        bilinear pad, ×20 flow scale, final bilinear upsample)."""
        b, _, h, w = im1.shape
        im1 = im1.flip(1) / 255.0            # RGB → BGR, [0, 1]
        im2 = im2.flip(1) / 255.0
        h64 = ((h + 63) // 64) * 64
        w64 = ((w + 63) // 64) * 64
        if (h64, w64) != (h, w):
            im1 = F.interpolate(im1, (h64, w64), mode='bilinear', align_corners=False)
            im2 = F.interpolate(im2, (h64, w64), mode='bilinear', align_corners=False)
        p1 = self.extractor(im1)
        p2 = self.extractor(im2)
        # dense: each decoder returns its level buffer, whose leading
        # out_channels are the cat path's feature tensor
        dense = self._dense(p1[0])
        decs = {6: self.decoder6, 5: self.decoder5, 4: self.decoder4,
                3: self.decoder3, 2: self.decoder2}

        def run(dec, *args):
            return dec.forward_dense(*args) if dense else dec(*args)

        nhwc = self._nhwc(p1[0])
        # pyramid list index: level l features are p[l-1] (1/2^l resolution)
        if nhwc:
            flow, feat = self.decoder6.forward_nhwc(
                p1[5], p2[5], self.decoder6.new_buffer(p1[5]), 0.0)
        else:
            flow, feat = run(self.decoder6, p1[5], p2[5], None, None, 0.0)
        for lvl in (5, 4, 3, 2):
            prev_dec = decs[lvl + 1]
            if nhwc:
                dec, f1 = decs[lvl], p1[lvl - 1]
                buf = dec.new_buffer(f1)
                o = dec.up_off(f1.shape[1])
                ops.conv_transpose2d_mod(prev_dec.upflow, flow, out=buf,
                                         out_off=o)
                ops.conv_transpose2d_mod(prev_dec.upfeat, feat, out=buf,
                                         out_off=o + 2, in_off=0)
                flow, feat = dec.forward_nhwc(f1, p2[lvl - 1], buf,
                                              self.WARP_SCALES[lvl])
                continue
            upflow = prev_dec.upflow(flow)
            upfeat = prev_dec.upfeat(
                feat[:, :prev_dec.out_channels] if dense else feat)
            flow, feat = run(decs[lvl], p1[lvl - 1], p2[lvl - 1], upflow,
                             upfeat, self.WARP_SCALES[lvl])
        flow = flow + (self.refiner.forward_dense(feat) if dense
                       else self.refiner(feat))
        # ×20 to pixel units at 1/4 res, then resize to the input resolution
        flow = F.interpolate(flow * 20.0, (h, w), mode='bilinear',
                             align_corners=False)
        flow[:, 0] *= float(w) / float(w64)
        flow[:, 1] *= float(h) / float(h64)
        return flow
