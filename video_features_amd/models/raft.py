"""Native RAFT optical flow (Teed & Deng, ECCV'20 architecture).

Re-implementation of the network the reference vendors
(reference models/raft/raft_src/{raft,extractor,update,corr}.py):
stride-8 feature/context encoders, all-pairs 4-level correlation pyramid,
iterative SepConvGRU updates, convex-combination 8× upsampling.

MI355X mapping (all decisions measured with rocprofv3, profiles/):
  * all-pairs correlation = one rocBLAS batched GEMM;
  * the per-iteration pyramid lookup (4 levels × 81 taps) is ONE fused HIP
    kernel (``ops.corr_lookup``) with the per-pixel correlation planes
    staged through LDS — the reference runs 4 grid_samples plus window
    tensor construction per iteration;
  * ``RAFT(corr='onthefly')`` skips the all-pairs volume, whose size is
    quadratic in the frame area: ``ops.corr_lookup_otf`` computes each
    lookup's 100 dot products per (pixel, level) from the feature maps
    (reference AlternateCorrBlock); ``'auto'`` switches by volume size;
  * the SepConvGRU z/r convs are merged into one conv and the gate
    elementwise is fused (``ops.gru_zr`` / ``ops.gru_out``), with the
    conv inputs kept in two persistent (B, 384, H/8, W/8) buffers instead
    of 4 torch.cat allocations per iteration;
  * the convex 8× upsample is one kernel (``ops.convex_upsample``) and —
    like the reference's test mode, which only returns the final flow
    (reference raft.py:170-172) — is computed on the LAST iteration only;
  * ``use_channels_last()`` flips the whole module to NHWC so MIOpen picks
    its NHWC igemm solvers without batched_transpose fixups; the fused
    kernels take an nhwc flag and address accordingly.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from ..config import RAFT_CORR_MODES


# --------------------------------------------------------------- encoders
class FusedInstanceNorm2d(nn.Module):
    """InstanceNorm2d(affine=False) with optional fused ReLU — one HIP
    kernel on GPU via ``ops.instance_norm`` (torch lowers InstanceNorm to
    batch-norm stats + transform + separate relu).  Stateless, so it is
    checkpoint-compatible with ``nn.InstanceNorm2d``."""

    def __init__(self, relu: bool = False):
        super().__init__()
        self.fuses_relu = relu

    def forward(self, x):
        if x.is_contiguous():
            return ops.instance_norm(x, relu=self.fuses_relu, nhwc=False)
        if x.is_contiguous(memory_format=torch.channels_last):
            return ops.instance_norm(x, relu=self.fuses_relu, nhwc=True)
        return ops.instance_norm(x.contiguous(), relu=self.fuses_relu,
                                 nhwc=False)


def _make_norm(norm: str, c: int, relu_after: bool = False):
    if norm == 'instance':
        return FusedInstanceNorm2d(relu=relu_after)
    if norm == 'batch':
        return nn.BatchNorm2d(c)
    return nn.Identity()


def _norm_act(norm_mod, relu, x):
    y = norm_mod(x)
    return y if getattr(norm_mod, 'fuses_relu', False) else relu(y)


class ResidualBlock(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, norm: str, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_ch, out_ch, 3, stride, 1)
        self.conv2 = nn.Conv2d(out_ch, out_ch, 3, 1, 1)
        self.norm1 = _make_norm(norm, out_ch, relu_after=True)
        self.norm2 = _make_norm(norm, out_ch, relu_after=True)
        self.relu = nn.ReLU(inplace=True)
        if stride == 1 and in_ch == out_ch:
            self.downsample = None
        else:
            self.downsample = nn.Sequential(
                nn.Conv2d(in_ch, out_ch, 1, stride), _make_norm(norm, out_ch))

    def forward(self, x):
        # 3x3 convs through the in-tree implicit-GEMM kernel; when the norm
        # is folded away (cnet's BN) the ReLU rides the conv epilogue.
        # NOTE the block is relu(x + relu(norm2(conv2(...)))) — the inner
        # ReLU precedes the residual add (reference extractor.py:47-55),
        # so the add cannot ride the conv epilogue.
        n1_id = isinstance(self.norm1, nn.Identity)
        n2_id = isinstance(self.norm2, nn.Identity)
        y = ops.conv2d_mod(self.conv1, x, 'relu' if n1_id else 'none')
        if not n1_id:
            y = _norm_act(self.norm1, self.relu, y)
        y = ops.conv2d_mod(self.conv2, y, 'relu' if n2_id else 'none')
        if not n2_id:
            y = _norm_act(self.norm2, self.relu, y)
        if self.downsample is None:
            identity = x
        else:
            identity = self.downsample[1](
                ops.conv2d_mod(self.downsample[0], x))
        return self.relu(identity + y)


class BasicEncoder(nn.Module):
    """Stride-8 ResNet encoder (reference extractor.py:118-192)."""

    def __init__(self, output_dim: int = 256, norm: str = 'instance'):
        super().__init__()
        self.norm1 = _make_norm(norm, 64, relu_after=True)
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3)
        self.relu1 = nn.ReLU(inplace=True)
        self.layer1 = nn.Sequential(ResidualBlock(64, 64, norm),
                                    ResidualBlock(64, 64, norm))
        self.layer2 = nn.Sequential(ResidualBlock(64, 96, norm, 2),
                                    ResidualBlock(96, 96, norm))
        self.layer3 = nn.Sequential(ResidualBlock(96, 128, norm, 2),
                                    ResidualBlock(128, 128, norm))
        self.conv2 = nn.Conv2d(128, output_dim, 1)

    def forward(self, x):
        # stem 7x7 (C=3) through the in-tree kernel via channel padding
        x = _norm_act(self.norm1, self.relu1,
                      ops.conv2d_mod(self.conv1, x))
        x = self.layer3(self.layer2(self.layer1(x)))
        return ops.conv2d_mod(self.conv2, x)


# ------------------------------------------------------------ correlation
class CorrPyramid:
    """All-pairs correlation + 4-level avg-pool pyramid + windowed lookup
    (reference corr.py:25-60)."""

    def __init__(self, fmap1: torch.Tensor, fmap2: torch.Tensor,
                 num_levels: int = 4, radius: int = 4):
        self.num_levels = num_levels
        self.radius = radius
        b, d, h, w = fmap1.shape
        f1 = fmap1.reshape(b, d, h * w).transpose(1, 2)  # (B, HW, D)
        f2 = fmap2.reshape(b, d, h * w)                  # (B, D, HW)
        corr = torch.matmul(f1, f2) / (d ** 0.5)     # rocBLAS batched GEMM
        corr = corr.reshape(b * h * w, 1, h, w)
        self.shape = (b, h, w)
        self.pyramid: List[torch.Tensor] = [corr.contiguous()]
        for _ in range(num_levels - 1):
            corr = F.avg_pool2d(corr, 2, 2)
            self.pyramid.append(corr.contiguous())

    def __call__(self, coords: torch.Tensor, nhwc: bool = False,
                 out_dtype: torch.dtype = None) -> torch.Tensor:
        """coords (B, 2, H, W) fp32 pixels at 1/8 res →
        (B, L*(2r+1)^2, H, W)."""
        return ops.corr_lookup(self.pyramid, coords.contiguous(),
                               self.radius, nhwc, out_dtype)


class CorrOnTheFly:
    """The same lookup without the all-pairs volume (reference
    AlternateCorrBlock, corr.py:63-91): holds fmap1 and the avg-pooled
    levels of fmap2 in f32, pixel-major, and ``ops.corr_lookup_otf``
    computes the 100 dot products per (pixel, level) a lookup needs.  Memory
    is linear in the frame area — ``nbytes`` — where CorrPyramid's is
    quadratic."""

    def __init__(self, fmap1: torch.Tensor, fmap2: torch.Tensor,
                 num_levels: int = 4, radius: int = 4):
        self.num_levels = num_levels
        self.radius = radius
        b, d, h, w = fmap1.shape
        self.shape = (b, h, w)
        self.f1 = fmap1.float().permute(0, 2, 3, 1).contiguous()
        f2 = fmap2.float()
        self.f2_levels: List[torch.Tensor] = []
        for lvl in range(num_levels):
            if lvl:
                f2 = F.avg_pool2d(f2, 2, 2)
            self.f2_levels.append(f2.permute(0, 2, 3, 1).contiguous())

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for t in [self.f1, *self.f2_levels])

    def __call__(self, coords: torch.Tensor, nhwc: bool = False,
                 out_dtype: torch.dtype = None) -> torch.Tensor:
        return ops.corr_lookup_otf(self.f1, self.f2_levels,
                                   coords.contiguous(), self.radius, nhwc,
                                   out_dtype)


def corr_mode_for(b: int, h8: int, w8: int, total_bytes: int) -> str:
    """'auto': on the fly once the all-pairs pyramid —
    4 * (1 + 1/4 + 1/16 + 1/64) * b * (h8 * w8)^2 bytes — would take more
    than a quarter of the device's memory."""
    return ('onthefly' if 5.3125 * b * (h8 * w8) ** 2 > total_bytes / 4
            else 'allpairs')


# ----------------------------------------------------------------- update
class FlowHead(nn.Module):
    def __init__(self, in_dim: int = 128, hidden: int = 256):
        super().__init__()
        self.conv1 = nn.Conv2d(in_dim, hidden, 3, 1, 1)
        self.conv2 = nn.Conv2d(hidden, 2, 3, 1, 1)

    def forward(self, x):
        # conv2 has N=2 outputs — routed via the padded-N path
        return ops.conv2d_mod(self.conv2,
                              ops.conv2d_mod(self.conv1, x, 'relu'))


class SepConvGRU(nn.Module):
    """Separable 1×5 / 5×1 ConvGRU (reference update.py:37-64), with the
    z and r convs merged into one ``convzr`` and the gate elementwise fused.

    ``forward`` operates on two persistent conv-input buffers ``hx``/``rhx``
    of shape (B, hidden+in_dim, H, W): channels [0, hidden) hold h (updated
    in place by ``ops.gru_out``), channels [hidden, ...) hold x (written
    once per RAFT iteration by the caller).
    """

    def __init__(self, hidden: int = 128, in_dim: int = 256):
        super().__init__()
        self.hidden = hidden
        c = hidden + in_dim
        self.convzr1 = nn.Conv2d(c, 2 * hidden, (1, 5), padding=(0, 2))
        self.convq1 = nn.Conv2d(c, hidden, (1, 5), padding=(0, 2))
        self.convzr2 = nn.Conv2d(c, 2 * hidden, (5, 1), padding=(2, 0))
        self.convq2 = nn.Conv2d(c, hidden, (5, 1), padding=(2, 0))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # accept reference-style checkpoints with separate convz/convr
        for i in ('1', '2'):
            zw = prefix + f'convz{i}.weight'
            rw = prefix + f'convr{i}.weight'
            if zw in state_dict and rw in state_dict:
                state_dict[prefix + f'convzr{i}.weight'] = torch.cat(
                    [state_dict.pop(zw), state_dict.pop(rw)])
                state_dict[prefix + f'convzr{i}.bias'] = torch.cat(
                    [state_dict.pop(prefix + f'convz{i}.bias'),
                     state_dict.pop(prefix + f'convr{i}.bias')])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, hx: torch.Tensor, rhx: torch.Tensor,
                nhwc: bool = False) -> None:
        # 1x5 / 5x1 convs through the in-tree implicit-GEMM kernel
        # (1.8-1.9x MIOpen on the GRU shapes, gpurun_out/bench_conv_r2b.log)
        z = ops.gru_zr(ops.conv2d_mod(self.convzr1, hx), hx, rhx, nhwc)
        ops.gru_out(ops.conv2d_mod(self.convq1, rhx), z, hx, nhwc)
        z = ops.gru_zr(ops.conv2d_mod(self.convzr2, hx), hx, rhx, nhwc)
        ops.gru_out(ops.conv2d_mod(self.convq2, rhx), z, hx, nhwc)


class BasicMotionEncoder(nn.Module):
    """(corr, flow) → 128-d motion features (reference update.py:83-101)."""

    def __init__(self, corr_levels: int = 4, corr_radius: int = 4):
        super().__init__()
        corr_planes = corr_levels * (2 * corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(corr_planes, 256, 1)
        self.convc2 = nn.Conv2d(256, 192, 3, 1, 1)
        self.convf1 = nn.Conv2d(2, 128, 7, 1, 3)
        self.convf2 = nn.Conv2d(128, 64, 3, 1, 1)
        self.conv = nn.Conv2d(192 + 64, 128 - 2, 3, 1, 1)

    def forward(self, flow, corr, out: torch.Tensor = None,
                out_off: int = 0):
        c1 = ops.conv2d_mod(self.convc1, corr, 'relu')
        f1 = ops.conv2d_mod(self.convf1, flow, 'relu')
        if out is not None and ops.native_ready(c1, channels_last=True):
            # cat-free path: convc2/convf2 write their channel slices of
            # ONE buffer via the conv epilogue's ldc, and the final conv
            # writes straight into the caller's (GRU input) buffer — the
            # three CatArrayBatchedCopy passes disappear
            b, _, h, w = c1.shape
            cat = torch.empty((b, h, w, 256), device=c1.device,
                              dtype=c1.dtype).permute(0, 3, 1, 2)
            ops.conv2d_act(c1, self.convc2.weight, self.convc2.bias, 1, 1,
                           'relu', out=cat, out_off=0)
            ops.conv2d_act(f1, self.convf2.weight, self.convf2.bias, 1, 1,
                           'relu', out=cat, out_off=192)
            ops.conv2d_act(cat, self.conv.weight, self.conv.bias, 1, 1,
                           'relu', out=out, out_off=out_off)
            out[:, out_off + 126:out_off + 128] = flow
            return None
        c = ops.conv2d_mod(self.convc2, c1, 'relu')
        f = ops.conv2d_mod(self.convf2, f1, 'relu')
        cat = torch.cat([c, f], dim=1)
        if cat.is_cuda and not cat.is_contiguous(
                memory_format=torch.channels_last):
            cat = cat.contiguous(memory_format=torch.channels_last)
        res = torch.cat([ops.conv2d_mod(self.conv, cat, 'relu'), flow],
                        dim=1)
        if out is not None:
            out[:, out_off:out_off + 128] = res
            return None
        return res


class BasicUpdateBlock(nn.Module):
    def __init__(self, hidden: int = 128, context: int = 128):
        super().__init__()
        self.encoder = BasicMotionEncoder()
        self.gru = SepConvGRU(hidden, in_dim=128 + context)
        self.flow_head = FlowHead(hidden, 256)
        # raw logits; the 0.25 scale of reference raft.py:158 is folded
        # into ops.convex_upsample
        self.mask = nn.Sequential(nn.Conv2d(hidden, 256, 3, 1, 1),
                                  nn.ReLU(inplace=True),
                                  nn.Conv2d(256, 64 * 9, 1))


# ------------------------------------------------------------------- RAFT
class RAFT(nn.Module):
    def __init__(self, hidden_dim: int = 128, context_dim: int = 128,
                 iters: int = 20, corr: str = 'allpairs'):
        super().__init__()
        if corr not in RAFT_CORR_MODES:
            raise ValueError(
                f'corr must be one of {RAFT_CORR_MODES}, got {corr!r}')
        self.hdim, self.cdim = hidden_dim, context_dim
        self.iters = iters
        self.corr = corr
        self.nhwc = False
        self.fnet = BasicEncoder(256, 'instance')
        self.cnet = BasicEncoder(hidden_dim + context_dim, 'batch')
        self.update_block = BasicUpdateBlock(hidden_dim, context_dim)

    def use_channels_last(self) -> 'RAFT':
        """Switch the conv path to NHWC (MIOpen igemm without transposes)."""
        self.nhwc = True
        return self.to(memory_format=torch.channels_last)

    @staticmethod
    def coords_grid(b: int, h: int, w: int, device, dtype):
        yy, xx = torch.meshgrid(torch.arange(h, device=device, dtype=dtype),
                                torch.arange(w, device=device, dtype=dtype),
                                indexing='ij')
        return torch.stack([xx, yy])[None].expand(b, -1, -1, -1).contiguous()

    def _corr_class(self, fmap1: torch.Tensor):
        """CorrPyramid or CorrOnTheFly for this forward; 'auto' asks
        ``corr_mode_for`` with the device's total memory (all-pairs on the
        CPU) — a host-side property read, no sync."""
        mode = self.corr
        if mode == 'auto':
            mode = 'allpairs'
            if fmap1.is_cuda:
                b, _, h8, w8 = fmap1.shape
                mode = corr_mode_for(b, h8, w8, torch.cuda.get_device_properties(
                    fmap1.device).total_memory)
        return CorrOnTheFly if mode == 'onthefly' else CorrPyramid

    def forward(self, image1: torch.Tensor, image2: torch.Tensor,
                iters: int = None, test_mode: bool = True):
        """uint8-range (B, 3, H, W) pairs (H, W divisible by 8) → (B, 2, H, W)
        flow (reference raft.py:113-174)."""
        iters = iters or self.iters
        dtype = self.fnet.conv1.weight.dtype
        mf = torch.channels_last if self.nhwc else torch.contiguous_format
        image1 = 2 * (image1.to(dtype) / 255.0) - 1.0
        image2 = 2 * (image2.to(dtype) / 255.0) - 1.0
        image1 = image1.contiguous(memory_format=mf)
        image2 = image2.contiguous(memory_format=mf)
        b = image1.shape[0]
        # one batched encoder pass over both images (fewer, larger GEMMs)
        fmap = self.fnet(torch.cat([image1, image2]))
        fmap1, fmap2 = fmap[:b], fmap[b:]
        corr_fn = self._corr_class(fmap1)(fmap1.float(), fmap2.float())
        cnet = self.cnet(image1)
        net, inp = torch.split(cnet, [self.hdim, self.cdim], dim=1)
        inp = F.relu(inp)
        _, _, h8, w8 = fmap1.shape

        # persistent GRU conv-input buffers: [h | x]
        cbuf = self.hdim + 128 + self.cdim
        hx = torch.empty(b, cbuf, h8, w8, device=image1.device, dtype=dtype,
                         memory_format=mf)
        rhx = torch.empty_like(hx, memory_format=mf)
        hx[:, :self.hdim] = torch.tanh(net)
        # context features are loop-invariant: written once into both
        # buffers; only the motion half is refreshed per iteration
        ctx_end = self.hdim + self.cdim
        hx[:, self.hdim:ctx_end] = inp
        rhx[:, self.hdim:ctx_end] = inp

        coords0 = self.coords_grid(b, h8, w8, image1.device, torch.float32)
        coords1 = coords0.clone()
        ub = self.update_block
        flow_up = None
        for it in range(iters):
            corr = corr_fn(coords1, nhwc=self.nhwc, out_dtype=dtype)
            flow = (coords1 - coords0).to(dtype).contiguous(memory_format=mf)
            # motion features written straight into hx's motion slice by
            # the encoder's conv epilogue; rhx mirrors with one copy
            ub.encoder(flow, corr, out=hx, out_off=ctx_end)
            rhx[:, ctx_end:] = hx[:, ctx_end:]
            ub.gru(hx, rhx, self.nhwc)
            net = hx[:, :self.hdim]
            if self.nhwc:
                # the channel slice of the CL buffer is strided; one copy
                # lets flow_head/mask take the in-tree conv kernel
                net = net.contiguous(memory_format=torch.channels_last)
            delta = ub.flow_head(net)
            coords1 = (coords1 + delta.float()).contiguous()
            if it == iters - 1 or not test_mode:
                # test mode only needs the final upsampled flow
                # (reference raft.py:170-172)
                up_mask = ub.mask(net)
                fl = (coords1 - coords0).to(dtype).contiguous(
                    memory_format=mf)
                flow_up = ops.convex_upsample(fl, up_mask, self.nhwc)
        if test_mode:
            return flow_up
        return coords1 - coords0, flow_up


class InputPadder:
    """Pad to a multiple of 8 (reference raft.py:27-44 semantics)."""

    def __init__(self, shape, mode: str = 'sintel'):
        h, w = shape[-2:]
        ph = ((h + 7) // 8) * 8 - h
        pw = ((w + 7) // 8) * 8 - w
        if mode == 'sintel':
            self._pad = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
        else:
            self._pad = [pw // 2, pw - pw // 2, 0, ph]

    def pad(self, *inputs):
        return [F.pad(x, self._pad, mode='replicate') for x in inputs]

    def unpad(self, x):
        h, w = x.shape[-2:]
        c = [self._pad[2], h - self._pad[3], self._pad[0], w - self._pad[1]]
        return x[..., c[0]:c[1], c[2]:c[3]]
