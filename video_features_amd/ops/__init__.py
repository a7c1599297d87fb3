"""Op dispatch layer: hand-written CDNA4 HIP kernels on GPU, PyTorch on CPU.

Policy (MI355X-first, no silent fallbacks): when a tensor lives on a GPU, the
in-tree HIP extension ``video_features_amd/ops/_vfa_hip.so`` (built by
``setup.py build_ext --inplace`` for gfx950) MUST be present — ops raise
rather than silently falling back to eager PyTorch, so a GPU run always
exercises the native path.  On CPU the pure-PyTorch reference implementations
run; they double as the numerics references the GPU tests compare against.

Set ``VFA_FORCE_TORCH_OPS=1`` to force the PyTorch path on GPU (A/B
benchmarking only).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

_ext = None
_ext_err: Optional[str] = None


def env_flag(name: str) -> bool:
    """Boolean env knob: '', '0', 'false', 'no', 'off' (any case) are False —
    so VFA_X=0 really disables (documented knob-table semantics)."""
    return os.environ.get(name, '').strip().lower() not in (
        '', '0', 'false', 'no', 'off')


def _load_extension():
    global _ext, _ext_err
    if _ext is not None or _ext_err is not None:
        return _ext
    try:
        from . import _vfa_hip  # built in-tree for gfx950
        _ext = _vfa_hip
    except ImportError as e:
        _ext_err = str(e)
    return _ext


def hip_available() -> bool:
    return _load_extension() is not None


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if env_flag('VFA_FORCE_TORCH_OPS'):
        return False
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            'Tensor is on GPU but the VFA HIP extension is not built '
            f'(import error: {_ext_err}). Build it in-tree with '
            '`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). '
            'Refusing to fall back to eager PyTorch on a GPU run.')
    return True


def native_ready(x: torch.Tensor, *, knob: Optional[str] = None,
                 channels_last: bool = False) -> bool:
    """The one answer to "does ``x`` take a model's in-tree bf16 path?":
    a bf16 GPU tensor with the extension loaded, ``VFA_FORCE_TORCH_OPS`` and
    the opt-out ``knob`` (if given) unset and, with ``channels_last``, that
    layout.  Never raises: a model asks it once and takes its fused or its
    module path as a whole; ``_use_hip`` does the raising inside each op."""
    return bool(x.is_cuda and x.dtype == torch.bfloat16 and hip_available()
                and not env_flag('VFA_FORCE_TORCH_OPS')
                and not (knob and env_flag(knob))
                and (not channels_last or (x.dim() == 4 and x.is_contiguous(
                    memory_format=torch.channels_last))))


# the dtypes the dtype-generic kernels instantiate (dispatch_dtype)
_FLOAT_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _store_slice(out: Optional[torch.Tensor], out_off: int,
                 y: torch.Tensor) -> torch.Tensor:
    """``y`` itself without ``out``; else ``out`` with ``y`` assigned to its
    channels [out_off, out_off + C_y)."""
    if out is None:
        return y
    out[:, out_off:out_off + y.shape[1]] = y
    return out


def _slice_width(name: str, x: torch.Tensor, in_off: int,
                 in_ch: Optional[int], aligned: bool = False) -> int:
    """Channels op ``name`` reads of ``x``: all of them without ``in_ch``,
    else [in_off, in_off + in_ch).  ``aligned``: the kernels read the slice
    in place, so it must sit on multiples of 8 inside the buffer."""
    if in_ch is None:
        if in_off:
            raise ValueError(f'{name}: in_off needs in_ch')
        return x.shape[1]
    if aligned and (in_off % 8 or x.shape[1] % 8
                    or in_off + in_ch > x.shape[1]):
        raise ValueError(
            f'{name}: slice [{in_off}, {in_off + in_ch}) of a '
            f'{x.shape[1]}-channel buffer needs in_off and the buffer '
            'width to be multiples of 8 and the rounded slice inside it')
    return in_ch


def derived(module: torch.nn.Module, attr: str, params, make, extra=None):
    """``make()`` — tensors derived from ``params`` (None entries skipped) —
    cached on ``module`` as ``attr`` = (key, value).  The key holds every
    parameter's version (an in-place write such as load_state_dict
    invalidates), dtype, device and pointer (``.to()`` replaces them), and
    ``extra``.  ``make`` runs under ``no_grad``: what is cached never hangs
    on an autograd graph."""
    key = tuple((p._version, p.dtype, p.device, p.data_ptr())
                for p in params if p is not None) + (extra,)
    ent = getattr(module, attr, None)
    if ent is None or ent[0] != key:
        with torch.no_grad():
            ent = (key, make())
        setattr(module, attr, ent)
    return ent[1]


# ---------------------------------------------------------------- layernorm
def layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
               eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm over the last dim. HIP path: one-pass fused kernel
    (vectorized bf16, wave reduction)."""
    if _use_hip(x) and x.dtype in _FLOAT_DTYPES:
        return _ext.layer_norm(x.contiguous(), weight, bias, eps)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """CLIP's QuickGELU: x * sigmoid(1.702 x)."""
    if _use_hip(x) and x.dtype in _FLOAT_DTYPES:
        return _ext.quick_gelu(x.contiguous())
    return x * torch.sigmoid(1.702 * x)


def gelu(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x) and x.dtype in _FLOAT_DTYPES:
        return _ext.gelu_tanh(x.contiguous())
    return torch.nn.functional.gelu(x, approximate='tanh')


# ---------------------------------------------------------------- attention
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              scale: Optional[float] = None) -> torch.Tensor:
    """Batched MHSA core: inputs (B, H, N, D) → (B, H, N, D).

    HIP path: fused flash-style MFMA kernel (bf16, one workgroup per (b, h)
    query tile, online softmax). Torch path: explicit softmax reference.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if (_use_hip(q) and q.dtype in _FLOAT_DTYPES
            and q.shape[-2] <= 64 and q.shape[-1] <= 128):
        # fused kernel covers the ViT shapes (N<=64 tokens); longer
        # sequences take the rocBLAS GEMM + softmax path below
        return _ext.mhsa(q.contiguous(), k.contiguous(), v.contiguous(),
                         float(scale))
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    return attn @ v


def layer_norm_residual(x: torch.Tensor, res: torch.Tensor,
                        weight: torch.Tensor, bias: torch.Tensor,
                        eps: float = 1e-5):
    """Fused ``s = x + res; y = layer_norm(s)`` → (y, s).  One kernel on the
    HIP path (removes the eager add + a full re-read)."""
    if _use_hip(x) and x.dtype in _FLOAT_DTYPES:
        y, s = _ext.layer_norm_residual(x.contiguous(), res.contiguous(),
                                        weight, bias, eps)
        return y, s
    s = x + res
    y = torch.nn.functional.layer_norm(s, (s.shape[-1],), weight, bias, eps)
    return y, s


def clip_embed_ln(pe: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor,
                  weight: torch.Tensor, bias: torch.Tensor,
                  eps: float = 1e-5) -> torch.Tensor:
    """CLIP ViT token embedding: ``pe`` (T, P, W) patch embeddings, ``cls``
    (W), ``pos`` (P+1, W) and the ``ln_pre`` affine give (T, P+1, W) with
    ``out[t, j] = LN((cls if j == 0 else pe[t, j-1]) + pos[j])``.

    HIP path (W % 8 == 0; bf16, fp16 and fp32 instantiate one template): one
    kernel reads ``pe`` once and writes the normalised tokens once, sum and
    statistics in f32, one rounding.  CPU tensors, W % 8 != 0 and
    ``VFA_FORCE_TORCH_OPS=1`` take the cat / add / ``layer_norm``
    composition."""
    if (_use_hip(pe) and pe.shape[-1] % 8 == 0
            and pe.dtype in _FLOAT_DTYPES):
        return _ext.clip_embed_ln(pe.contiguous(), cls, pos, weight, bias,
                                  eps)
    c = cls.to(pe.dtype).expand(pe.shape[0], 1, -1)
    x = torch.cat([c, pe], dim=1) + pos.to(pe.dtype)
    return layer_norm(x, weight, bias, eps)


def preprocess_u8_chw(frames_u8: torch.Tensor, mean, std,
                      bf16: bool = True) -> torch.Tensor:
    """(T, H, W, 3) uint8 → (T, 3, H, W) normalized bf16/f32 in one fused
    kernel on GPU; eager chain on CPU (and for H*W not divisible by 4 —
    the kernel vectorizes 4 pixels per thread)."""
    if _use_hip(frames_u8) and \
            (frames_u8.shape[1] * frames_u8.shape[2]) % 4 == 0:
        return _ext.u8_chw_norm(frames_u8.contiguous(), list(map(float, mean)),
                                list(map(float, std)), bf16)
    x = frames_u8.permute(0, 3, 1, 2).float() / 255.0
    mean_t = torch.as_tensor(mean, dtype=x.dtype, device=x.device)
    std_t = torch.as_tensor(std, dtype=x.dtype, device=x.device)
    x = (x - mean_t[:, None, None]) / std_t[:, None, None]
    return x.to(torch.bfloat16) if bf16 else x


def patchify(x: torch.Tensor, p: int) -> torch.Tensor:
    """(T, C, H, W) → (T, (H/p)·(W/p), C·p·p): the rows a stride == kernel
    conv reads, patch order (gy, gx), K order (c, py, px) — the layout of
    ``conv.weight.reshape(out, -1)``.  Pure data movement, bit-identical on
    every path.

    HIP path (itemsize 2 or 4, p·itemsize % 16 == 0, H % p == W % p == 0,
    16-B aligned storage): one pass of 16-B vectors, writes coalesced.
    Everything else — CPU tensors, other shapes, ``VFA_FORCE_TORCH_OPS=1`` —
    takes the reshape / permute composition."""
    t, c, h, w = x.shape
    if h % p or w % p:
        raise ValueError(f'patchify: H, W = {h}, {w} must be multiples of '
                         f'p = {p}')
    es = x.element_size()
    if (_use_hip(x) and es in (2, 4) and (p * es) % 16 == 0
            and x.numel() > 0):
        xc = x.contiguous()
        if xc.data_ptr() % 16 == 0:
            return _ext.patchify(xc, int(p))
    gy, gx = h // p, w // p
    xp = x.reshape(t, c, gy, p, gx, p).permute(0, 2, 4, 1, 3, 5)
    return xp.reshape(t, gy * gx, c * p * p)


# kernels ops.mhsa_fused can run on the HIP path: 0 is the routing every
# caller gets (N <= 64: the register-resident kernel; longer: the general
# flash kernel), 1 the general kernel at any N (its single-tile branch for
# N <= 64)
MHSA_VARIANTS = (0, 1)


def mhsa_fused(qkv: torch.Tensor, heads: int,
               scale: Optional[float] = None, variant: int = 0) -> torch.Tensor:
    """Fused MHSA from the packed qkv projection: (B, N, 3*E) → (B, N, E).

    HIP path (bf16, head_dim 64): the MFMA flash kernel consumes the packed
    layout directly — no permute/contiguous copies on either side.
    ``variant`` picks the kernel per call (``MHSA_VARIANTS``; tests and A/B
    replays run several in one process) and means nothing on the torch path:
    explicit reshape + softmax reference.
    """
    if variant not in MHSA_VARIANTS:
        raise ValueError(f'mhsa_fused: variant must be one of {MHSA_VARIANTS}')
    b, n, three_e = qkv.shape
    e = three_e // 3
    d = e // heads
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if _use_hip(qkv) and qkv.dtype == torch.bfloat16 and d == 64:
        qkv5 = qkv.view(b, n, 3, heads, d)
        return _ext.flash_qkv(qkv5.contiguous(), float(scale), int(variant))
    q, k, v = qkv.view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4).unbind(0)
    o = attention(q.contiguous(), k.contiguous(), v.contiguous(), scale)
    return o.permute(0, 2, 1, 3).reshape(b, n, e)


# ---------------------------------------------------------------- flow ops
def pwc_correlation(f1: torch.Tensor, f2: torch.Tensor,
                    max_disp: int = 4, out: Optional[torch.Tensor] = None,
                    out_off: int = 0, act: str = 'none') -> torch.Tensor:
    """PWC cost volume: (B, C, H, W) × 2 → (B, (2*max_disp+1)^2, H, W).

    Channel-mean dot products over a (2d+1)^2 displacement window of f2
    (reference vendors this as 4 CuPy CUDA kernels,
    models/pwc/pwc_src/correlation.py; here it is ONE fused CDNA4 kernel on
    GPU and a vectorized torch implementation on CPU).

    ``act`` is 'none' or 'leaky_relu' (slope 0.1), applied to the cost
    volume.  With ``out`` (B, >= out_off + 81, H, W) the result goes into
    its channels [out_off, out_off + 81) and ``out`` is returned; on GPU
    ``out`` is a channels_last bf16 buffer and the kernels store the slice
    themselves (no f32 NCHW tensor, cast or copy).

    bf16 ``f1`` and ``f2`` that are channels_last-contiguous (and not also
    NCHW-contiguous) are read in place by the NHWC kernel variants: no
    repack, no padded copy, any C <= 256; a result without ``out`` is then
    channels_last as well.  NCHW inputs keep the repack kernels.
    """
    if act not in ('none', 'leaky_relu'):
        raise ValueError(f'pwc_correlation: unsupported act {act!r}')
    leaky = act == 'leaky_relu'
    if _use_hip(f1):
        direct = out is None or (
            out.dtype == torch.bfloat16
            and out.is_contiguous(memory_format=torch.channels_last))
        if (max_disp == 4 and f1.dtype == torch.bfloat16
                and f2.dtype == torch.bfloat16 and _cl_only(f1)
                and _cl_only(f2)):
            y = _ext.pwc_correlation_nhwc(f1, f2, out if direct else None,
                                          out_off, leaky)
        else:
            y = _ext.pwc_correlation(f1.contiguous(), f2.contiguous(),
                                     max_disp, out if direct else None,
                                     out_off, leaky)
        if direct:
            return y
    else:
        y = _pwc_correlation_torch(f1, f2, max_disp)
        if leaky:
            y = torch.nn.functional.leaky_relu(y, 0.1)
    return _store_slice(out, out_off, y)


def _pwc_correlation_torch(f1: torch.Tensor, f2: torch.Tensor,
                           max_disp: int) -> torch.Tensor:
    b, c, h, w = f1.shape
    d = max_disp
    f2p = torch.nn.functional.pad(f2, (d, d, d, d))
    out = f1.new_empty(b, (2 * d + 1) ** 2, h, w)
    i = 0
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out[:, i] = (f1 * f2p[:, :, dy:dy + h, dx:dx + w]).mean(dim=1)
            i += 1
    return out


def _cl_only(t: torch.Tensor) -> bool:
    """4-D, channels_last-contiguous and not also NCHW-contiguous (C == 1 or
    H == W == 1 tensors are both; they count as NCHW)."""
    return (t.dim() == 4
            and t.is_contiguous(memory_format=torch.channels_last)
            and not t.is_contiguous())


def bilinear_warp(x: torch.Tensor, flow: torch.Tensor,
                  scale: float = 1.0) -> torch.Tensor:
    """Backward-warp ``x`` (B, C, H, W) by ``flow`` (B, 2, H, W) with border
    zero-masking semantics matching the reference's PWC ``Backward`` warp
    (reference models/pwc/pwc_src/pwc_net.py:23-41).  The sample point is
    (x + scale*fx, y + scale*fy); a sample counts only when it lies fully
    inside the image.

    A bf16 ``x`` that is channels_last-contiguous (and not also
    NCHW-contiguous) with C % 8 == 0 runs the NHWC kernel: the result is
    channels_last, the scale is applied in f32 inside the kernel and
    ``flow`` is read through its strides (a 2-channel slice view of a wider
    channels_last buffer included), no copy of it is made.  NCHW inputs keep
    the NCHW kernel; there and on the CPU ``scale`` multiplies the flow."""
    if _use_hip(x):
        if (x.dtype == torch.bfloat16 and _cl_only(x)
                and x.shape[1] % 8 == 0):
            if flow.dtype != torch.bfloat16:
                flow = flow.to(torch.bfloat16)
            return _ext.bilinear_warp_nhwc(x, flow, float(scale))
        if scale != 1.0:
            flow = flow * scale
        return _ext.bilinear_warp(x.contiguous(), flow.contiguous())
    if scale != 1.0:
        flow = flow * scale
    b, c, h, w = x.shape
    yy, xx = torch.meshgrid(
        torch.arange(h, device=x.device, dtype=x.dtype),
        torch.arange(w, device=x.device, dtype=x.dtype), indexing='ij')
    grid_x = (xx[None] + flow[:, 0]) / max(w - 1, 1) * 2 - 1
    grid_y = (yy[None] + flow[:, 1]) / max(h - 1, 1) * 2 - 1
    grid = torch.stack([grid_x, grid_y], dim=-1)
    warped = torch.nn.functional.grid_sample(x, grid, mode='bilinear',
                                             padding_mode='zeros',
                                             align_corners=True)
    mask = torch.nn.functional.grid_sample(torch.ones_like(x[:, :1]), grid,
                                           mode='bilinear', padding_mode='zeros',
                                           align_corners=True)
    return warped * (mask > 0.999).to(x.dtype)


def corr_lookup(pyramid, coords: torch.Tensor, radius: int = 4,
                nhwc: bool = False,
                out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Fused RAFT correlation-pyramid lookup.

    ``pyramid``: list of up to 4 levels, each (B*H*W, 1, h_l, w_l) fp32
    (one correlation plane per query pixel, as built by CorrPyramid);
    ``coords``: (B, 2, H, W) fp32 pixel coords at level 0.  Returns
    (B, L*(2r+1)^2, H, W) — the concatenation over levels of the bilinear
    samples of the (2r+1)^2 displacement window, matching the reference
    lookup (models/raft/raft_src/corr.py:36-50) but as ONE kernel with the
    per-pixel planes staged through LDS.
    """
    if out_dtype is None:
        out_dtype = coords.dtype
    if _use_hip(coords) and radius == 4:
        return _ext.corr_lookup(list(pyramid), coords.contiguous(), nhwc,
                                out_dtype,
                                env_flag('VFA_CORR_GMEM'))
    # torch reference: per-level grid_sample of the displacement window
    b, _, h, w = coords.shape
    r = radius
    cc = coords.permute(0, 2, 3, 1)
    out = []
    for lvl, corr in enumerate(pyramid):
        dx = torch.linspace(-r, r, 2 * r + 1, device=coords.device,
                            dtype=torch.float32)
        # channel t = i*9+j offsets (x + d_i, y + d_j) — the REFERENCE's
        # order (corr.py:39 stacks meshgrid(dy, dx) last and adds it to
        # (x, y) coords), which pretrained motion-encoder weights consume
        delta = torch.stack(torch.meshgrid(dx, dx, indexing='ij'), dim=-1)
        centroid = cc.reshape(b * h * w, 1, 1, 2) / (2 ** lvl)
        window = centroid + delta[None]
        sampled = grid_sample_bilinear(corr, window)
        out.append(sampled.reshape(b, h, w, -1))
    res = torch.cat(out, dim=-1).permute(0, 3, 1, 2).to(out_dtype)
    return res.contiguous(memory_format=torch.channels_last) if nhwc \
        else res.contiguous()


def _corr_otf_axis(c: torch.Tensor, lvl: int, n: int):
    """One axis of one level: (integer origin of the 10-point grid, shared
    fractional part) of pixel coordinate ``c / 2**lvl`` on a level ``n``
    points long.  floor is clamped to [-16, n + 16] (a window wholly outside
    either way), so huge or non-finite coordinates index nothing."""
    s = c / (2 ** lvl)
    f = torch.floor(s)
    fc = torch.nan_to_num(f, nan=-16.0).clamp(-16.0, n + 16.0)
    a = torch.where(f == fc, s - f, torch.zeros_like(s))
    return fc.long() - 4, a


def corr_lookup_otf(f1: torch.Tensor, f2_levels, coords: torch.Tensor,
                    radius: int = 4, nhwc: bool = False,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """RAFT correlation lookup computed on the fly from the features: what
    ``corr_lookup`` returns for the all-pairs pyramid of the same feature
    maps, without building that pyramid (reference AlternateCorrBlock,
    models/raft/raft_src/corr.py:63-91).

    ``f1``: (B, H, W, D) fp32, pixel-major; ``f2_levels``: up to 4 levels
    (B, h_l, w_l, D) fp32, the second feature map avg-pooled l times;
    ``coords``: (B, 2, H, W) fp32 pixel coords at level 0.  Returns
    (B, L*(2r+1)^2, H, W), tap t = i*(2r+1)+j offsetting X by i-r and Y by
    j-r.  Average pooling and the dot product are linear, so level l of the
    pooled volume is f1 . f2_l; the (2r+1)^2 taps of a pixel share one
    fractional part and read the (2r+2)^2 integer grid around
    floor(coords / 2^l): that many dot products, then four-term blends.

    GPU tensors with radius 4, D % 32 == 0 and D <= 256 run the HIP kernel
    (``corr_otf``: one wave per query pixel, one dispatch for all levels).
    CPU tensors and other shapes run the torch composition below, which
    indexes in pixel units (a level 1 wide or 1 high is sampled where the
    mathematics puts it)."""
    if out_dtype is None:
        out_dtype = coords.dtype
    b, h, w, d = f1.shape
    if (_use_hip(coords) and radius == 4 and d % 32 == 0 and d <= 256
            and len(f2_levels) <= 4):
        return _ext.corr_lookup_otf(f1, list(f2_levels),
                                    coords.float().contiguous(), nhwc,
                                    out_dtype)
    n = 2 * radius + 2               # grid points per axis
    ar = torch.arange(n, device=coords.device)
    cx, cy = coords[:, 0].float(), coords[:, 1].float()     # (B, H, W)
    bi = torch.arange(b, device=coords.device).view(b, 1, 1, 1, 1)
    out = []
    for lvl, f2 in enumerate(f2_levels):
        hl, wl = f2.shape[1:3]
        x0, ax = _corr_otf_axis(cx, lvl, wl)
        y0, ay = _corr_otf_axis(cy, lvl, hl)
        if radius != 4:
            x0, y0 = x0 + 4 - radius, y0 + 4 - radius
        x = (x0[..., None] + ar)[..., :, None]              # (B, H, W, n, 1)
        y = (y0[..., None] + ar)[..., None, :]              # (B, H, W, 1, n)
        ok = (x >= 0) & (x < wl) & (y >= 0) & (y < hl)
        g = f2[bi, y.clamp(0, hl - 1), x.clamp(0, wl - 1)]  # (B,H,W,n,n,D)
        c = torch.einsum('bhwd,bhwijd->bhwij', f1, g) / math.sqrt(d)
        c = c * ok.to(c.dtype)
        ax, ay = ax[..., None, None], ay[..., None, None]
        v = ((1 - ax) * (1 - ay) * c[..., :-1, :-1]
             + ax * (1 - ay) * c[..., 1:, :-1]
             + (1 - ax) * ay * c[..., :-1, 1:]
             + ax * ay * c[..., 1:, 1:])
        out.append(v.reshape(b, h, w, -1))
    res = torch.cat(out, dim=-1).permute(0, 3, 1, 2).to(out_dtype)
    return res.contiguous(memory_format=torch.channels_last) if nhwc \
        else res.contiguous()


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor,
                    nhwc: bool = False) -> torch.Tensor:
    """RAFT convex-combination 8x flow upsample (reference raft.py:100-111).

    ``flow`` (B, 2, h, w); ``mask`` (B, 576, h, w) RAW conv output — the
    0.25 scale and the softmax over the 9 neighbors happen inside.  Returns
    (B, 2, 8h, 8w) contiguous.  One kernel on GPU (replaces unfold + softmax
    + mul-sum + two permutes).
    """
    if _use_hip(flow):
        return _ext.convex_upsample(flow, mask, nhwc)
    b, _, h, w = flow.shape
    m = (0.25 * mask.float()).view(b, 1, 9, 8, 8, h, w).softmax(dim=2)
    up = torch.nn.functional.unfold(8 * flow.float(), 3, padding=1)
    up = up.view(b, 2, 9, 1, 1, h, w)
    up = (m * up).sum(dim=2)
    return up.permute(0, 1, 4, 2, 5, 3).reshape(b, 2, 8 * h, 8 * w) \
        .to(flow.dtype)


def gru_zr(zr: torch.Tensor, hx: torch.Tensor, rhx: torch.Tensor,
           nhwc: bool = False) -> torch.Tensor:
    """Fused SepConvGRU z/r gates: ``zr`` (B, 2C, h, w) is the merged
    z|r conv output; ``hx``/``rhx`` are the persistent (B, C+X, h, w)
    conv-input buffers whose first C channels hold h.  Computes
    z = sigmoid(zr[:, :C]), writes sigmoid(zr[:, C:]) * h into rhx[:, :C]
    in place, returns z."""
    c = zr.shape[1] // 2
    if _use_hip(zr):
        return _ext.gru_zr(zr, hx, rhx, nhwc)
    z = torch.sigmoid(zr[:, :c])
    r = torch.sigmoid(zr[:, c:])
    rhx[:, :c] = r * hx[:, :c]
    return z


def gru_out(q: torch.Tensor, z: torch.Tensor, hx: torch.Tensor,
            nhwc: bool = False) -> None:
    """Fused GRU update: hx[:, :C] = (1-z)*hx[:, :C] + z*tanh(q), in place."""
    if _use_hip(q):
        _ext.gru_out(q, z, hx, nhwc)
        return
    c = q.shape[1]
    hx[:, :c] = (1 - z) * hx[:, :c] + z * torch.tanh(q)


def instance_norm(x: torch.Tensor, eps: float = 1e-5, relu: bool = False,
                  nhwc: bool = False) -> torch.Tensor:
    """InstanceNorm2d (affine=False) with optional fused ReLU — ONE kernel
    on GPU (torch lowers this to batch-norm stats + transform + separate
    relu, three HBM round-trips)."""
    if _use_hip(x):
        return _ext.instance_norm2d(x, eps, relu, nhwc)
    y = torch.nn.functional.instance_norm(x, eps=eps)
    return torch.nn.functional.relu(y) if relu else y


def _pad1(n, k, s):
    """TF-SAME (before, after) zero padding of one dim: size n, window k,
    stride s; the odd cell goes at the end."""
    total = max(k - s, 0) if n % s == 0 else max(k - (n % s), 0)
    return total // 2, total - total // 2


def maxpool3d_same(x: torch.Tensor, kernel, stride) -> torch.Tensor:
    """TF-SAME max_pool3d (zero padding, asymmetric, extra cell at the end —
    reference i3d_net.py:108-120).  GPU: one fused kernel, no padded copy,
    no argmax indices."""
    t, h, w = x.shape[-3:]
    pt, ph, pw = (_pad1(t, kernel[0], stride[0]), _pad1(h, kernel[1], stride[1]),
                  _pad1(w, kernel[2], stride[2]))
    if _use_hip(x):
        out_sz = [(t + pt[0] + pt[1] - kernel[0]) // stride[0] + 1,
                  (h + ph[0] + ph[1] - kernel[1]) // stride[1] + 1,
                  (w + pw[0] + pw[1] - kernel[2]) // stride[2] + 1]
        return _ext.maxpool3d_same(x.contiguous(), list(kernel), list(stride),
                                   [pt[0], ph[0], pw[0]], out_sz)
    xp = torch.nn.functional.pad(
        x, (pw[0], pw[1], ph[0], ph[1], pt[0], pt[1]))
    return torch.nn.functional.max_pool3d(xp, tuple(kernel), tuple(stride))


def maxpool2d_same(x: torch.Tensor, kernel, stride,
                   nhwc: bool = False) -> torch.Tensor:
    """Spatial TF-SAME max_pool2d (zero padding, extra cell at the end) —
    the spatial half of I3D's TF-SAME 3D pools in the flattened
    (B*T, C, H, W) path; the temporal half is a shifted elementwise max."""
    h, w = x.shape[-2:]
    ph, pw = _pad1(h, kernel[0], stride[0]), _pad1(w, kernel[1], stride[1])
    if _use_hip(x):
        # resolve the layout defensively: a tensor can be CL-contiguous,
        # NCHW-contiguous, both (trivial dims), or neither (strided view);
        # what is not NCHW-contiguous runs (converted if need be) as NHWC
        return _maxpool2d_hip(x, kernel, stride, (ph, pw),
                              nhwc or not x.is_contiguous())
    xp = torch.nn.functional.pad(x, (pw[0], pw[1], ph[0], ph[1]))
    return torch.nn.functional.max_pool2d(xp, tuple(kernel), tuple(stride))


def _maxpool2d_hip(x: torch.Tensor, kernel, stride, pads,
                   nhwc: bool) -> torch.Tensor:
    """The max-pool kernel with (before, after) zero ``pads`` of H and W; an
    ``nhwc`` input that is not channels_last-contiguous is converted."""
    if nhwc and not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    out_sz = [(n + sum(p) - k) // s + 1
              for n, p, k, s in zip(x.shape[-2:], pads, kernel, stride)]
    return _ext.maxpool2d_same(x, list(kernel), list(stride),
                               [p[0] for p in pads], out_sz, nhwc)


def maxpool2d(x: torch.Tensor, kernel, stride, padding,
              nhwc: bool = False) -> torch.Tensor:
    """torch-semantics max_pool2d (symmetric padding, clamped windows —
    identical to torch's -inf padding) on the same HIP kernel; replaces
    torch's NHWC maxpool (which always computes argmax indices) for the
    ResNet stem."""
    if _use_hip(x):
        return _maxpool2d_hip(x, kernel, stride, [(padding, padding)] * 2,
                              nhwc)
    return torch.nn.functional.max_pool2d(x, tuple(kernel), tuple(stride),
                                          padding)


def avgpool2d_nhwc(x: torch.Tensor, k: int = 2) -> torch.Tensor:
    """``nn.AvgPool2d(k)`` (window = stride = k, floor output size) on a
    channels_last bf16 (B, C, H, W) map — CLIP's ModifiedResNet pools where
    torchvision's ResNet strides.  HIP path: one memory-bound kernel, 16-B
    loads over channels, f32 sum, one rounding to bf16; the result is
    channels_last.  It requires C % 8 == 0 and raises otherwise.  CPU and
    non-bf16 tensors take ``F.avg_pool2d``."""
    if _use_hip(x) and x.dtype == torch.bfloat16:
        if x.shape[1] % 8 != 0:
            raise ValueError('avgpool2d_nhwc: C % 8 == 0 required on the '
                             f'HIP path, got C={x.shape[1]}')
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        return _ext.avgpool2d_nhwc(x, int(k))
    return torch.nn.functional.avg_pool2d(x, k)


def attnpool_tokens(x: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """Token matrix of CLIP's ``AttentionPool2d``: ``x`` (B, HW, C) — a free
    view of the channels_last trunk output — and the learned positional
    embedding ``pos`` (HW+1, C) give ``t`` (B, HW+1, C) with
    ``t[:, 0] = mean_j x[:, j] + pos[0]`` (mean in f32) and
    ``t[:, 1 + j] = x[:, j] + pos[1 + j]``.  HIP path (bf16): one read of
    ``x``, one write of ``t``, each value rounded once; requires C % 8 == 0
    and raises otherwise.  CPU and non-bf16 tensors take the torch
    construction in f32."""
    if pos.shape != (x.shape[1] + 1, x.shape[2]):
        raise ValueError(f'attnpool_tokens: pos must be (HW+1, C) = '
                         f'{(x.shape[1] + 1, x.shape[2])}, got '
                         f'{tuple(pos.shape)}')
    if _use_hip(x) and x.dtype == torch.bfloat16:
        if x.shape[2] % 8 != 0:
            raise ValueError('attnpool_tokens: C % 8 == 0 required on the '
                             f'HIP path, got C={x.shape[2]}')
        return _ext.attnpool_tokens(x.contiguous(),
                                    pos.to(torch.bfloat16).contiguous())
    xf = x.float()
    t = torch.cat([xf.mean(dim=1, keepdim=True), xf], dim=1) + pos.float()
    return t.to(x.dtype)


def attention_pool(q: torch.Tensor, kv: torch.Tensor,
                   heads: int) -> torch.Tensor:
    """Single-query multi-head attention, the attention step of CLIP's
    ``AttentionPool2d``: ``q`` (B, C) is the projection of token 0 only,
    ``kv`` (B, L, 2C) is packed ``[k | v]`` as one GEMM with the
    concatenated ``[k_proj; v_proj]`` weight writes it; returns (B, C) with
    ``o[b, h] = softmax_j(q_h . k_jh / sqrt(d)) . v_jh``, d = C / heads.

    HIP path (bf16, d == 64 — all four CLIP ResNet towers): one wave per
    (b, h), f32 arithmetic, max-subtracted online softmax over 64-key
    chunks, any L >= 1.  Any other head dim, dtype, or a CPU tensor takes
    the torch composition below (f32 math, result in ``q``'s dtype)."""
    b, c = q.shape
    l = kv.shape[1]
    d = c // heads
    if (_use_hip(q) and q.dtype == torch.bfloat16
            and kv.dtype == torch.bfloat16 and d == 64 and c == heads * 64):
        return _ext.attention_pool(q.contiguous(), kv.contiguous(),
                                   int(heads))
    qh = q.float().view(b, heads, 1, d)
    kh = kv[..., :c].float().reshape(b, l, heads, d).permute(0, 2, 1, 3)
    vh = kv[..., c:].float().reshape(b, l, heads, d).permute(0, 2, 1, 3)
    attn = (qh @ kh.transpose(-2, -1)) / math.sqrt(d)
    o = attn.softmax(dim=-1) @ vh                     # (B, H, 1, d)
    return o.reshape(b, c).to(q.dtype)


_ACT_IDS = {'none': 0, 'relu': 1, 'quick_gelu': 2, 'gelu': 3,
            'leaky_relu': 4}


def _act_id(act: str) -> int:
    if act not in _ACT_IDS:
        raise ValueError(f'unknown activation {act!r}; expected one of '
                         f'{sorted(_ACT_IDS)}')
    return _ACT_IDS[act]


def _apply_act(y: torch.Tensor, act: str) -> torch.Tensor:
    """The torch form of the kernels' fused epilogue activation."""
    _act_id(act)
    if act == 'relu':
        return torch.nn.functional.relu(y)
    if act == 'quick_gelu':
        return y * torch.sigmoid(1.702 * y)
    if act == 'gelu':
        return torch.nn.functional.gelu(y, approximate='tanh')
    if act == 'leaky_relu':
        return torch.nn.functional.leaky_relu(y, 0.1)
    return y


def linear_act(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None,
               act: str = 'none',
               res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(x @ weight^T + bias [+ res])`` — one fused MFMA GEMM on GPU
    (bf16, 128/256-wide tiles, glds-staged LDS with st_16x32 swizzle; bias,
    residual add, and activation in the epilogue).  Falls back to F.linear
    (+ add + activation) on CPU or unsupported shapes."""
    k = x.shape[-1]
    n = weight.shape[0]
    if (_use_hip(x) and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and k % 8 == 0 and n >= 16
            and not env_flag('VFA_NO_LTGEMM')):
        x2 = x.reshape(-1, k).contiguous()
        r2 = res.reshape(-1, n).contiguous() if res is not None else None
        out = _ext.linear_act(x2, weight.contiguous(), bias, r2,
                              _act_id(act))
        return out.reshape(*x.shape[:-1], n)
    y = torch.nn.functional.linear(x, weight, bias)
    if res is not None:
        y = y + res.reshape(y.shape)
    return _apply_act(y, act)


# ------------------------------------------------- LayerNorm folded into GEMMs
# linear -> (+ residual) -> LayerNorm -> linear without the LayerNorm pass:
# the first GEMM's epilogue adds the residual and emits row statistics
# (linear_res_stats), the second runs on the un-normalised rows with the LN
# affine folded into its weight (fold_ln_linear, linear_ln_act).  The
# statistics travel as partials, (M, T, 2) f32: for each row the (mean, M2 =
# Σ (x - mean)²) of T equal-width column groups — one per 256-column tile
# of the producing GEMM, T = 1 from the torch composition.  The consumer's
# epilogue merges them (Chan's formula); ln_stats does the same in torch.
def fused_ln_tiles(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """True when ``linear_res_stats`` / ``linear_ln_act`` of ``x`` (..., K)
    with ``weight`` (N, K) run their fused kernel: bf16 on the GPU and all
    full 256x256x64 tiles.  Anything else takes their torch composition."""
    k, n = x.shape[-1], weight.shape[0]
    m = x.numel() // max(k, 1)
    return bool(native_ready(x, knob='VFA_NO_LTGEMM')
                and weight.dtype == torch.bfloat16
                and m > 0 and m % 256 == 0 and n % 256 == 0 and k % 64 == 0)


def linear_res_stats(x: torch.Tensor, weight: torch.Tensor,
                     bias: Optional[torch.Tensor], res: torch.Tensor):
    """``s = x @ weight^T + bias + res`` and the statistics partials of its
    rows → (s, stats (M, T, 2) f32), taken from the rounded ``s``.  One
    persistent MFMA GEMM on the fused route (``fused_ln_tiles``), T = N/256;
    otherwise ``linear_act`` with the residual and T = 1 in torch."""
    n = weight.shape[0]
    if fused_ln_tiles(x, weight):
        s, stats = _ext.linear_res_stats(
            x.reshape(-1, x.shape[-1]).contiguous(), weight.contiguous(),
            bias, res.reshape(-1, n).contiguous())
        return s.reshape(*x.shape[:-1], n), stats
    s = linear_act(x, weight, bias, 'none', res)
    sf = s.reshape(-1, n).float()
    var, mean = torch.var_mean(sf, dim=1, unbiased=False)
    return s, torch.stack([mean, var * n], dim=1).unsqueeze(1)


def ln_stats(stats: torch.Tensor, n: int, eps: float = 1e-5) -> torch.Tensor:
    """Statistics partials (M, T, 2) of rows of width ``n`` → (M, 2) rows of
    LayerNorm (mean, rstd), in the partials' dtype."""
    gmean, gm2 = stats[..., 0], stats[..., 1]
    mean = gmean.mean(dim=1, keepdim=True)
    m2 = (gm2 + (n / stats.shape[1]) * (gmean - mean) ** 2).sum(dim=1)
    return torch.stack([mean[:, 0], torch.rsqrt(m2 / n + eps)], dim=1)


def fold_ln_linear(weight: torch.Tensor, bias: Optional[torch.Tensor],
                   ln_weight: torch.Tensor, ln_bias: torch.Tensor):
    """Fold a LayerNorm affine (γ, β) into the linear layer that follows it
    → (W', c, b') with, for un-normalised rows s with statistics (μ, rstd),

        layer_norm(s) @ W^T + b  =  rstd * (s @ W'^T - μ c) + b'

    W' = γ ⊙ W in the weight's dtype, c[n] = Σ_k W'[n, k] summed from the
    *rounded* W' (so acc - μ c is Σ (s_k - μ) W'_k whatever μ is), b' = b +
    W β.  c and b' are f32 (f64 for an f64 weight).  Weights only: computed
    once per model, not per call."""
    acc = torch.float64 if weight.dtype == torch.float64 else torch.float32
    w32 = weight.detach().to(acc)
    wf = (w32 * ln_weight.detach().to(acc)).to(weight.dtype)
    c = wf.double().sum(dim=1).to(acc)
    bf = w32 @ ln_bias.detach().to(acc)
    if bias is not None:
        bf = bf + bias.detach().to(acc)
    return wf.contiguous(), c.contiguous(), bf.contiguous()


def linear_ln_act(s: torch.Tensor, stats: torch.Tensor, wf: torch.Tensor,
                  c: torch.Tensor, bf: torch.Tensor, act: str = 'none',
                  eps: float = 1e-5, unfolded=None) -> torch.Tensor:
    """``act(linear(layer_norm(s)))`` from the un-normalised rows ``s``, their
    statistics partials (``linear_res_stats``) and the folded layer
    (``fold_ln_linear``): ``act(rstd * (s @ W'^T - μ c) + b')`` in the GEMM
    epilogue on the fused route, (μ, rstd) merged from the partials there.
    Off it (``fused_ln_tiles``) the result is ``layer_norm`` then
    ``linear_act`` with ``unfolded`` = (weight, bias, ln_weight, ln_bias), or
    the folded formula in torch without it."""
    n, k = wf.shape
    if fused_ln_tiles(s, wf):
        out = _ext.linear_ln_act(s.reshape(-1, k).contiguous(),
                                 stats.contiguous(), wf.contiguous(), c, bf,
                                 eps, _act_id(act))
        return out.reshape(*s.shape[:-1], n)
    if unfolded is not None:
        weight, bias, ln_weight, ln_bias = unfolded
        return linear_act(layer_norm(s, ln_weight, ln_bias, eps), weight,
                          bias, act)
    acc = torch.float64 if s.dtype == torch.float64 else torch.float32
    st = ln_stats(stats.to(acc), k, eps)
    y = s.reshape(-1, k).to(acc) @ wf.to(acc).t()
    y = st[:, 1:2] * (y - st[:, 0:1] * c.to(acc)) + bf.to(acc)
    return _apply_act(y, act).to(s.dtype).reshape(*s.shape[:-1], n)


def temporal_merge_fused(y: torch.Tensor, b: int, kt: int, st: int,
                         p0: int, relu: bool = False,
                         p1: Optional[int] = None) -> Optional[torch.Tensor]:
    """One-kernel temporal tap merge for the flattened-time conv3d
    decomposition (see models/_flat3d.py), with optional fused ReLU.
    Returns None when the HIP path does not apply (caller falls back to
    the strided-add composition)."""
    if (_use_hip(y)
            and y.is_contiguous(memory_format=torch.channels_last)):
        return _ext.temporal_merge(y, b, kt, st, p0,
                                   p0 if p1 is None else p1, relu)
    return None


def conv1x1_act(x: torch.Tensor, weight: torch.Tensor,
                bias: Optional[torch.Tensor] = None, act: str = 'none',
                res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """1x1 conv on a channels_last (B, C, H, W) tensor as ONE fused MFMA
    GEMM (M = B*H*W) with optional residual + activation epilogue — zero
    layout copies: the CL tensor IS the (M, C) matrix."""
    b, cin, h, w = x.shape
    x2 = x.permute(0, 2, 3, 1).reshape(-1, cin)
    r2 = res.permute(0, 2, 3, 1).reshape(-1, weight.shape[0]) \
        if res is not None else None
    y = linear_act(x2, weight.reshape(weight.shape[0], cin), bias, act, r2)
    return y.reshape(b, h, w, weight.shape[0]).permute(0, 3, 1, 2)


def conv2d_act(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None,
               stride=1, padding=0, act: str = 'none',
               res: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None,
               out_off: int = 0, dilation=1, in_off: int = 0,
               in_ch: Optional[int] = None) -> torch.Tensor:
    """Fused conv2d + bias + activation (+ residual) on channels_last bf16.

    GPU path: the in-tree implicit-GEMM MFMA kernel (conv2d.hip) — the
    hand-written CDNA4 replacement for MIOpen's igemm on the 3x3 / 1x5 /
    5x1 conv shapes of the ResNet / RAFT / I3D / VGGish stacks (reference
    conv stacks at models/raft/raft_src/extractor.py:118-192,
    models/i3d/i3d_src/i3d_net.py:37-105).  CPU / unsupported shapes:
    F.conv2d composition.

    ``dilation`` is an int or a pair.  ``in_ch`` makes ``x`` a wider buffer
    of which the conv reads channels [in_off, in_off + in_ch); the kernel
    reads the slice in place (in_off, in_ch and the buffer width multiples
    of 8).  ``out`` / ``out_off`` write a channel slice of a wider buffer,
    which may be ``x`` itself when the two slices are disjoint: the
    cat-free DenseNet step ``x = cat([conv(x), x], 1)``.
    """
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    dh, dw = (dilation, dilation) if isinstance(dilation, int) else dilation
    cx = _slice_width('conv2d_act', x, in_off, in_ch)
    if isinstance(padding, int):
        pt = pb = pl = pr = padding
    elif len(padding) == 2:
        pt = pb = padding[0]
        pl = pr = padding[1]
    else:                      # 4-way (TF-SAME even-input stems): t,b,l,r
        pt, pb, pl, pr = padding
    # weight.shape[1] may be x's channel count zero-padded up to 8 (the
    # caller pads the weight; the kernel's pad pass widens the input)
    if (_use_hip(x) and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and weight.shape[1] == (cx + 7) // 8 * 8
            and (in_ch is None or (in_ch % 8 == 0 and in_off % 8 == 0
                                   and x.shape[1] % 8 == 0))
            and x.is_contiguous(memory_format=torch.channels_last)
            and not env_flag('VFA_NO_CONV')):
        if (weight.shape[2] == 1 and weight.shape[3] == 1
                and (sh, sw) == (1, 1) and (pt, pb, pl, pr) == (0, 0, 0, 0)
                and weight.shape[1] == x.shape[1] and out is None
                and in_ch is None
                and weight.shape[0] % 8 == 0):
            # pure 1x1: the linear stack's router picks the right GEMM
            # structure — in particular the thin-K streaming kernel for
            # the M-huge R21D temporal convs (profiled 3.5x off the memory
            # floor on the tiled conv path at their ragged K)
            return conv1x1_act(x, weight, bias, act, res)
        w_cl = weight.contiguous(memory_format=torch.channels_last)
        r = res.contiguous(memory_format=torch.channels_last) \
            if res is not None else None
        return _ext.conv2d_nhwc(x, w_cl, bias, r, sh, sw, pt, pb, pl, pr,
                                _act_id(act), out, out_off, dh, dw, in_off,
                                0 if in_ch is None else in_ch)
    if in_ch is not None:
        x = x[:, in_off:in_off + in_ch]
    if weight.shape[1] > x.shape[1]:
        # caller passed a channel-padded weight but the GPU path declined
        # (VFA_NO_CONV, forced torch ops, ...): slice the zero pad back off
        weight = weight[:, :x.shape[1]]
    if pt != pb or pl != pr:
        x = torch.nn.functional.pad(x, (pl, pr, pt, pb))
        pt = pl = 0
        y = torch.nn.functional.conv2d(x, weight, bias, (sh, sw), 0,
                                       (dh, dw))
    else:
        y = torch.nn.functional.conv2d(x, weight, bias, (sh, sw), (pt, pl),
                                       (dh, dw))
    if res is not None:
        y = y + res
    return _store_slice(out, out_off, _apply_act(y, act))


def conv2d_mod(conv: torch.nn.Module, x: torch.Tensor, act: str = 'none',
               res: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, out_off: int = 0,
               in_off: Optional[int] = None) -> torch.Tensor:
    """Route an ``nn.Conv2d`` module call through ``conv2d_act`` (which
    sends an unpadded 1x1 to the fused MFMA GEMM and everything else,
    dilation included, to the implicit-GEMM conv), with the weight padding
    its kernels need cached on the module; the module's own forward
    otherwise (CPU, groups, other dtypes or layouts).

    ``out`` / ``out_off``: write the result into channels
    [out_off, out_off + K_out) of the wider buffer ``out`` and return it.

    ``in_off``: ``x`` is a wide buffer and the conv reads
    ``conv.in_channels`` channels starting at ``in_off``.  On the kernel
    path the slice width is ``conv.in_channels`` rounded up to a multiple
    of 8 and the cached weight is zero-padded to that width, so the
    channels the rounding adds must exist in the buffer and be finite: the
    zero weight columns cancel them.  ``out`` may be ``x`` when the read
    and written slices are disjoint."""
    w = conv.weight
    sliced = in_off is not None
    c = conv.in_channels if sliced else x.shape[1]
    c8 = (c + 7) // 8 * 8
    eligible = (native_ready(x, knob='VFA_NO_CONV', channels_last=True)
                and w.dtype == torch.bfloat16 and conv.groups == 1)
    if eligible and sliced:
        _slice_width('conv2d_mod', x, in_off, c8, aligned=True)
    kw_slice = dict(in_off=in_off, in_ch=c8) if sliced else {}

    def padded(cpad, npad):
        return torch.nn.functional.pad(
            w, (0, 0, 0, 0, 0, cpad, 0, npad)).contiguous(
                memory_format=torch.channels_last)

    if eligible and w.shape[0] < 16 and res is None:
        # tiny-N heads (RAFT flow head N=2, per GRU iteration): pad the
        # OUTPUT channels to 16 (cached), run in-tree, slice back.  A slice
        # input also gets its input channels padded to the slice width.
        kout = w.shape[0]
        cpad = c8 - c if sliced else 0
        wp, bp = derived(conv, '_vfa_wnpad', (w, conv.bias), lambda: (
            padded(cpad, 16 - kout),
            torch.nn.functional.pad(conv.bias, (0, 16 - kout))
            if conv.bias is not None else None), cpad)
        y = conv2d_act(x, wp, bp, conv.stride, conv.padding, act,
                       dilation=conv.dilation, **kw_slice)[:, :kout]
        if out is None:
            return y.contiguous(memory_format=torch.channels_last)
        return _store_slice(out, out_off, y)
    if eligible:
        # stems (C=3/2/1) and the RAFT corr input (C=324): the weight's
        # channel dim is zero-padded once and cached; the input is padded
        # inside the conv's (fused) pad pass, or, as a slice, read in place
        # at the padded width
        wp = w if c % 8 == 0 else derived(
            conv, '_vfa_wpad', (w,), lambda: padded(c8 - c, 0))
        return conv2d_act(x, wp, conv.bias, conv.stride, conv.padding, act,
                          res, out, out_off, conv.dilation, **kw_slice)
    y = conv(x[:, in_off:in_off + c] if sliced else x)
    if res is not None:
        y = y + res
    return _store_slice(out, out_off, _apply_act(y, act))


# ------------------------------------------------- transposed convolution
def _pack_tconv_weight(w: torch.Tensor, c8: int) -> torch.Tensor:
    """(C, K_out, 4, 4) transposed-conv weight -> the (16*K_out, c8) matrix
    of the P-form GEMM: row (ky*4 + kx)*K_out + ko holds W[:, ko, ky, kx],
    zero columns for the channels c8 adds."""
    c, kout, kh, kw = w.shape
    if (kh, kw) != (4, 4) or c8 < c:
        raise ValueError(f'_pack_tconv_weight: weight {tuple(w.shape)}, '
                         f'c8={c8}')
    wp = w.permute(2, 3, 1, 0).reshape(16 * kout, c)
    if c8 > c:
        wp = torch.nn.functional.pad(wp, (0, c8 - c))
    return wp.contiguous()


def _conv_transpose2d_pform(x: torch.Tensor, w: torch.Tensor,
                            bias: Optional[torch.Tensor] = None
                            ) -> torch.Tensor:
    """Pure-torch P-form of the 4x4 / stride 2 / padding 1 transposed conv,
    with the index arithmetic of the kernels (tconv.hip): the partials
    P[pixel, (ky, kx, ko)] = x[pixel, :] @ Wp^T, then the col2im gather in
    which output row oy takes tap ky = (oy + 1) % 2 from input row
    (oy + 1 - ky) / 2 and tap ky + 2 from the row above it."""
    b, c, h, wd = x.shape
    kout = w.shape[1]
    wp = _pack_tconv_weight(w, c)
    p = (x.permute(0, 2, 3, 1).reshape(-1, c) @ wp.t()).reshape(
        b, h, wd, 4, 4, kout)
    out = x.new_zeros(b, 2 * h, 2 * wd, kout)
    oy = torch.arange(2 * h)
    ox = torch.arange(2 * wd)
    ky0, kx0 = (oy + 1) % 2, (ox + 1) % 2
    iy0, ix0 = (oy + 1 - ky0) // 2, (ox + 1 - kx0) // 2
    for ty in (0, 1):
        iy, ky = iy0 - ty, ky0 + 2 * ty
        vy = (iy >= 0) & (iy < h)
        for tx in (0, 1):
            ix, kx = ix0 - tx, kx0 + 2 * tx
            vx = (ix >= 0) & (ix < wd)
            g = p[:, iy.clamp(0, h - 1)[:, None], ix.clamp(0, wd - 1)[None],
                  ky[:, None], kx[None]]               # (B, 2H, 2W, K_out)
            out += g * (vy[:, None] & vx[None])[None, :, :, None].to(g.dtype)
    if bias is not None:
        out = out + bias
    return out.permute(0, 3, 1, 2)


def _tconv_kernel_ok(x: torch.Tensor, weight: torch.Tensor, stride, padding
                     ) -> bool:
    """The geometry, dtype and device tconv.hip covers (layout aside)."""
    st = (stride, stride) if isinstance(stride, int) else tuple(stride)
    pd = (padding, padding) if isinstance(padding, int) else tuple(padding)
    return (native_ready(x, knob='VFA_NO_TCONV') and x.dim() == 4
            and weight.dtype == torch.bfloat16 and weight.dim() == 4
            and tuple(weight.shape[2:]) == (4, 4) and weight.shape[1] <= 2
            and st == (2, 2) and pd == (1, 1))


def _tconv_check_out(x: torch.Tensor, out: Optional[torch.Tensor],
                     name: str) -> None:
    if out is not None and (out.untyped_storage().data_ptr()
                            == x.untyped_storage().data_ptr()):
        raise ValueError(f'{name}: out must not share storage with x')


def _tconv_out_direct(out: Optional[torch.Tensor]) -> bool:
    """Whether the kernels can store into ``out`` themselves."""
    return out is None or (
        out.is_cuda and out.dtype == torch.bfloat16 and out.dim() == 4
        and out.is_contiguous(memory_format=torch.channels_last))


# widest input slice whose packed weight (32 rows) fits the 64 KiB of LDS
_TCONV_MAX_C = 992


def _tconv_kernels(x: torch.Tensor, weight: torch.Tensor,
                   bias: Optional[torch.Tensor],
                   out: Optional[torch.Tensor], out_off: int, in_off: int,
                   in_ch: Optional[int], packed) -> Optional[torch.Tensor]:
    """The tconv.hip route of a call whose geometry, dtype, device and
    ``out`` the kernels cover: the direct kernel for an unsliced ``x`` of
    C <= 16, the P-form for a channels_last ``x`` whose slice sits on
    multiples of 8, with ``packed(width)`` the packed weight; None when the
    layout fits neither."""
    cx = x.shape[1] if in_ch is None else in_ch
    if in_ch is None and cx <= 16:
        return _ext.conv_transpose2d_small(x, weight.contiguous(), bias, out,
                                           out_off)
    if (x.is_contiguous(memory_format=torch.channels_last)
            and cx % 8 == 0 and in_off % 8 == 0 and x.shape[1] % 8 == 0
            and cx <= _TCONV_MAX_C):
        return _ext.conv_transpose2d_nhwc(x, packed(cx), bias, out, out_off,
                                          in_off, 0 if in_ch is None else in_ch)
    return None


def conv_transpose2d_act(x: torch.Tensor, weight: torch.Tensor,
                         bias: Optional[torch.Tensor] = None,
                         stride=2, padding=1,
                         out: Optional[torch.Tensor] = None,
                         out_off: int = 0, in_off: int = 0,
                         in_ch: Optional[int] = None) -> torch.Tensor:
    """Transposed convolution, ``weight`` (C_in, K_out, KH, KW).

    GPU kernel path (tconv.hip): kernel 4x4, stride 2, padding 1 (no
    output_padding, dilation 1, groups 1), K_out <= 2, bf16 in and out with
    f32 accumulation and one rounding.  Channels_last ``x`` with
    C % 8 == 0 runs the P-form (an MFMA GEMM to f32 partials, then a col2im
    gather); any unsliced ``x`` with C <= 16, NCHW or channels_last, runs
    the direct kernel.  Everything else -- the CPU, other dtypes, other
    geometry, other layouts -- is the ``F.conv_transpose2d`` composition:
    slice, call, assign into ``out[:, out_off:...]``.

    ``in_ch`` makes ``x`` a wider buffer of which channels
    [in_off, in_off + in_ch) are read, in place on the kernel path (in_off,
    in_ch and the buffer width multiples of 8).  ``out`` / ``out_off`` write
    channels [out_off, out_off + K_out) of a wider buffer and nothing else
    (out_off may be odd); ``out`` must not share storage with ``x``
    (ValueError).  Without ``out`` the kernel path returns a new
    channels_last (B, K_out, 2H, 2W) tensor.  ``VFA_NO_TCONV=1`` forces
    the composition."""
    cx = _slice_width('conv_transpose2d_act', x, in_off, in_ch)
    _tconv_check_out(x, out, 'conv_transpose2d_act')
    if (weight.shape[0] == cx and _tconv_out_direct(out)
            and _tconv_kernel_ok(x, weight, stride, padding)):
        y = _tconv_kernels(x, weight, bias, out, out_off, in_off, in_ch,
                           lambda c: _pack_tconv_weight(weight, c))
        if y is not None:
            return y
    if in_ch is not None:
        x = x[:, in_off:in_off + in_ch]
    y = torch.nn.functional.conv_transpose2d(x, weight, bias, stride, padding)
    return _store_slice(out, out_off, y)


def conv_transpose2d_mod(m: torch.nn.Module, x: torch.Tensor,
                         out: Optional[torch.Tensor] = None,
                         out_off: int = 0,
                         in_off: Optional[int] = None) -> torch.Tensor:
    """Route an ``nn.ConvTranspose2d`` call through tconv.hip (see
    ``conv_transpose2d_act`` for the geometry the kernels cover); the
    module's own forward otherwise.

    ``in_off``: ``x`` is a wide buffer and the conv reads ``m.in_channels``
    channels starting at ``in_off``.  On the kernel path the slice width is
    ``m.in_channels`` rounded up to a multiple of 8 and the packed weight
    (cached on the module, keyed on the weight's version, dtype, device and
    pointer) has zero rows for the channels the rounding adds -- the
    contract of ``conv2d_mod``: those channels must exist in the buffer and
    be finite."""
    w = m.weight
    sliced = in_off is not None
    c = m.in_channels if sliced else x.shape[1]
    c8 = (c + 7) // 8 * 8
    _tconv_check_out(x, out, 'conv_transpose2d_mod')
    eligible = (m.groups == 1 and tuple(m.dilation) == (1, 1)
                and tuple(m.output_padding) == (0, 0)
                and c == m.in_channels and _tconv_out_direct(out)
                and _tconv_kernel_ok(x, w, m.stride, m.padding))
    if eligible:
        if (sliced and c8 <= _TCONV_MAX_C
                and x.is_contiguous(memory_format=torch.channels_last)):
            _slice_width('conv_transpose2d_mod', x, in_off, c8, aligned=True)

        def packed(width):
            return derived(m, '_vfa_tconv_wp', (w,),
                           lambda: _pack_tconv_weight(w, width), width)

        y = _tconv_kernels(x, w, m.bias, out, out_off,
                           in_off if sliced else 0, c8 if sliced else None,
                           packed)
        if y is not None:
            return y
    y = m(x[:, in_off:in_off + c] if sliced else x)
    return _store_slice(out, out_off, y)


def grid_sample_bilinear(x: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """RAFT-style bilinear lookup: ``coords`` (B, Ho, Wo, 2) in *pixel* units,
    zero padding outside (reference models/raft/raft_src/utils/utils.py:57-71)."""
    if _use_hip(x):
        return _ext.grid_sample_bilinear(x.contiguous(), coords.contiguous())
    h, w = x.shape[-2:]
    gx = coords[..., 0] / max(w - 1, 1) * 2 - 1
    gy = coords[..., 1] / max(h - 1, 1) * 2 - 1
    grid = torch.stack([gx, gy], dim=-1)
    return torch.nn.functional.grid_sample(x, grid, mode='bilinear',
                                           padding_mode='zeros',
                                           align_corners=True)
