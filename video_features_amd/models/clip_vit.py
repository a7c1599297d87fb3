"""Native CLIP image encoder (ViT-B/32 and ViT-B/16).

The reference imports OpenAI's ``clip`` pip package (reference
models/CLIP/extract_clip.py:46-63); this is a from-scratch implementation of
the same architecture: patch-embed conv → [CLS] + learned positional
embeddings → pre-LN transformer (MHSA + QuickGELU MLP) → final LN → linear
projection to the 512-d joint space.

Hot ops (LayerNorm, QuickGELU, the attention core) dispatch through
``video_features_amd.ops`` — hand-written CDNA4 HIP kernels on MI355X,
PyTorch reference implementations on CPU.  Plain GEMMs (qkv/proj/MLP) go to
rocBLAS/hipBLASLt via ``torch.nn.Linear``.

Only what the output needs is computed.  The [CLS] token, the positional
embedding and ``ln_pre`` are one kernel (``ops.clip_embed_ln``).  The feature
is ``ln_post`` of token 0 of the last block, so the last block runs ``ln_1``
and the K/V projection over all tokens and everything after them — query,
single-query attention (``ops.attention_pool``), ``proj``, ``ln_2``, the MLP
and the residual adds — for the [CLS] row of each frame only
(``VisionTransformer._cls_tail``).  ``VFA_CLIP_FULL_TAIL=1`` runs the last
block in full instead, for A/B runs and tests; the parameters and
``state_dict`` keys are the same either way.

``ln_2`` of the full blocks is not a pass over memory either: ``proj`` adds
the residual and emits row statistics partials in its GEMM epilogue
(``ops.linear_res_stats``) and fc1 runs on the un-normalised stream with the
``ln_2`` affine folded into its weight (``ops.linear_ln_act``).  The folded
weight is derived state, cached per block and rebuilt when a source
parameter changes; it is no parameter and no buffer.  ``VFA_NO_LNFOLD=1``
restores the ``layer_norm_residual`` pass, for A/B runs and tests.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops


@dataclass
class ViTConfig:
    input_resolution: int = 224
    patch_size: int = 32
    width: int = 768
    layers: int = 12
    heads: int = 12
    output_dim: int = 512


VIT_B32 = ViTConfig(patch_size=32)
VIT_B16 = ViTConfig(patch_size=16)


class LayerNorm(nn.LayerNorm):
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.layer_norm(x, self.weight, self.bias, self.eps)


class MultiheadSelfAttention(nn.Module):
    def __init__(self, width: int, heads: int):
        super().__init__()
        self.heads = heads
        self.head_dim = width // heads
        self.qkv = nn.Linear(width, 3 * width)
        self.proj = nn.Linear(width, width)

    def heads_out(self, x: torch.Tensor) -> torch.Tensor:
        """Attention up to, not including, the output projection."""
        return ops.mhsa_fused(self.qkv(x), self.heads)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(self.heads_out(x))


class MLP(nn.Module):
    def __init__(self, width: int):
        super().__init__()
        self.c_fc = nn.Linear(width, 4 * width)
        self.c_proj = nn.Linear(4 * width, width)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # fc1 + QuickGELU fused into one MFMA GEMM epilogue on GPU (the
        # persistent 256^2 kernel of gemm.hip: 766-793 TF vs 363 TF for
        # hipBLASLt + a separate activation pass at the 384-frame chunk
        # shape, profiles/clip_fc1_epilogue.md); fc2 stays on hipBLASLt,
        # which wins at K=3072 (919 vs 660 TF).  The full blocks of the
        # ViT do not come through here: their fc1 is the same kernel on the
        # un-normalised stream with ln_2 folded in
        # (ResidualAttentionBlock.attn_mlp_folded,
        # profiles/clip_ln_fold.md); this is the [CLS] tail's MLP, M = T
        h = ops.linear_act(x, self.c_fc.weight, self.c_fc.bias, 'quick_gelu')
        return self.c_proj(h)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, width: int, heads: int):
        super().__init__()
        self.ln_1 = LayerNorm(width)
        self.attn = MultiheadSelfAttention(width, heads)
        self.ln_2 = LayerNorm(width)
        self.mlp = MLP(width)
        self._fold = None           # (key, (W', c, b')) of ln_2 -> c_fc

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x + self.attn(self.ln_1(x))
        x = x + self.mlp(self.ln_2(x))
        return x

    def _ln2_fold(self):
        """``ops.fold_ln_linear`` of (``mlp.c_fc``, ``ln_2``), built on first
        use and again whenever one of the four parameters was written in
        place (``load_state_dict``, ``copy_``: ``_version``) or replaced
        (``.to()``: ``data_ptr`` / dtype / device)."""
        src = (self.mlp.c_fc.weight, self.mlp.c_fc.bias, self.ln_2.weight,
               self.ln_2.bias)
        return ops.derived(self, '_fold', src,
                           lambda: ops.fold_ln_linear(*src))

    def fold_routed(self, x: torch.Tensor) -> bool:
        """Whether ``attn_mlp_folded`` replaces the ``ln_2`` pass for a
        stream like ``x``: always on the CPU (the ops' torch compositions,
        same arithmetic as the pass), on the GPU when both GEMMs run their
        fused kernel — all full 256-row tiles, so not ViT-B/16's 197 tokens
        at most batch sizes."""
        if ops.env_flag('VFA_NO_LNFOLD'):
            return False
        return not x.is_cuda or (
            ops.fused_ln_tiles(x, self.attn.proj.weight)
            and ops.fused_ln_tiles(x, self.mlp.c_fc.weight))

    def attn_mlp_folded(self, y1: torch.Tensor, s1: torch.Tensor):
        """``ln_1`` output ``y1`` and stream ``s1`` → (MLP delta, stream
        ``s2 = s1 + attn``), with no ``ln_2`` pass: ``proj`` writes ``s2`` and
        its row statistics, fc1 + QuickGELU reads ``s2`` through the folded
        weight."""
        proj, fc, ln = self.attn.proj, self.mlp.c_fc, self.ln_2
        s2, st2 = ops.linear_res_stats(self.attn.heads_out(y1), proj.weight,
                                       proj.bias, s1)
        h = ops.linear_ln_act(
            s2, st2, *self._ln2_fold(), act='quick_gelu', eps=ln.eps,
            unfolded=(fc.weight, fc.bias, ln.weight, ln.bias))
        return self.mlp.c_proj(h), s2


class VisionTransformer(nn.Module):
    def __init__(self, cfg: ViTConfig = VIT_B32):
        super().__init__()
        self.cfg = cfg
        w = cfg.width
        self.conv1 = nn.Conv2d(3, w, kernel_size=cfg.patch_size,
                               stride=cfg.patch_size, bias=False)
        n_patches = (cfg.input_resolution // cfg.patch_size) ** 2
        scale = w ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(w))
        self.positional_embedding = nn.Parameter(
            scale * torch.randn(n_patches + 1, w))
        self.ln_pre = LayerNorm(w)
        self.blocks = nn.ModuleList(
            [ResidualAttentionBlock(w, cfg.heads) for _ in range(cfg.layers)])
        self.ln_post = LayerNorm(w)
        self.proj = nn.Parameter(scale * torch.randn(w, cfg.output_dim))

    def _patch_embed(self, x: torch.Tensor) -> torch.Tensor:
        """Patch embedding.  Stride==kernel conv IS a patch gather + GEMM; on
        GPU the gather is one ``ops.patchify`` pass and the GEMM goes to
        hipBLASLt directly instead of an im2col conv."""
        if x.is_cuda:
            xp = ops.patchify(x, self.cfg.patch_size)   # (T, P, 3*p*p)
            w = self.conv1.weight.reshape(self.cfg.width, -1)
            return xp @ w.t()                           # (T, P, W)
        x = self.conv1(x)                               # (T, W, R/p, R/p)
        return x.flatten(2).transpose(1, 2)             # (T, P, W)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(T, 3, R, R) preprocessed frames → (T, output_dim) features."""
        x = self._patch_embed(x)
        # [cls | patches] + positional embedding + ln_pre: one kernel on GPU
        x = ops.clip_embed_ln(x, self.class_embedding,
                              self.positional_embedding, self.ln_pre.weight,
                              self.ln_pre.bias, self.ln_pre.eps)
        full_tail = ops.env_flag('VFA_CLIP_FULL_TAIL')
        # residual stream carried as (delta, res): every add is fused into
        # the next LayerNorm (ops.layer_norm_residual)
        delta, res = None, x
        for blk in (self.blocks if full_tail else self.blocks[:-1]):
            if delta is None:
                y1, s1 = blk.ln_1(res), res
            else:
                y1, s1 = ops.layer_norm_residual(delta, res, blk.ln_1.weight,
                                                 blk.ln_1.bias, blk.ln_1.eps)
            if blk.fold_routed(s1):
                delta, res = blk.attn_mlp_folded(y1, s1)
                continue
            a = blk.attn(y1)
            y2, s2 = ops.layer_norm_residual(a, s1, blk.ln_2.weight,
                                             blk.ln_2.bias, blk.ln_2.eps)
            delta, res = blk.mlp(y2), s2
        if full_tail:
            x = delta + res
            x = self.ln_post(x[:, 0, :])
        else:
            x = self._cls_tail(self.blocks[-1], delta, res)
        return x @ self.proj.to(x.dtype)

    def _cls_tail(self, blk: ResidualAttentionBlock,
                  delta: Optional[torch.Tensor],
                  res: torch.Tensor) -> torch.Tensor:
        """Last block + ``ln_post`` for the [CLS] row alone.  Attention mixes
        tokens, so ``ln_1`` and the K/V projection still cover every token;
        the query, ``proj``, ``ln_2``, the MLP and the residual adds are
        needed for one row per frame.  The weight slices are row views of
        the block's own parameters."""
        w = self.cfg.width
        if delta is None:
            y1, s1 = blk.ln_1(res), res
        else:
            y1, s1 = ops.layer_norm_residual(delta, res, blk.ln_1.weight,
                                             blk.ln_1.bias, blk.ln_1.eps)
        qkv = blk.attn.qkv
        kv = F.linear(y1, qkv.weight[w:], qkv.bias[w:])      # (T, N, 2W)
        q = F.linear(y1[:, 0], qkv.weight[:w], qkv.bias[:w])  # (T, W)
        o = ops.attention_pool(q, kv, blk.attn.heads)        # (T, W)
        a = blk.attn.proj(o)
        y2, s2 = ops.layer_norm_residual(a, s1[:, 0], blk.ln_2.weight,
                                         blk.ln_2.bias, blk.ln_2.eps)
        d = blk.mlp(y2)                                      # M = T
        y, _ = ops.layer_norm_residual(d, s2, self.ln_post.weight,
                                       self.ln_post.bias, self.ln_post.eps)
        return y

    # reference parity name (reference extract_clip.py:128 uses
    # model.encode_image)
    def encode_image(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward(x)


def build_clip_vit(feature_type: str) -> VisionTransformer:
    if feature_type in ('CLIP-ViT-B/32', 'CLIP4CLIP-ViT-B-32'):
        return VisionTransformer(VIT_B32)
    if feature_type == 'CLIP-ViT-B/16':
        return VisionTransformer(VIT_B16)
    raise ValueError(f'unknown CLIP feature type {feature_type!r}')
