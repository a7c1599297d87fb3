#!/usr/bin/env python3
"""Microbench: ops.linear_act (fused MFMA GEMM) vs torch F.linear(+act)
on the CLIP / VGGish / RAFT shapes.  Run on a GPU box.

A row may carry a sixth field, the mode:
  res        linear_act with a residual operand (torch: F.linear + add)
  res_stats  ops.linear_res_stats: residual + per-row LayerNorm statistics
             (torch: F.linear + add, no statistics)
  ln_act     ops.linear_ln_act on un-normalised rows with a folded weight
             (torch: F.linear on the already normalised rows)
After the rows come the LayerNorm-fold chains (CHAINS): what a ViT block
runs today against the folded pair, each chain replayed from one graph, and
ops.instance_norm alone at the calls of RAFT's feature net (VFA_GEMM_ONLY=
instance_norm selects them).

VFA_GEMM_GRAPH=1 times every row from a captured graph (kernel time without
launch gaps); the chains always do."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))

import torch

from video_features_amd import ops

assert torch.cuda.is_available()
dev = torch.device('cuda:0')

SHAPES = [
    # (M, N, K, act, label)
    (9600, 3072, 768, 'quick_gelu', 'CLIP fc1 (fb192)'),
    (9600, 768, 3072, 'none', 'CLIP fc2'),
    (9600, 2304, 768, 'none', 'CLIP qkv'),
    (9600, 768, 768, 'none', 'CLIP proj'),
    (38400, 3072, 768, 'quick_gelu', 'CLIP fc1 (fb768)'),
    (4096, 4096, 12288, 'relu', 'VGGish fc1'),
    (200704, 256, 1920, 'none', 'RAFT GRU-zr-as-GEMM'),
    (4096, 4096, 4096, 'none', 'ladder 4096^3'),
    (8192, 8192, 8192, 'none', 'ladder 8192^3'),
    (19200, 3072, 768, 'quick_gelu', 'CLIP fc1 (fb384)'),
    (19200, 2304, 768, 'none', 'CLIP qkv (fb384)'),
    # fc1's shape without the activation: the difference to the fc1 row is
    # the cost of the fused QuickGELU epilogue
    (19200, 3072, 768, 'none', 'CLIP fc1-noact (fb384)'),
    (19200, 768, 768, 'none', 'CLIP proj (fb384)'),
    (19200, 768, 768, 'none', 'CLIP proj+res (fb384)', 'res'),
    (19200, 768, 3072, 'none', 'CLIP fc2 (fb384)'),
    (19200, 768, 3072, 'none', 'CLIP fc2+res (fb384)', 'res'),
    (19200, 768, 768, 'none', 'CLIP proj res_stats (fb384)', 'res_stats'),
    (19200, 768, 3072, 'none', 'CLIP fc2 res_stats (fb384)', 'res_stats'),
    (19200, 3072, 768, 'quick_gelu', 'CLIP fc1 ln_act (fb384)', 'ln_act'),
    (19200, 2304, 768, 'none', 'CLIP qkv ln_act (fb384)', 'ln_act'),
    (1204224, 64, 64, 'relu', 'rn50 l1 conv1 (thin)'),
    (1204224, 256, 64, 'relu', 'rn50 l1 conv3 (thin)'),
    (1204224, 128, 256, 'relu', 'rn50 l2 conv1 (thin)'),
    (301056, 512, 128, 'relu', 'rn50 l2 conv3 (thin)'),
    (301056, 256, 512, 'relu', 'rn50 l3 conv1 (not thin)'),
]


def timeit(fn, iters=50):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def timeit_graph(fn, iters=50):
    """Per-call time of fn replayed from a captured graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        g.replay()
    torch.cuda.synchronize()
    del keep
    return (time.perf_counter() - t0) / iters


# VFA_GEMM_ONLY=substring: run only the rows whose label contains it
ONLY = os.environ.get('VFA_GEMM_ONLY', '')
GRAPH = os.environ.get('VFA_GEMM_GRAPH', '') not in ('', '0')
HAVE_FOLD = hasattr(ops, 'linear_res_stats')
EPS = 1e-5

for row in SHAPES:
    m, n, k, act, label = row[:5]
    mode = row[5] if len(row) > 5 else 'plain'
    if ONLY and ONLY not in label:
        continue
    if mode in ('res_stats', 'ln_act') and not HAVE_FOLD:
        continue
    torch.manual_seed(0)
    # VFA_GEMM_COLD=N: rotate N input buffers so A can't stay resident in
    # the 256 MiB Infinity Cache between iterations (in-model conditions —
    # cdna_hip_programming.md §2 L3 over-fetch masking); default 1 = warm
    ncold = max(1, int(os.environ.get('VFA_GEMM_COLD', '1')))
    xs = [(torch.randn(m, k, device=dev) / (k ** 0.25)).to(torch.bfloat16)
          for _ in range(ncold)]
    x = xs[0]
    w = (torch.randn(n, k, device=dev) / (k ** 0.25)).to(torch.bfloat16)
    b = torch.randn(n, device=dev).to(torch.bfloat16)
    it = [0]
    res = (torch.randn(m, n, device=dev).to(torch.bfloat16)
           if mode in ('res', 'res_stats') else None)
    if mode == 'ln_act':
        # xs are the un-normalised rows; torch gets them normalised
        g = torch.randn(k, device=dev).to(torch.bfloat16)
        be = torch.randn(k, device=dev).to(torch.bfloat16)
        fold = ops.fold_ln_linear(w, b, g, be)
        xf = [xi.float() for xi in xs]
        sts = [torch.stack([xi.mean(1), xi.var(1, unbiased=False) * k], 1)
               .unsqueeze(1).contiguous() for xi in xf]
        ys = [torch.nn.functional.layer_norm(xi, (k,), g.float(), be.float(),
                                             EPS).to(torch.bfloat16)
              for xi in xf]
        del xf

    def torch_path():
        it[0] += 1
        src = ys if mode == 'ln_act' else xs
        y = torch.nn.functional.linear(src[it[0] % ncold], w, b)
        if res is not None:
            y = y + res
        if act == 'relu':
            y = y.relu()
        elif act == 'quick_gelu':
            y = y * torch.sigmoid(1.702 * y)
        return y

    def ours():
        it[0] += 1
        i = it[0] % ncold
        if mode == 'res_stats':
            return ops.linear_res_stats(xs[i], w, b, res)[0]
        if mode == 'ln_act':
            return ops.linear_ln_act(xs[i], sts[i], *fold, act, EPS)
        return ops.linear_act(xs[i], w, b, act, res=res)

    flops = 2.0 * m * n * k
    timer = timeit_graph if GRAPH else timeit
    tt = timer(torch_path)
    to = timer(ours)
    # correctness spot-check (same buffer both paths)
    it[0] = -1
    ref_t = torch.nn.functional.linear(ys[0] if mode == 'ln_act' else x, w, b)
    if res is not None:
        ref_t = ref_t + res
    if act == 'relu':
        ref_t = ref_t.relu()
    elif act == 'quick_gelu':
        ref_t = ref_t * torch.sigmoid(1.702 * ref_t)
    d = (ours().float() - ref_t.float()).abs().max().item()
    ref = ref_t.float().abs().max().item()
    print(f'{label:<24} M{m:>7} N{n:>5} K{k:>6} {act:<11} '
          f'torch {tt * 1e6:7.1f}us ({flops / tt / 1e12:6.1f} TF) | '
          f'ours {to * 1e6:7.1f}us ({flops / to / 1e12:6.1f} TF) | '
          f'x{tt / to:4.2f} relerr {d / ref:.2e}', flush=True)


# ------------------------------------------------------- LayerNorm-fold chains
# (label, M, width, K1, N2, act2, route of GEMM 2 today): GEMM 1 (M, width,
# K1) feeds the residual stream, whose LayerNorm feeds GEMM 2 (M, N2, width).
CHAINS = [
    ('ln_2 half: proj -> ln_2 -> fc1+QuickGELU (fb384)',
     19200, 768, 768, 3072, 'quick_gelu', 'in-tree'),
    ('ln_1 half: fc2 -> ln_1 -> qkv (fb384)',
     19200, 768, 3072, 2304, 'none', 'hipBLASLt'),
]

for label, m, wd, k1, n2, act2, gemm2 in CHAINS:
    if ONLY and ONLY not in label:
        continue
    torch.manual_seed(0)
    x = (torch.randn(m, k1, device=dev) / (k1 ** 0.25)).to(torch.bfloat16)
    res = torch.randn(m, wd, device=dev).to(torch.bfloat16)
    w1 = (torch.randn(wd, k1, device=dev) / (k1 ** 0.25)).to(torch.bfloat16)
    b1 = torch.randn(wd, device=dev).to(torch.bfloat16)
    w2 = (torch.randn(n2, wd, device=dev) / (wd ** 0.25)).to(torch.bfloat16)
    b2 = torch.randn(n2, device=dev).to(torch.bfloat16)
    g = torch.randn(wd, device=dev).to(torch.bfloat16)
    be = torch.randn(wd, device=dev).to(torch.bfloat16)

    def today():
        d = torch.nn.functional.linear(x, w1, b1)
        y, s = ops.layer_norm_residual(d, res, g, be, EPS)
        if gemm2 == 'in-tree':
            return ops.linear_act(y, w2, b2, act2), s
        return torch.nn.functional.linear(y, w2, b2), s

    def parts():
        return [
            ('GEMM 1 hipBLASLt',
             lambda: torch.nn.functional.linear(x, w1, b1)),
            ('layer_norm_residual',
             lambda d=torch.nn.functional.linear(x, w1, b1):
             ops.layer_norm_residual(d, res, g, be, EPS)),
        ]

    runs = [timeit_graph(today) * 1e6 for _ in range(3)]
    print(f'{label}\n  today  (hipBLASLt + layer_norm_residual + {gemm2}): '
          + ' '.join(f'{t:7.1f}' for t in runs) + ' us', flush=True)
    for name, fn in parts():
        print(f'    {name:<22} {timeit_graph(fn) * 1e6:7.1f} us', flush=True)
    if not HAVE_FOLD:
        continue
    fold = ops.fold_ln_linear(w2, b2, g, be)

    def folded():
        s, st = ops.linear_res_stats(x, w1, b1, res)
        return ops.linear_ln_act(s, st, *fold, act2, EPS), s

    runs = [timeit_graph(folded) * 1e6 for _ in range(3)]
    print('  folded (linear_res_stats + linear_ln_act):            '
          + ' '.join(f'{t:7.1f}' for t in runs) + ' us', flush=True)
    s, st = ops.linear_res_stats(x, w1, b1, res)
    for name, fn in [
            ('linear_res_stats', lambda: ops.linear_res_stats(x, w1, b1, res)),
            ('linear_ln_act', lambda: ops.linear_ln_act(s, st, *fold, act2,
                                                        EPS))]:
        print(f'    {name:<22} {timeit_graph(fn) * 1e6:7.1f} us', flush=True)
    d = (folded()[0].float() - today()[0].float()).abs().max().item()
    print(f'    max |folded - today| {d:.3e}', flush=True)


# ------------------------------------------------------------- InstanceNorm
# ops.instance_norm alone, replayed from a graph like the chains, at the
# shapes, layout and ReLU flags with which the RAFT feature net calls it in
# ``bench.py --model i3d_raft`` (16 clips x 64 frame pairs, both images in
# one batch: 2048 frames of 224 x 224, bf16 channels_last).  The calls are
# read off the model with forward hooks on a 2-frame batch and printed once.
# Two inputs per shape: planes with mean 0, whose variance the kernel takes
# from sumsq/n - mean^2, and planes with mean 2 sigma, which it sweeps once
# more for the variance about the mean.  VFA_NORM_FRAMES overrides the 2048.
def fnet_norm_calls():
    """{(C, H, W, nhwc, relu): count} of one feature-net forward."""
    from video_features_amd.models.raft import (BasicEncoder,
                                                FusedInstanceNorm2d)
    cl = torch.channels_last
    net = BasicEncoder(256, 'instance').to(dev, torch.bfloat16) \
        .to(memory_format=cl).eval()
    calls = {}

    def hook(mod, inp, out):
        x = inp[0]
        key = (*x.shape[1:], not x.is_contiguous(), mod.fuses_relu)
        calls[key] = calls.get(key, 0) + 1
    for mod in net.modules():
        if isinstance(mod, FusedInstanceNorm2d):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        net(torch.randn(2, 3, 224, 224, device=dev).to(torch.bfloat16)
            .contiguous(memory_format=cl))
    return calls


if not ONLY or ONLY in 'instance_norm':
    frames = int(os.environ.get('VFA_NORM_FRAMES', '2048'))
    for (c, h, w, nhwc, relu), count in fnet_norm_calls().items():
        label = (f'instance_norm ({frames}, {c}, {h}, {w}) '
                 f'{"nhwc" if nhwc else "nchw"} relu={int(relu)} '
                 f'x{count} per forward')
        torch.manual_seed(0)
        x = torch.randn(frames, c, h, w, device=dev).to(torch.bfloat16)
        if nhwc:
            x = x.contiguous(memory_format=torch.channels_last)
        for name, xin in (('mean 0', x), ('mean 2 sigma', x + 2)):
            runs = [timeit_graph(lambda: ops.instance_norm(
                xin, relu=relu, nhwc=nhwc), iters=20) * 1e6 for _ in range(3)]
            print(f'{label}, {name}: '
                  + ' '.join(f'{t:8.1f}' for t in runs) + ' us', flush=True)
        del x, xin
