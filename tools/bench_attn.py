#!/usr/bin/env python3
"""Microbench: the attention and patch-gather kernels of the CLIP ViT chunk
(384 frames of ViT-B/32), each replayed from a captured graph and set against
the bytes it has to move.  Run on a GPU box.

Rows:
  mhsa_fused      ops.mhsa_fused at (384, 50, 2304), 12 heads
  attention_pool  ops.attention_pool at (384, 12 heads, L = 50)
  patch gather    (384, 3, 224, 224) -> (384, 49, 3072), p = 32

Each row prints three runs: time per call, the bytes of one call (inputs read
once + outputs written once) and the TB/s that gives.

VFA_ATTN_BUFS=N   capture N calls on N different input buffers per graph and
                  report the mean (default 1: inputs stay resident in the
                  256 MiB Infinity Cache; 4 rotates about 0.5 GB through it,
                  closer to what the kernel meets inside the model)
VFA_ATTN_ONLY=s   run only the rows whose label contains s
VFA_ATTN_FRAMES=n frames per call (default 384)
Builds without ops.patchify time the reshape / permute copy for that row."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))

import torch

from video_features_amd import ops

assert torch.cuda.is_available()
dev = torch.device('cuda:0')

NBUF = max(1, int(os.environ.get('VFA_ATTN_BUFS', '1')))
ONLY = os.environ.get('VFA_ATTN_ONLY', '')
T = int(os.environ.get('VFA_ATTN_FRAMES', '384'))
HEADS, L, W, P, RES = 12, 50, 768, 32, 224


def timeit_graph(fns, iters=1000):
    """Mean per-call time of the calls in fns, replayed from one graph (the
    calls take tens of microseconds: 1000 replays make a window of tens of
    milliseconds or more)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            for fn in fns:
                fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for fn in fns]
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        g.replay()
    torch.cuda.synchronize()
    del keep
    return (time.perf_counter() - t0) / iters / len(fns)


def torch_gather(x, p):
    t, c, h, w = x.shape
    g = h // p
    xp = x.reshape(t, c, g, p, g, p).permute(0, 2, 4, 1, 3, 5)
    return xp.reshape(t, g * g, c * p * p)


def rows():
    torch.manual_seed(0)
    bf = torch.bfloat16
    qkv = [torch.randn(T, L, 3 * W, device=dev).to(bf) for _ in range(NBUF)]
    yield ('mhsa_fused (%d, %d, %d)' % (T, L, 3 * W),
           [lambda x=x: ops.mhsa_fused(x, HEADS) for x in qkv],
           T * L * 4 * W * 2)
    # further kernels of the same op, where the build has them
    for v in getattr(ops, 'MHSA_VARIANTS', ())[1:]:
        yield ('mhsa_fused variant=%d' % v,
               [lambda x=x, v=v: ops.mhsa_fused(x, HEADS, variant=v)
                for x in qkv],
               T * L * 4 * W * 2)
    del qkv
    q = [torch.randn(T, W, device=dev).to(bf) for _ in range(NBUF)]
    kv = [torch.randn(T, L, 2 * W, device=dev).to(bf) for _ in range(NBUF)]
    yield ('attention_pool (%d, %d heads, L=%d)' % (T, HEADS, L),
           [lambda a=a, b=b: ops.attention_pool(a, b, HEADS)
            for a, b in zip(q, kv)],
           (T * L * 2 * W + 2 * T * W) * 2)
    del q, kv
    x = [torch.randn(T, 3, RES, RES, device=dev).to(bf) for _ in range(NBUF)]
    if hasattr(ops, 'patchify'):
        fns = [lambda a=a: ops.patchify(a, P) for a in x]
        ref = torch_gather(x[0], P)
        assert torch.equal(fns[0](), ref)
        name = 'patch gather, ops.patchify'
    else:
        fns = [lambda a=a: torch_gather(a, P) for a in x]
        name = 'patch gather, torch copy'
    yield (name + ' (%d, 3, %d, %d) p=%d' % (T, RES, RES, P), fns,
           2 * T * 3 * RES * RES * 2)
    if hasattr(ops, 'patchify'):
        yield ('patch gather, torch copy',
               [lambda a=a: torch_gather(a, P) for a in x],
               2 * T * 3 * RES * RES * 2)


print(f'frames {T}, buffers per graph {NBUF}', flush=True)
for label, fns, nbytes in rows():
    if ONLY and ONLY not in label:
        continue
    runs = [timeit_graph(fns) for _ in range(3)]
    print(f'{label:<48} '
          + ' '.join(f'{t * 1e6:7.1f}' for t in runs) + ' us | '
          f'{nbytes / 1e6:6.1f} MB | '
          + ' '.join(f'{nbytes / t / 1e12:5.2f}' for t in runs) + ' TB/s',
          flush=True)
