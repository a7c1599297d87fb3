#!/usr/bin/env python3
"""Microbench: RAFT's two correlation forms — the all-pairs pyramid
(CorrPyramid + ops.corr_lookup) and the on-the-fly lookup (CorrOnTheFly +
ops.corr_lookup_otf) — at 1/8-resolution shapes from a 224^2 crop to a 1080p
frame, B = 1, D = 256.  Run on a GPU box.

Per shape and form: time to build the object, time of 20 lookups (one RAFT
forward's worth), their sum, and the peak device memory of build + lookups.
The two forms alternate within each repetition; the table shows the median
and the spread (min..max) of the sums.  For the on-the-fly form it also
prints the cache bandwidth its lookups imply: a lookup reads
HW * 400 * D * 4 bytes of f2 (100 grid points x 4 levels per query pixel).

  --shapes 28x28,46x80    1/8-resolution H8xW8 list
  --reps N                repetitions per shape (default 5)
  --f32                   f32 contiguous output (default: bf16 channels_last,
                          what the bf16 RAFT forward asks for)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))

import torch

from video_features_amd.models.raft import CorrOnTheFly, CorrPyramid

LOOKUPS = 20


def one_run(cls, fmap1, fmap2, coords, nhwc, dtype):
    """(build ms, lookups ms, peak bytes) of one build + LOOKUPS lookups."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    fn = cls(fmap1, fmap2)
    ev[1].record()
    for c in coords:
        out = fn(c, nhwc=nhwc, out_dtype=dtype)
    ev[2].record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del fn, out
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='28x28,46x80,90x160,135x240')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--f32', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_corr needs a GPU'
    dev = torch.device('cuda:0')
    nhwc, dtype = (False, torch.float32) if args.f32 else \
        (True, torch.bfloat16)
    d = 256
    forms = (('allpairs', CorrPyramid), ('onthefly', CorrOnTheFly))
    for shape in args.shapes.split(','):
        h, w = (int(v) for v in shape.split('x'))
        torch.manual_seed(0)
        fmap1 = torch.randn(1, d, h, w, device=dev)
        fmap2 = torch.randn(1, d, h, w, device=dev)
        yy, xx = torch.meshgrid(torch.arange(h, device=dev).float(),
                                torch.arange(w, device=dev).float(),
                                indexing='ij')
        grid = torch.stack([xx, yy])[None]
        # a different smooth-ish flow of a few pixels per lookup
        coords = [(grid + 4 * torch.randn(1, 2, 1, 1, device=dev)
                   + torch.randn(1, 2, h, w, device=dev)).contiguous()
                  for _ in range(LOOKUPS)]
        runs = {name: [] for name, _ in forms}
        for rep in range(args.reps + 1):
            for name, cls in forms:
                r = one_run(cls, fmap1, fmap2, coords, nhwc, dtype)
                if rep:                      # repetition 0 warms up
                    runs[name].append(r)
        for name, _ in forms:
            tot = sorted(r[0] + r[1] for r in runs[name])
            med = sorted(runs[name], key=lambda r: r[0] + r[1])[len(tot) // 2]
            row = {'shape': shape, 'hw': h * w, 'form': name,
                   'build_ms': round(med[0], 3),
                   'lookups_ms': round(med[1], 3),
                   'total_ms': round(med[0] + med[1], 3),
                   'total_min_ms': round(tot[0], 3),
                   'total_max_ms': round(tot[-1], 3),
                   'peak_mb': round(max(r[2] for r in runs[name]) / 1e6, 1)}
            if name == 'onthefly':
                nbytes = h * w * 400 * d * 4
                row['read_gb_per_lookup'] = round(nbytes / 1e9, 3)
                row['implied_tb_s'] = round(
                    nbytes * LOOKUPS / (med[1] * 1e-3) / 1e12, 2)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
