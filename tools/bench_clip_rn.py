#!/usr/bin/env python3
"""A/B bench of the CLIP ModifiedResNet tower: fused in-tree path vs the
eager composition (``VFA_NO_CLIPRN=1``: MIOpen NCHW convs, eager pools and
attention pool — the behaviour before the fused path existed).

Run on a GPU box:  python tools/bench_clip_rn.py [--iters 20] [--repeats 7]

Times ``encode_image`` in bf16 with BatchNorms folded, random weights and a
random NCHW batch (what the extractor hands the model):

- ``CLIP-RN50`` at batch 64, eager and fused, ``--rounds`` times alternating;
- ``CLIP-RN50x4`` at batch 32 and ``CLIP-RN50x16`` at batch 16, fused only
  (a run that is out of memory is repeated at half the batch, and says so).

Every configuration runs in a fresh child process under its own
``timeout -k 10``; the first child that exits abnormally ends the run.  A
child warms up, then times ``--repeats`` windows of ``--iters`` forwards with
device events and reports the median window as one JSON line.

``--child`` runs one configuration in-process (the form to put behind
``rocprofv3 --kernel-trace --stats --``).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

OOM_EXIT = 3


def child(args) -> int:
    import torch
    sys.path.insert(0, '.')
    from video_features_amd import ops
    from video_features_amd.models.clip_resnet import build_clip_resnet
    from video_features_amd.utils.fold_bn import fold_batchnorms
    assert torch.cuda.is_available(), 'bench_clip_rn needs a GPU'
    assert ops.hip_available(), 'HIP extension not built'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = build_clip_resnet(args.feature_type).eval()
    fold_batchnorms(model)
    model = model.to(dev, torch.bfloat16)
    res = model.input_resolution
    path = 'eager' if ops.env_flag('VFA_NO_CLIPRN') else 'fused'
    try:
        x = torch.randn(args.batch, 3, res, res, device=dev) \
            .to(torch.bfloat16)
        with torch.no_grad():
            for _ in range(args.warmup):
                out = model.encode_image(x)
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all()
            windows = []
            for _ in range(args.repeats):
                s = torch.cuda.Event(enable_timing=True)
                e = torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.iters):
                    model.encode_image(x)
                e.record()
                torch.cuda.synchronize()
                windows.append(s.elapsed_time(e) / args.iters)   # ms/forward
    except torch.cuda.OutOfMemoryError:
        print(json.dumps({'feature_type': args.feature_type, 'path': path,
                          'batch': args.batch, 'oom': True}), flush=True)
        return OOM_EXIT
    med = statistics.median(windows)
    print(json.dumps({
        'feature_type': args.feature_type, 'path': path,
        'batch': args.batch, 'resolution': res, 'dtype': 'bf16',
        'iters': args.iters, 'repeats': args.repeats,
        'ms_per_forward_median': round(med, 4),
        'ms_per_forward_min': round(min(windows), 4),
        'ms_per_forward_max': round(max(windows), 4),
        'frames_per_sec': round(args.batch / med * 1e3, 1)}), flush=True)
    return 0


def run_child(args, feature_type, batch, eager):
    """One configuration in a fresh process.  Returns (exit status, result
    dict or None)."""
    env = dict(os.environ)
    env.pop('VFA_NO_CLIPRN', None)
    if eager:
        env['VFA_NO_CLIPRN'] = '1'
    cmd = ['timeout', '-k', '10', str(args.child_timeout), sys.executable,
           os.path.abspath(__file__), '--child',
           '--feature_type', feature_type, '--batch', str(batch),
           '--iters', str(args.iters), '--repeats', str(args.repeats),
           '--warmup', str(args.warmup)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    res = None
    for line in p.stdout.splitlines():
        if line.startswith('{'):
            res = json.loads(line)
            print(line, flush=True)
    return p.returncode, res


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=20)
    p.add_argument('--repeats', type=int, default=7)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--rounds', type=int, default=2,
                   help='eager/fused alternations for CLIP-RN50')
    p.add_argument('--child_timeout', type=int, default=240)
    p.add_argument('--skip_large', action='store_true',
                   help='only the CLIP-RN50 A/B')
    p.add_argument('--child', action='store_true')
    p.add_argument('--feature_type', default='CLIP-RN50')
    p.add_argument('--batch', type=int, default=64)
    args = p.parse_args()
    if args.child:
        return child(args)

    ab = {'eager': [], 'fused': []}
    for _ in range(args.rounds):
        for eager in (True, False):
            rc, res = run_child(args, 'CLIP-RN50', 64, eager)
            if rc != 0 or res is None:
                print(f'child exited with status {rc}; stopping',
                      file=sys.stderr)
                return 1
            ab[res['path']].append(res['frames_per_sec'])
    large = []
    if not args.skip_large:
        for ft, batch in (('CLIP-RN50x4', 32), ('CLIP-RN50x16', 16)):
            while True:
                rc, res = run_child(args, ft, batch, False)
                if rc == OOM_EXIT and batch > 1:
                    print(f'{ft}: out of memory at batch {batch}, halving',
                          flush=True)
                    batch //= 2
                    continue
                break
            if rc != 0 or res is None:
                print(f'child exited with status {rc}; stopping',
                      file=sys.stderr)
                return 1
            large.append(res)
    e, f = statistics.median(ab['eager']), statistics.median(ab['fused'])
    print(json.dumps({
        'summary': 'CLIP-RN50 batch 64 bf16 encode_image',
        'eager_frames_per_sec': ab['eager'],
        'fused_frames_per_sec': ab['fused'],
        'fused_over_eager': round(f / e, 3),
        'large_fused': [{k: r[k] for k in ('feature_type', 'batch',
                                            'frames_per_sec')}
                        for r in large]}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
