#!/usr/bin/env python3
"""Flagship benchmark: frames/sec of CLIP-ViT-B/32 ``uni_12`` extraction.

Driver contract:
  python bench.py --gpus N --steps K --warmup W
For N > 1 the driver launches this under ``torch.distributed.run`` with one
rank per GPU (RCCL); ranks read RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the
environment.  Work is synthetic (no network): random-init ViT-B/32 weights,
random uint8 224x224 RGB frames, 12 frames per "video" (the ``uni_12``
sampling config of BASELINE.json).  Each step runs the full per-batch GPU
pipeline — double-buffered H2D upload of uint8 frames on a copy stream,
fused u8→CHW normalization, bf16 ViT forward through the hand-written HIP
ops (fused LayerNorm(+residual), packed-qkv MFMA flash attention, the
fc1+QuickGELU fused MFMA GEMM), hipGraph replay per chunk, and the D2H
feature pull that the extractor performs per video batch.

Weak scaling: per-GPU work is fixed (``--videos-per-step`` per rank);
``value`` is the WHOLE-JOB frames/sec aggregated over all ranks.

Other BASELINE configs: ``--model i3d_raft`` (config 4; ``--flow pwc``
for the PWC variant), ``--model resnet50`` (config 3), ``--model
vggish_r21d`` (config 5).

A plain run sets up, warms up, times ``--steps`` steps and prints one JSON
line; ``ms_per_step`` is the wall time of one timed step.  ``--dump-outputs
DIR`` additionally writes the feature array the last timed step returned to
``DIR/features.npy`` (float32) — inputs and weights are seeded, so two builds
run with the same arguments can be compared output for output.  ``--full``
is where any measurement beyond the headline figure belongs (baselines,
other precisions, per-kernel runs); none exists yet, so it changes nothing.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch

# CK-solver "[Init] Not found" spam from MIOpen is harmless; keep the
# driver-visible output to the single JSON line
os.environ.setdefault('MIOPEN_LOG_LEVEL', '1')


def get_dist():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(rank)))
    return rank, local_rank, world


def setup(world: int, rank: int, local_rank: int, device: torch.device):
    if world > 1:
        import torch.distributed as dist
        backend = 'nccl' if device.type == 'cuda' else 'gloo'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29511')
        dist.init_process_group(backend, rank=rank, world_size=world)


def sync(device: torch.device, world: int):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    if device.type == 'cuda':
        torch.cuda.synchronize(device)


def max_over_ranks(value: float, device: torch.device, world: int) -> float:
    if world <= 1:
        return value
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.float64,
                     device=device if device.type == 'cuda' else 'cpu')
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# --------------------------------------------------------------------- CLIP
def bench_clip(args, device, dtype, rank, world):
    from video_features_amd import transforms as T
    from video_features_amd.models.clip_vit import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer().to(device=device, dtype=dtype).eval()
    if world > 1:
        from video_features_amd.runtime.dist import broadcast_models
        broadcast_models(model)

    from video_features_amd import ops

    frames_per_video = 12
    videos = args.videos_per_step
    n_frames = videos * frames_per_video
    g = torch.Generator().manual_seed(rank + 1)
    host_frames = torch.randint(0, 256, (n_frames, 224, 224, 3),
                                dtype=torch.uint8, generator=g)
    if device.type == 'cuda':
        host_frames = host_frames.pin_memory()
    fb = min(args.frame_batch, n_frames)
    bf16 = dtype == torch.bfloat16

    def fwd(frames_u8_dev):
        x = ops.preprocess_u8_chw(frames_u8_dev, T.CLIP_MEAN, T.CLIP_STD, bf16)
        return model.encode_image(x.to(dtype))

    feats_dev = torch.empty(n_frames, 512, device=device, dtype=dtype)
    # the per-step feature pull lands in a PINNED preallocated host buffer
    # (a fresh pageable .cpu() tensor per step costs ~1 ms/MB)
    feats_host = torch.empty(n_frames, 512, dtype=torch.float32,
                             pin_memory=device.type == 'cuda')
    use_graph = device.type == 'cuda' and not args.no_graphs
    if use_graph:
        # hipGraph-capture the whole per-chunk pipeline (preprocess + ViT),
        # TWICE — one graph per input buffer — so the 115 MB/step H2D frame
        # upload double-buffers on a copy stream and overlaps compute
        # (copy_ + replay on one stream serializes; measured ~17%/step)
        static_in = [torch.empty(fb, 224, 224, 3, dtype=torch.uint8,
                                 device=device) for _ in range(2)]
        warm = torch.cuda.Stream()
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm), torch.no_grad():
            for _ in range(2):
                fwd(static_in[0])
        torch.cuda.current_stream().wait_stream(warm)
        graphs, static_out = [], []
        pool = None
        for i in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool), torch.no_grad():
                static_out.append(fwd(static_in[i]))
            pool = g.pool()
            graphs.append(g)
        copy_stream = torch.cuda.Stream()
        done_ev = [torch.cuda.Event(), torch.cuda.Event()]
        for e in done_ev:
            e.record()        # buffers start free

    def step():
        if use_graph:
            main = torch.cuda.current_stream()
            chunks = [host_frames[st:st + fb]
                      for st in range(0, n_frames, fb)]
            # prefetch chunk 0
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done_ev[0])
                static_in[0].copy_(chunks[0], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(copy_stream)
            for ci, chunk in enumerate(chunks):
                buf = ci & 1
                main.wait_event(ready)
                # prefetch the next chunk into the other buffer while the
                # graph for this one runs
                if ci + 1 < len(chunks):
                    nxt = 1 - buf
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done_ev[nxt])
                        static_in[nxt].copy_(chunks[ci + 1],
                                             non_blocking=True)
                    ready = torch.cuda.Event()
                    ready.record(copy_stream)
                if chunk.shape[0] == fb:
                    graphs[buf].replay()
                    st = ci * fb
                    feats_dev[st:st + fb].copy_(static_out[buf])
                else:
                    dev_chunk = chunk.to(device, non_blocking=True)
                    st = ci * fb
                    feats_dev[st:st + chunk.shape[0]].copy_(fwd(dev_chunk))
                done_ev[buf].record(main)
        else:
            for st in range(0, n_frames, fb):
                chunk = host_frames[st:st + fb]
                dev_chunk = chunk.to(device, non_blocking=True)
                feats_dev[st:st + chunk.shape[0]].copy_(fwd(dev_chunk))
        # one per-step D2H pull, as the extractor does per video batch
        feats_host.copy_(feats_dev.float())
        return feats_host

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        sync(device, world)
        t0 = time.perf_counter()
        last = None
        for _ in range(args.steps):
            last = step()
        sync(device, world)
        dt = time.perf_counter() - t0
    dt = max_over_ranks(dt, device, world)
    total_frames = n_frames * world * args.steps
    return {
        'metric': 'frames/sec CLIP-ViT-B/32 uni_12',
        'value': total_frames / dt,
        'unit': 'frames/sec',
        'ms_per_step': dt / args.steps * 1000.0,
        'outputs': {'features': last},
        'config': {'model': 'CLIP-ViT-B/32', 'global_batch': videos * world,
                   'seq_len': frames_per_video, 'resolution': 224,
                   'parallelism': f'dp{world}'},
    }


# ---------------------------------------------------------------- I3D+RAFT
def bench_i3d_raft(args, device, dtype, rank, world):
    from video_features_amd import transforms as T
    from video_features_amd.models.i3d import I3D
    from video_features_amd.models.raft import RAFT
    from video_features_amd.models.pwc import PWCNet
    torch.manual_seed(0)
    from video_features_amd.utils.fold_bn import fold_batchnorms
    i3d_rgb = I3D(modality='rgb').to(device, dtype).eval()
    i3d_flow = I3D(modality='flow').to(device, dtype).eval()
    if args.flow == 'pwc':
        raft = PWCNet().to(device, dtype).eval()
    else:
        raft = RAFT(iters=args.raft_iters).to(device, dtype).eval()
    # inference-only: fold BN affine maps into the convs (see fold_bn.py)
    fold_batchnorms(i3d_rgb)
    fold_batchnorms(i3d_flow)
    fold_batchnorms(raft)
    nhwc = args.layout == 'nhwc' and device.type == 'cuda'
    if nhwc and hasattr(raft, 'use_channels_last'):
        raft = raft.use_channels_last()
    cl3d = args.i3d_cl3d and device.type == 'cuda'
    if cl3d:
        i3d_rgb = i3d_rgb.to(memory_format=torch.channels_last_3d)
        i3d_flow = i3d_flow.to(memory_format=torch.channels_last_3d)
    if world > 1:
        from video_features_amd.runtime.dist import broadcast_models
        broadcast_models({'a': i3d_rgb, 'b': i3d_flow, 'c': raft})

    stack = 64
    clips = args.clips_per_step
    g = torch.Generator().manual_seed(rank + 1)
    host = torch.randint(0, 256, (clips, stack + 1, 224, 224, 3),
                         dtype=torch.uint8, generator=g)
    if device.type == 'cuda':
        host = host.pin_memory()

    gathered = [None]

    def clips_fwd(frames_u8_dev):
        # (clips, 65, 224, 224, 3) u8 — ALL clips batched through one RAFT
        # pass (clips*64 frame pairs) and one I3D pass per stream (batch =
        # clips): bigger GEMMs, 1/clips the kernel launches
        x = frames_u8_dev.permute(0, 1, 4, 2, 3).to(dtype)
        i1 = x[:, :-1].reshape(-1, 3, 224, 224)
        i2 = x[:, 1:].reshape(-1, 3, 224, 224)
        if args.flow == 'pwc':
            flow = raft(i1, i2)                      # (clips*64, 2, H, W)
        else:
            flow = raft(i1, i2, test_mode=True)
        rgb_in = T.scale_to_pm1(x[:, :-1]).transpose(1, 2)
        flow_in = T.i3d_flow_preprocess(flow, 224) \
            .reshape(clips, stack, 2, 224, 224).transpose(1, 2)
        if cl3d:
            rgb_in = rgb_in.contiguous(memory_format=torch.channels_last_3d)
            flow_in = flow_in.contiguous(memory_format=torch.channels_last_3d)
        f_rgb = i3d_rgb.forward_features(rgb_in)
        f_flow = i3d_flow.forward_features(flow_in)
        return torch.cat([f_rgb, f_flow], dim=1)     # (clips, 2048)

    use_graph = device.type == 'cuda' and not args.no_graphs
    if use_graph:
        # hipGraph-capture the whole per-step pipeline (RAFT 20-iteration
        # loop + both I3D streams): replay removes thousands of per-step
        # kernel-launch gaps
        static_in = torch.empty(clips, stack + 1, 224, 224, 3,
                                dtype=torch.uint8, device=device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):
                clips_fwd(static_in)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            static_out = clips_fwd(static_in)

    def step():
        if use_graph:
            static_in.copy_(host, non_blocking=True)
            graph.replay()
            out = static_out.clone()
        else:
            out = clips_fwd(host.to(device, non_blocking=True))
        # RCCL all-gather of stack features (BASELINE.json config 4)
        if world > 1:
            import torch.distributed as dist
            buf = [torch.empty_like(out) for _ in range(world)]
            dist.all_gather(buf, out)
            gathered[0] = buf
        return out.float().to('cpu', non_blocking=False)

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        sync(device, world)
        t0 = time.perf_counter()
        last = None
        for _ in range(args.steps):
            last = step()
        sync(device, world)
        dt = time.perf_counter() - t0
    dt = max_over_ranks(dt, device, world)
    total_clips = clips * world * args.steps
    return {
        'metric': f'clips/sec I3D rgb+flow ({args.flow.upper()})',
        'value': total_clips / dt,
        'unit': 'clips/sec',
        'ms_per_step': dt / args.steps * 1000.0,
        'outputs': {'features': last},
        'config': {'model': f'I3D+{args.flow.upper()}',
                   'global_batch': clips * world,
                   'seq_len': stack, 'resolution': 224,
                   'raft_iters': args.raft_iters, 'layout': args.layout,
                   'parallelism': f'dp{world}'},
    }


# ---------------------------------------------------------------- ResNet-50
def bench_resnet(args, device, dtype, rank, world):
    """BASELINE.json config 3: ResNet-50 fix_2 frames/sec, DP-sharded."""
    from video_features_amd import transforms as T
    from video_features_amd.models.resnet import build_resnet
    from video_features_amd import ops
    torch.manual_seed(0)
    from video_features_amd.utils.fold_bn import fold_batchnorms
    model = build_resnet('resnet50').to(device, dtype).eval()
    fold_batchnorms(model)
    if device.type == 'cuda':
        model = model.to(memory_format=torch.channels_last)
    if world > 1:
        from video_features_amd.runtime.dist import broadcast_models
        broadcast_models(model)

    n_frames = args.videos_per_step * 12
    g = torch.Generator().manual_seed(rank + 1)
    host = torch.randint(0, 256, (n_frames, 224, 224, 3), dtype=torch.uint8,
                         generator=g)
    if device.type == 'cuda':
        host = host.pin_memory()
    fb = min(args.frame_batch, n_frames)
    bf16 = dtype == torch.bfloat16

    def fwd(frames_u8):
        x = ops.preprocess_u8_chw(frames_u8, T.IMAGENET_MEAN, T.IMAGENET_STD,
                                  bf16).to(dtype)
        if device.type == 'cuda':
            x = x.contiguous(memory_format=torch.channels_last)
        return model.forward_features(x)

    feats = torch.empty(n_frames, 2048, device=device, dtype=dtype)
    feats_host = torch.empty(n_frames, 2048, dtype=torch.float32,
                             pin_memory=device.type == 'cuda')
    use_graph = device.type == 'cuda' and not args.no_graphs
    if use_graph:
        # double-buffered H2D on a copy stream (as the CLIP bench does) —
        # a single static_in on the main stream serialized the 57 MB/chunk
        # upload with compute (~6%/step in the rocprof trace)
        static_in = [torch.empty(fb, 224, 224, 3, dtype=torch.uint8,
                                 device=device) for _ in range(2)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):
                fwd(static_in[0])
        torch.cuda.current_stream().wait_stream(s)
        graphs, static_out = [], []
        pool = None
        for i in range(2):
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=pool), torch.no_grad():
                static_out.append(fwd(static_in[i]))
            pool = g2.pool()
            graphs.append(g2)
        copy_stream = torch.cuda.Stream()
        done_ev = [torch.cuda.Event(), torch.cuda.Event()]
        for e in done_ev:
            e.record()

    def step():
        if use_graph:
            main = torch.cuda.current_stream()
            chunks = [host[st:st + fb] for st in range(0, n_frames, fb)]
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(done_ev[0])
                static_in[0].copy_(chunks[0], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(copy_stream)
            for ci, chunk in enumerate(chunks):
                buf = ci & 1
                main.wait_event(ready)
                if ci + 1 < len(chunks):
                    nxt = 1 - buf
                    with torch.cuda.stream(copy_stream):
                        copy_stream.wait_event(done_ev[nxt])
                        static_in[nxt].copy_(chunks[ci + 1],
                                             non_blocking=True)
                    ready = torch.cuda.Event()
                    ready.record(copy_stream)
                st = ci * fb
                if chunk.shape[0] == fb:
                    graphs[buf].replay()
                    feats[st:st + fb].copy_(static_out[buf])
                else:
                    feats[st:st + chunk.shape[0]].copy_(
                        fwd(chunk.to(device, non_blocking=True)))
                done_ev[buf].record(main)
        else:
            for st in range(0, n_frames, fb):
                chunk = host[st:st + fb]
                feats[st:st + chunk.shape[0]].copy_(
                    fwd(chunk.to(device, non_blocking=True)))
        feats_host.copy_(feats.float())
        return feats_host

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        sync(device, world)
        t0 = time.perf_counter()
        last = None
        for _ in range(args.steps):
            last = step()
        sync(device, world)
        dt = time.perf_counter() - t0
    dt = max_over_ranks(dt, device, world)
    total = n_frames * world * args.steps
    return {
        'metric': 'frames/sec ResNet-50 fix_2',
        'value': total / dt,
        'unit': 'frames/sec',
        'ms_per_step': dt / args.steps * 1000.0,
        'outputs': {'features': last},
        'config': {'model': 'ResNet-50', 'global_batch': n_frames * world,
                   'seq_len': 1, 'resolution': 224,
                   'parallelism': f'dp{world}'},
    }


# -------------------------------------------------- VGGish + R(2+1)D dual
def bench_vggish_r21d(args, device, dtype, rank, world):
    """BASELINE.json config 5: dual-stream audio (VGGish) + visual
    (R(2+1)D-34, the depth config 5 names; ``--r21d-depth 18`` for the
    reference extractor's torchvision depth) clips/sec."""
    from video_features_amd.models.vggish import VGGish
    from video_features_amd.models.r21d import R2Plus1D18, R2Plus1D34
    from video_features_amd import transforms as T
    torch.manual_seed(0)
    from video_features_amd.utils.fold_bn import fold_batchnorms
    vgg = VGGish().to(device, dtype).eval()
    r21d = (R2Plus1D34() if args.r21d_depth == 34
            else R2Plus1D18()).to(device, dtype).eval()
    fold_batchnorms(r21d)
    if world > 1:
        from video_features_amd.runtime.dist import broadcast_models
        broadcast_models({'a': vgg, 'b': r21d})

    clips = max(args.clips_per_step, 1)
    g = torch.Generator().manual_seed(rank + 1)
    # visual: 16-frame 112x112 stacks; audio: 0.96 s log-mel examples.
    # The H2D upload is INSIDE the timed step (as the CLIP/ResNet benches
    # time it) — pinned buffers, async copies.
    host_v = torch.rand(clips, 3, 16, 112, 112, generator=g).to(dtype)
    host_a = torch.rand(clips, 96, 64, generator=g).to(dtype)
    if device.type == 'cuda':
        host_v = host_v.pin_memory()
        host_a = host_a.pin_memory()

    def step():
        vis = host_v.to(device, non_blocking=True)
        aud = host_a.to(device, non_blocking=True)
        fa = vgg(aud)
        fv = r21d.forward_features(vis)
        return torch.cat([fv, fa.to(fv.dtype)], dim=1).float().cpu()

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        sync(device, world)
        t0 = time.perf_counter()
        last = None
        for _ in range(args.steps):
            last = step()
        sync(device, world)
        dt = time.perf_counter() - t0
    dt = max_over_ranks(dt, device, world)
    total = clips * world * args.steps
    return {
        'metric': 'clips/sec VGGish+R(2+1)D dual-stream',
        'value': total / dt,
        'unit': 'clips/sec',
        'ms_per_step': dt / args.steps * 1000.0,
        'outputs': {'features': last},
        'config': {'model': f'VGGish+R(2+1)D-{args.r21d_depth}',
                   'global_batch': clips * world,
                   'seq_len': 16, 'resolution': 112,
                   'parallelism': f'dp{world}'},
    }


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir: str, outputs: dict) -> None:
    """Write what the last timed step returned as ``out_dir/<name>.npy``
    (float32).  An array over its share of the 64 MB budget is stored as a
    fixed, seeded sample of its flattened elements, so two builds run with
    the same arguments still compare element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(outputs), 1)
    for name, t in outputs.items():
        a = t.detach().to('cpu', torch.float32).numpy()
        if a.nbytes > share:
            keep = share // a.itemsize
            idx = np.random.default_rng(0).choice(a.size, keep, replace=False)
            idx.sort()
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f'{name}.npy'), a)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--steps', type=int, default=16)
    p.add_argument('--warmup', type=int, default=4)
    p.add_argument('--model', choices=['clip', 'i3d_raft', 'resnet50', 'vggish_r21d'],
                   default='clip')
    p.add_argument('--videos-per-step', type=int, default=256,
                   help='CLIP: synthetic videos (x12 frames) per rank per '
                        'step (256 = the measured throughput knee; per-step '
                        'launch/copy overheads amortize: 65.7k -> 71.4k f/s '
                        'vs 64)')
    p.add_argument('--frame-batch', type=int, default=384,
                   help='CLIP: frames per forward chunk')
    p.add_argument('--clips-per-step', type=int, default=None,
                   help='clips per rank per step (default: 16 for i3d_raft, '
                        '128 for vggish_r21d — measured throughput knees)')
    p.add_argument('--raft-iters', type=int, default=20)
    p.add_argument('--r21d-depth', type=int, choices=[18, 34], default=34,
                   help='R(2+1)D depth for vggish_r21d (BASELINE config 5 '
                        'names -34; the reference extractor uses -18)')
    p.add_argument('--flow', choices=['raft', 'pwc'], default='raft',
                   help='flow net for the i3d_raft bench')
    p.add_argument('--layout', choices=['nhwc', 'nchw'], default='nhwc',
                   help='RAFT conv layout on GPU (nhwc = channels_last)')
    p.add_argument('--i3d-cl3d', action='store_true',
                   help='run I3D in channels_last_3d (NDHWC)')
    p.add_argument('--dtype', choices=['bf16', 'fp32'], default=None)
    p.add_argument('--no-graphs', action='store_true',
                   help='disable hipGraph capture of the forward')
    p.add_argument('--dump-outputs', metavar='DIR', default=None,
                   help='after the timed steps, write the arrays the last '
                        'timed step returned as DIR/<name>.npy (float32)')
    p.add_argument('--full', action='store_true',
                   help='also run every measurement beyond the headline '
                        'figure; a plain run already times only the selected '
                        'config, so there is nothing extra to run yet')
    args = p.parse_args()

    if args.clips_per_step is None:
        args.clips_per_step = 128 if args.model == 'vggish_r21d' else 16

    rank, local_rank, world = get_dist()
    if torch.cuda.is_available():
        device = torch.device(f'cuda:{local_rank}')
        torch.cuda.set_device(device)
        dtype = torch.bfloat16 if args.dtype != 'fp32' else torch.float32
    else:
        device = torch.device('cpu')
        dtype = torch.float32
        args.videos_per_step = min(args.videos_per_step, 2)
        args.clips_per_step = 1
        args.raft_iters = min(args.raft_iters, 3)
    setup(world, rank, local_rank, device)

    bench_fns = {'clip': bench_clip, 'i3d_raft': bench_i3d_raft,
                 'resnet50': bench_resnet, 'vggish_r21d': bench_vggish_r21d}
    res = bench_fns[args.model](args, device, dtype, rank, world)

    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, res['outputs'])
        out = {
            'metric': res['metric'],
            'value': round(res['value'], 2),
            'unit': res['unit'],
            'n_gpus': world,
            'steps': args.steps,
            'warmup': args.warmup,
            'ms_per_step': round(res['ms_per_step'], 3),
            'higher_is_better': True,
            'scaling': 'weak',
            'vs_baseline': None,   # the reference publishes no numbers
            'dtype': 'bf16' if dtype == torch.bfloat16 else 'fp32',
            'data': 'synthetic',
            'config': res['config'],
        }
        print(json.dumps(out))

    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
