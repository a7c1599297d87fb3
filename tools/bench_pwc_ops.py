#!/usr/bin/env python3
"""A/B bench of the PWC-Net glue ops: the route the dense path ran before
the channels_last change against the channels_last route, per level.

Run on a GPU box:  python tools/bench_pwc_ops.py [--iters 50]
64 frame pairs at the 256x256 input, so the levels are 4^2 .. 64^2.  Event
timing, 10 warm-up iterations.  Rows:

  upfeat  old: nn.ConvTranspose2d on the strided NCHW view of the leading
               channels of the channels_last buffer, then the slice
               assignment into the next buffer
          new: ops.conv_transpose2d_mod, buffer slice in, buffer slice out
  upflow  old: nn.ConvTranspose2d on the flow + slice assignment
          new: ops.conv_transpose2d_mod (direct kernel), slice out
  warp    old: f2.contiguous(), upflow * scale, the NCHW warp kernel
          new: the NHWC kernel on f2 and the upflow slice view, scale inside
  corr    old: f1.contiguous(), warped NCHW f2, repack + cost-volume kernels
          new: the NHWC cost-volume kernels on the channels_last tensors

For upfeat the table also states the bytes the new route must move (x once,
the f32 partials written and read, the output) divided by 6.29 TB/s, the
copy rate measured on the MI355X, and the ratio of the measured time to it.
"""
import argparse
import sys

import torch

sys.path.insert(0, '.')
from video_features_amd import ops  # noqa: E402
from video_features_amd.models.pwc import PWCNet  # noqa: E402

COPY_RATE = 6.29e12       # bytes/s


def bench(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--iters', type=int, default=50)
    p.add_argument('--pairs', type=int, default=64)
    args = p.parse_args()
    assert ops.hip_available()
    dev, dt = 'cuda:0', torch.bfloat16
    torch.manual_seed(0)
    net = PWCNet().eval().to(dev, dt)
    decs = {6: net.decoder6, 5: net.decoder5, 4: net.decoder4,
            3: net.decoder3, 2: net.decoder2}
    fch = {5: 128, 4: 96, 3: 64, 2: 32}
    b = args.pairs
    print(f"{'op':22s} {'old us':>9s} {'new us':>9s} {'old/new':>8s}  note")

    def row(name, t_old, t_new, note=''):
        print(f'{name:22s} {t_old:9.1f} {t_new:9.1f} {t_old / t_new:8.2f}  '
              f'{note}')

    def rnd(*shape):
        return (torch.randn(*shape, device=dev) * 0.5).to(dt)

    with torch.no_grad():
        for lvl in (5, 4, 3, 2):
            prev, dec, fc = decs[lvl + 1], decs[lvl], fch[lvl]
            hp = 256 >> (lvl + 1)                  # previous level's H = W
            h = 2 * hp
            wprev = (prev.out_channels + 7) // 8 * 8
            pbuf = rnd(b, hp, hp, wprev).permute(0, 3, 1, 2)
            pflow = rnd(b, hp, hp, 2).permute(0, 3, 1, 2)
            buf = dec.new_buffer(rnd(b, fc, h, h))
            o = dec.up_off(fc)
            f1 = rnd(b, h, h, fc).permute(0, 3, 1, 2)
            f2 = rnd(b, h, h, fc).permute(0, 3, 1, 2)
            buf[:, o:o + 2] = rnd(b, 2, h, h)
            scale = net.WARP_SCALES[lvl]
            tag = f'l{lvl + 1}>{lvl} {hp}²>{h}²'

            def upfeat_old():
                buf[:, o + 2:o + 4] = prev.upfeat(
                    pbuf[:, :prev.out_channels])

            def upfeat_new():
                ops.conv_transpose2d_mod(prev.upfeat, pbuf, out=buf,
                                         out_off=o + 2, in_off=0)

            c8 = (prev.out_channels + 7) // 8 * 8
            m = b * hp * hp
            nbytes = m * c8 * 2 + 2 * m * 32 * 4 + 4 * m * 2 * 2
            floor = nbytes / COPY_RATE * 1e6
            t_old, t_new = (bench(upfeat_old, args.iters),
                            bench(upfeat_new, args.iters))
            row(f'upfeat {tag}', t_old, t_new,
                f'C={prev.out_channels} {nbytes / 1e6:.2f} MB '
                f'floor {floor:.1f} us, new/floor {t_new / floor:.1f}')

            def upflow_old():
                buf[:, o:o + 2] = prev.upflow(pflow)

            def upflow_new():
                ops.conv_transpose2d_mod(prev.upflow, pflow, out=buf,
                                         out_off=o)

            row(f'upflow {tag}', bench(upflow_old, args.iters),
                bench(upflow_new, args.iters))

            upflow = buf[:, o:o + 2].contiguous()    # the old route's tensor

            def warp_old():
                return ops.bilinear_warp(f2.contiguous(), upflow * scale)

            def warp_new():
                return ops.bilinear_warp(f2, buf[:, o:o + 2], scale=scale)

            row(f'warp l{lvl} C={fc} {h}²', bench(warp_old, args.iters),
                bench(warp_new, args.iters))

            wn, wc = warp_old(), warp_new()

            def corr_old():
                ops.pwc_correlation(f1.contiguous(), wn, out=buf,
                                    out_off=dec.CORR_OFF, act='leaky_relu')

            def corr_new():
                ops.pwc_correlation(f1, wc, out=buf, out_off=dec.CORR_OFF,
                                    act='leaky_relu')

            row(f'corr l{lvl} C={fc} {h}²', bench(corr_old, args.iters),
                bench(corr_new, args.iters))

        # the top level's cost volume: C = 196 at 4x4, no warp
        f1 = rnd(b, 4, 4, 196).permute(0, 3, 1, 2)
        f2 = rnd(b, 4, 4, 196).permute(0, 3, 1, 2)
        buf = net.decoder6.new_buffer(f1)
        row('corr l6 C=196 4²',
            bench(lambda: ops.pwc_correlation(
                f1.contiguous(), f2.contiguous(), out=buf, out_off=448,
                act='leaky_relu'), args.iters),
            bench(lambda: ops.pwc_correlation(
                f1, f2, out=buf, out_off=448, act='leaky_relu'), args.iters))


if __name__ == '__main__':
    main()
