// TF-SAME max_pool3d for gfx950 (I3D's MaxPool3dTFPadding, reference
// models/i3d/i3d_src/i3d_net.py:108-120).
//
// The reference (and our CPU path) does F.pad(zeros) + nn.MaxPool3d; torch's
// GPU max_pool3d always computes argmax indices as well.  This kernel folds
// the asymmetric TF-SAME padding into the window bounds (no padded copy)
// and skips the indices — one dispatch, one read of the tensor.
// Zero-padding max semantics match F.pad(0) + maxpool exactly: positions
// outside the input contribute the value 0.
//
// Also here: the NHWC bf16 average pool of CLIP's ModifiedResNet
// (avgpool2d_nhwc, below the max pools).
#include "vfa_common.h"

namespace {

template <typename T>
__global__ void maxpool3d_same_kernel(const T* __restrict__ x,
                                      T* __restrict__ out, long long bc,
                                      int it, int ih, int iw, int ot, int oh,
                                      int ow, int kt, int kh, int kw, int st,
                                      int sh, int sw, int pt, int ph,
                                      int pw) {
  const long long ohw = (long long)ot * oh * ow;
  const long long total = bc * ohw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / ohw;
    const int rem = (int)(i % ohw);
    const int to = rem / (oh * ow);
    const int yo = (rem / ow) % oh;
    const int xo = rem % ow;
    const int t0 = to * st - pt, y0 = yo * sh - ph, x0 = xo * sw - pw;
    const T* xb = x + n * (long long)it * ih * iw;
    float m = -INFINITY;
    bool padded = false;
    for (int dt = 0; dt < kt; ++dt) {
      const int t = t0 + dt;
      if (t < 0 || t >= it) { padded = true; continue; }
      for (int dy = 0; dy < kh; ++dy) {
        const int y = y0 + dy;
        if (y < 0 || y >= ih) { padded = true; continue; }
        const T* row = xb + ((long long)t * ih + y) * iw;
        for (int dx = 0; dx < kw; ++dx) {
          const int xx = x0 + dx;
          if (xx < 0 || xx >= iw) { padded = true; continue; }
          m = fmaxf(m, to_f32<T>(row[xx]));
        }
      }
    }
    if (padded) m = fmaxf(m, 0.f);  // zero-padding participates in the max
    out[i] = from_f32<T>(m);
  }
}

// spatial 2D TF-SAME max pool (zero padding), NCHW or NHWC — used by the
// flattened (B*T, C, H, W) I3D path where the temporal max is a separate
// shifted elementwise maximum
template <typename T, bool NHWC>
__global__ void maxpool2d_same_kernel(const T* __restrict__ x,
                                      T* __restrict__ out, long long n,
                                      int c, int ih, int iw, int oh, int ow,
                                      int kh, int kw, int sh, int sw, int ph,
                                      int pw) {
  const long long ohwc = (long long)oh * ow * c;
  const long long total = n * ohwc;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    long long ni;
    int yo, xo, ci;
    if (NHWC) {
      ni = i / ohwc;
      const long long r = i % ohwc;
      yo = (int)(r / ((long long)ow * c));
      xo = (int)((r / c) % ow);
      ci = (int)(r % c);
    } else {
      ni = i / ohwc;
      const long long r = i % ohwc;
      ci = (int)(r / ((long long)oh * ow));
      yo = (int)((r / ow) % oh);
      xo = (int)(r % ow);
    }
    const int y0 = yo * sh - ph, x0 = xo * sw - pw;
    const T* xb = x + ni * (long long)c * ih * iw;
    float m = -INFINITY;
    bool padded = false;
    for (int dy = 0; dy < kh; ++dy) {
      const int y = y0 + dy;
      if (y < 0 || y >= ih) { padded = true; continue; }
      for (int dx = 0; dx < kw; ++dx) {
        const int xx = x0 + dx;
        if (xx < 0 || xx >= iw) { padded = true; continue; }
        const long long xi = NHWC ? (((long long)y * iw + xx) * c + ci)
                                  : (((long long)ci * ih + y) * iw + xx);
        m = fmaxf(m, to_f32<T>(xb[xi]));
      }
    }
    if (padded) m = fmaxf(m, 0.f);
    out[i] = from_f32<T>(m);
  }
}

// NHWC bf16 average pool, window = stride = k, floor output size
// (nn.AvgPool2d(k)): CLIP's ModifiedResNet downsamples with this where
// torchvision's ResNet strides.  One thread per 8 output channels: k*k
// 16-B loads, f32 sum, one multiply by 1/k^2, ONE rounding to bf16, one
// 16-B store.  Memory-bound; grid-stride, no LDS.  Requires C % 8 == 0.
__global__ void avgpool2d_nhwc_kernel(const uint4* __restrict__ x,
                                      uint4* __restrict__ out, long long n,
                                      int c8, int ih, int iw, int oh, int ow,
                                      int k, float inv) {
  const long long total = n * oh * ow * c8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % c8);
    long long r = i / c8;
    const int xo = (int)(r % ow);
    r /= ow;
    const int yo = (int)(r % oh);
    const long long ni = r / oh;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // (yo*k + dy) <= oh*k - 1 <= ih - 1: the floor keeps windows in-image
    for (int dy = 0; dy < k; ++dy) {
      const uint4* row =
          x + ((ni * ih + (long long)yo * k + dy) * iw + (long long)xo * k) *
                  c8 + ci;
      for (int dx = 0; dx < k; ++dx) {
        float f[8];
        bf16x8_to_f32(row[(long long)dx * c8], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    out[i] = f32_to_bf16x8(acc);
  }
}

}  // namespace

extern "C" {

void vfa_avgpool2d_nhwc(const void* x, void* out, long long n, int c, int ih,
                        int iw, int oh, int ow, int k, hipStream_t stream) {
  const long long total = n * oh * ow * (c / 8);
  if (total <= 0) return;
  const int grid = (int)min((total + 255) / 256, (long long)2048);
  hipLaunchKernelGGL(avgpool2d_nhwc_kernel, dim3(grid), dim3(256), 0, stream,
                     (const uint4*)x, (uint4*)out, n, c / 8, ih, iw, oh, ow,
                     k, 1.f / (float)(k * k));
}

void vfa_maxpool2d_same(const void* x, void* out, long long n, int c,
                        const PoolGeom& g, int nhwc, int dtype,
                        hipStream_t stream) {
  const long long total = n * (long long)c * g.out[0] * g.out[1];
  const int grid = (int)min((total + 255) / 256, (long long)65536);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      hipLaunchKernelGGL((maxpool2d_same_kernel<T, decltype(cl)::value>),
                         dim3(grid), dim3(256), 0, stream, (const T*)x,
                         (T*)out, n, c, g.in[0], g.in[1], g.out[0], g.out[1],
                         g.k[0], g.k[1], g.s[0], g.s[1], g.pad[0], g.pad[1]);
    });
  });
}

void vfa_maxpool3d_same(const void* x, void* out, long long bc,
                        const PoolGeom& g, int dtype, hipStream_t stream) {
  const long long total = bc * g.out[0] * g.out[1] * g.out[2];
  const int grid = (int)min((total + 255) / 256, (long long)16384);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((maxpool3d_same_kernel<T>), dim3(grid), dim3(256), 0,
                       stream, (const T*)x, (T*)out, bc, g.in[0], g.in[1],
                       g.in[2], g.out[0], g.out[1], g.out[2], g.k[0], g.k[1],
                       g.k[2], g.s[0], g.s[1], g.s[2], g.pad[0], g.pad[1],
                       g.pad[2]);
  });
}

}  // extern "C"
