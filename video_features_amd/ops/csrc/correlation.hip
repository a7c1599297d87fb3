// PWC cost-volume correlation for gfx950.
//
// The reference JIT-compiles four CUDA kernels via CuPy (reference
// models/pwc/pwc_src/correlation.py): NCHW->padded-NHWC rearrange + an
// 81-channel updateOutput with a 32-thread block and __shared__ float
// sum[32] — a Volta-era shape.  Re-designed for CDNA4:
//
//  * repack: NCHW -> zero-padded NHWC (pad = max_disp), coalesced writes.
//  * corr_tiled (C <= 64, the high-resolution pyramid levels): one wave64
//    per 8x8 pixel tile; the f1 tile (8x8xC) and the f2 tile (16x16xC,
//    padding-inclusive) are staged in LDS once and reused by all 81
//    displacements — an 81x reuse factor no cache gives reliably; lane =
//    pixel, no cross-lane reduction at all.
//  * corr_wave (C > 64, the tiny deep levels): one wave per pixel, lanes
//    stride channels (coalesced NHWC reads), f1 cached in VGPRs,
//    wave shuffle reduction per displacement.
//
// Output (B, (2d+1)^2, H, W) = channel-MEAN dot products (reference
// semantics), float32 NCHW.  With ldo > 0 the kernels instead write bf16
// into the channel slice [out_off, out_off + 81) of an NHWC buffer whose
// pixel stride is ldo elements (the host folds out_off into the pointer):
// the PWC decoder's dense buffer, no NCHW tensor, cast or cat in between.
// leaky != 0 applies LeakyReLU(0.1) before the store in either mode.
//
// channels_last inputs (vfa_pwc_correlation_nhwc): the NHWC = true variants
// of both kernels read the unpadded tensors directly, out-of-image taps
// contribute zero through a bounds check at staging (tiled) or a
// wave-uniform check per displacement (wave): no repack, no padded copy.
#include "vfa_common.h"

namespace {

constexpr int MAXD = 4;           // displacement radius (9x9 window)
constexpr int NDISP = 81;

// one cost-volume value: displacement d of pixel pix (= y*w + x) of image bi
__device__ __forceinline__ void corr_store(void* __restrict__ out, int bi,
                                           long long pix, int d,
                                           long long hw, int ldo, int leaky,
                                           float v) {
  if (leaky && v < 0.f) v *= 0.1f;
  if (ldo > 0)
    static_cast<__hip_bfloat16*>(out)[((long long)bi * hw + pix) * ldo + d] =
        from_f32<__hip_bfloat16>(v);
  else
    static_cast<float*>(out)[((long long)bi * NDISP + d) * hw + pix] = v;
}

// ---------------------------------------------------------------- repack
template <typename T>
__global__ void repack_kernel(const T* __restrict__ in, T* __restrict__ out,
                              int b, int c, int h, int w) {
  // out: (b, h+2p, w+2p, c), zero border
  const int hp = h + 2 * MAXD, wp = w + 2 * MAXD;
  const long long total = (long long)b * hp * wp * c;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % c);
    long long r = i / c;
    const int xp = (int)(r % wp);
    r /= wp;
    const int yp = (int)(r % hp);
    const int bi = (int)(r / hp);
    const int y = yp - MAXD, x = xp - MAXD;
    T v = from_f32<T>(0.f);
    if (y >= 0 && y < h && x >= 0 && x < w)
      v = in[(((long long)bi * c + ci) * h + y) * w + x];
    out[i] = v;
  }
}

// ------------------------------------------------------------ corr_tiled
// NHWC = false: f1 NCHW, f2p the zero-padded NHWC repack.
// NHWC = true: f1 and f2p are the UNPADDED channels_last tensors; the f2
// staging bounds-checks and zero-fills the out-of-image taps.
template <typename T, bool NHWC>
__global__ void corr_tiled_kernel(const T* __restrict__ f1,
                                  const T* __restrict__ f2p,
                                  void* __restrict__ out, int b, int c,
                                  int h, int w, int ldo, int leaky) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cp = c + 1;   // +1 element pad breaks the power-of-2 bank stride
  T* s_f1 = reinterpret_cast<T*>(smem);                 // [64][cp]
  T* s_f2 = s_f1 + 64 * cp;                             // [256][cp]
  const int tileX = blockIdx.x * 8, tileY = blockIdx.y * 8;
  const int bi = blockIdx.z;
  const int lane = threadIdx.x;                         // 0..63
  const int tx = lane & 7, ty = lane >> 3;
  const int x = tileX + tx, y = tileY + ty;
  const int wp = w + 2 * MAXD;
  const long long hw = (long long)h * w;

  // stage f1: each lane loads its own pixel's channel vector (NCHW reads,
  // stride hw — hits L2; done once per 81 reuses)
  if (x < w && y < h) {
    if constexpr (NHWC) {
      const T* src = f1 + ((long long)bi * hw + (long long)y * w + x) * c;
      for (int ci = 0; ci < c; ++ci) s_f1[lane * cp + ci] = src[ci];
    } else {
      const T* src = f1 + (long long)bi * c * hw + (long long)y * w + x;
      for (int ci = 0; ci < c; ++ci)
        s_f1[lane * cp + ci] = src[(long long)ci * hw];
    }
  }
  // stage f2: 16x16 padded-NHWC patch rooted at (tileY, tileX) in padded
  // coords; 4 pixels per lane, contiguous channel reads
  for (int p = lane; p < 256; p += 64) {
    const int fy = p >> 4, fx = p & 15;
    const int gy = tileY + fy, gx = tileX + fx;   // padded coords
    T* dst = s_f2 + p * cp;
    if constexpr (NHWC) {
      const int iy = gy - MAXD, ix = gx - MAXD;   // image coords
      if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
        const T* src = f2p + ((long long)bi * hw + (long long)iy * w + ix) * c;
        for (int ci = 0; ci < c; ++ci) dst[ci] = src[ci];
      } else {
        for (int ci = 0; ci < c; ++ci) dst[ci] = from_f32<T>(0.f);
      }
    } else if (gy < h + 2 * MAXD && gx < wp) {
      const T* src = f2p + (((long long)bi * (h + 2 * MAXD) + gy) * wp + gx) * c;
      for (int ci = 0; ci < c; ++ci) dst[ci] = src[ci];
    }
  }
  __syncthreads();
  if (x >= w || y >= h) return;

  const float inv_c = 1.0f / c;
  const T* my_f1 = s_f1 + lane * cp;
  const long long pix = (long long)y * w + x;
#pragma unroll 3
  for (int d = 0; d < NDISP; ++d) {
    const int dy = d / 9, dx = d % 9;            // 0..8 == offset -4..+4
    const T* other = s_f2 + ((ty + dy) * 16 + (tx + dx)) * cp;
    float acc = 0.f;
    for (int ci = 0; ci < c; ++ci)
      acc += to_f32<T>(my_f1[ci]) * to_f32<T>(other[ci]);
    corr_store(out, bi, pix, d, hw, ldo, leaky, acc * inv_c);
  }
}

// ------------------------------------------------------------- corr_wave
// NHWC = false: both inputs are the zero-padded NHWC repacks.
// NHWC = true: both are the UNPADDED channels_last tensors; a displacement
// that leaves the image is a wave-uniform test and stores zero.
template <typename T, bool NHWC>
__global__ void corr_wave_kernel(const T* __restrict__ f1p,
                                 const T* __restrict__ f2p,
                                 void* __restrict__ out, int b, int c,
                                 int h, int w, int ldo, int leaky) {
  const int wp = w + 2 * MAXD;
  const long long hw = (long long)h * w;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves_per_block = blockDim.x >> 6;
  const long long pix_id =
      (long long)blockIdx.x * waves_per_block + wave;
  if (pix_id >= (long long)b * hw) return;
  const int bi = (int)(pix_id / hw);
  const int pix = (int)(pix_id % hw);
  const int y = pix / w, x = pix % w;

  // f1 channel chunk in registers (lane-strided)
  float reg1[4];
  const T* src1 =
      NHWC ? f1p + ((long long)bi * hw + pix) * c
           : f1p + (((long long)bi * (h + 2 * MAXD) + y + MAXD) * wp + x +
                    MAXD) * c;
  const int nchunk = (c + 63) / 64;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ci = k * 64 + lane;
    reg1[k] = (k < nchunk && ci < c) ? to_f32<T>(src1[ci]) : 0.f;
  }
  const float inv_c = 1.0f / c;
  for (int d = 0; d < NDISP; ++d) {
    const int dy = d / 9, dx = d % 9;
    const T* src2;
    if constexpr (NHWC) {
      const int y2 = y + dy - MAXD, x2 = x + dx - MAXD;
      if (y2 < 0 || y2 >= h || x2 < 0 || x2 >= w) {
        if (lane == 0) corr_store(out, bi, pix, d, hw, ldo, leaky, 0.f);
        continue;
      }
      src2 = f2p + ((long long)bi * hw + (long long)y2 * w + x2) * c;
    } else {
      src2 =
          f2p + (((long long)bi * (h + 2 * MAXD) + y + dy) * wp + x + dx) * c;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ci = k * 64 + lane;
      if (k < nchunk && ci < c) acc += reg1[k] * to_f32<T>(src2[ci]);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) corr_store(out, bi, pix, d, hw, ldo, leaky, acc * inv_c);
  }
}

template <typename T, bool NHWC = false>
void launch_corr(const void* f1, const void* f1p, const void* f2p, void* out,
                 int b, int c, int h, int w, int ldo, int leaky,
                 hipStream_t stream) {
  if (c <= 64) {
    dim3 grid((w + 7) / 8, (h + 7) / 8, b);
    size_t lds = (size_t)(64 + 256) * (c + 1) * sizeof(T);
    hipLaunchKernelGGL((corr_tiled_kernel<T, NHWC>), grid, dim3(64), lds, stream,
                       (const T*)f1, (const T*)f2p, out, b, c, h, w, ldo,
                       leaky);
  } else {
    const int waves_per_block = 4;
    long long npix = (long long)b * h * w;
    long long nblocks = (npix + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL((corr_wave_kernel<T, NHWC>), dim3((unsigned)nblocks),
                       dim3(waves_per_block * 64), 0, stream, (const T*)f1p,
                       (const T*)f2p, out, b, c, h, w, ldo, leaky);
  }
}

}  // namespace

extern "C" {

void vfa_corr_repack(const void* in, void* out, int b, int c, int h, int w,
                     int dtype, hipStream_t stream) {
  const int hp = h + 2 * MAXD, wp = w + 2 * MAXD;
  long long total = (long long)b * hp * wp * c;
  int block = 256;
  int grid = (int)min((total + block - 1) / block, (long long)8192);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((repack_kernel<T>), dim3(grid), dim3(block), 0, stream,
                       (const T*)in, (T*)out, b, c, h, w);
  });
}

// f1: NCHW original; f1p/f2p: padded NHWC (from vfa_corr_repack);
// out: (B, 81, H, W) float32 when ldo == 0; with ldo > 0 the first of the
// 81 bf16 slice channels of pixel 0 in an NHWC buffer of pixel stride ldo
void vfa_pwc_correlation(const void* f1, const void* f1p, const void* f2p,
                         void* out, int b, int c, int h, int w, int dtype,
                         int ldo, int leaky, hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    launch_corr<typename decltype(t)::type>(f1, f1p, f2p, out, b, c, h, w,
                                            ldo, leaky, stream);
  });
}

// f1, f2: unpadded channels_last bf16 (B, C, H, W), C <= 256; out: the first
// of the 81 bf16 slice channels of pixel 0 in an NHWC buffer of pixel
// stride ldo > 0.  No repack and no padded copy.
void vfa_pwc_correlation_nhwc(const void* f1, const void* f2, void* out,
                              int b, int c, int h, int w, int ldo, int leaky,
                              hipStream_t stream) {
  launch_corr<__hip_bfloat16, true>(f1, f1, f2, out, b, c, h, w, ldo, leaky,
                                    stream);
}

}  // extern "C"
