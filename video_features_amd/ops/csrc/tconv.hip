// Transposed convolution for gfx950: kernel 4x4, stride 2, padding 1,
// K_out <= 2 (the PWC-Net `upflow` / `upfeat` upsamplers), channels_last
// bf16 in, bf16 out, f32 accumulation, ONE rounding.
//
//   out[b,ko,oy,ox] = bias[ko] + sum_{c,ky,kx} x[b,c,iy,ix] * W[c,ko,ky,kx]
//   with oy = 2*iy - 1 + ky, ox = 2*ix - 1 + kx (taps outside the image
//   dropped): every output pixel sums exactly 2x2 input pixels.
//
// "P-form", two kernels:
//  * tconv_p_kernel: P[pixel, n] = sum_c x[pixel, c] * Wp[n, c] with
//    n = (ky*4 + kx)*K_out + ko — a GEMM with M = B*H*W, K = C,
//    N = 16*K_out.  The packed weight Wp (N x C) is resident in LDS, loaded
//    once per block; x streams global -> MFMA fragments with 16-B loads and
//    is read ONCE; grid-stride over M; run-time K loop in steps of 32 with
//    the last step masked at 8-element granularity.  Partials are f32.
//  * tconv_gather_kernel: col2im — each output pixel adds its <= 4 partials
//    and the bias in f32 and rounds once.
//  x may be the channel slice [in_off, in_off + C) of a wider buffer (pixel
//  stride ldx), out the slice [out_off, out_off + K_out) of a buffer of
//  pixel stride ldo (the host folds both offsets into the pointers); out_off
//  may be odd, so the stores are 2-byte.
//
// tconv_direct_kernel (C <= 16, the `upflow` path, C = 2): one thread per
// output pixel, x read through its strides (NCHW or channels_last), f32
// math, one rounding.
#include "vfa_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// NT = K_out = number of 16-column MFMA tiles of P
template <int NT>
__global__ __launch_bounds__(256, 2)
void tconv_p_kernel(const __bf16* __restrict__ x,    // slice start
                    const __bf16* __restrict__ wp,   // (16*NT, c) packed
                    float* __restrict__ p,           // (m, 16*NT)
                    long long m, int c, int ldx) {
  constexpr int N = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi4 = lane >> 4;
  // LDS: Wp rows of kc + 8 elements (kc = c rounded up to 32, the tail
  // zero-filled; +8 breaks the ds_read bank pattern)
  extern __shared__ __attribute__((aligned(16))) char smem_tc[];
  __bf16* wl = reinterpret_cast<__bf16*>(smem_tc);
  const int kc = (c + 31) / 32 * 32;
  const int ldw = kc + 8;
  const int segs = kc / 8;
  for (int t = threadIdx.x; t < N * segs; t += 256) {
    const int row = t / segs, seg = t % segs;
    uint4 v = {0u, 0u, 0u, 0u};
    if (seg * 8 < c)
      v = *reinterpret_cast<const uint4*>(wp + (long long)row * c + seg * 8);
    *reinterpret_cast<uint4*>(wl + row * ldw + seg * 8) = v;
  }
  __syncthreads();

  const long long mstep = (long long)gridDim.x * 128;
  for (long long m0 = (long long)blockIdx.x * 128; m0 < m; m0 += mstep) {
    const long long r0 = m0 + wave * 32;
    if (r0 >= m) continue;                       // wave-uniform
    long long row0 = r0 + lo, row1 = r0 + 16 + lo;
    if (row0 >= m) row0 = m - 1;                 // clamped load, masked store
    if (row1 >= m) row1 = m - 1;
    const __bf16* a0 = x + row0 * ldx + hi4 * 8;
    const __bf16* a1 = x + row1 * ldx + hi4 * 8;
    const __bf16* bp = wl + lo * ldw + hi4 * 8;
    // accumulator indices are compile-time (run-time-indexed vector arrays
    // go to scratch)
    f32x4 acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int jj = 0; jj < NT; ++jj) acc[mi][jj] = f32x4{0, 0, 0, 0};
    for (int k0 = 0; k0 < kc; k0 += 32) {
      bf16x8 af0{}, af1{};                       // masked K tail: x * 0
      if (k0 + hi4 * 8 < c) {
        af0 = *reinterpret_cast<const bf16x8*>(a0 + k0);
        af1 = *reinterpret_cast<const bf16x8*>(a1 + k0);
      }
#pragma unroll
      for (int jj = 0; jj < NT; ++jj) {
        const bf16x8 bfr =
            *reinterpret_cast<const bf16x8*>(bp + jj * 16 * ldw + k0);
        acc[0][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af0, bfr, acc[0][jj], 0, 0, 0);
        acc[1][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af1, bfr, acc[1][jj], 0, 0, 0);
      }
    }
    // fragment (row hi4*4 + r, column lo) -> P: 16 lanes write 64 B runs
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long row = r0 + mi * 16 + hi4 * 4 + r;
        if (row < m) {
#pragma unroll
          for (int jj = 0; jj < NT; ++jj)
            p[row * N + jj * 16 + lo] = acc[mi][jj][r];
        }
      }
  }
}

// the two (tap, input index) pairs of one output coordinate o along one
// axis: tap k has the parity of o + 1, i = (o + 1 - k) / 2
__device__ __forceinline__ void tconv_taps(int o, int& k0, int& i0) {
  k0 = (o + 1) & 1;
  i0 = (o + 1 - k0) >> 1;       // tap k0 reads i0, tap k0 + 2 reads i0 - 1
}

template <int KOUT>
__global__ void tconv_gather_kernel(const float* __restrict__ p,
                                    const __bf16* __restrict__ bias,
                                    __bf16* __restrict__ out,  // slice start
                                    int b, int h, int w, int ldo) {
  constexpr int N = 16 * KOUT;
  const int oh = 2 * h, ow = 2 * w;
  const long long total = (long long)b * oh * ow;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    const long long t = i / ow;
    const int oy = (int)(t % oh);
    const int bi = (int)(t / oh);
    int ky0, iy0, kx0, ix0;
    tconv_taps(oy, ky0, iy0);
    tconv_taps(ox, kx0, ix0);
    float acc[KOUT];
#pragma unroll
    for (int ko = 0; ko < KOUT; ++ko)
      acc[ko] = bias ? (float)bias[ko] : 0.f;
#pragma unroll
    for (int ty = 0; ty < 2; ++ty) {
      const int iy = iy0 - ty, ky = ky0 + 2 * ty;
      if (iy < 0 || iy >= h) continue;
#pragma unroll
      for (int tx = 0; tx < 2; ++tx) {
        const int ix = ix0 - tx, kx = kx0 + 2 * tx;
        if (ix < 0 || ix >= w) continue;
        const float* pp = p + (((long long)bi * h + iy) * w + ix) * N +
                          (ky * 4 + kx) * KOUT;
#pragma unroll
        for (int ko = 0; ko < KOUT; ++ko) acc[ko] += pp[ko];
      }
    }
    __bf16* op = out + i * ldo;
#pragma unroll
    for (int ko = 0; ko < KOUT; ++ko) op[ko] = (__bf16)acc[ko];
  }
}

// C <= 16: x through element strides (sb, sc, sh, sw); w (C, KOUT, 4, 4)
template <int KOUT>
__global__ void tconv_direct_kernel(const __bf16* __restrict__ x,
                                    const __bf16* __restrict__ wgt,
                                    const __bf16* __restrict__ bias,
                                    __bf16* __restrict__ out, int b, int c,
                                    int h, int w, long long sb, long long sc,
                                    long long sh, long long sw, int ldo) {
  const int oh = 2 * h, ow = 2 * w;
  const long long total = (long long)b * oh * ow;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    const long long t = i / ow;
    const int oy = (int)(t % oh);
    const int bi = (int)(t / oh);
    int ky0, iy0, kx0, ix0;
    tconv_taps(oy, ky0, iy0);
    tconv_taps(ox, kx0, ix0);
    float acc[KOUT];
#pragma unroll
    for (int ko = 0; ko < KOUT; ++ko)
      acc[ko] = bias ? (float)bias[ko] : 0.f;
#pragma unroll
    for (int ty = 0; ty < 2; ++ty) {
      const int iy = iy0 - ty, ky = ky0 + 2 * ty;
      if (iy < 0 || iy >= h) continue;
#pragma unroll
      for (int tx = 0; tx < 2; ++tx) {
        const int ix = ix0 - tx, kx = kx0 + 2 * tx;
        if (ix < 0 || ix >= w) continue;
        const __bf16* xp = x + bi * sb + iy * sh + ix * sw;
        for (int ci = 0; ci < c; ++ci) {
          const float xv = (float)xp[ci * sc];
          const __bf16* wq = wgt + (ci * KOUT) * 16 + ky * 4 + kx;
#pragma unroll
          for (int ko = 0; ko < KOUT; ++ko)
            acc[ko] += xv * (float)wq[ko * 16];
        }
      }
    }
    __bf16* op = out + i * ldo;
#pragma unroll
    for (int ko = 0; ko < KOUT; ++ko) op[ko] = (__bf16)acc[ko];
  }
}

int stream_grid(long long total, int block) {
  return (int)min((total + block - 1) / block, (long long)8192);
}

}  // namespace

extern "C" {

// bytes of dynamic LDS tconv_p_kernel needs for c input channels
long long vfa_tconv_lds_bytes(int c, int kout) {
  return (long long)16 * kout * ((c + 31) / 32 * 32 + 8) * 2;
}

// x: first element of the input slice (pixel stride ldx, c % 8 == 0);
// wp: (16*kout, c) packed bf16; part: (b*h*w, 16*kout) f32 workspace;
// out: first element of the output slice (pixel stride ldo)
void vfa_tconv_pform(const void* x, const void* wp, const void* bias,
                     void* part, void* out, int b, int h, int w, int c,
                     int ldx, int kout, int ldo, hipStream_t stream) {
  const long long m = (long long)b * h * w;
  const int m_blocks = (int)min((m + 127) / 128, 1024LL);
  const size_t lds = (size_t)vfa_tconv_lds_bytes(c, kout);
  const int gg = stream_grid(m * 4, 256);
  if (kout == 1) {
    hipLaunchKernelGGL((tconv_p_kernel<1>), dim3(m_blocks), dim3(256), lds,
                       stream, (const __bf16*)x, (const __bf16*)wp,
                       (float*)part, m, c, ldx);
    hipLaunchKernelGGL((tconv_gather_kernel<1>), dim3(gg), dim3(256), 0,
                       stream, (const float*)part, (const __bf16*)bias,
                       (__bf16*)out, b, h, w, ldo);
  } else {
    hipLaunchKernelGGL((tconv_p_kernel<2>), dim3(m_blocks), dim3(256), lds,
                       stream, (const __bf16*)x, (const __bf16*)wp,
                       (float*)part, m, c, ldx);
    hipLaunchKernelGGL((tconv_gather_kernel<2>), dim3(gg), dim3(256), 0,
                       stream, (const float*)part, (const __bf16*)bias,
                       (__bf16*)out, b, h, w, ldo);
  }
}

void vfa_tconv_direct(const void* x, const void* wgt, const void* bias,
                      void* out, int b, int c, int h, int w, long long sb,
                      long long sc, long long sh, long long sw, int kout,
                      int ldo, hipStream_t stream) {
  const int gg = stream_grid((long long)b * h * w * 4, 256);
  if (kout == 1)
    hipLaunchKernelGGL((tconv_direct_kernel<1>), dim3(gg), dim3(256), 0,
                       stream, (const __bf16*)x, (const __bf16*)wgt,
                       (const __bf16*)bias, (__bf16*)out, b, c, h, w, sb, sc,
                       sh, sw, ldo);
  else
    hipLaunchKernelGGL((tconv_direct_kernel<2>), dim3(gg), dim3(256), 0,
                       stream, (const __bf16*)x, (const __bf16*)wgt,
                       (const __bf16*)bias, (__bf16*)out, b, c, h, w, sb, sc,
                       sh, sw, ldo);
}

}  // extern "C"
