// Fused frame preprocessing for gfx950: (T, H, W, 3) uint8 RGB ->
// (T, 3, H, W) normalized bf16/f32 planes in ONE pass (replaces the eager
// permute -> cast -> div -> sub -> div chain, 5 kernels and 3x the traffic).
// Each thread handles 4 pixels: 3 dword loads (12 B), 3 x 8 B plane writes.
// Also patchify, the patch gather in front of a ViT's patch-embedding GEMM.
#include "vfa_common.h"
#include <type_traits>

namespace {

template <typename T>
__global__ void u8_chw_norm_kernel(const unsigned char* __restrict__ in,
                                   T* __restrict__ out, long long t, int h,
                                   int w, float m0, float m1, float m2,
                                   float s0, float s1, float s2) {
  const long long hw = (long long)h * w;
  const long long quads_per_img = hw / 4;
  const long long total = t * quads_per_img;
  const float inv255 = 1.0f / 255.0f;
  const float im[3] = {m0, m1, m2};
  const float is[3] = {1.0f / s0, 1.0f / s1, 1.0f / s2};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long ti = i / quads_per_img;
    const long long q = i % quads_per_img;          // 4-pixel group in image
    const unsigned char* src = in + (ti * hw + q * 4) * 3;   // 12 bytes
    const uint3 raw = *reinterpret_cast<const uint3*>(src);
    unsigned char px[12];
    *reinterpret_cast<uint3*>(px) = raw;
    T planes[3][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = (float)px[p * 3 + c] * inv255;
        planes[c][p] = from_f32<T>((v - im[c]) * is[c]);
      }
    }
    // 4 elements per plane write: 8 B (bf16/f16) or 16 B (f32)
    using VecElt =
        typename std::conditional<sizeof(T) == 2, unsigned short, unsigned>::type;
    using Vec = __attribute__((ext_vector_type(4))) VecElt;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T* dst = out + (ti * 3 + c) * hw + q * 4;
      *reinterpret_cast<Vec*>(dst) = *reinterpret_cast<Vec*>(planes[c]);
    }
  }
}

// patchify: (T, C, H, W) -> (T, gy*gx, C*p*p), the A matrix of a
// stride == kernel conv run as a GEMM; K order (c, py, px), patch order
// (gy, gx).  Pure data movement in 16-B units (p*itemsize % 16 == 0), one
// pass.  A thread owns ONE 16-B unit of the destination frame — unit u of
// the frame is written at u, so a wave's stores are 1 KiB contiguous — and
// walks the frames (blockIdx.y, stride gridDim.y): the index split into
// (gy, gx, c, py, segment) is done once per thread, and four frames' loads
// are in flight before the first store.  Reads are runs of p elements.
__global__ __launch_bounds__(256) void patchify_kernel(
    const uint4* __restrict__ in, uint4* __restrict__ out, int t, unsigned c,
    unsigned h, unsigned p, unsigned gx, unsigned segs,
    unsigned frame_units) {
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= frame_units) return;
  const unsigned seg = u % segs;        // 16-B unit inside the p-element run
  unsigned r = u / segs;
  const unsigned py = r % p;
  r /= p;
  const unsigned ci = r % c;
  r /= c;
  const unsigned gxi = r % gx, gyi = r / gx;
  // source unit inside the frame: a row of W is gx*segs units
  const unsigned src =
      (ci * h + gyi * p + py) * (gx * segs) + gxi * segs + seg;
  const uint4* ip = in + src;
  uint4* op = out + u;
  const long long fs = frame_units;
  const int step = gridDim.y;
  int ti = blockIdx.y;
  for (; ti + 3 * step < t; ti += 4 * step) {
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ip[(ti + (long long)i * step) * fs];
#pragma unroll
    for (int i = 0; i < 4; ++i) op[(ti + (long long)i * step) * fs] = v[i];
  }
  for (; ti < t; ti += step) op[ti * fs] = ip[ti * fs];
}

}  // namespace

extern "C" void vfa_patchify(const void* in, void* out, long long t, int c,
                             int h, int w, int p, int itemsize,
                             hipStream_t stream) {
  const int v = 16 / itemsize;                    // elements per 16-B unit
  const long long frame_units = (long long)c * h * w / v;
  if (t <= 0 || frame_units <= 0) return;
  const unsigned bx = (unsigned)((frame_units + 255) / 256);
  // about 4096 blocks over the device, at most one frame row of them per
  // frame; grid.y <= 65535
  const long long want = (4096 + bx - 1) / bx;
  const unsigned by = (unsigned)max(1LL, min(min(t, want), 65535LL));
  hipLaunchKernelGGL(patchify_kernel, dim3(bx, by), dim3(256), 0, stream,
                     (const uint4*)in, (uint4*)out, (int)t, (unsigned)c,
                     (unsigned)h, (unsigned)p, (unsigned)(w / p),
                     (unsigned)(p / v), (unsigned)frame_units);
}

extern "C" void vfa_u8_chw_norm(const void* in, void* out, long long t,
                                int h, int w, const float* mean,
                                const float* std, int dtype,
                                hipStream_t stream) {
  long long total = t * ((long long)h * w / 4);
  int block = 256;
  int grid = (int)min((total + block - 1) / block, (long long)4096);
  if (dtype == VFA_BF16) {
    hipLaunchKernelGGL((u8_chw_norm_kernel<__hip_bfloat16>), dim3(grid),
                       dim3(block), 0, stream, (const unsigned char*)in,
                       (__hip_bfloat16*)out, t, h, w, mean[0], mean[1],
                       mean[2], std[0], std[1], std[2]);
  } else {
    hipLaunchKernelGGL((u8_chw_norm_kernel<float>), dim3(grid), dim3(block),
                       0, stream, (const unsigned char*)in, (float*)out, t, h,
                       w, mean[0], mean[1], mean[2], std[0], std[1], std[2]);
  }
}
