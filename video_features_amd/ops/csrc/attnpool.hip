// CLIP ModifiedResNet attention pool (AttentionPool2d) for gfx950, bf16.
//
// attnpool_tokens: the trunk output x (B, HW, C) — a free view of the
// channels_last map — becomes the pool's token matrix t (B, HW+1, C):
//   t[b, 0]     = mean_j x[b, j] + pos[0]      (mean in f32)
//   t[b, 1 + j] = x[b, j]        + pos[1 + j]
// in ONE read of x and ONE write of t (replaces eager mean + cat + add and
// a layout copy).  One thread owns 8 channels of one image and walks the HW
// positions: every load/store is 16 B, consecutive lanes are consecutive in
// memory, each value is rounded to bf16 once.  Requires C % 8 == 0.
//
// attention_pool: single-query multi-head attention.  q (B, C) is the
// projection of token 0 only; kv (B, L, 2C) is packed [k | v] exactly as
// one GEMM with the concatenated [k_proj; v_proj] weight writes it.
//   o[b, h] = softmax_j(q_h . k_jh / sqrt(d)) . v_jh,   d = 64
// One wave per (b, h); 8 lanes share a key, each with one 16-B segment of
// its 128-B head slice, so every K and V load is 16 B and a wave instruction
// covers 8 whole keys.  Scores: 8-element partial dots summed over the 8
// segment lanes.  PV: each lane accumulates its 8 output dims over its key
// group's keys; the 8 groups are summed once at the end and lanes 0-7 write
// 16 B each.  All arithmetic in f32, softmax max-subtracted, one rounding;
// keys are consumed in 64-key chunks with an online rescale, so any L >= 1
// works (the towers use 50, 82, 145).  L == 1 returns V's values exactly
// (p = 1, denom = 1, the other groups add zeros).
#include "vfa_common.h"

namespace {

__global__ void attnpool_tokens_kernel(const uint4* __restrict__ x,
                                       const uint4* __restrict__ pos,
                                       uint4* __restrict__ t, long long b,
                                       int hw, int c8) {
  const long long total = b * c8;
  const float inv = 1.f / (float)hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long bi = i / c8;
    const int ci = (int)(i % c8);
    const uint4* xb = x + bi * hw * c8 + ci;
    uint4* tb = t + bi * (hw + 1) * c8 + ci;
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < hw; ++j) {
      float xv[8], pv[8];
      bf16x8_to_f32(xb[(long long)j * c8], xv);
      bf16x8_to_f32(pos[(long long)(j + 1) * c8 + ci], pv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sum[e] += xv[e];
        xv[e] += pv[e];
      }
      tb[(long long)(j + 1) * c8] = f32_to_bf16x8(xv);
    }
    float pv[8];
    bf16x8_to_f32(pos[ci], pv);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = sum[e] * inv + pv[e];
    tb[0] = f32_to_bf16x8(sum);
  }
}

// 4 waves per block, one (b, h) pair per wave; no LDS, no barrier (waves
// past the last pair simply exit).  Lane = (key group g = lane >> 3, 16-B
// segment sg = lane & 7): round r of a 64-key chunk reads keys c0 + 8r + g,
// 8 keys x 128 B per wave instruction, and all 8 rounds of K and of V are
// issued before the first use.
__global__ __launch_bounds__(256) void attention_pool_d64_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ kv,
    __hip_bfloat16* __restrict__ out, long long bh, int heads, int l,
    float scale) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 3, sg = lane & 7;
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= bh) return;
  const long long bi = pair / heads;
  const int h = (int)(pair % heads);
  const long long c = (long long)heads * 64;
  // this lane's 8 dims of the (pre-scaled) query head
  float qf[8];
  bf16x8_to_f32(
      *reinterpret_cast<const uint4*>(q + bi * c + h * 64 + sg * 8), qf);
#pragma unroll
  for (int e = 0; e < 8; ++e) qf[e] *= scale;
  // k of key 0, this lane's segment; v sits c elements further
  const __hip_bfloat16* kb = kv + bi * l * 2 * c + h * 64 + sg * 8;
  float m = -INFINITY, denom = 0.f;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < l; c0 += 64) {
    uint4 kr[8], vr[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j = c0 + 8 * r + g;
      kr[r] = vr[r] = uint4{0u, 0u, 0u, 0u};
      if (j < l) {
        const __hip_bfloat16* kp = kb + (long long)j * 2 * c;
        kr[r] = *reinterpret_cast<const uint4*>(kp);
        vr[r] = *reinterpret_cast<const uint4*>(kp + c);
      }
    }
    // scores: 8-element partial dot, summed over the 8 segment lanes
    float s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      float kf[8];
      bf16x8_to_f32(kr[r], kf);
      float dot = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) dot += qf[e] * kf[e];
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) dot += __shfl_xor(dot, off, 64);
      s[r] = (c0 + 8 * r + g < l) ? dot : -INFINITY;
      mx = fmaxf(mx, s[r]);
    }
    // max and sum over the key groups (the 8 lanes of a group agree)
#pragma unroll
    for (int off = 8; off < 64; off <<= 1)
      mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float m_new = fmaxf(m, mx);      // finite: key c0 is valid
    const float alpha = __expf(m - m_new); // 0 on chunk 0
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float p = __expf(s[r] - m_new);            // 0 for a padded key
      psum += p;
      float vf[8];
      bf16x8_to_f32(vr[r], vf);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += p * vf[e];
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) psum += __shfl_xor(psum, off, 64);
    denom = denom * alpha + psum;
    m = m_new;
  }
  // sum the key groups' partial outputs; lanes 0-7 hold segment sg
#pragma unroll
  for (int e = 0; e < 8; ++e) {
#pragma unroll
    for (int off = 8; off < 64; off <<= 1)
      acc[e] += __shfl_xor(acc[e], off, 64);
    acc[e] /= denom;
  }
  if (g == 0)
    *reinterpret_cast<uint4*>(out + bi * c + h * 64 + sg * 8) =
        f32_to_bf16x8(acc);
}

}  // namespace

extern "C" {

void vfa_attnpool_tokens(const void* x, const void* pos, void* t, long long b,
                         int hw, int c, hipStream_t stream) {
  const long long total = b * (c / 8);
  if (total <= 0) return;
  // 64-thread blocks: B*C/8 items is small (16k at B=64, C=2048), spread
  // them over the CUs
  const int grid = (int)min((total + 63) / 64, (long long)2048);
  hipLaunchKernelGGL(attnpool_tokens_kernel, dim3(grid), dim3(64), 0, stream,
                     (const uint4*)x, (const uint4*)pos, (uint4*)t, b, hw,
                     c / 8);
}

void vfa_attention_pool_d64(const void* q, const void* kv, void* out,
                            long long b, int heads, int l, float scale,
                            hipStream_t stream) {
  const long long bh = b * heads;
  if (bh <= 0) return;
  const long long grid = (bh + 3) / 4;
  hipLaunchKernelGGL(attention_pool_d64_kernel, dim3((unsigned)grid),
                     dim3(256), 0, stream, (const __hip_bfloat16*)q,
                     (const __hip_bfloat16*)kv, (__hip_bfloat16*)out, bh,
                     heads, l, scale);
}

}  // extern "C"
