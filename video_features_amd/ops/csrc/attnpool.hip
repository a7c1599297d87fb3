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
// One wave per (b, h).  Scores: lane <-> key, each lane reads its key's
// 128-B head slice as 8 x 16-B loads.  Max / sum cross the wave with
// shuffles.  PV: lane <-> output dim, keys looped, so each key's V slice is
// one coalesced 128-B read.  All arithmetic in f32, softmax max-subtracted;
// keys are consumed in 64-key chunks with an online rescale, so any L >= 1
// works (the towers use 50, 82, 145).
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
// past the last pair simply exit).
__global__ __launch_bounds__(256) void attention_pool_d64_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ kv,
    __hip_bfloat16* __restrict__ out, long long bh, int heads, int l,
    float scale) {
  const int lane = threadIdx.x & 63;
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= bh) return;
  const long long bi = pair / heads;
  const int h = (int)(pair % heads);
  const long long c = (long long)heads * 64;
  // every lane holds the whole (pre-scaled) query head: same address across
  // the wave, served as a broadcast
  float qf[64];
  {
    const uint4* qp = reinterpret_cast<const uint4*>(q + bi * c + h * 64);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      bf16x8_to_f32(qp[s], qf + 8 * s);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[8 * s + e] *= scale;
    }
  }
  const __hip_bfloat16* kb = kv + bi * l * 2 * c + h * 64;   // k of key 0
  const __hip_bfloat16* vb = kb + c;                         // v of key 0
  float m = -INFINITY, denom = 0.f, acc = 0.f;
  for (int c0 = 0; c0 < l; c0 += 64) {
    const int nk = min(64, l - c0);          // wave-uniform, >= 1
    const int j = c0 + lane;
    float s = -INFINITY;
    if (j < l) {
      const uint4* kp =
          reinterpret_cast<const uint4*>(kb + (long long)j * 2 * c);
      float dot = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float kf[8];
        bf16x8_to_f32(kp[u], kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot += qf[8 * u + e] * kf[e];
      }
      s = dot;
    }
    const float m_new = fmaxf(m, wave_allreduce_max(s));   // finite: nk >= 1
    const float p = (j < l) ? __expf(s - m_new) : 0.f;
    const float alpha = __expf(m - m_new);                 // 0 on chunk 0
    denom = denom * alpha + wave_allreduce_sum(p);
    acc *= alpha;
    const __hip_bfloat16* vp = vb + (long long)c0 * 2 * c + lane;
    for (int jj = 0; jj < nk; ++jj) {
      const float pj = __shfl(p, jj, 64);
      acc += pj * __bfloat162float(vp[(long long)jj * 2 * c]);
    }
    m = m_new;
  }
  out[bi * c + h * 64 + lane] = __float2bfloat16(acc / denom);
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
