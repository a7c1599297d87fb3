// Fused MFMA linear kernel for gfx950:  C = act(A @ W^T + bias), bf16.
//
//   A (M, K) row-major, W (N, K) row-major (torch nn.Linear layout), both
//   bf16; C (M, N) bf16; f32 accumulation; bias + residual + activation
//   applied in the epilogue (QuickGELU / tanh-GELU / ReLU / LeakyReLU(0.1)
//   / none) — the separate activation kernel's full HBM round trip
//   disappears.
//
// Two more entry points run linear256p_kernel with a template mode of its
// epilogue, for linear -> (+ residual) -> LayerNorm -> linear chains without
// the LayerNorm pass: vfa_linear_res_stats (residual add + per-row
// statistics partials out) and vfa_linear_ln_act (LayerNorm folded into the
// weight, statistics partials in); see epilogue_strips.
//
// Kernels, in routing order (launch_linear):
//   linear_thin_kernel  M-huge / K-shallow streaming (W resident in LDS)
//   linear256p_kernel   256x256 full tiles, >= 150 of them: persistent
//                       tile walk, K pipeline continuous across tiles,
//                       shared vectorised epilogue (epilogue_strips)
//   linear8p_kernel     256x256 full tiles, 8-phase pipeline, same
//                       epilogue; act-none problems of 64..149 tiles
//   linear_act_kernel   everything else: 128x128 tiles, and the guarded
//                       256x256 tiles (ragged N column, ragged K)
//
// Structure (cdna_hip_programming.md §5): BIG tiles 256x256 (8 waves as
// 2M x 4N, 128x64 C per wave, 128 KiB LDS) for the transformer shapes,
// 128x128 (4 waves, 2x2) when N < 256 or M is small.  The tile machinery —
// LDS swizzle, glds / guarded staging, the K-step, the fragment-layout
// epilogue, the activation table — is mfma_tile.h, shared with
// conv2d.hip; this file holds the kernels' K loops and tile walks, the
// vectorised 256^2 epilogue and the routing.
#include "mfma_tile.h"
#include <cstdlib>

namespace {

// Shared full-tile epilogue of the two 256x256 kernels: one wave's 128x64
// f32 accumulator block (8x4 MFMA tiles) -> bias + residual + activation
// in f32 -> bf16, stored as row-contiguous 16-B vectors.
//
// The MFMA fragment layout gives a lane 4 rows x 1 column per tile, i.e.
// 2-byte stores where 16 lanes cover 32 contiguous bytes.  Each 16x64
// strip is instead bounced through a wave-private 4 KiB f32 LDS tile `ep`
// and read back as (row, 8 columns) per lane, so bias / residual / output
// are 16-B accesses on 128-B-contiguous rows and the arithmetic stays in
// f32 up to the single bf16 rounding.  The tile is [16][64] f32 with the
// 16-column group XORed by (row>>2)&3: the four hi4 lane groups of a
// fragment write then hit disjoint bank groups, and the read side's 8-col
// segments stay inside one group.  Wave-local only (lgkmcnt waits, no
// barrier), so it can run while another tile's glds is in flight.
//
// MODE selects what else the epilogue does (linear256p_kernel only):
//   EPI_STATS  after the bf16 rounding, the (mean, M2) of the row's 64
//              rounded outputs of this strip.  The 8 lanes lane & 7 hold
//              one row of the strip, so it is two 8-lane DPP reduces (sum,
//              then squares about the strip mean: safe for rows whose mean
//              dwarfs their spread).  The wave's 128 (mean, M2) pairs are
//              left in its bounce tile ep, as float2 [128]; the kernel
//              merges the four strips of a tile row and writes one partial
//              per (row, tile column) — one writer each, no atomics.
//   EPI_LN     the A rows are un-normalised LayerNorm inputs and W has
//              the LN affine folded in (ops.fold_ln_linear):
//              v = rstd * (acc - mean * c[col]) + b'[col], with c, b' f32
//              vectors; (mean, rstd) of a row come from merging its
//              x.groups partials, once per tile and row.  bias and res
//              are not used.
enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_LN = 2 };

struct EpiExtra {
  const float* ln_c;        // EPI_LN: c (N), row sums of the folded W
  const float* ln_b;        // EPI_LN: b' (N)
  const float2* stats;      // EPI_LN: (M, groups) of (group mean, M2)
  float2* part;             // EPI_STATS: (M, N/256) of (group mean, M2)
  int groups;               // EPI_LN: partials per row, K / groups wide each
  float eps;                // EPI_LN
};

// sum over the 8 lanes lane & 7 == 0..7, result in all of them: quad_perm
// [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ float sum8(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x),
                                           decltype(ctrl)::value, 0xf, 0xf,
                                           true));
  };
  v += dpp(v, std::integral_constant<int, 0xb1>{});
  v += dpp(v, std::integral_constant<int, 0x4e>{});
  v += dpp(v, std::integral_constant<int, 0x141>{});
  return v;
}

// the value of lane (lane & 7) == j to all 8 lanes of its group: broadcast
// inside the quads (quad_perm), then the quad that does not hold lane j
// takes the other quad's (row_half_mirror).  j is a constant after
// unrolling, so the switch folds.
__device__ __forceinline__ float bcast8(float v, int j, int l7) {
  const int i = __builtin_bit_cast(int, v);
  int b;
  switch (j & 3) {
    case 0: b = __builtin_amdgcn_update_dpp(0, i, 0x00, 0xf, 0xf, true); break;
    case 1: b = __builtin_amdgcn_update_dpp(0, i, 0x55, 0xf, 0xf, true); break;
    case 2: b = __builtin_amdgcn_update_dpp(0, i, 0xaa, 0xf, 0xf, true); break;
    default: b = __builtin_amdgcn_update_dpp(0, i, 0xff, 0xf, 0xf, true);
  }
  const int m = __builtin_amdgcn_update_dpp(0, b, 0x141, 0xf, 0xf, true);
  return __builtin_bit_cast(float, (l7 >> 2) == (j >> 2) ? b : m);
}

template <int ACT, bool HAS_RES, int MODE = EPI_PLAIN>
__device__ __forceinline__ void epilogue_strips(
    const f32x4 (&acc)[8][4], float* ep, const __bf16* __restrict__ bias,
    const __bf16* __restrict__ res, __bf16* __restrict__ c, int n,
    long long row0, int col0, int lane, const EpiExtra& x = EpiExtra{},
    int kdim = 0) {
  const int lo = lane & 15, hi4 = lane >> 4;
  const int ec = (lane & 7) * 8;
  const int col = col0 + ec;
  float bf[8], cf[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bf[e] = cf[e] = 0.f;
  // EPI_LN: 1 / groups and the group width
  const float gi = MODE == EPI_LN ? 1.f / (float)x.groups : 0.f;
  const float gw = MODE == EPI_LN ? (float)(kdim / x.groups) : 0.f;
  const int l7 = lane & 7;
  // a row's 8 lanes all hold its reduced (mean, M2); lane l7 keeps those
  // of the two (mi, p) steps with (mi * 2 + p) & 7 == l7
  float2 sp[2] = {float2{0.f, 0.f}, float2{0.f, 0.f}};
  // EPI_LN: the same distribution the other way round.  Lane l7 merges the
  // partials of the rows of those two steps into (mean, rstd) here, once
  // per tile — Chan's formula for equal-width groups, sums taken about the
  // first group's mean — and each step fetches its row's pair with bcast8.
  float2 own[2] = {float2{0.f, 1.f}, float2{0.f, 1.f}};
  if (MODE == EPI_LN) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long r =
          row0 + h * 64 + (l7 >> 1) * 16 + (l7 & 1) * 8 + (lane >> 3);
      const float2* pp = x.stats + r * x.groups;
      const float m0 = pp[0].x;
      float q = pp[0].y, s1 = 0.f, s2 = 0.f;
      for (int i = 1; i < x.groups; ++i) {
        const float2 g = pp[i];
        const float d = g.x - m0;
        s1 += d;
        s2 = fmaf(d, d, s2);
        q += g.y;
      }
      const float m2 = fmaf(gw, s2 - s1 * s1 * gi, q);
      own[h] = float2{fmaf(s1, gi, m0), rsqrtf(fmaf(m2, gi / gw, x.eps))};
    }
  }
  if (MODE == EPI_LN) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(x.ln_b + col + h * 4);
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(x.ln_c + col + h * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf[h * 4 + e] = b4[e];
        cf[h * 4 + e] = c4[e];
      }
    }
  } else if (bias) {
    const bf16x8 b8 = *reinterpret_cast<const bf16x8*>(bias + col);
#pragma unroll
    for (int e = 0; e < 8; ++e) bf[e] = (float)b8[e];
  }
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ep[(hi4 * 4 + r) * 64 + (((jj ^ hi4) << 4) | lo)] = acc[mi][jj][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0), wave-local tile
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int er = p * 8 + (lane >> 3);
      const float* src = ep + er * 64 + (ec ^ (((er >> 2) & 3) << 4));
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 4);
      const long long row = row0 + mi * 16 + er;
      const long long o = row * n + col;
      bf16x8 rr8{};
      if (HAS_RES) rr8 = *reinterpret_cast<const bf16x8*>(res + o);
      float2 st{0.f, 1.f};                   // (mean, rstd) of the row
      if (MODE == EPI_LN) {
        st.x = bcast8(own[mi >> 2].x, (mi * 2 + p) & 7, l7);
        st.y = bcast8(own[mi >> 2].y, (mi * 2 + p) & 7, l7);
      }
      bf16x8 o8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = e < 4 ? v0[e & 3] : v1[e & 3];
        if (MODE == EPI_LN)
          v = fmaf(st.y, fmaf(-st.x, cf[e], v), bf[e]);
        else
          v += bf[e];
        if (HAS_RES) v += (float)rr8[e];
        o8[e] = (__bf16)act_f(v, ACT);
      }
      *reinterpret_cast<bf16x8*>(c + o) = o8;
      if (MODE == EPI_STATS) {
        // from the ROUNDED values: they are what the consumer's MFMAs sum
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (float)o8[e];
        const float mean = sum8(s) * (1.f / 64.f);
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = (float)o8[e] - mean;
          q = fmaf(d, d, q);
        }
        q = sum8(q);
        if (((mi * 2 + p) & 7) == l7) sp[mi >> 2] = float2{mean, q};
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);      // reads done before reuse
  }
  if (MODE == EPI_STATS) {
    // step (mi, p) is tile rows mi * 16 + p * 8 + (lane >> 3)
    float2* ep2 = reinterpret_cast<float2*>(ep) + (l7 >> 1) * 16 +
                  (l7 & 1) * 8 + (lane >> 3);
    ep2[0] = sp[0];
    ep2[64] = sp[1];
  }
}

// BIG: 256x256 tile, 8 waves (2Mx4N), 128x64 C per wave (8x4 MFMA tiles).
// else: 128x128 tile, 4 waves (2x2), 64x64 per wave (4x4 tiles).
template <int ACT, bool FULL, bool BIG>
__global__ __launch_bounds__(BIG ? 512 : 256)
void linear_act_kernel(const __bf16* __restrict__ a,
                       const __bf16* __restrict__ w,
                       const __bf16* __restrict__ bias,
                       const __bf16* __restrict__ res,
                       __bf16* __restrict__ c, int m, int n, int k,
                       int tiles_m, int tile_base) {
  constexpr int BM = BIG ? 256 : 128, BN = BIG ? 256 : 128;
  constexpr int WAVES = BIG ? 8 : 4;
  constexpr int WN = BIG ? 4 : 2;              // waves along N
  constexpr int MI = BIG ? 8 : 4;              // 16-row MFMA tiles per wave
  constexpr int NJ = 4;                        // 16-col MFMA tiles per wave
  constexpr int TILE_A = BM * BK * 2, TILE_BB = BN * BK * 2;
  constexpr int THREADS = BIG ? 512 : 256;

  extern __shared__ __attribute__((aligned(1024))) char smem[];
  auto sA = [&](int buf) { return smem + buf * (TILE_A + TILE_BB); };
  auto sB = [&](int buf) {
    return smem + buf * (TILE_A + TILE_BB) + TILE_A;
  };

  // the grid covers tiles tile_base .. tile_base + gridDim.x (tile id =
  // tile_n * tiles_m + tile_m); tile_base > 0 when the interior tiles of
  // the problem went to linear256p_kernel and only the edge column is here
  const int wg = tile_base + xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = wg / tiles_m, tile_m = wg % tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int nk = (k + BK - 1) / BK;
  const int valid_m = m - m0, valid_n = n - n0;
  // interior tiles take the glds fast path even when the problem has
  // edge tiles; FULL means k % BK == 0 (no ragged K-step anywhere)
  const bool tile_full = valid_m >= BM && valid_n >= BN;

  auto stage = [&](int buf, int kt) {
    const long long ko = (long long)kt * BK;
    if (tile_full && (FULL || kt + 1 < nk)) {
      stage_glds<BM, WAVES>(a + (long long)m0 * k + ko, k, sA(buf), wave,
                            lane);
      stage_glds<BN, WAVES>(w + (long long)n0 * k + ko, k, sB(buf), wave,
                            lane);
    } else {
      const int vk = (int)min((long long)BK, (long long)k - ko);
      stage_guard<BM, THREADS>(a + (long long)m0 * k + ko, k, valid_m, vk,
                               sA(buf), threadIdx.x);
      stage_guard<BN, THREADS>(w + (long long)n0 * k + ko, k, valid_n, vk,
                               sB(buf), threadIdx.x);
    }
  };

  stage(0, 0);

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                           // tile kt resident
    const int cur = kt & 1;
    const long long ko_nxt = (long long)(kt + 1) * BK;
    const bool glds_nxt =
        (kt + 1 < nk) && tile_full && (FULL || kt + 2 < nk);
    if ((kt + 1 < nk) && !glds_nxt) stage(1 - cur, kt + 1);
    // compute on tile kt; the next tile's glds issue is spread across the
    // two MFMA half-steps so the memory pipe overlaps the math instead of
    // bursting at the barrier (PMC: 39% of wave cycles were parked)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {           // two 32-deep MFMA steps
      mfma_kstep<MI, NJ>(sA(cur), sB(cur), wm * (MI * 16), wn * (NJ * 16),
                         kk, lane, acc, [&] {
        if (glds_nxt) {
          stage_glds_piece<BM, WAVES>(a + (long long)m0 * k + ko_nxt, k,
                                      sA(1 - cur), wave, lane, kk, 2);
          stage_glds_piece<BN, WAVES>(w + (long long)n0 * k + ko_nxt, k,
                                      sB(1 - cur), wave, lane, kk, 2);
        }
      });
    }
    // no trailing barrier: the next iteration's top __syncthreads() both
    // drains the in-flight glds and orders reads before buffer reuse
  }

  // fragment-layout epilogue, guards hoisted.  (The 256^2 hot path is
  // linear256p_kernel's epilogue; this one serves the small tile and the
  // edge / ragged-K tiles.)  BIG: edge column / ragged-K tiles only, at 256
  // VGPRs: splitting on the residual as well spills 8-12 registers, so
  // that test stays inside
  epilogue_frag_hoisted<ACT, MI, NJ, !BIG>(
      tile_full, acc, bias, res, c, m, n, n, m0 + wm * (MI * 16),
      n0 + wn * (NJ * 16), lane);
}

// ------------------------------------------------- persistent 256^2 tiles
// The full-tile (m0+256 <= m, n0+256 <= n, k % 64 == 0) hot path of the
// 2-buffer kernel above, as a persistent loop: min(tiles, CUs) blocks, each
// walking tiles blockIdx.x, +gridDim.x, ... through the XCD remap.  Same
// staging, swizzle and MFMA schedule; what changes is the tile boundary:
//  - the K pipeline never stops.  Buffer parity runs over a counter that
//    continues across tiles, so in a tile's LAST K-step the "next K-tile"
//    glds are simply the next tile's K-tile 0 (into the buffer every wave
//    left at the previous barrier — the same ordering argument as inside
//    a tile).  The first-load latency of tile t+1 is hidden behind tile
//    t's last MFMAs and its epilogue instead of being exposed per tile;
//  - the epilogue (epilogue_strips) bounces through its own 32 KiB LDS
//    region beside the 128 KiB of staging, wave-local, no barrier — so it
//    neither touches the buffers the prefetch is landing in nor drains it.
//    The next tile's first __syncthreads() does the vmcnt(0) drain.
// No grid-wide synchronisation: blocks are independent, co-residency is
// not assumed, graph capture is unaffected.
template <int ACT, int MODE = EPI_PLAIN>
__global__ __launch_bounds__(512, 1)
void linear256p_kernel(const __bf16* __restrict__ a,
                       const __bf16* __restrict__ w,
                       const __bf16* __restrict__ bias,
                       const __bf16* __restrict__ res,
                       __bf16* __restrict__ c, int n, int k, int tiles_m,
                       int ntiles, EpiExtra x) {
  constexpr int TILE = 256 * BK * 2;           // one operand, one K-tile
  extern __shared__ __attribute__((aligned(1024))) char smem_p[];
  auto sA = [&](int buf) { return smem_p + buf * (2 * TILE); };
  auto sB = [&](int buf) { return smem_p + buf * (2 * TILE) + TILE; };

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  float* ep = reinterpret_cast<float*>(smem_p + 4 * TILE) + wave * (16 * 64);

  const int nk = k / BK;
  int v = blockIdx.x;                          // virtual block id
  int wg = xcd_remap(v, ntiles);
  int m0 = (wg % tiles_m) * 256, n0 = (wg / tiles_m) * 256;
  const __bf16* ap = a + (long long)m0 * k;
  const __bf16* wp = w + (long long)n0 * k;

  stage_glds<256, 8>(ap, k, sA(0), wave, lane);
  stage_glds<256, 8>(wp, k, sB(0), wave, lane);

  int it = 0;                                  // K-steps done, all tiles
  for (;;) {
    const int vn = v + gridDim.x;
    const bool more = vn < ntiles;
    int m0n = m0, n0n = n0;
    if (more) {
      const int wgn = xcd_remap(vn, ntiles);
      m0n = (wgn % tiles_m) * 256;
      n0n = (wgn / tiles_m) * 256;
    }
    const __bf16* apn = a + (long long)m0n * k;
    const __bf16* wpn = w + (long long)n0n * k;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nk; ++kt, ++it) {
      __syncthreads();                         // K-tile resident, drained
      const int cur = it & 1;
      const bool last = kt + 1 == nk;
      // what the other buffer gets: this tile's next K-tile, or — in the
      // last K-step — the next tile's first
      const __bf16* an = last ? apn : ap + (long long)(kt + 1) * BK;
      const __bf16* wn_ = last ? wpn : wp + (long long)(kt + 1) * BK;
      const bool issue = !last || more;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {         // two 32-deep MFMA steps
        mfma_kstep<8, 4>(sA(cur), sB(cur), wm * 128, wn * 64, kk, lane, acc,
                         [&] {
          if (issue) {
            stage_glds_piece<256, 8>(an, k, sA(1 - cur), wave, lane, kk, 2);
            stage_glds_piece<256, 8>(wn_, k, sB(1 - cur), wave, lane, kk, 2);
          }
        });
      }
    }

    const long long row0 = m0 + wm * 128;
    const int col0 = n0 + wn * 64;
    if (MODE == EPI_LN)          // no bias / residual operand in this mode
      epilogue_strips<ACT, false, MODE>(acc, ep, nullptr, nullptr, c, n,
                                        row0, col0, lane, x, k);
    else if (res)
      epilogue_strips<ACT, true, MODE>(acc, ep, bias, res, c, n, row0, col0,
                                       lane, x);
    else
      epilogue_strips<ACT, false, MODE>(acc, ep, bias, res, c, n, row0,
                                        col0, lane, x);
    if (MODE == EPI_STATS) {
      // the four waves wn of a wave row hold the four 64-column strips of
      // the tile's rows: merge them (equal counts: mean of the means, M2 =
      // sum M2_i + 64 * sum (mean_i - mean)^2) into the one partial this
      // tile owns per row.  LDS only, so the wait is lgkmcnt and the next
      // tile's prefetch stays in flight; the bounce tiles are written again
      // only after the next tile's K loop and its barriers.
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_s_barrier();
      if (threadIdx.x < 256) {
        const float2* b2 =
            reinterpret_cast<const float2*>(smem_p + 4 * TILE) +
            (threadIdx.x >> 7) * 4 * 512 + (threadIdx.x & 127);
        float2 g[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = b2[i * 512];
        const float mean = 0.25f * ((g[0].x + g[1].x) + (g[2].x + g[3].x));
        float m2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = g[i].x - mean;
          m2 += fmaf(64.f * d, d, g[i].y);
        }
        x.part[(long long)(m0 + (int)threadIdx.x) * (n >> 8) + (n0 >> 8)] =
            float2{mean, m2};
      }
    }
    if (!more) break;
    v = vn; m0 = m0n; n0 = n0n; ap = apn; wp = wpn;
  }
}

// --------------------------------------------------- deep-pipelined 256^2
// The 8-phase 256x256 structure (cdna_hip_programming.md §5 template): one
// phase per C-quadrant, 16 MFMA per phase, TWO glds per phase, raw
// s_barrier with a counted vmcnt(6) — staged loads stay in flight ACROSS
// barriers (the plain-__syncthreads 2-buffer loop drains vmcnt(0) at every
// barrier; that stall was ~20% per the guide).
//
// Provably-correct schedule with uniform 2 glds/phase:
//  - A ring: 2 tiles x 4 quadrant blocks of 8 KiB.  Block q holds the 64
//    rows quadrant q reads (rows q*32..+32 and 128+q*32..+32).  A(T+1, q)
//    is staged at phase (T, q) -> stage-to-use distance EXACTLY 4 phases.
//  - B ring: 3 tiles x 4 quarter blocks of 8 KiB (quarter h = tile cols
//    h*64..+64 = wave wn=h's fragment rows).  B(T+2, q) staged at phase
//    (T, q) -> distance 5..8 phases.
//  - vmcnt(6) leaves at most the newest 3 phases' stages (2 glds each) in
//    flight, so anything >= 4 phases old has landed.  Past the end of K
//    the stages keep issuing into dead blocks (source redirected to tile
//    0) so the rate stays uniform and the invariant holds at ramp-down.
// FULL tiles only (m%256==0, n%256==0, k%64==0) — no edge guards anywhere.
template <int ACT>
__global__ __launch_bounds__(512, 1)
void linear8p_kernel(const __bf16* __restrict__ a,
                     const __bf16* __restrict__ w,
                     const __bf16* __restrict__ bias,
                     const __bf16* __restrict__ res,
                     __bf16* __restrict__ c, int m, int n, int k,
                     int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(1024))) char smem8[];
  const int nk = k >> 6;

  const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tile_n = wg / tiles_m, tile_m = wg % tiles_m;
  const int m0 = tile_m * 256, n0 = tile_n * 256;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi4 = lane >> 4;
  const int wm = wave >> 2, wn = wave & 3;

  auto LA = [&](int t, int q) { return smem8 + (t * 4 + q) * 8192; };
  auto LB = [&](int t, int h) {
    return smem8 + 65536 + (t * 4 + h) * 8192;
  };

  // per-wave glds geometry: each wave writes 1 KiB of an 8 KiB block
  // (lane-linear dest); the st_16x32 swizzle rides the SOURCE address
  const int off = (wave * 1024 + lane * 16);
  const int off_log = swz(off);
  const int rib = off_log >> 7;            // row in block (0..63)
  const int kfrac = (off_log & 127) >> 1;  // k elems within the K-tile

  // A: block q, row-in-block rib -> global row
  const int a_row_off = rib < 32 ? rib : 96 + rib;  // +128-32 for wm=1 half
  auto stage_a = [&](int T, int q) {
    // beyond-K stages read tile 0 into the dead block (rate uniformity)
    const int kt = T < nk ? T : 0;
    const __bf16* src =
        a + (long long)(m0 + q * 32 + a_row_off) * k + kt * 64 + kfrac;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(src),
        reinterpret_cast<unsigned int*>(LA(T & 1, q) + wave * 1024), 16, 0,
        0);
  };
  auto stage_b = [&](int T, int h) {
    const int kt = T < nk ? T : 0;
    const __bf16* src =
        w + (long long)(n0 + h * 64 + rib) * k + kt * 64 + kfrac;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(src),
        reinterpret_cast<unsigned int*>(LB(T % 3, h) + wave * 1024), 16, 0,
        0);
  };

  // prologue: A(0).q0-3, B(0).h0-3, B(1).h0-3 — 12 glds per wave; wait
  // the first 8 (A0 + B0), leave B1 in flight
  for (int q = 0; q < 4; ++q) stage_a(0, q);
  for (int h = 0; h < 4; ++h) stage_b(0, h);
  for (int h = 0; h < 4; ++h) stage_b(1, h);
  // s_waitcnt imm: vmcnt [3:0]+[15:14], expcnt [6:4], lgkmcnt [13:8]
  __builtin_amdgcn_s_waitcnt(0x3f74);      // vmcnt(4) only
  __builtin_amdgcn_s_barrier();

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int T = 0; T < nk; ++T) {
    char* la_t = LA(T & 1, 0);
    char* lb_t = LB(T % 3, wn);
    // B fragments are quadrant-invariant: read ONCE per K-tile (phase 0)
    // and hold in registers — halves the LDS read traffic per tile
    bf16x8 bfr[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {            // one C-quadrant per phase
      if (q == 0) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int brow = j * 16 + lo;
            bfr[j][kk] = *reinterpret_cast<const bf16x8*>(
                lb_t + swz(brow * 128 + kk * 64 + hi4 * 16));
          }
      }
      bf16x8 afr[2][2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int mi2 = 0; mi2 < 2; ++mi2) {
          const int arow = wm * 32 + mi2 * 16 + lo;
          afr[mi2][kk] = *reinterpret_cast<const bf16x8*>(
              la_t + q * 8192 + swz(arow * 128 + kk * 64 + hi4 * 16));
        }
      // vmcnt(4): stages issue MID-phase (between the MFMA halves below),
      // so leaving 2 phases' stages (4 loads) in flight guarantees the
      // 3-phase-old stage — and A's stage-to-use distance is 4
      __builtin_amdgcn_s_waitcnt(0x3f74);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi2 = 0; mi2 < 2; ++mi2)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[q * 2 + mi2][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr[mi2][0], bfr[j][0], acc[q * 2 + mi2][j], 0, 0, 0);
      // the fine interleave: issue this phase's 2 glds between the MFMA
      // halves so the memory pipe overlaps the math (§5.5: the per-phase
      // interleave is the lever; a coarse phase-split HURTS)
      stage_a(T + 1, q);
      stage_b(T + 2, q);
#pragma unroll
      for (int mi2 = 0; mi2 < 2; ++mi2)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[q * 2 + mi2][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afr[mi2][1], bfr[j][1], acc[q * 2 + mi2][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();          // phase lockstep
    }
  }

  // epilogue: the shared f32 LDS bounce (epilogue_strips), here inside the
  // dead staging rings.  __syncthreads drains the dummy glds in flight.
  __syncthreads();
  float* ep = reinterpret_cast<float*>(smem8) + wave * (16 * 64);
  const long long row0 = m0 + wm * 128;
  const int col0 = n0 + wn * 64;
  if (res)
    epilogue_strips<ACT, true>(acc, ep, bias, res, c, n, row0, col0, lane);
  else
    epilogue_strips<ACT, false>(acc, ep, bias, res, c, n, row0, col0, lane);
}

// caller: vfa_linear_route said VFA_ROUTE_8P (full tiles, k / 64 >= 3, at
// least 64 tiles)
template <int ACT>
void launch_8p(const void* a, const void* w, const void* bias,
               const void* res, void* c, int m, int n, int k,
               hipStream_t stream) {
  const long long tiles = (long long)(m / 256) * (n / 256);
  static bool attr_set[5] = {};
  if (!attr_set[ACT]) {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&linear8p_kernel<ACT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set[ACT] = true;
  }
  hipLaunchKernelGGL((linear8p_kernel<ACT>), dim3((unsigned)tiles),
                     dim3(512), 160 * 1024, stream, (const __bf16*)a,
                     (const __bf16*)w, (const __bf16*)bias,
                     (const __bf16*)res, (__bf16*)c, m, n, k, m / 256,
                     n / 256);
}

// ------------------------------------------------------- thin-K streaming
// M-huge / K-shallow GEMMs (the ResNet/I3D 1x1 convs as GEMM: M = B*H*W up
// to ~1.2M rows, K = 64..256) are HBM-streaming problems: the tiled
// double-buffered kernel above degenerates to a 1-iteration K-loop and
// runs ~2x off the bandwidth floor (profiles/, round 2).  This kernel
// keeps W resident in LDS (loaded once per block), streams A directly
// global -> MFMA fragments (A is read ONCE for all N columns), grid-strides
// over M, and has no per-K barriers.  vgpr budget: A frags 2*K/32*4 +
// B frags K/32*4 + acc 8 -> ~130 at K=256 (2 blocks/CU).
constexpr int THIN_ET_BYTES = 8 * 64 * 4;    // one wave's f32 epilogue tile

template <int ACT, int KF>
__global__ __launch_bounds__(256, 2)
void linear_thin_kernel(const __bf16* __restrict__ a,
                        const __bf16* __restrict__ w,
                        const __bf16* __restrict__ bias,
                        const __bf16* __restrict__ res,
                        __bf16* __restrict__ c, int m, int n, int nch,
                        int k) {
  // grid: (m_blocks, n_outer); block 256 = 4 waves, each wave 32 rows.
  // KF = ceil(K/32) is COMPILE-TIME: runtime-indexed ext_vector arrays go
  // to scratch (cdna_hip_programming.md §5.4 rule 20 — the first version
  // of this kernel hit exactly that: 4 TF/s from scratch traffic).
  // K itself may be any multiple of 8 (the R21D temporal 1x1 convs have
  // K = mid-planes like 144/232): each lane's last A fragment is either
  // fully valid or fully masked to zero (8-elem granularity), and the W
  // LDS rows are zero-filled up to the KC boundary.
  constexpr int KC = KF * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi4 = lane >> 4;

  // LDS layout: W chunk (rows of KC+8 elems, breaks the ds_read bank
  // pattern; K..KC zero-filled) + per-wave 8x64 f32 epilogue tiles
  // (THIN_ET_BYTES each).  The tiles hold f32 accumulators, so bias,
  // residual and activation are applied in f32 and the result is rounded
  // to bf16 once, as in epilogue_strips.  8 rows, not that one's 16: the
  // four tiles (8 KiB) then take no more LDS than the bf16 tiles they
  // replace and the N-chunk stays what it was.  A 16-row MFMA tile goes
  // through in two passes q of 8 rows, hi4 * 4 + q * 2 + {0, 1} (a lane
  // holds rows hi4 * 4 + 0..3, so every lane writes in both passes).
  // Tile row t = hi4 * 2 + {0, 1}; with b = (t >> 1) & 1, column c sits at
  // c ^ b * 20: the 16 of it puts the two hi4 lane groups of a 32-lane
  // ds_write_b32 group on disjoint halves of the 32 banks; the 4 of it
  // swaps the 16-B halves of an 8-column segment on tile rows 2, 3 (mod
  // 4), so the 16 lanes a ds_read_b128 serves at a time -- 4 segments on
  // each of 4 consecutive rows, all at the same offset mod 64 banks --
  // cover the 64 banks exactly once.
  extern __shared__ __attribute__((aligned(16))) char smem_t[];
  __bf16* wl = reinterpret_cast<__bf16*>(smem_t);
  constexpr int LDW = KC + 8;
  const int n0 = blockIdx.y * nch;
  const int ncols = min(nch, n - n0);
  float* et = reinterpret_cast<float*>(smem_t + (size_t)nch * LDW * 2) +
              wave * (THIN_ET_BYTES / 4);
  for (int t = threadIdx.x; t < ncols * (KC / 8); t += 256) {
    const int row = t / (KC / 8), seg = t % (KC / 8);
    uint4 v = {0u, 0u, 0u, 0u};
    if (seg * 8 < k)
      v = *reinterpret_cast<const uint4*>(w + (long long)(n0 + row) * k +
                                          seg * 8);
    *reinterpret_cast<uint4*>(wl + row * LDW + seg * 8) = v;
  }
  __syncthreads();

  const long long mstep = (long long)gridDim.x * 128;
  for (long long m0 = (long long)blockIdx.x * 128; m0 < m; m0 += mstep) {
    const long long r0 = m0 + wave * 32;
    // A fragments for this wave's 32 rows (2 x 16), K resident in regs
    bf16x8 afr[2][KF];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      long long row = r0 + mi * 16 + lo;
      if (row >= m) row = m - 1;               // clamped load, masked store
      const __bf16* ap = a + row * k + hi4 * 8;
#pragma unroll
      for (int kk = 0; kk < KF; ++kk) {
        if (kk * 32 + hi4 * 8 < k)
          afr[mi][kk] = *reinterpret_cast<const bf16x8*>(ap + kk * 32);
        else
          afr[mi][kk] = bf16x8{};              // masked K tail (x * 0-W)
      }
    }
    // 64 columns per outer step: the epilogue then sees 128-B contiguous
    // output rows (the naive fragment-layout epilogue's 2-B scalar
    // res-gathers/stores ran 3x slower than the MFMA+stream itself)
    for (int j0 = 0; j0 < ncols; j0 += 64) {
      f32x4 acc[2][4];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[mi][jj] = f32x4{0, 0, 0, 0};
      const int njj = min(4, (ncols - j0 + 15) / 16);
      // jj stays COMPILE-TIME (runtime-indexed acc -> scratch, rule 20);
      // the tail guard is a wave-uniform predicate around each step
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (jj < njj) {
          const __bf16* wp = wl + (j0 + jj * 16 + lo) * LDW + hi4 * 8;
#pragma unroll
          for (int kk = 0; kk < KF; ++kk) {
            const bf16x8 bfr =
                *reinterpret_cast<const bf16x8*>(wp + kk * 32);
            acc[0][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afr[0][kk], bfr, acc[0][jj], 0, 0, 0);
            acc[1][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afr[1][kk], bfr, acc[1][jj], 0, 0, 0);
          }
        }
      }
      const int jcols = min(64, ncols - j0);   // columns this step
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        // fragment -> LDS -> (row, 8-col seg) per lane, in f32, 8 rows
        // per pass (wave-local, no barrier); 16-B res loads + stores on
        // 128-B-contiguous rows
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2)
              et[(hi4 * 2 + r2) * 64 +
                 (((jj ^ (hi4 & 1)) << 4) | (lo ^ ((hi4 & 1) << 2)))] =
                  acc[mi][jj][q * 2 + r2];
          __builtin_amdgcn_s_waitcnt(/*lgkmcnt(0)*/ 0xc07f);
          const int tr = lane >> 3;                      // tile row
          const int tb = (tr >> 1) & 1;
          const int er = (tr >> 1) * 4 + q * 2 + (tr & 1);
          const int ec = (lane & 7) * 8;
          const long long row = r0 + mi * 16 + er;
          const int col = n0 + j0 + ec;
          if (row < m && ec < jcols) {
            const float* src = et + tr * 64 + (ec ^ (tb << 4));
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (tb << 2));
            const f32x4 v1 =
                *reinterpret_cast<const f32x4*>(src + (4 ^ (tb << 2)));
            if (ec + 8 <= jcols && col + 8 <= n) {
              bf16x8 o8;
              bf16x8 b8{}, rr8{};
              if (bias)
                b8 = *reinterpret_cast<const bf16x8*>(bias + col);
              if (res)
                rr8 = *reinterpret_cast<const bf16x8*>(res + row * n + col);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                float v = e < 4 ? v0[e & 3] : v1[e & 3];
                if (bias) v += (float)b8[e];
                if (res) v += (float)rr8[e];
                o8[e] = (__bf16)act_f(v, ACT);
              }
              *reinterpret_cast<bf16x8*>(c + row * n + col) = o8;
            } else {
              // ragged segment, element-wise; e stays compile-time (a
              // runtime-indexed vector would go to scratch)
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                if (ec + e < jcols && col + e < n) {
                  float v = e < 4 ? v0[e & 3] : v1[e & 3];
                  if (bias) v += (float)bias[col + e];
                  if (res) v += (float)res[row * n + col + e];
                  c[row * n + col + e] = (__bf16)act_f(v, ACT);
                }
              }
            }
          }
          __builtin_amdgcn_s_waitcnt(0xc07f);  // reads done before reuse
        }
      }
    }
  }
}

template <int ACT, int KF>
void launch_thin_kf(const void* a, const void* w, const void* bias,
                    const void* res, void* c, int m, int n, int nch, int k,
                    int m_blocks, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL((linear_thin_kernel<ACT, KF>),
                     dim3(m_blocks, (n + nch - 1) / nch), dim3(256), lds,
                     stream, (const __bf16*)a, (const __bf16*)w,
                     (const __bf16*)bias, (const __bf16*)res, (__bf16*)c,
                     m, n, nch, k);
}

// The thin kernel's N-chunk (W rows resident in LDS per block) for an
// (m, n, k) problem, 0 when the kernel does not take it.
int thin_nch(int m, int n, int k) {
  // n % 8: the vectorized epilogue's 16-B res/out accesses need 8-elem
  // row alignment.  K any multiple of 8 (<= 256): the last A fragment is
  // masked per lane, W LDS rows zero-fill to the 32-elem boundary.
  // K < 64: not worth MFMA
  if (k > 256 || k % 8 != 0 || k < 64 || m < 65536 || n % 8 != 0) return 0;
  const int kc = (k + 31) / 32 * 32;
  // W chunk + the four waves' epilogue tiles bounded by 80 KiB LDS (2
  // blocks/CU).  9 KiB stay set aside for the tiles, 1 KiB more than
  // they take, so the N-chunks are those the kernel was measured with.
  static_assert(4 * THIN_ET_BYTES <= 9 * 1024, "epilogue tiles > budget");
  const int nch_cap = (80 * 1024 - 9 * 1024) / 2 / (kc + 8) / 16 * 16;
  const int nch = min((n + 15) & ~15, nch_cap);
  return nch < 16 ? 0 : nch;
}

// caller: nch = thin_nch(m, n, k) > 0, so 64 <= k <= 256
template <int ACT>
void launch_thin(const void* a, const void* w, const void* bias,
                 const void* res, void* c, int m, int n, int nch, int k,
                 hipStream_t stream) {
  const int kc = (k + 31) / 32 * 32;
  // enough M-blocks to fill the chip; grid-stride handles the rest
  const int m_blocks = (int)min(((long long)m + 127) / 128, 4096LL);
  const size_t lds = (size_t)nch * (kc + 8) * 2 + 4 * THIN_ET_BYTES;
  switch (kc / 32) {
    case 2: launch_thin_kf<ACT, 2>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 3: launch_thin_kf<ACT, 3>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 4: launch_thin_kf<ACT, 4>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 5: launch_thin_kf<ACT, 5>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 6: launch_thin_kf<ACT, 6>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 7: launch_thin_kf<ACT, 7>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    case 8: launch_thin_kf<ACT, 8>(a, w, bias, res, c, m, n, nch, k, m_blocks, lds, stream); break;
    default: break;                            // unreachable, see thin_nch
  }
}

// the persistent kernel over ntiles full 256^2 tiles (tile columns
// 0 .. ntiles / tiles_m of an n-wide C), min(ntiles, CUs) blocks
template <int ACT, int MODE>
void launch_256p(const void* a, const void* w, const void* bias,
                 const void* res, void* c, int n, int k, int tiles_m,
                 int ntiles, const EpiExtra& x, hipStream_t stream) {
  static const int ncu = [] {
    int dev = 0, v = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                                dev);
    return v > 0 ? v : 256;
  }();
  constexpr size_t lds_p = 160 * 1024;         // 128 staging + 32 bounce
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&linear256p_kernel<ACT, MODE>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_p);
    attr_set = true;
  }
  hipLaunchKernelGGL((linear256p_kernel<ACT, MODE>),
                     dim3((unsigned)min(ntiles, ncu)), dim3(512), lds_p,
                     stream, (const __bf16*)a, (const __bf16*)w,
                     (const __bf16*)bias, (const __bf16*)res, (__bf16*)c, n,
                     k, tiles_m, ntiles, x);
}

// route: what vfa_linear_route said; BIG for every route but VFA_ROUTE_SMALL
template <int ACT, bool BIG>
void launch_tile(const void* a, const void* w, const void* bias,
                 const void* res, void* c, int m, int n, int k, int route,
                 hipStream_t stream) {
  constexpr int BM = BIG ? 256 : 128, BN = BIG ? 256 : 128;
  const int tiles_m = (m + BM - 1) / BM, tiles_n = (n + BN - 1) / BN;
  const size_t lds = 2 * (size_t)(BM + BN) * BK * 2;
  const bool full = (k % BK == 0);   // per-tile M/N edges handled inside
  int tile_base = 0;
  if (BIG && (route == VFA_ROUTE_256P || route == VFA_ROUTE_256P_EDGE)) {
    // interior tile columns -> the persistent kernel; what is left for
    // the guarded kernel below is at most the ragged last column
    const int ntiles = tiles_m * (n / 256);
    launch_256p<ACT, EPI_PLAIN>(a, w, bias, res, c, n, k, tiles_m, ntiles,
                                EpiExtra{}, stream);
    if (route == VFA_ROUTE_256P) return;
    tile_base = ntiles;
  }
  const dim3 grid(tiles_m * tiles_n - tile_base);
  if (full)
    hipLaunchKernelGGL((linear_act_kernel<ACT, true, BIG>), grid,
                       dim3(BIG ? 512 : 256), lds, stream, (const __bf16*)a,
                       (const __bf16*)w, (const __bf16*)bias,
                       (const __bf16*)res, (__bf16*)c, m, n, k, tiles_m,
                       tile_base);
  else
    hipLaunchKernelGGL((linear_act_kernel<ACT, false, BIG>), grid,
                       dim3(BIG ? 512 : 256), lds, stream, (const __bf16*)a,
                       (const __bf16*)w, (const __bf16*)bias,
                       (const __bf16*)res, (__bf16*)c, m, n, k, tiles_m,
                       tile_base);
}

template <int ACT>
void launch_linear(const void* a, const void* w, const void* bias,
                   const void* res, void* c, int m, int n, int k,
                   hipStream_t stream) {
  int nch = 0;
  const int route = vfa_linear_route(m, n, k, ACT, &nch);
  switch (route) {
    case VFA_ROUTE_THIN:
      launch_thin<ACT>(a, w, bias, res, c, m, n, nch, k, stream);
      break;
    case VFA_ROUTE_8P:
      launch_8p<ACT>(a, w, bias, res, c, m, n, k, stream);
      break;
    case VFA_ROUTE_SMALL:
      launch_tile<ACT, false>(a, w, bias, res, c, m, n, k, route, stream);
      break;
    default:
      launch_tile<ACT, true>(a, w, bias, res, c, m, n, k, route, stream);
  }
}

}  // namespace

extern "C" {

// Every routing decision of vfa_linear_act, in one place: the launchers
// above act on what this returns, and it is bound to Python as
// _ext.linear_route so that a test can pin a shape to its kernel.
int vfa_linear_route(int m, int n, int k, int act, int* nch) {
  // M-huge / K-shallow -> the streaming kernel (reads A once, no K-loop
  // barriers); else BIG tiles when M tiles evenly (a half-empty 256-row
  // tail tile and the block-round quantization cost more than the smaller
  // tile's overhead — measured 339 vs 528 TF at M=9600) and the grid
  // still fills the chip
  // Both 256^2 kernels share one epilogue (epilogue_strips).  With it and
  // the persistent tile walk the 2-buffer kernel wins every shape it takes
  // (>= 150 tiles), with or without an activation — us/call, persistent
  // vs 8-phase, same box: fc1+QuickGELU 19200x3072x768 114-118 vs 125,
  // the same shape act-none 101 vs 113, qkv 19200x2304x768 83 vs 92,
  // 4096^3 129 vs 134-137, 8192^3 906 vs 920-928, 4096x4096x12288+relu
  // 334-337 vs 359 — so it goes first.  The 8-phase kernel keeps the
  // act-none full-tile problems of 64..149 tiles, which the persistent
  // route does not take.  VFA_8P forces the 8-phase kernel wherever it
  // can run, VFA_NO_8P disables it, VFA_NO_THIN disables the streaming
  // kernel, for A/B.
  static const int env8p = getenv("VFA_8P") ? 1
                           : getenv("VFA_NO_8P") ? -1 : 0;
  static const bool no_thin = getenv("VFA_NO_THIN") != nullptr;
  *nch = no_thin ? 0 : thin_nch(m, n, k);
  if (*nch) return VFA_ROUTE_THIN;
  const long long tiles = (long long)((m + 255) / 256) * ((n + 255) / 256);
  const bool big = n >= 256 && m % 256 == 0 && tiles >= 150;
  const bool want8p = env8p > 0 || (env8p == 0 && act == 0 && !big);
  // 8-phase: full tiles only, k / 64 >= 3 for its pipeline depth, and at
  // least 64 tiles (chip fill)
  if (want8p && m % 256 == 0 && n % 256 == 0 && k % 64 == 0 &&
      k / 64 >= 3 && tiles >= 64)
    return VFA_ROUTE_8P;
  if (!big) return VFA_ROUTE_SMALL;
  // interior tile columns -> the persistent kernel when K has no ragged
  // step (n % 8: its 16-B bias/res/out vectors need 8-element row
  // alignment); the guarded kernel then takes only the ragged last column
  if (k % BK != 0 || n % 8 != 0) return VFA_ROUTE_BIG_GUARD;
  return n % 256 == 0 ? VFA_ROUTE_256P : VFA_ROUTE_256P_EDGE;
}

// act: 0 none, 1 relu, 2 quick_gelu, 3 gelu_tanh, 4 leaky_relu(0.1)
void vfa_linear_act(const void* a, const void* w, const void* bias,
                    const void* res, void* c, int m, int n, int k, int act,
                    hipStream_t stream) {
  // any other id is rejected by the binding
  dispatch_act(act, [&](auto id) {
    launch_linear<decltype(id)::value>(a, w, bias, res, c, m, n, k, stream);
  });
}

// s = a @ w^T + bias + res (bf16) and, per row of s and 256-column group
// (tile column), the (mean, M2) of the rounded values: part (M, N/256)
// float2.  Full tiles only (m % 256 == n % 256 == k % 64 == 0; the binding
// checks).
void vfa_linear_res_stats(const void* a, const void* w, const void* bias,
                          const void* res, void* c, void* part, int m, int n,
                          int k, hipStream_t stream) {
  EpiExtra x{};
  x.part = (float2*)part;
  launch_256p<0, EPI_STATS>(a, w, bias, res, c, n, k, m / 256,
                            (m / 256) * (n / 256), x, stream);
}

// c = act(rstd * (a @ w^T - mean * ln_c) + ln_b): LayerNorm folded into the
// linear layer (w, ln_c, ln_b from ops.fold_ln_linear), a un-normalised,
// stats (M, groups) float2 partials of a's rows over k / groups columns
// each.  Full tiles only, as above.
void vfa_linear_ln_act(const void* a, const void* stats, int groups,
                       const void* w, const void* ln_c, const void* ln_b,
                       void* c, int m, int n, int k, float eps, int act,
                       hipStream_t stream) {
  EpiExtra x{};
  x.ln_c = (const float*)ln_c;
  x.ln_b = (const float*)ln_b;
  x.stats = (const float2*)stats;
  x.groups = groups;
  x.eps = eps;
  dispatch_act(act, [&](auto id) {
    launch_256p<decltype(id)::value, EPI_LN>(a, w, nullptr, nullptr, c, n, k,
                                             m / 256, (m / 256) * (n / 256),
                                             x, stream);
  });
}

}  // extern "C"
