// Implicit-GEMM conv2d for gfx950 (CDNA4), NHWC bf16 — hand-written MFMA
// replacement for MIOpen's igemm on the 3x3 / 1x5 / 5x1 / 7x7 hot shapes
// of the ResNet / RAFT / I3D(flattened) / VGGish conv stacks (reference
// conv stacks: models/resnet & models/raft/raft_src/extractor.py:118-192,
// models/i3d/i3d_src/i3d_net.py:37-105, vggish_src/vggish.py:108-118).
//
// GEMM view:  C[M, N] = act( A[M, Kr] @ W[N, Kr]^T + bias [+ res] )
//   M  = B*OH*OW output pixels, N = K_out channels,
//   Kr = KH*KW*C with reduction index k = (r*KW + s)*C + c.
// A is the im2col view of the PRE-PADDED input (B, Hp, Wp, C) — never
// materialized: each staged A row is an input pixel's C-slice at tap
// (r, s), address  base(m) + (r*Wp + s)*C + c  with
// base(m) = ((b*Hp + oy*sh)*Wp + ox*sw)*C precomputed PER THREAD before
// the K-loop (each thread always stages the same tile rows; only the
// k-offset changes per K-tile).  W is torch's channels_last conv weight —
// physically (K_out, KH, KW, C) = exactly the (N, Kr) row-major B operand,
// so weights need NO reshuffling and B staging is identical to the linear
// kernel's.
//
// The tile machinery is mfma_tile.h, shared with gemm.hip: 256x256 /
// 128x128 / 256x64 tiles, BK=64, double-buffered LDS staged by glds with
// the conflict-free XOR swizzle on the per-lane *source* address, the
// K-step (the next K-tile's glds spread across its two MFMA half-steps),
// the fused bias+activation(+residual) epilogue.  This file adds the A
// operand's im2col staging, the guarded W staging, the K loop around the
// shared K-step, the pad pass and the tile choice.  Requires C % 8 == 0
// (each lane's 16-B segment stays inside one tap).
//
// Dilation (dh, dw) moves tap (r, s) to (y0 + r*dh, x0 + s*dw).  The input
// pixel stride ldx may exceed C: the conv then reads a C-wide channel slice
// of a wider NHWC buffer (the host folds the slice's channel offset into
// the x pointer), element address  base + (iy*Wp + ix)*ldx + c  with
// base = b*Hp*Wp*ldx.  ldx % 8 == 0 and a slice offset % 8 == 0 keep every
// 16-B segment aligned.  dh = dw = 1, ldx = C is the plain conv: its
// kernels are the GEN = false instantiations, where the three values are
// compile-time 1, 1 and cin, so the hot shapes run the code they ran before
// dilation existed (with the three values as run-time fields two hot shapes
// measured 0.6% and 1% behind the previous build, at or above the spread
// of its own two runs; profiles/pwc_decoder.md).
#include "mfma_tile.h"

namespace {

// ConvGeom / ConvAddr (the geometry the host fills and the kernel takes by
// value) are declared in vfa_api.h

// decompose output-pixel index m -> (image base, receptive-field origin)
struct PixRef {
  long long base;           // bi * H * W * ldx
  int y0, x0;               // oy*sh - pt, ox*sw - pl (may be negative)
};

__device__ __forceinline__ PixRef pix_ref(const ConvGeom& g,
                                          const ConvAddr& a, int m) {
  const int ox = m % g.ow;
  const int t = m / g.ow;
  const int oy = t % g.oh;
  const int bi = t / g.oh;
  return PixRef{(long long)bi * g.hp * g.wp * a.ldx,
                oy * g.sh - g.pt, ox * g.sw - g.pl};
}

// Stage the (ROWS x 64) A-tile via glds: per-thread row refs precomputed;
// the per-lane k position picks tap (r, s) and channel; out-of-image taps
// redirect the load to a zero page (the inline zero-padding — no
// materialized pad pass).  piece splits the wave's glds issues across MFMA
// half-steps (-1 = all).
template <int ROWS, int WAVES>
__device__ __forceinline__ void conv_stage_a(
    const __bf16* __restrict__ x, const __bf16* __restrict__ zp,
    const ConvGeom& g, const ConvAddr& a, const PixRef* __restrict__ aref,
    int k0, char* lds_base, int wave, int lane, int kfrac0, int arin_half,
    int piece, int npieces) {
  constexpr int NSUB = ROWS * 128 / 1024;
  constexpr int PER_WAVE = NSUB / WAVES;
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    if (piece >= 0 && (i * npieces) / PER_WAVE != piece) continue;
    const int sub = wave * PER_WAVE + i;
    // per-subtile swizzle: f = ((sub&1)<<2)|(r_in>>1) on element bits 3..5
    const int k = k0 + (kfrac0 ^
                        ((((sub & 1) << 2) | arin_half) << 3));
    const int tap = k / g.cin;          // uniform-cost u32 div
    const int c = k - tap * g.cin;
    const int r = tap / g.kw;
    const int s = tap - r * g.kw;
    const int iy = aref[i].y0 + r * a.dh, ix = aref[i].x0 + s * a.dw;
    const bool ok = (unsigned)iy < (unsigned)g.hp &&
                    (unsigned)ix < (unsigned)g.wp;
    const __bf16* src =
        ok ? x + aref[i].base + ((long long)iy * g.wp + ix) * a.ldx + c
           : zp + (lane & 63) * 8;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(src),
        reinterpret_cast<unsigned int*>(lds_base + sub * 1024), 16, 0, 0);
  }
}

// Bounds-checked A staging (M-edge tiles and the ragged last K-tile):
// same LDS image, zero fill (covers out-of-image taps too).
template <int ROWS, int THREADS>
__device__ __forceinline__ void conv_guard_a(
    const __bf16* __restrict__ x, const ConvGeom& g, const ConvAddr& a,
    int m0, int mtotal, int k0, char* lds_base, int tid) {
  for (int t = tid; t < ROWS * 8; t += THREADS) {  // 8 16-B segs per row
    const int row = t >> 3, seg = t & 7;
    uint4 v = {0u, 0u, 0u, 0u};
    const int m = m0 + row;
    const int k = k0 + seg * 8;
    if (m < mtotal && k < g.kr) {
      const PixRef pr = pix_ref(g, a, m);
      const int tap = k / g.cin;
      const int c = k - tap * g.cin;
      const int r = tap / g.kw;
      const int s = tap - r * g.kw;
      const int iy = pr.y0 + r * a.dh, ix = pr.x0 + s * a.dw;
      if ((unsigned)iy < (unsigned)g.hp && (unsigned)ix < (unsigned)g.wp)
        v = *reinterpret_cast<const uint4*>(
            x + pr.base + ((long long)iy * g.wp + ix) * a.ldx + c);
    }
    *reinterpret_cast<uint4*>(lds_base + swz(row * 128 + seg * 16)) = v;
  }
}

// Bounds-checked W staging.  What mfma_tile.h's stage_guard does when
// Kr % 8 == 0, kept as its own 16-B-only loop: with stage_guard here the
// 256x256 tile (256 VGPRs, spilling) measured 3-6% slower on its full-tile
// rows (profiles/mfma_tile_refactor.md).
template <int ROWS, int THREADS>
__device__ __forceinline__ void conv_guard_w(
    const __bf16* __restrict__ wgt, long long row_stride, int n0, int ntotal,
    int k0, int kr, char* lds_base, int tid) {
  for (int t = tid; t < ROWS * 8; t += THREADS) {
    const int row = t >> 3, seg = t & 7;
    uint4 v = {0u, 0u, 0u, 0u};
    if (n0 + row < ntotal && k0 + seg * 8 < kr) {
      v = *reinterpret_cast<const uint4*>(wgt + (long long)row * row_stride +
                                          seg * 8);
    }
    *reinterpret_cast<uint4*>(lds_base + swz(row * 128 + seg * 16)) = v;
  }
}

// Tile variants: 256x256 (8 waves, 2Mx4N), 128x128 (4 waves, 2x2),
// 256x64 (4 waves, 4Mx1N — for K_out = 64/192 nets where a 128-wide N
// tile is half empty).  GEN: dilation and the input pixel stride come from
// the trailing arguments; otherwise they are 1, 1 and cin.
template <int ACT, int BM, int BN, int WAVES, int WN, bool GEN>
__global__ __launch_bounds__(WAVES * 64)
void conv2d_nhwc_kernel(const __bf16* __restrict__ x,
                        const __bf16* __restrict__ wgt,
                        const __bf16* __restrict__ bias,
                        const __bf16* __restrict__ res,
                        const __bf16* __restrict__ zp,
                        __bf16* __restrict__ out, ConvGeom g, int mtotal,
                        int ldc, int tiles_m, int tiles_n, int dh, int dw,
                        int ldx) {
  const ConvAddr a = GEN ? ConvAddr{dh, dw, ldx} : ConvAddr{1, 1, g.cin};
  constexpr int MI = BM / (WAVES / WN) / 16;   // 16-row MFMA tiles / wave
  constexpr int NJ = BN / WN / 16;             // 16-col MFMA tiles / wave
  constexpr int TILE_A = BM * BK * 2, TILE_B = BN * BK * 2;
  constexpr int THREADS = WAVES * 64;
  constexpr int PER_WAVE = (BM * 128 / 1024) / WAVES;

  extern __shared__ __attribute__((aligned(1024))) char smem[];
  auto sA = [&](int buf) { return smem + buf * (TILE_A + TILE_B); };
  auto sB = [&](int buf) { return smem + buf * (TILE_A + TILE_B) + TILE_A; };

  const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tile_n = wg / tiles_m, tile_m = wg % tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int kr = g.kr, n = g.kout;
  const int nk = (kr + BK - 1) / BK;
  const int valid_m = mtotal - m0, valid_n = n - n0;
  const bool tile_full = valid_m >= BM && valid_n >= BN;
  const bool kfull = (kr % BK) == 0;

  // per-thread A row refs for the glds path (same rows every K-tile);
  // the per-lane swizzled byte offset contributes kfrac elements
  const int a_rin = (lane * 16) >> 7;
  const int kfrac0 = ((lane * 16) & 127) >> 1;   // pre-swizzle elements
  PixRef aref[PER_WAVE];
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int sub = wave * PER_WAVE + i;
    const int m = m0 + sub * 8 + a_rin;
    aref[i] = pix_ref(g, a, m < mtotal ? m : mtotal - 1);
  }

  auto stage = [&](int buf, int kt) {
    const int k0 = kt * BK;
    if (tile_full && (kfull || kt + 1 < nk)) {
      conv_stage_a<BM, WAVES>(x, zp, g, a, aref, k0, sA(buf), wave, lane,
                              kfrac0, a_rin >> 1, -1, 1);
      stage_glds<BN, WAVES>(wgt + (long long)n0 * kr + k0, kr, sB(buf),
                            wave, lane);
    } else {
      conv_guard_a<BM, THREADS>(x, g, a, m0, mtotal, k0, sA(buf),
                                threadIdx.x);
      conv_guard_w<BN, THREADS>(wgt + (long long)n0 * kr + k0, kr, n0, n,
                                k0, kr, sB(buf), threadIdx.x);
    }
  };

  stage(0, 0);

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();
    const int cur = kt & 1;
    const int k0_nxt = (kt + 1) * BK;
    const bool glds_nxt = (kt + 1 < nk) && tile_full &&
                          (kfull || kt + 2 < nk);
    if ((kt + 1 < nk) && !glds_nxt) stage(1 - cur, kt + 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      mfma_kstep<MI, NJ>(sA(cur), sB(cur), wm * (MI * 16), wn * (NJ * 16),
                         kk, lane, acc, [&] {
        if (glds_nxt) {
          conv_stage_a<BM, WAVES>(x, zp, g, a, aref, k0_nxt, sA(1 - cur),
                                  wave, lane, kfrac0, a_rin >> 1, kk, 2);
          stage_glds_piece<BN, WAVES>(wgt + (long long)n0 * kr + k0_nxt, kr,
                                      sB(1 - cur), wave, lane, kk, 2);
        }
      });
    }
  }

  // ldc > n: writing a channel slice of a wider NHWC buffer (the caller
  // eliminated a cat copy); res stays logically (M, n)
  epilogue_frag<ACT, MI, NJ, 2>(acc, bias, res, out, mtotal, n, ldc,
                                m0 + wm * (MI * 16), n0 + wn * (NJ * 16),
                                lane, !tile_full);
}

template <int ACT, int BM, int BN, int WAVES, int WN>
void launch_cfg(const void* x, const void* w, const void* bias,
                const void* res, const void* zp, void* out,
                const ConvGeom& g, const ConvAddr& a, int m, int ldc,
                hipStream_t stream) {
  const int tiles_m = (m + BM - 1) / BM, tiles_n = (g.kout + BN - 1) / BN;
  const dim3 grid(tiles_m * tiles_n);
  const size_t lds = 2 * (size_t)(BM + BN) * BK * 2;
  auto launch = [&](auto gen) {
    hipLaunchKernelGGL(
        (conv2d_nhwc_kernel<ACT, BM, BN, WAVES, WN, decltype(gen)::value>),
        grid, dim3(WAVES * 64), lds, stream, (const __bf16*)x,
        (const __bf16*)w, (const __bf16*)bias, (const __bf16*)res,
        (const __bf16*)zp, (__bf16*)out, g, m, ldc, tiles_m, tiles_n, a.dh,
        a.dw, a.ldx);
  };
  if (a.dh == 1 && a.dw == 1 && a.ldx == g.cin)
    launch(std::false_type{});
  else
    launch(std::true_type{});
}

template <int ACT>
void launch_conv(const void* x, const void* w, const void* bias,
                 const void* res, const void* zp, void* out,
                 const ConvGeom& g, const ConvAddr& a, int ldc,
                 hipStream_t stream) {
  const int m = g.b * g.oh * g.ow;
  int bm, bn;
  vfa_conv2d_pick_tile(m, g.kout, &bm, &bn);
  if (bm == 256 && bn == 256)
    launch_cfg<ACT, 256, 256, 8, 4>(x, w, bias, res, zp, out, g, a, m, ldc,
                                   stream);
  else if (bm == 256)
    launch_cfg<ACT, 256, 64, 4, 1>(x, w, bias, res, zp, out, g, a, m, ldc,
                                   stream);
  else
    launch_cfg<ACT, 128, 128, 4, 2>(x, w, bias, res, zp, out, g, a, m, ldc,
                                   stream);
}

// ------------------------------------------------------------- pad kernel
// zero-pad H/W and optionally CHANNELS of an NHWC tensor:
// (B, H, W, Cin) -> (B, H+pt+pb, W+pl+pr, Cout), Cout % 8 == 0, zeros for
// c >= Cin.  The channel pad is how C=3/C=2 stems (ResNet/RAFT/I3D) and
// the C=324 RAFT corr input reach the implicit-GEMM kernel (which needs
// C % 8 == 0).  Memory-bound; 16-B vectorized, elementwise on the one
// segment straddling Cin.
__global__ void pad2d_nhwc_kernel(const __bf16* __restrict__ x,
                                  __bf16* __restrict__ out, int b, int h,
                                  int w, int cin, int cout, int pt, int pb,
                                  int pl, int pr) {
  const int hp = h + pt + pb, wp = w + pl + pr;
  const long long total = (long long)b * hp * wp * (cout / 8);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cseg = (int)(i % (cout / 8));
    long long t = i / (cout / 8);
    const int xw = (int)(t % wp);
    t /= wp;
    const int xh = (int)(t % hp);
    const int bi = (int)(t / hp);
    uint4 v = {0u, 0u, 0u, 0u};
    const int sy = xh - pt, sx = xw - pl;
    if (sy >= 0 && sy < h && sx >= 0 && sx < w) {
      const long long src = (((long long)bi * h + sy) * w + sx) * cin;
      if (cseg * 8 + 8 <= cin) {
        v = *reinterpret_cast<const uint4*>(x + src + cseg * 8);
      } else if (cseg * 8 < cin) {
        __bf16* e = reinterpret_cast<__bf16*>(&v);
        for (int j = 0; cseg * 8 + j < cin; ++j)
          e[j] = x[src + cseg * 8 + j];
      }
    }
    *reinterpret_cast<uint4*>(
        out + (((long long)bi * hp + xh) * wp + xw) * cout + cseg * 8) = v;
  }
}

}  // namespace

extern "C" {

// Tile (BM x BN) launch_conv runs for M = B*OH*OW output pixels and kout
// channels: the one minimizing padded work, preferring the bigger tile
// when waste ties and the grid still fills the chip (256 CUs).
void vfa_conv2d_pick_tile(int m, int kout, int* bm, int* bn) {
  auto cost = [&](int tbm, int tbn, long long min_wgs) {
    const long long tm = (m + tbm - 1) / tbm, tn = (kout + tbn - 1) / tbn;
    long long padded = tm * tbm * tn * tbn;
    if (tm * tn < min_wgs) padded = padded * 4;   // fill penalty
    return padded;
  };
  const long long c256 = (kout >= 256 && m >= 4096)
                             ? cost(256, 256, 150) : (1LL << 62);
  const long long c128 = cost(128, 128, 120);
  const long long c64 = cost(256, 64, 120);
  if (c256 <= c128 && c256 <= c64) {
    *bm = 256; *bn = 256;
  } else if (c64 < c128) {
    *bm = 256; *bn = 64;
  } else {
    *bm = 128; *bn = 128;
  }
}

void vfa_conv2d_nhwc(const void* x, const void* w, const void* bias,
                     const void* res, const void* zp, void* out,
                     const ConvGeom& g, const ConvAddr& a, int ldc, int act,
                     hipStream_t stream) {
  dispatch_act(act, [&](auto id) {
    launch_conv<decltype(id)::value>(x, w, bias, res, zp, out, g, a, ldc,
                                     stream);
  });
}

void vfa_pad2d_nhwc(const void* x, void* out, int b, int h, int w, int cin,
                    int cout, int pt, int pb, int pl, int pr,
                    hipStream_t stream) {
  const long long total = (long long)b * (h + pt + pb) * (w + pl + pr) *
                          (cout / 8);
  const int threads = 256;
  const int blocks = (int)min((total + threads - 1) / threads, 2048LL);
  hipLaunchKernelGGL(pad2d_nhwc_kernel, dim3(blocks), dim3(threads), 0,
                     stream, (const __bf16*)x, (__bf16*)out, b, h, w, cin,
                     cout, pt, pb, pl, pr);
}

}  // extern "C"
