// RAFT-specific fused kernels for gfx950 (CDNA4).
//
// The reference RAFT (models/raft/raft_src/{corr,raft,update}.py) runs its
// 20-iteration update loop as dozens of small torch ops per iteration:
// 4 grid_sample lookups + window-coordinate construction + cat/permute for
// the correlation pyramid (corr.py:36-50), F.unfold + softmax + mul-sum for
// the convex 8x upsample (raft.py:100-111), and 6 convs + 6 elementwise for
// the SepConvGRU (update.py:37-64).  On MI355X that is launch-bound; these
// kernels fuse each group into one dispatch:
//
//  - vfa_corr_lookup: all 4 pyramid levels x 81 taps in one kernel, the
//    per-pixel correlation planes staged through LDS (each output pixel owns
//    a whole (h_l, w_l) plane per level; total ~4.2 KB for 28x28 feature
//    maps, far under the 160 KB LDS/CU).  Zero-padding bilinear semantics
//    identical to torch grid_sample(align_corners=True, padding='zeros').
//  - vfa_corr_otf: the same lookup computed from the feature maps, for
//    frames whose all-pairs volume (quadratic in frame area) does not fit:
//    100 dot products + 81 blends per (pixel, level), memory linear in area.
//  - vfa_convex_upsample: softmax(0.25*mask) convex combination of the 3x3
//    neighborhood of 8*flow, one thread per upsampled pixel.
//  - vfa_gru_zr / vfa_gru_out: the SepConvGRU gate elementwise, fused so the
//    z,r sigmoid + r*h product and the (1-z)*h + z*tanh(q) update are one
//    kernel each, writing r*h / h_new directly into the channel slice of the
//    persistent conv-input buffers (no cat per step).
//
// All kernels take an `nhwc` flag: the RAFT GPU path runs channels_last so
// MIOpen uses its NHWC igemm solvers without batched_transpose fixups.
#include "vfa_common.h"

namespace {

// ------------------------------------------------------------ corr lookup
// Pyramid: LV levels, level l is (N, 1, h[l], w[l]) fp32, N = B*H*W planes
// (one correlation plane per query pixel).  coords: (B, 2, H, W) fp32 pixel
// units at level 0.  out: (B, LV*81, H, W) or NHWC (B, H, W, LV*81) in T.
// PPB query pixels per block (one 64-lane wave each): 16 waves in flight
// per block hide the LDS-staging load latency
template <typename T, int RAD, bool NHWC, int PPB>
__global__ void corr_lookup_lds_kernel(const float* __restrict__ l0,
                                       const float* __restrict__ l1,
                                       const float* __restrict__ l2,
                                       const float* __restrict__ l3,
                                       const float* __restrict__ coords,
                                       T* __restrict__ out, int levels,
                                       int4 hs, int4 ws, long long npix,
                                       int hw, int lds_floats) {
  extern __shared__ float lds_all[];
  const int K = 2 * RAD + 1;          // 9
  const int KK = K * K;               // 81 taps per level
  const long long pix = blockIdx.x * (long long)PPB + threadIdx.y;
  if (pix >= npix) return;
  float* lds = lds_all + (long long)threadIdx.y * lds_floats;
  const int tid = threadIdx.x;

  const int lh[4] = {hs.x, hs.y, hs.z, hs.w};
  const int lw[4] = {ws.x, ws.y, ws.z, ws.w};
  const float* lp[4] = {l0, l1, l2, l3};

  // cooperative stage of this pixel's planes (all levels) into LDS
  int off = 0;
  int loff[4];
  for (int l = 0; l < levels; ++l) {
    const int n = lh[l] * lw[l];
    const float* src = lp[l] + pix * (long long)n;
    loff[l] = off;
    for (int i = tid; i < n; i += 64) lds[off + i] = src[i];
    off += n;
  }
  __builtin_amdgcn_wave_barrier();  // each wave stages its own pixel's planes

  const long long b = pix / hw;
  const int p = (int)(pix % hw);
  const float cx = coords[(b * 2 + 0) * hw + p];
  const float cy = coords[(b * 2 + 1) * hw + p];

  const int ctot = levels * KK;
  for (int c = tid; c < ctot; c += 64) {
    const int l = c / KK, t = c % KK;
    const int dx = t / K - RAD, dy = t % K - RAD;  // tap t = i*9+j: i
    // offsets X, j offsets Y — the reference's channel order
    // (corr.py:39 stacks (dy,dx) last, added to (x,y) coords)
    const float inv = 1.0f / (float)(1 << l);
    const float sx = cx * inv + dx, sy = cy * inv + dy;
    const int h = lh[l], w = lw[l];
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    const float ax = sx - x0, ay = sy - y0;
    const float w00 = (1 - ax) * (1 - ay), w01 = ax * (1 - ay);
    const float w10 = (1 - ax) * ay, w11 = ax * ay;
    const float* pl = lds + loff[l];
    float v = 0.f;
    if (x0 >= 0 && x0 < w && y0 >= 0 && y0 < h) v += w00 * pl[y0 * w + x0];
    if (x0 + 1 >= 0 && x0 + 1 < w && y0 >= 0 && y0 < h)
      v += w01 * pl[y0 * w + x0 + 1];
    if (x0 >= 0 && x0 < w && y0 + 1 >= 0 && y0 + 1 < h)
      v += w10 * pl[(y0 + 1) * w + x0];
    if (x0 + 1 >= 0 && x0 + 1 < w && y0 + 1 >= 0 && y0 + 1 < h)
      v += w11 * pl[(y0 + 1) * w + x0 + 1];
    const long long oi = NHWC ? (pix * ctot + c)
                              : ((b * ctot + c) * hw + p);
    out[oi] = from_f32<T>(v);
  }
}

// global-memory fallback for feature maps too large to stage in LDS
template <typename T, int RAD, bool NHWC>
__global__ void corr_lookup_gmem_kernel(const float* __restrict__ l0,
                                        const float* __restrict__ l1,
                                        const float* __restrict__ l2,
                                        const float* __restrict__ l3,
                                        const float* __restrict__ coords,
                                        T* __restrict__ out, int levels,
                                        int4 hs, int4 ws, long long npix,
                                        int hw) {
  const int K = 2 * RAD + 1, KK = K * K;
  const int ctot = levels * KK;
  const long long total = npix * ctot;
  const int lh[4] = {hs.x, hs.y, hs.z, hs.w};
  const int lw[4] = {ws.x, ws.y, ws.z, ws.w};
  const float* lp[4] = {l0, l1, l2, l3};
  long long loffs[4];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long pix = i / ctot;
    const int c = (int)(i % ctot);
    const long long b = pix / hw;
    const int p = (int)(pix % hw);
    const float cx = coords[(b * 2 + 0) * hw + p];
    const float cy = coords[(b * 2 + 1) * hw + p];
    const int l = c / KK, t = c % KK;
    const int dx = t / K - RAD, dy = t % K - RAD;  // tap t = i*9+j: i
    // offsets X, j offsets Y — the reference's channel order
    // (corr.py:39 stacks (dy,dx) last, added to (x,y) coords)
    const float inv = 1.0f / (float)(1 << l);
    const float sx = cx * inv + dx, sy = cy * inv + dy;
    const int h = lh[l], w = lw[l];
    const float* pl = lp[l] + pix * (long long)(h * w);
    const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    const float ax = sx - x0, ay = sy - y0;
    const float w00 = (1 - ax) * (1 - ay), w01 = ax * (1 - ay);
    const float w10 = (1 - ax) * ay, w11 = ax * ay;
    float v = 0.f;
    if (x0 >= 0 && x0 < w && y0 >= 0 && y0 < h) v += w00 * pl[y0 * w + x0];
    if (x0 + 1 >= 0 && x0 + 1 < w && y0 >= 0 && y0 < h)
      v += w01 * pl[y0 * w + x0 + 1];
    if (x0 >= 0 && x0 < w && y0 + 1 >= 0 && y0 + 1 < h)
      v += w10 * pl[(y0 + 1) * w + x0];
    if (x0 + 1 >= 0 && x0 + 1 < w && y0 + 1 >= 0 && y0 + 1 < h)
      v += w11 * pl[(y0 + 1) * w + x0 + 1];
    const long long oi = NHWC ? (pix * ctot + c)
                              : ((b * ctot + c) * hw + p);
    out[oi] = from_f32<T>(v);
  }
  (void)loffs;
}

// ------------------------------------------------- on-the-fly corr lookup
// The same lookup without the all-pairs volume: avg-pooling and the dot
// product are linear, so level l of the pooled volume is f1 . avgpool_l(f2),
// and the 81 taps of a (pixel, level) sample the 10x10 integer grid around
// floor(coords / 2^l) with ONE shared fractional part.  Per (pixel, level):
// 100 dots C[i][j] = f1[p] . f2_l[y0 + j][x0 + i] / sqrt(D) (0 outside the
// level), then 81 four-term blends of C; tap t = i*9+j as above.
//
// f1 (B, H, W, D), f2 level l (B, h_l, w_l, D): f32, pixel-major.  One wave
// per query pixel, OTF_WPB waves per block, no workgroup barrier.  Lane =
// (grid-point group g = lane >> 3, 16-B segment sg = lane & 7); chunk k of a
// lane is channels [32k + 4sg, 32k + 4sg + 4), so the 8 lanes of a group
// read 128 contiguous bytes per load and f1[p] stays in registers (D <= 256:
// 8 chunks).  The levels' grids are one list of levels*100 points; a round
// takes 8 of them, OTF_RPI rounds have all their loads issued before the
// first use.  Loads of points outside their level are predicated off.
// Partial dots are summed over the 8 segment lanes, C goes to a wave-private
// LDS tile, and after a wave_barrier the 64 lanes form the levels*81 blends.
constexpr int OTF_WPB = 4;   // waves (query pixels) per block
constexpr int OTF_RPI = 2;   // rounds in flight
constexpr int OTF_NCH = 8;   // 32-channel chunks a lane can hold (D <= 256)

// integer origin (leftmost grid column / top row) and fractional part of
// one axis at one level.  floor(s) is clamped before the int conversion, so
// a huge or non-finite coordinate gives a window wholly outside the level
// (and a zero fraction) instead of an out-of-range index.
__device__ __forceinline__ void otf_origin(float c, float inv, int n, int& i0,
                                           float& a) {
  const float s = c * inv;
  const float f = floorf(s);
  const float fc = fminf(fmaxf(f, -16.f), (float)n + 16.f);
  i0 = (int)fc - 4;
  a = (f == fc) ? s - f : 0.f;
}

template <typename T, bool NHWC>
__global__ __launch_bounds__(64 * OTF_WPB) void corr_otf_kernel(
    const float* __restrict__ f1, const float* __restrict__ l0,
    const float* __restrict__ l1, const float* __restrict__ l2,
    const float* __restrict__ l3, const float* __restrict__ coords,
    T* __restrict__ out, int levels, int4 hs, int4 ws, long long npix, int hw,
    int d, float rsqrt_d) {
  __shared__ float tiles[OTF_WPB][400];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int g = lane >> 3, sg = lane & 7;
  const long long pix = (long long)blockIdx.x * OTF_WPB + wv;
  if (pix >= npix) return;
  float* tile = tiles[wv];
  const long long b = pix / hw;
  const int p = (int)(pix % hw);
  const float cx = coords[(b * 2 + 0) * hw + p];
  const float cy = coords[(b * 2 + 1) * hw + p];
  const int nch = d >> 5;

  // this lane's share of f1[p]
  float q[OTF_NCH][4];
#pragma unroll
  for (int k = 0; k < OTF_NCH; ++k) {
    q[k][0] = q[k][1] = q[k][2] = q[k][3] = 0.f;
    if (k < nch) load16(q[k], f1 + pix * d + k * 32 + sg * 4);
  }

  const int npts = levels * 100;
  for (int r0 = 0; r0 < npts; r0 += 8 * OTF_RPI) {
    float v[OTF_RPI][OTF_NCH][4];
#pragma unroll
    for (int r = 0; r < OTF_RPI; ++r) {
      const int gp = r0 + 8 * r + g;
      const int l = gp / 100, ij = gp % 100;
      const int h = l == 0 ? hs.x : l == 1 ? hs.y : l == 2 ? hs.z : hs.w;
      const int w = l == 0 ? ws.x : l == 1 ? ws.y : l == 2 ? ws.z : ws.w;
      const float* fl = l == 0 ? l0 : l == 1 ? l1 : l == 2 ? l2 : l3;
      const float inv = 1.0f / (float)(1 << l);
      int x0, y0;
      float ax, ay;
      otf_origin(cx, inv, w, x0, ax);
      otf_origin(cy, inv, h, y0, ay);
      const int x = x0 + ij / 10, y = y0 + ij % 10;
      const bool ok = gp < npts && x >= 0 && x < w && y >= 0 && y < h;
      const float* src = fl + ((b * h + y) * w + x) * d + sg * 4;
#pragma unroll
      for (int k = 0; k < OTF_NCH; ++k) {
        v[r][k][0] = v[r][k][1] = v[r][k][2] = v[r][k][3] = 0.f;
        if (k < nch && ok) load16(v[r][k], src + k * 32);
      }
    }
#pragma unroll
    for (int r = 0; r < OTF_RPI; ++r) {
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < OTF_NCH; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) dot += q[k][e] * v[r][k][e];
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) dot += __shfl_xor(dot, off, 64);
      const int gp = r0 + 8 * r + g;
      if (sg == 0 && gp < npts) tile[gp] = dot * rsqrt_d;
    }
  }
  __builtin_amdgcn_wave_barrier();  // the tile is this wave's own

  const int ctot = levels * 81;
  for (int c = lane; c < ctot; c += 64) {
    const int l = c / 81, t = c % 81;
    const int ix = t / 9, iy = t % 9;
    const int h = l == 0 ? hs.x : l == 1 ? hs.y : l == 2 ? hs.z : hs.w;
    const int w = l == 0 ? ws.x : l == 1 ? ws.y : l == 2 ? ws.z : ws.w;
    const float inv = 1.0f / (float)(1 << l);
    int x0, y0;
    float ax, ay;
    otf_origin(cx, inv, w, x0, ax);
    otf_origin(cy, inv, h, y0, ay);
    const float* cp = tile + l * 100 + ix * 10 + iy;
    const float val = (1 - ax) * (1 - ay) * cp[0] + ax * (1 - ay) * cp[10] +
                      (1 - ax) * ay * cp[1] + ax * ay * cp[11];
    const long long oi = NHWC ? (pix * ctot + c)
                              : ((b * ctot + c) * hw + p);
    out[oi] = from_f32<T>(val);
  }
}

// -------------------------------------------------------- convex upsample
// flow: (B,2,h,w); mask: (B,576,h,w) raw conv output (the 0.25 scale of
// reference raft.py:158 is folded in here); out: (B,2,8h,8w) NCHW always.
// Each thread handles one upsampled pixel (both channels): softmax over the
// 9 mask logits, convex-combine the 3x3 neighborhood of 8*flow.
template <typename T, bool NHWC>
__global__ void convex_upsample_kernel(const T* __restrict__ flow,
                                       const T* __restrict__ mask,
                                       T* __restrict__ out, int b, int h,
                                       int w) {
  const long long hw = (long long)h * w;
  const long long total = (long long)b * hw * 64;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(i % 64);           // fy*8+fx
    const long long pix = i / 64;          // b*hw + ly*w + lx
    const long long bi = pix / hw;
    const int p = (int)(pix % hw);
    const int ly = p / w, lx = p % w;
    // 9 mask logits for this upsampled position
    float m[9], mmax = -1e30f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int ch = k * 64 + f;
      const long long mi = NHWC ? (pix * 576 + ch) : ((bi * 576 + ch) * hw + p);
      m[k] = 0.25f * to_f32<T>(mask[mi]);
      mmax = fmaxf(mmax, m[k]);
    }
    float msum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      m[k] = __expf(m[k] - mmax);
      msum += m[k];
    }
    const float rs = 1.0f / msum;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int yy = ly + k / 3 - 1, xx = lx + k % 3 - 1;
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
      const float wk = m[k] * rs;
      const long long fp = (long long)yy * w + xx;
      const long long f0 = NHWC ? ((bi * hw + fp) * 2 + 0)
                                : ((bi * 2 + 0) * hw + fp);
      const long long f1 = NHWC ? ((bi * hw + fp) * 2 + 1)
                                : ((bi * 2 + 1) * hw + fp);
      acc0 += wk * to_f32<T>(flow[f0]);
      acc1 += wk * to_f32<T>(flow[f1]);
    }
    const int oy = ly * 8 + f / 8, ox = lx * 8 + f % 8;
    const long long ohw = hw * 64;
    const long long op = (long long)oy * (8 * w) + ox;
    out[(bi * 2 + 0) * ohw + op] = from_f32<T>(8.f * acc0);
    out[(bi * 2 + 1) * ohw + op] = from_f32<T>(8.f * acc1);
  }
}

// ------------------------------------------------------------- GRU gates
// zr: (B, 2C, h, w) conv output; hx/rhx: persistent (B, C+X, h, w) buffers
// whose first C channels hold h / r*h; z: (B, C, h, w) scratch.
//   z = sigmoid(zr[:, :C]);  r = sigmoid(zr[:, C:2C]);  rhx[:, :C] = r * h
template <typename T, bool NHWC>
__global__ void gru_zr_kernel(const T* __restrict__ zr,
                              const T* __restrict__ hx, T* __restrict__ rhx,
                              T* __restrict__ z, int b, int c, int cx,
                              long long hw) {
  const long long total = (long long)b * c * hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    long long bi, zi0, zi1, si;  // batch, z-idx, r-idx, slice idx (h / rh)
    int ci;
    long long p;
    if (NHWC) {
      const long long pixc = i;            // b*hw*c ordering: pix-major
      const long long pix = pixc / c;
      ci = (int)(pixc % c);
      bi = pix / hw;
      p = pix % hw;
      zi0 = pix * (2 * c) + ci;
      zi1 = zi0 + c;
      si = pix * (c + cx) + ci;
    } else {
      bi = i / (c * hw);
      const long long r = i % (c * hw);
      ci = (int)(r / hw);
      p = r % hw;
      zi0 = (bi * 2 * c + ci) * hw + p;
      zi1 = zi0 + (long long)c * hw;
      si = (bi * (c + cx) + ci) * hw + p;
    }
    const float zv = 1.0f / (1.0f + __expf(-to_f32<T>(zr[zi0])));
    const float rv = 1.0f / (1.0f + __expf(-to_f32<T>(zr[zi1])));
    z[i] = from_f32<T>(zv);
    rhx[si] = from_f32<T>(rv * to_f32<T>(hx[si]));
  }
}

//   h_new = (1-z)*h + z*tanh(q), written in place into hx[:, :C]
template <typename T, bool NHWC>
__global__ void gru_out_kernel(const T* __restrict__ q,
                               const T* __restrict__ z, T* __restrict__ hx,
                               int b, int c, int cx, long long hw) {
  const long long total = (long long)b * c * hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < total; i += (long long)gridDim.x * blockDim.x) {
    long long si;
    if (NHWC) {
      const long long pix = i / c;
      const int ci = (int)(i % c);
      si = pix * (c + cx) + ci;
    } else {
      const long long bi = i / (c * hw);
      const long long r = i % (c * hw);
      si = (bi * (c + cx) + r / hw) * hw + r % hw;
    }
    const float zv = to_f32<T>(z[i]);
    const float qv = tanhf(to_f32<T>(q[i]));
    hx[si] = from_f32<T>((1.0f - zv) * to_f32<T>(hx[si]) + zv * qv);
  }
}

}  // namespace

extern "C" {

void vfa_corr_lookup(const CorrPyramid& pyr, const void* coords, void* out,
                     int levels, long long npix, int hw, int lds_floats,
                     int nhwc, int dtype, hipStream_t stream) {
  const int4 hs = {pyr.hs[0], pyr.hs[1], pyr.hs[2], pyr.hs[3]};
  const int4 ws = {pyr.ws[0], pyr.ws[1], pyr.ws[2], pyr.ws[3]};
  const float* l0 = (const float*)pyr.lvl[0];
  const float* l1 = (const float*)pyr.lvl[1];
  const float* l2 = (const float*)pyr.lvl[2];
  const float* l3 = (const float*)pyr.lvl[3];
  const float* xy = (const float*)coords;
  constexpr int PPB = 8;
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      constexpr bool NHWC = decltype(cl)::value;
      if (lds_floats > 0 && lds_floats * 4 * PPB <= 64 * 1024) {
        const dim3 grid((unsigned)((npix + PPB - 1) / PPB));
        const dim3 block(64, PPB);
        hipLaunchKernelGGL((corr_lookup_lds_kernel<T, 4, NHWC, PPB>), grid,
                           block, lds_floats * 4 * PPB, stream, l0, l1, l2,
                           l3, xy, (T*)out, levels, hs, ws, npix, hw,
                           lds_floats);
      } else {
        const long long total = npix * levels * 81;
        const int grid = (int)min((total + 255) / 256, (long long)16384);
        hipLaunchKernelGGL((corr_lookup_gmem_kernel<T, 4, NHWC>), dim3(grid),
                           dim3(256), 0, stream, l0, l1, l2, l3, xy, (T*)out,
                           levels, hs, ws, npix, hw);
      }
    });
  });
}

void vfa_corr_otf(const void* f1, const CorrPyramid& f2, const void* coords,
                  void* out, int levels, long long npix, int hw, int d,
                  int nhwc, int dtype, hipStream_t stream) {
  if (npix <= 0) return;
  const int4 hs = {f2.hs[0], f2.hs[1], f2.hs[2], f2.hs[3]};
  const int4 ws = {f2.ws[0], f2.ws[1], f2.ws[2], f2.ws[3]};
  const dim3 grid((unsigned)((npix + OTF_WPB - 1) / OTF_WPB));
  const float rsqrt_d = 1.0f / sqrtf((float)d);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      hipLaunchKernelGGL((corr_otf_kernel<T, decltype(cl)::value>), grid,
                         dim3(64 * OTF_WPB), 0, stream, (const float*)f1,
                         (const float*)f2.lvl[0], (const float*)f2.lvl[1],
                         (const float*)f2.lvl[2], (const float*)f2.lvl[3],
                         (const float*)coords, (T*)out, levels, hs, ws, npix,
                         hw, d, rsqrt_d);
    });
  });
}

void vfa_convex_upsample(const void* flow, const void* mask, void* out, int b,
                         int h, int w, int nhwc, int dtype,
                         hipStream_t stream) {
  const long long total = (long long)b * h * w * 64;
  const int grid = (int)min((total + 255) / 256, (long long)16384);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      hipLaunchKernelGGL((convex_upsample_kernel<T, decltype(cl)::value>),
                         dim3(grid), dim3(256), 0, stream, (const T*)flow,
                         (const T*)mask, (T*)out, b, h, w);
    });
  });
}

void vfa_gru_zr(const void* zr, const void* hx, void* rhx, void* z, int b,
                int c, int cx, long long hw, int nhwc, int dtype,
                hipStream_t stream) {
  const long long total = (long long)b * c * hw;
  const int grid = (int)min((total + 255) / 256, (long long)16384);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      hipLaunchKernelGGL((gru_zr_kernel<T, decltype(cl)::value>), dim3(grid),
                         dim3(256), 0, stream, (const T*)zr, (const T*)hx,
                         (T*)rhx, (T*)z, b, c, cx, hw);
    });
  });
}

void vfa_gru_out(const void* q, const void* z, void* hx, int b, int c, int cx,
                 long long hw, int nhwc, int dtype, hipStream_t stream) {
  const long long total = (long long)b * c * hw;
  const int grid = (int)min((total + 255) / 256, (long long)16384);
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_bool(nhwc, [&](auto cl) {
      hipLaunchKernelGGL((gru_out_kernel<T, decltype(cl)::value>), dim3(grid),
                         dim3(256), 0, stream, (const T*)q, (const T*)z,
                         (T*)hx, b, c, cx, hw);
    });
  });
}

}  // extern "C"

