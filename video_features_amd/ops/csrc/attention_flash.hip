// MFMA flash attention for ViT on gfx950 (bf16, head_dim = 64).
//
// Consumes the packed qkv projection output directly — (B, N, 3, H, 64)
// bf16, no permute/contiguous copies — and writes (B, N, H*64) ready for
// the output projection.  ViT-length sequences (N <= 64) run the
// register-resident flash_qkv_regs_kernel (described at its definition).
// The general flash_qkv_kernel, any N: one workgroup (4 waves) per
// (batch*head, 64-query-row block); KV tiles of 64 keys staged per tile:
//   K as [key][d]      (row-major, +8-element row pad -> conflict-free
//                       ds_read_b128 of 16 distinct rows, guide G4)
//   V as [d][key]      (transposed at staging so the PV B-fragment reads
//                       16 B contiguous)
// Each wave owns 16 query rows:
//   QK^T : 4x2 v_mfma_f32_16x16x32_bf16 per kv tile (A = Q frag from LDS,
//          B = K frag from LDS, both 16 B contiguous reads)
//   online softmax in C-fragment registers (rowmax/rowsum over the 16-lane
//   column group via 4 shfl_xor each; m/l/O-rescale per kv tile)
//   P -> LDS (bf16, wave-local) -> A-fragment reads; PV accumulates into
//   the O C-fragments via MFMA with C = O.
//
// Fragment layouts (v_mfma_f32_16x16x32_bf16, verified by the
// mfma_gemm16 probe + GPU numerics tests):
//   A[i][k]: lane l holds i = l&15, k = (l>>4)*8 + j   (bf16x8)
//   B[k][j]: lane l holds j = l&15, k = (l>>4)*8 + j'  (bf16x8)
//   C/D[r][c]: lane l holds c = l&15, r = (l>>4)*4 + reg (f32x4)
#include "vfa_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QBLK = 64;       // query rows per workgroup (16 per wave)
constexpr int KVBLK = 64;      // keys per LDS tile
constexpr int D = 64;          // head dim (ViT-B)
constexpr int LSTR = D + 8;    // LDS row stride in elements (144 B, 16 B
                               // aligned; r*36 mod 64 distinct for r<16)

__device__ __forceinline__ float group16_max(float v) {
  // reduce over the 16-lane column group (lanes differing in bits 0..3)
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// stage one row-major (rows x 64) bf16 tile from global into LDS with row
// stride LSTR; 256 threads, uint4 (8-elem) segments, coalesced.
__device__ __forceinline__ void stage_rows(const __bf16* g, int rows,
                                           long long row_stride, __bf16* lds,
                                           int nvalid) {
  const int tid = threadIdx.x;
  for (int t = tid; t < rows * 8; t += 256) {
    const int row = t >> 3, seg = t & 7;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < nvalid)
      v = *reinterpret_cast<const uint4*>(g + row * row_stride + seg * 8);
    *reinterpret_cast<uint4*>(lds + row * LSTR + seg * 8) = v;
  }
}

// stage V transposed: global rows are keys (64 x 64), LDS is [d][key].
// Lane mapping is KEY-major: a wave's 64 lanes cover 64 distinct keys at
// one d-segment, so the transposing u16 scatter touches all 32 LDS banks
// (~2-way) instead of 4 (16-way with the seg-major mapping — PMC showed
// 3.5 conflict cycles per LDS instruction on this store).  The global
// reads lose lane-contiguity but V is L2-hot (the qkv projection just
// wrote it).
__device__ __forceinline__ void stage_vt(const __bf16* g, long long row_stride,
                                         __bf16* lds, int nvalid) {
  const int tid = threadIdx.x;
  for (int t = tid; t < KVBLK * 8; t += 256) {
    const int key = t & 63, seg = t >> 6;
    uint4 v = {0u, 0u, 0u, 0u};
    if (key < nvalid)
      v = *reinterpret_cast<const uint4*>(g + key * row_stride + seg * 8);
    const __bf16* e = reinterpret_cast<const __bf16*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) lds[(seg * 8 + j) * LSTR + key] = e[j];
  }
}

__global__ __launch_bounds__(256)
void flash_qkv_kernel(const __bf16* __restrict__ qkv,   // (B,N,3,H,D)
                      __bf16* __restrict__ out,         // (B,N,H*D)
                      int b_total, int n, int h_total, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* s_q = reinterpret_cast<__bf16*>(smem);            // [QBLK][LSTR]
  __bf16* s_k = s_q + QBLK * LSTR;                          // [KVBLK][LSTR]
  __bf16* s_vt = s_k + KVBLK * LSTR;                        // [D][LSTR]
  __bf16* s_p = s_vt + D * LSTR;                            // [4][16][LSTR]

  const int qbase = blockIdx.y * QBLK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi4 = lane >> 4;
  // grid-stride over (batch, head) pairs: ViT-sized problems have tiny
  // per-pair work (N=50), so several pairs per block amortize the block
  // launch/tail and keep the staging pipeline warm
  for (int bh = blockIdx.x; bh < b_total * h_total; bh += gridDim.x) {
  const int bi = bh / h_total, hi = bh % h_total;

  const long long row_stride = 3LL * h_total * D;
  const __bf16* q_g = qkv + ((long long)bi * n + qbase) * row_stride +
                      (long long)hi * D;                    // +0 for q
  const int n_kv0 = (n + KVBLK - 1) / KVBLK;
  if (n_kv0 == 1) {
    // ViT-length sequences (N <= 64): one KV tile — stage K and V behind a
    // SINGLE barrier (PMC: this kernel was 66% wave-parked with the
    // 3-barrier schedule); Q skips LDS entirely — each Q row is read by
    // exactly ONE wave, so its fragments load straight from global below
    const __bf16* k_g0 = qkv + (long long)bi * n * row_stride +
                         ((long long)1 * h_total + hi) * D;
    const __bf16* v_g0 = qkv + (long long)bi * n * row_stride +
                         ((long long)2 * h_total + hi) * D;
    stage_rows(k_g0, KVBLK, row_stride, s_k, n);
    stage_vt(v_g0, row_stride, s_vt, n);
  } else {
    stage_rows(q_g, QBLK, row_stride, s_q, max(0, n - qbase));
  }
  __syncthreads();

  // per-wave state: 16 query rows [wave*16, wave*16+16)
  f32x4 o_acc[4];   // d-tiles
  float m_run[4], l_run[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o_acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -1e30f; l_run[r] = 0.f; }

  const int n_kv = n_kv0;
  for (int kv = 0; kv < n_kv; ++kv) {
    const int kvbase = kv * KVBLK;
    const int valid = min(KVBLK, n - kvbase);
    if (n_kv > 1) {   // single-tile case staged K/V with Q above
      __syncthreads();
      const __bf16* k_g = qkv + ((long long)bi * n + kvbase) * row_stride +
                          ((long long)1 * h_total + hi) * D;
      const __bf16* v_g = qkv + ((long long)bi * n + kvbase) * row_stride +
                          ((long long)2 * h_total + hi) * D;
      stage_rows(k_g, KVBLK, row_stride, s_k, valid);
      stage_vt(v_g, row_stride, s_vt, valid);
      __syncthreads();
    }

    // ---- S = Q K^T for this wave's 16 rows x 64 keys
    f32x4 s_frag[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s_frag[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Q A-fragment: straight from global in the single-tile case (valid
    // rows clamped — rows >= n are never written in the epilogue)
    const int qv = max(0, n - qbase);
    const int qr = min(wave * 16 + lo, max(qv - 1, 0));
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      bf16x8 a;
      if (n_kv == 1)
        a = *reinterpret_cast<const bf16x8*>(
            q_g + (long long)qr * row_stride + kt * 32 + hi4 * 8);
      else
        a = *reinterpret_cast<const bf16x8*>(
            s_q + (wave * 16 + lo) * LSTR + kt * 32 + hi4 * 8);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
            s_k + (nt * 16 + lo) * LSTR + kt * 32 + hi4 * 8);
        s_frag[nt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, s_frag[nt], 0, 0, 0);
      }
    }

    // ---- online softmax over keys
    float p_vals[4][4];   // [nt][reg] exp values (bf16-packed later)
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        float s = s_frag[nt][r] * scale;
        if (kvbase + nt * 16 + lo >= n) s = -1e30f;
        s_frag[nt][r] = s;
        mx = fmaxf(mx, s);
      }
      mx = group16_max(mx);
      const float m_new = fmaxf(m_run[r], mx);
      alpha[r] = __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float rowsum = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float p = __expf(s_frag[nt][r] - m_new);
        p_vals[nt][r] = p;
        rowsum += p;
      }
      l_run[r] = l_run[r] * alpha[r] + group16_sum(rowsum);
    }
    // rescale O by alpha (per row r)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) o_acc[t][r] *= alpha[r];

    // ---- P through LDS (wave-local) into A-fragment layout
    __bf16* p_lds = s_p + wave * 16 * LSTR;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p_lds[(hi4 * 4 + r) * LSTR + nt * 16 + lo] = (__bf16)p_vals[nt][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- O += P V
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      bf16x8 a = *reinterpret_cast<const bf16x8*>(
          p_lds + lo * LSTR + kt * 32 + hi4 * 8);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        bf16x8 bfr = *reinterpret_cast<const bf16x8*>(
            s_vt + (nt * 16 + lo) * LSTR + kt * 32 + hi4 * 8);
        o_acc[nt] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfr, o_acc[nt], 0, 0, 0);
      }
    }
  }

  // ---- normalize + write (B, N, H*D)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int grow = qbase + wave * 16 + hi4 * 4 + r;
    if (grow >= n) continue;
    const float inv_l = 1.0f / l_run[r];
    __bf16* orow = out + ((long long)bi * n + grow) * (h_total * D) +
                   (long long)hi * D;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      orow[nt * 16 + lo] = (__bf16)(o_acc[nt][r] * inv_l);
  }
  __syncthreads();   // LDS K/V reuse by the next (b, h) pair
  }
}

// ---------------------------------------------------------------------------
// Register-resident attention for ViT-length sequences (n <= 64, one KV
// tile).  A unit is one (b, h) pair x one block of 32 queries; one WAVE owns
// a unit, and waves walk the units from a flat index (wave, wave + #waves,
// ...), so there is no workgroup barrier anywhere.
//
//   S^T = K Q^T   v_mfma_f32_32x32x16_bf16, A = K (key row on the lane),
//                 B = Q^T (query on the lane); both fragments are 16-B global
//                 loads of 8 contiguous d, rows clamped to n - 1.  The result
//                 has the QUERY on the lane (col = lane & 31) and 32 of its
//                 64 keys in registers: key = 32 kt + (reg & 3) + 8 (reg >> 2)
//                 + 4 (lane >> 5); the other 32 sit in lane ^ 32.
//   softmax       max and sum over the lane's registers + one
//                 v_permlane32_swap each between the two halves; padded keys
//                 are -inf before the max; P rounded to bf16 once, the sum
//                 taken from the f32 values, 1 / l applied after PV.
//   O^T = V^T P^T P^T is the B operand straight from the S^T registers:
//                 registers 8s .. 8s+7 of key tile kt are k-step s, so
//                 element j of lane half h is key 32 kt + 16 s + 8 (j >> 2) +
//                 4 h + (j & 3), and the V^T A fragment follows that order.
//                 O^T has the query on the lane and d = 32 dt + 8 g + 4 h +
//                 (0..3) in register group g; a v_permlane32_swap per dword
//                 pairs the halves into 16-B stores.
//
// V is the one operand in LDS: a wave-private row-major [64 key][64 d] image
// (16-B writes, rows clamped so every row is finite), read back transposed
// with ds_read_b64_tr_b16.  Row stride 192 B.  Bank check (bank = (addr / 4)
// % 64, conflicts counted per 32-lane half): a half reads 4 consecutive keys
// x 64 B; the rows start 48 banks apart, i.e. at banks 0, 48, 32, 16 (+ a
// constant), each covering 16 banks -> all 64 banks once, conflict degree 1.
// (With 128-B rows keys q and q + 2 would share banks: degree 2.)  Every
// lane's address is 8-B aligned and inside the padded image; EXEC is all
// ones (the unit loop is wave-uniform, no lane returns early).
//
// The next unit's K / Q / V loads are issued right after the QK MFMAs, in
// front of the softmax, and land in registers while the current unit
// finishes.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int RSTR = 192;                  // V image row stride, bytes
constexpr int RIMG = 64 * RSTR;            // one wave's V image, bytes
constexpr int RWAVES = 4;                  // waves per block
constexpr int RBLOCKS = 768;               // 3 blocks per CU x 256 CUs

struct RegsLoads {
  bf16x8 k[2][4];   // [key tile][k-step of 16 d]
  bf16x8 q[4];
  uint4 v[8];       // 64 keys x 8 segments, unit idx = i * 64 + lane
};

__device__ __forceinline__ void regs_load(RegsLoads& ld,
                                          const __bf16* __restrict__ qkv,
                                          int u, int nqb, int n, int h_total,
                                          int lane) {
  const int pair = u / nqb, qb = u - pair * nqb;
  const int bi = pair / h_total, hi = pair - bi * h_total;
  const long long row_stride = 3LL * h_total * D;
  const __bf16* base = qkv + (long long)bi * n * row_stride + (long long)hi * D;
  const int r = lane & 31, h8 = (lane >> 5) * 8;
  const __bf16* qp = base + (long long)min(qb * 32 + r, n - 1) * row_stride + h8;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    ld.q[s] = *reinterpret_cast<const bf16x8*>(qp + s * 16);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    const __bf16* kp = base + (long long)h_total * D +
                       (long long)min(kt * 32 + r, n - 1) * row_stride + h8;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      ld.k[kt][s] = *reinterpret_cast<const bf16x8*>(kp + s * 16);
  }
  const __bf16* vp = base + 2LL * h_total * D + (lane & 7) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    ld.v[i] = *reinterpret_cast<const uint4*>(
        vp + (long long)min(i * 8 + (lane >> 3), n - 1) * row_stride);
}

// The 8 transposed reads of d tile DT (byte offset 64 DT in a row): read m
// takes keys 8 m + 4 h + (0..3) -> fragment (kt = m >> 2, s = (m >> 1) & 1),
// elements 4 (m & 1) .. 4 (m & 1) + 3.  One asm block, so no result is used
// before the lgkmcnt wait at its end.
#define VFA_TR8(OFF)                                            \
  asm volatile(                                                 \
      "ds_read_b64_tr_b16 %0, %8 offset:" #OFF "+0\n\t"         \
      "ds_read_b64_tr_b16 %1, %8 offset:" #OFF "+1536\n\t"      \
      "ds_read_b64_tr_b16 %2, %8 offset:" #OFF "+3072\n\t"      \
      "ds_read_b64_tr_b16 %3, %8 offset:" #OFF "+4608\n\t"      \
      "ds_read_b64_tr_b16 %4, %8 offset:" #OFF "+6144\n\t"      \
      "ds_read_b64_tr_b16 %5, %8 offset:" #OFF "+7680\n\t"      \
      "ds_read_b64_tr_b16 %6, %8 offset:" #OFF "+9216\n\t"      \
      "ds_read_b64_tr_b16 %7, %8 offset:" #OFF "+10752\n\t"     \
      "s_waitcnt lgkmcnt(0)"                                    \
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]),     \
        "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])      \
      : "v"(tr_addr)                                            \
      : "memory")

__device__ __forceinline__ bf16x8 regs_join(u32x2 lo, u32x2 hi) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8, v);
}

__global__ __launch_bounds__(RWAVES * 64)
__attribute__((amdgpu_waves_per_eu(3, 3)))
void flash_qkv_regs_kernel(const __bf16* __restrict__ qkv,   // (B,N,3,H,D)
                           __bf16* __restrict__ out,         // (B,N,H*D)
                           int units, int nqb, int n, int h_total,
                           float scale) {
  __shared__ __attribute__((aligned(16))) char s_v[RWAVES * RIMG];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = gridDim.x * RWAVES;
  int u = blockIdx.x * RWAVES + wave;
  if (u >= units) return;                                    // whole wave
  char* img = s_v + wave * RIMG;
  const int r = lane & 31, h = lane >> 5;
  // staging write of load i: key i * 8 + (lane >> 3), segment lane & 7
  char* st_addr = img + (lane >> 3) * RSTR + (lane & 7) * 16;
  // transposed read: lane 4q + p of 16-lane group g gives key q + 4h, d
  // 16 (g & 1) + 4 p; key block and d tile go into the offset immediate
  const unsigned tr_addr =
      (unsigned)(size_t)img +   // LDS pointers are 32-bit offsets
      (((lane & 15) >> 2) + 4 * h) * RSTR + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;

  RegsLoads cur;
  regs_load(cur, qkv, u, nqb, n, h_total, lane);
  for (; u < units; u += nwaves) {
    // ---- V image (this wave's own; LDS operations of a wave are ordered)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<uint4*>(st_addr + i * 8 * RSTR) = cur.v[i];

    // ---- S^T = K Q^T
    f32x16 st[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[kt][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur.k[kt][s], cur.q[s],
                                                         st[kt], 0, 0, 0);
    }

    // ---- next unit's loads (a wave without one re-reads its own unit)
    const int un = (u + nwaves < units) ? u + nwaves : u;
    RegsLoads nxt;
    regs_load(nxt, qkv, un, nqb, n, h_total, lane);

    // ---- softmax over the query's 64 keys: 32 here, 32 in lane ^ 32
    float mx = -INFINITY;
    // (the empty asm keeps the 32 loop-invariant compare masks from being
    // hoisted into 64 SGPRs)
    int nl = n - 4 * h;
    asm volatile("" : "+v"(nl));
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = 32 * kt + (e & 3) + 8 * (e >> 2);   // + 4 h
        const float s = key < nl ? st[kt][e] * scale : -INFINITY;
        st[kt][e] = s;
        mx = fmaxf(mx, s);
      }
    {
      const unsigned b = __float_as_uint(mx);
      const u32x2 sw = __builtin_amdgcn_permlane32_swap(b, b, false, false);
      mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    }
    float l = 0.f;
    bf16x8 pf[2][2];                 // [key tile][k-step]: P^T B fragments
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __expf(st[kt][e] - mx);   // 0 for a padded key
        l += p;
        pf[kt][e >> 3][e & 7] = (__bf16)p;
      }
    {
      const unsigned b = __float_as_uint(l);
      const u32x2 sw = __builtin_amdgcn_permlane32_swap(b, b, false, false);
      l = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    const float inv_l = 1.0f / l;

    // ---- O^T = V^T P^T, one 32-d tile at a time; store
    const int pair = u / nqb, qb = u - pair * nqb;
    const int bi = pair / h_total, hi = pair - bi * h_total;
    const int qrow = qb * 32 + r;
    __bf16* orow = out + ((long long)bi * n + min(qrow, n - 1)) * (h_total * D) +
                   (long long)hi * D + 8 * h;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      u32x2 t[8];
      if (dt == 0) VFA_TR8(0); else VFA_TR8(64);
      f32x16 o;
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              regs_join(t[4 * kt + 2 * s], t[4 * kt + 2 * s + 1]), pf[kt][s],
              o, 0, 0, 0);
      // register group g holds d = 8 g + 4 h + (0..3): the two halves of a
      // 16-B run sit in lanes l and l ^ 32.  One v_permlane32_swap per dword
      // (vdst = group g, src = group g + 1) leaves d = 8 g .. 8 g + 7 in the
      // lower half and 8 (g + 1) .. 8 (g + 1) + 7 in the upper one.
      typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
      uint4 w[2];
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        bf16x4 a, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = (__bf16)(o[4 * g + e] * inv_l);
          b[e] = (__bf16)(o[4 * g + 4 + e] * inv_l);
        }
        const u32x2 ua = __builtin_bit_cast(u32x2, a);
        const u32x2 ub = __builtin_bit_cast(u32x2, b);
        const u32x2 x = __builtin_amdgcn_permlane32_swap(ua[0], ub[0], false, false);
        const u32x2 y = __builtin_amdgcn_permlane32_swap(ua[1], ub[1], false, false);
        w[g >> 1] = uint4{x[0], y[0], x[1], y[1]};
      }
      if (qrow < n) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
          *reinterpret_cast<uint4*>(orow + 32 * dt + 16 * g) = w[g];
      }
    }
    cur = nxt;
  }
}

// layout probe: D(16x16) = A(16x32) @ B(32x16), row-major f32 in/out
__global__ void mfma_gemm16_kernel(const float* a, const float* b, float* d) {
  const int l = threadIdx.x, lo = l & 15, hi4 = l >> 4;
  bf16x8 av, bv;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    av[j] = (__bf16)a[lo * 32 + hi4 * 8 + j];
    bv[j] = (__bf16)b[(hi4 * 8 + j) * 16 + lo];
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) d[(hi4 * 4 + r) * 16 + lo] = c[r];
}

}  // namespace

extern "C" {

void vfa_flash_qkv(const void* qkv, void* out, int b, int n, int h,
                   float scale, int variant, hipStream_t stream) {
  if ((long long)b * h <= 0 || n <= 0) return;
  if (n <= KVBLK && variant == 0) {
    // ViT-length path: one wave per (pair, 32-query block), waves walk the
    // units from a flat index.  3 blocks of 4 waves per CU (48 KiB of LDS
    // and at most 168 VGPRs each): 3072 waves, 3 units each at 384 x 12
    const int nqb = (n + 31) / 32;
    const int units = b * h * nqb;
    dim3 grid(min((units + RWAVES - 1) / RWAVES, RBLOCKS));
    hipLaunchKernelGGL(flash_qkv_regs_kernel, grid, dim3(RWAVES * 64), 0,
                       stream, (const __bf16*)qkv, (__bf16*)out, units, nqb,
                       n, h, scale);
    return;
  }
  // cap grid.x: blocks grid-stride over (b, h) pairs (4 blocks/CU fit)
  dim3 grid(min(b * h, 2048), (n + QBLK - 1) / QBLK);
  size_t lds = (size_t)(QBLK + KVBLK + D + 4 * 16) * LSTR * sizeof(__bf16);
  hipLaunchKernelGGL(flash_qkv_kernel, grid, dim3(256), lds, stream,
                     (const __bf16*)qkv, (__bf16*)out, b, n, h, scale);
}

void vfa_mfma_gemm16(const void* a, const void* b, void* d,
                     hipStream_t stream) {
  hipLaunchKernelGGL(mfma_gemm16_kernel, dim3(1), dim3(64), 0, stream,
                     (const float*)a, (const float*)b, (float*)d);
}

}  // extern "C"
