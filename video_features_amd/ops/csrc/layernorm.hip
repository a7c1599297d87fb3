// Fused LayerNorm forward for gfx950: one two-pass row kernel for
// layer_norm, layer_norm_residual and clip_embed_ln.  Pass 1 accumulates
// sum / sumsq in f32 over 16-B vectors plus a scalar tail, one reduction
// gives mean and rstd (row_stats; a row whose mean exceeds its spread gets
// its variance from a sweep of (x - mean)^2 instead), pass 2 normalises with
// the affine and rounds once.
// Memory-bound: the target is HBM BW.  Two template parameters:
//   Src    where a row element comes from (PlainSrc, ResidualSrc, EmbedSrc)
//   BLOCK  how wide the reduction is: 0 = one wave per row, 4 rows per
//          256-thread block, wave allreduce only (no LDS, no barriers, all
//          lanes loaded; d <= 4096); N = one N-thread block per row through
//          LDS (d > 4096).
#include "vfa_common.h"

namespace {

// A row source positions itself on a row (seek) and yields the row's elements
// as f32.  For the 16-B vector i: load<PASS>(i, t) fills up to two register
// vectors, value<PASS>(t, j) is its element j, keep(i, t) follows the last
// value of pass 1.  at<PASS>(i) is element i of the scalar tail.  PASS 1 feeds
// the statistics, PASS 2 the normalisation; PASS 0 yields the values of pass
// 1 once more and writes nothing (row_stats' second sweep).  Values are
// handed over one by one: returned as a float array they make the compiler
// pair the f16 conversions another way, which moves f16 results by a last
// bit.

// layer_norm: x[row, i]
template <typename T>
struct PlainSrc {
  using type = T;
  static constexpr int VEC = 16 / sizeof(T);
  static constexpr bool kWaveOnly = false;
  const T* x;
  __device__ void seek(long long row, int d) { x += row * d; }
  template <int PASS> __device__ void load(int i, T (*t)[VEC]) const {
    load16(t[0], x + (long long)i * VEC);
  }
  template <int PASS> __device__ float value(T (*t)[VEC], int j) const {
    return to_f32<T>(t[0][j]);
  }
  __device__ void keep(int, T (*)[VEC]) const {}
  template <int PASS> __device__ float at(int i) const {
    return to_f32<T>(x[i]);
  }
};

// layer_norm_residual: s = x + res is written once, rounded, in pass 1 and
// read back in pass 2, so y is the stored s normalised with the mean and
// variance of the f32 sums (removes the separate add kernel + one full
// re-read).  Each thread re-reads only what it wrote itself.
template <typename T>
struct ResidualSrc {
  using type = T;
  static constexpr int VEC = 16 / sizeof(T);
  static constexpr bool kWaveOnly = false;
  const T* x;
  const T* res;
  T* s;
  __device__ void seek(long long row, int d) {
    x += row * d; res += row * d; s += row * d;
  }
  template <int PASS> __device__ void load(int i, T (*t)[VEC]) const {
    const long long o = (long long)i * VEC;
    if constexpr (PASS == 2) return load16(t[0], s + o);
    load16(t[0], x + o);
    load16(t[1], res + o);
  }
  template <int PASS> __device__ float value(T (*t)[VEC], int j) const {
    if constexpr (PASS == 2) return to_f32<T>(t[0][j]);
    const float v = to_f32<T>(t[0][j]) + to_f32<T>(t[1][j]);
    if constexpr (PASS == 1) t[0][j] = from_f32<T>(v);
    return v;
  }
  __device__ void keep(int i, T (*t)[VEC]) const {
    store16(s + (long long)i * VEC, t[0]);
  }
  template <int PASS> __device__ float at(int i) const {
    if constexpr (PASS == 2) return to_f32<T>(s[i]);
    const float v = to_f32<T>(x[i]) + to_f32<T>(res[i]);
    if constexpr (PASS == 1) s[i] = from_f32<T>(v);
    return v;
  }
};

// CLIP ViT token embedding, rows = frames * (p + 1):
//   row (t, j) = (j == 0 ? cls : pe[t, j - 1]) + pos[j],  j in [0, p]
// The sum is formed in f32 in both passes (the second re-reads the sources,
// which are L2-resident, instead of a rounded intermediate), so the output
// is rounded once.  Requires d % VEC == 0; wave per row at every d.
template <typename T>
struct EmbedSrc {
  using type = T;
  static constexpr int VEC = 16 / sizeof(T);
  static constexpr bool kWaveOnly = true;
  const T* pe;   // after seek: the row's cls or patch embedding
  const T* cls;
  const T* pos;  // after seek: pos[j]
  int p;
  __device__ void seek(long long row, int d) {
    const long long t = row / (p + 1);
    const int j = (int)(row % (p + 1));
    pe = j == 0 ? cls : pe + (t * p + (j - 1)) * d;
    pos += (long long)j * d;
  }
  template <int PASS> __device__ void load(int i, T (*t)[VEC]) const {
    load16(t[0], pe + (long long)i * VEC);
    load16(t[1], pos + (long long)i * VEC);
  }
  template <int PASS> __device__ float value(T (*t)[VEC], int j) const {
    return to_f32<T>(t[0][j]) + to_f32<T>(t[1][j]);
  }
  __device__ void keep(int, T (*)[VEC]) const {}
  template <int PASS> __device__ float at(int i) const {
    return to_f32<T>(pe[i]) + to_f32<T>(pos[i]);
  }
};

// Sum a and b over the threads that share a row; every thread gets both.
// On the block path every thread of the block has to call it, and a barrier
// has to separate two calls.
template <int BLOCK>
__device__ __forceinline__ void row_allreduce(float& a, float& b, int tid) {
  if constexpr (BLOCK == 0) {
    a = wave_allreduce_sum(a);
    b = wave_allreduce_sum(b);
  } else {
    constexpr int NWAVES = BLOCK / 64;
    __shared__ float red[2][NWAVES];  // per-wave partials
    a = wave_reduce_sum(a);
    b = wave_reduce_sum(b);
    if ((tid & 63) == 0) { red[0][tid >> 6] = a; red[1][tid >> 6] = b; }
    __syncthreads();
    a = b = 0.f;
    for (int w = 0; w < NWAVES; ++w) { a += red[0][w]; b += red[1][w]; }
  }
}

// mean and 1/std of a row from its f32 sum and sum of squares.  The one
// place that forms the variance.  sumsq/d - mean^2 loses log2(1 + mean^2/var)
// bits to cancellation, so it stands only where that is at most one bit
// (var > mean^2, which also makes it positive).  A row that fails this is
// swept once more, out of the caches it was just read into: centred(m, s1,
// m2) returns the row's sums of x - m and (x - m)^2.  s1 takes the rounding
// of the first sum out of the mean, and m2/d, the spread about m, is at
// least 0 and above the variance by (s1/d)^2, the square of a rounding
// error.  Every thread of a row decides alike.
template <typename F>
__device__ __forceinline__ void row_stats(float sum, float sumsq, int d,
                                          float eps, float& mean, float& rstd,
                                          F centred) {
  mean = sum / d;
  float var = sumsq / d - mean * mean;
  if (__builtin_expect(!(var > mean * mean), 0)) {
    float s1 = 0.f, m2 = 0.f;
    centred(mean, s1, m2);
    mean += s1 / d;
    var = m2 / d;
  }
  rstd = rsqrtf(var + eps);
}

template <typename T, typename Src, int BLOCK>
__global__ void ln_rows_kernel(Src src, const T* __restrict__ weight,
                               const T* __restrict__ bias, T* __restrict__ out,
                               long long rows, int d, float eps) {
  constexpr int VEC = 16 / sizeof(T);
  constexpr bool WAVE = BLOCK == 0;
  constexpr int STRIDE = WAVE ? 64 : BLOCK;  // threads sharing one row
  const long long row =
      WAVE ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (row >= rows) return;
  const int tid = WAVE ? threadIdx.x & 63 : threadIdx.x;
  src.seek(row, d);
  T* y = out + row * d;
  const int dvec = d / VEC;

  float sum = 0.f, sumsq = 0.f;
  for (int i = tid; i < dvec; i += STRIDE) {
    T t[2][VEC];
    src.template load<1>(i, t);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float v = src.template value<1>(t, j);
      sum += v;
      sumsq += v * v;
    }
    src.keep(i, t);
  }
  for (int i = dvec * VEC + tid; i < d; i += STRIDE) {
    float v = src.template at<1>(i);
    sum += v;
    sumsq += v * v;
  }
  row_allreduce<BLOCK>(sum, sumsq, tid);

  float mean, rstd;
  row_stats(sum, sumsq, d, eps, mean, rstd, [&](float m, float& s1, float& m2) {
    for (int i = tid; i < dvec; i += STRIDE) {
      T t[2][VEC];
      src.template load<0>(i, t);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float c = src.template value<0>(t, j) - m;
        s1 += c;
        m2 += c * c;
      }
    }
    for (int i = dvec * VEC + tid; i < d; i += STRIDE) {
      float c = src.template at<0>(i) - m;
      s1 += c;
      m2 += c * c;
    }
    if constexpr (!WAVE) __syncthreads();
    row_allreduce<BLOCK>(s1, m2, tid);
  });

  for (int i = tid; i < dvec; i += STRIDE) {
    T t[2][VEC], tw[VEC], tb[VEC], ty[VEC];
    src.template load<2>(i, t);
    load16(tw, weight + (long long)i * VEC);
    load16(tb, bias + (long long)i * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float n = (src.template value<2>(t, j) - mean) * rstd;
      ty[j] = from_f32<T>(n * to_f32<T>(tw[j]) + to_f32<T>(tb[j]));
    }
    store16(y + (long long)i * VEC, ty);
  }
  for (int i = dvec * VEC + tid; i < d; i += STRIDE) {
    float n = (src.template at<2>(i) - mean) * rstd;
    y[i] = from_f32<T>(n * to_f32<T>(weight[i]) + to_f32<T>(bias[i]));
  }
}

// wave per row for d <= 4096 (and for a wave-only source), else one
// 512-thread block per row
template <typename Src>
void launch_ln_rows(Src src, const void* w, const void* b, void* out,
                    long long rows, int d, float eps, hipStream_t stream) {
  using T = typename Src::type;
  if (rows <= 0) return;
  if (Src::kWaveOnly || d <= 4096) {
    hipLaunchKernelGGL((ln_rows_kernel<T, Src, 0>),
                       dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream,
                       src, (const T*)w, (const T*)b, (T*)out, rows, d, eps);
    return;
  }
  if constexpr (!Src::kWaveOnly) {
    hipLaunchKernelGGL((ln_rows_kernel<T, Src, 512>), dim3((unsigned)rows),
                       dim3(512), 0, stream, src, (const T*)w, (const T*)b,
                       (T*)out, rows, d, eps);
  }
}

}  // namespace

extern "C" void vfa_layer_norm(const void* in, const void* w, const void* b,
                               void* out, long long rows, int d, float eps,
                               int dtype, hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    launch_ln_rows(PlainSrc<T>{(const T*)in}, w, b, out, rows, d, eps, stream);
  });
}

// d % 8 == 0 (checked by the binding)
extern "C" void vfa_clip_embed_ln(const void* pe, const void* cls,
                                  const void* pos, const void* w,
                                  const void* b, void* out, long long rows,
                                  int p, int d, float eps, int dtype,
                                  hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    launch_ln_rows(EmbedSrc<T>{(const T*)pe, (const T*)cls, (const T*)pos, p},
                   w, b, out, rows, d, eps, stream);
  });
}

extern "C" void vfa_layer_norm_residual(const void* x, const void* res,
                                        const void* w, const void* b,
                                        void* y, void* s_out, long long rows,
                                        int d, float eps, int dtype,
                                        hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    launch_ln_rows(ResidualSrc<T>{(const T*)x, (const T*)res, (T*)s_out}, w,
                   b, y, rows, d, eps, stream);
  });
}
