// Fused InstanceNorm2d (+optional ReLU) for gfx950.
//
// RAFT's fnet uses InstanceNorm after nearly every conv (reference
// raft_src/extractor.py:118-192).  PyTorch lowers InstanceNorm to
// batch_norm with per-(b,c) stats: one statistics kernel + one transform
// kernel + a separate ReLU — three full HBM round-trips.  This kernel does
// the whole thing in one dispatch (stats pass + normalize pass back to
// back; the tile usually stays in L2 between the passes).
//
// No affine (RAFT's InstanceNorm2d(affine=False)); fp32 accumulation.
//
// NCHW: one block per (b, c), threads grid-stride HW (coalesced).
// NHWC: one block per (b, chunk of 64 channels); lane = channel, the
// block's 4 sub-rows stride over pixels so reads stay coalesced.
#include "vfa_common.h"

namespace {

// Mean and variance of a plane of n values, for both layouts, from the f32
// sums of x - k and (x - k)^2 about the plane's first value k.  With m the
// mean of x - k, s2/n - m^2 loses log2(1 + m^2/var) bits to cancellation; k
// is a sample of the plane, so that is a bit or two whatever offset the
// plane carries, and a constant plane gives exactly 0.  It stands where at
// most 4 bits go (m^2 <= 15 var, which also makes it non-negative).  A first
// value further out (an outlier) sets `centre`: the kernel then sweeps the
// plane once more for the sums of x - mean and (x - mean)^2 and hands them
// to centred(): s1 takes the rounding of the first sum out of the mean, and
// m2/n, the spread about the old mean, is at least 0 and above the variance
// by (s1/n)^2, the square of a rounding error.
struct PlaneStats {
  float mean, var;
  bool centre;
  __device__ PlaneStats(float k, float sum, float sumsq, int n) {
    const float m = sum / n;
    mean = k + m;
    var = sumsq / n - m * m;
    centre = !(m * m <= 15.f * var);
  }
  __device__ void centred(float s1, float m2, int n) {
    mean += s1 / n;
    var = m2 / n;
  }
  __device__ float rstd(float eps) const { return rsqrtf(var + eps); }
};

template <typename T, bool RELU>
__global__ void in2d_nchw_kernel(const T* __restrict__ x, T* __restrict__ out,
                                 int hw, float eps) {
  const long long base = (long long)blockIdx.x * hw;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int nwave = blockDim.x / 64;
  __shared__ float red[2][16];
  // a and b summed over the block, in every thread; a barrier has to
  // separate two calls
  auto block_sum = [&](float& a, float& b) {
    a = wave_allreduce_sum(a);
    b = wave_allreduce_sum(b);
    if (lane == 0) { red[0][wave] = a; red[1][wave] = b; }
    __syncthreads();
    a = wave_allreduce_sum(lane < nwave ? red[0][lane] : 0.f);
    b = wave_allreduce_sum(lane < nwave ? red[1][lane] : 0.f);
  };

  const float k = to_f32<T>(x[base]);
  float s = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < hw; i += blockDim.x) {
    const float v = to_f32<T>(x[base + i]) - k;
    s += v;
    s2 += v * v;
  }
  block_sum(s, s2);
  PlaneStats st(k, s, s2, hw);
  if (__builtin_expect(st.centre, 0)) {  // block-uniform
    float s1 = 0.f, m2 = 0.f;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) {
      const float d = to_f32<T>(x[base + i]) - st.mean;
      s1 += d;
      m2 += d * d;
    }
    __syncthreads();
    block_sum(s1, m2);
    st.centred(s1, m2, hw);
  }
  const float mean = st.mean, rstd = st.rstd(eps);
  for (int i = threadIdx.x; i < hw; i += blockDim.x) {
    float v = (to_f32<T>(x[base + i]) - mean) * rstd;
    if (RELU) v = fmaxf(v, 0.f);
    out[base + i] = from_f32<T>(v);
  }
}

// NHWC: grid (chunks_per_batch, B); block (64, ROWS). lane = channel within
// the 64-wide chunk, sub-row strides over pixels.
template <typename T, bool RELU, int ROWS>
__global__ void in2d_nhwc_kernel(const T* __restrict__ x, T* __restrict__ out,
                                 int c, int hw, float eps) {
  const int ch = blockIdx.x * 64 + threadIdx.x;  // channel
  const int row = threadIdx.y;
  const long long base = (long long)blockIdx.y * hw * c;
  __shared__ float red[2][ROWS][64];
  // a and b summed over the ROWS sub-rows of each lane, in every sub-row;
  // a barrier has to separate two calls
  auto column_sum = [&](float& a, float& b) {
    red[0][row][threadIdx.x] = a;
    red[1][row][threadIdx.x] = b;
    __syncthreads();
    a = red[0][0][threadIdx.x];
    b = red[1][0][threadIdx.x];
#pragma unroll
    for (int r = 1; r < ROWS; ++r) {
      a += red[0][r][threadIdx.x];
      b += red[1][r][threadIdx.x];
    }
  };

  float k = 0.f, s = 0.f, s2 = 0.f;
  if (ch < c) {
    k = to_f32<T>(x[base + ch]);
    for (int p = row; p < hw; p += ROWS) {
      const float v = to_f32<T>(x[base + (long long)p * c + ch]) - k;
      s += v;
      s2 += v * v;
    }
  }
  column_sum(s, s2);
  PlaneStats st(k, s, s2, hw);
  const bool centre = ch < c && st.centre;  // the same in a lane's sub-rows
  // some channel of this block; also the barrier between the column_sums
  if (__builtin_expect(__syncthreads_or(centre), 0)) {
    float s1 = 0.f, m2 = 0.f;
    if (centre) {
      for (int p = row; p < hw; p += ROWS) {
        const float d = to_f32<T>(x[base + (long long)p * c + ch]) - st.mean;
        s1 += d;
        m2 += d * d;
      }
    }
    column_sum(s1, m2);
    if (centre) st.centred(s1, m2, hw);
  }
  const float mean = st.mean, rstd = st.rstd(eps);
  if (ch < c) {
    for (int p = row; p < hw; p += ROWS) {
      const long long i = base + (long long)p * c + ch;
      float v = (to_f32<T>(x[i]) - mean) * rstd;
      if (RELU) v = fmaxf(v, 0.f);
      out[i] = from_f32<T>(v);
    }
  }
}

template <typename T>
void launch_in2d(const void* x, void* out, int b, int c, int hw, float eps,
                 int relu, int nhwc, hipStream_t stream) {
  if (nhwc) {
    // 16 pixel sub-rows per block: enough waves in flight to hide the
    // strided-load latency of the two passes (941us -> bandwidth-bound
    // at ROWS=4 this kernel was 3x off the HBM floor)
    const dim3 grid((c + 63) / 64, b);
    const dim3 block(64, 16);
    if (relu)
      hipLaunchKernelGGL((in2d_nhwc_kernel<T, true, 16>), grid, block, 0,
                         stream, (const T*)x, (T*)out, c, hw, eps);
    else
      hipLaunchKernelGGL((in2d_nhwc_kernel<T, false, 16>), grid, block, 0,
                         stream, (const T*)x, (T*)out, c, hw, eps);
  } else {
    const dim3 grid(b * c);
    const dim3 block(256);
    if (relu)
      hipLaunchKernelGGL((in2d_nchw_kernel<T, true>), grid, block, 0, stream,
                         (const T*)x, (T*)out, hw, eps);
    else
      hipLaunchKernelGGL((in2d_nchw_kernel<T, false>), grid, block, 0, stream,
                         (const T*)x, (T*)out, hw, eps);
  }
}

}  // namespace

extern "C" {

void vfa_instance_norm2d(const void* x, void* out, int b, int c, int hw,
                         float eps, int relu, int nhwc, int dtype,
                         hipStream_t stream) {
  dispatch_dtype(dtype, [&](auto t) {
    launch_in2d<typename decltype(t)::type>(x, out, b, c, hw, eps, relu, nhwc,
                                            stream);
  });
}

}  // extern "C"
