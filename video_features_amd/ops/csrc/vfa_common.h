// Common helpers for the VFA CDNA4 kernels (gfx950-only; no CUDA compat).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <type_traits>
#include "vfa_api.h"

#define VFA_WAVE 64  // CDNA4 wavefront width (not 32)

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(_e),        \
              __FILE__, __LINE__);                                             \
      abort();                                                                 \
    }                                                                          \
  } while (0)

// dtype tags used across the C-linkage launcher ABI
enum VfaDType : int { VFA_F32 = 0, VFA_BF16 = 1, VFA_F16 = 2 };

// runtime dtype tag -> compile-time type: calls f(type_tag<T>) with T =
// float / __hip_bfloat16 / __half, read back in the lambda as
// `using T = typename decltype(t)::type`; any other tag is a no-op (the
// bindings reject it, as for dispatch_act).
template <typename T>
struct type_tag { using type = T; };

template <typename F>
inline void dispatch_dtype(int dtype, F&& f) {
  switch (dtype) {
    case VFA_F32: f(type_tag<float>{}); break;
    case VFA_BF16: f(type_tag<__hip_bfloat16>{}); break;
    case VFA_F16: f(type_tag<__half>{}); break;
    default: break;
  }
}

// runtime flag -> compile-time bool: f(std::true_type) or f(std::false_type)
template <typename F>
inline void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}

template <typename T>
__device__ __forceinline__ float to_f32(T v);
template <>
__device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <>
__device__ __forceinline__ float to_f32<__half>(__half v) {
  return __half2float(v);
}

template <typename T>
__device__ __forceinline__ T from_f32(float v);
template <>
__device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}
template <>
__device__ __forceinline__ __half from_f32<__half>(float v) {
  return __float2half(v);
}

// One 16-B access for 16 / sizeof(T) elements of T: memory -> register array
// and back.  `mem` must be 16-B aligned.
template <typename T>
__device__ __forceinline__ void load16(T* reg, const T* mem) {
  using VecT = __attribute__((ext_vector_type(4))) unsigned;
  *reinterpret_cast<VecT*>(reg) = *reinterpret_cast<const VecT*>(mem);
}

template <typename T>
__device__ __forceinline__ void store16(T* mem, const T* reg) {
  using VecT = __attribute__((ext_vector_type(4))) unsigned;
  *reinterpret_cast<VecT*>(mem) = *reinterpret_cast<const VecT*>(reg);
}

// 8 bf16 in one 16-B vector <-> 8 f32 (memory-bound kernels move bf16 as
// uint4; the f32 -> bf16 direction rounds to nearest even, NaN kept quiet)
__device__ __forceinline__ void bf16x8_to_f32(const uint4& v, float* f) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(w[j] << 16);
    f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ unsigned f32_to_bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ uint4 f32_to_bf16x8(const float* f) {
  unsigned o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = f32_to_bf16_bits(f[2 * j]) | (f32_to_bf16_bits(f[2 * j + 1]) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// all-lanes variants (every lane ends with the value)
__device__ __forceinline__ float wave_allreduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_allreduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
