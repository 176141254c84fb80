// Scaffolding shared by the .hip translation units of the MI355X (gfx950)
// extension: error check, storage-dtype dispatch, MFMA vector types,
// storage load/store, tensor pointers, the current stream and the wave
// reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

#define HIP_OK(expr)                                                          \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));      \
  } while (0)

// dispatch on storage dtype (f32 | bf16)
#define DISPATCH_F32_BF16(TYPE, NAME, ...)                                    \
  switch (TYPE) {                                                             \
    case at::kFloat: {                                                        \
      using scalar_t = float;                                                 \
      __VA_ARGS__;                                                            \
      break;                                                                  \
    }                                                                         \
    case at::kBFloat16: {                                                     \
      using scalar_t = __hip_bfloat16;                                        \
      __VA_ARGS__;                                                            \
      break;                                                                  \
    }                                                                         \
    default:                                                                  \
      TORCH_CHECK(false, NAME, ": unsupported dtype ", TYPE);                 \
  }

namespace mi355x {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const __hip_bfloat16* p) {
  return __bfloat162float(*p);
}
__device__ __forceinline__ void stf(float* p, float v) { *p = v; }
__device__ __forceinline__ void stf(__hip_bfloat16* p, float v) {
  *p = __float2bfloat16(v);
}

template <typename T>
static T* dptr(torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}
template <typename T>
static const T* cdptr(const torch::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace mi355x
