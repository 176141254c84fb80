// The 128 x 128 x 32 MFMA tile step shared by the tiled GEMMs
// (gemm_kernels.hip) and the implicit-GEMM convolutions (conv_kernels.hip):
// the geometry of the LDS images, the thread map that stages an operand's
// 16-byte chunks into its image, the 16 MFMAs of one wave over one staged
// contraction block, and the storage helpers around them. How a chunk's
// ADDRESS is formed (a plain row, a gathered pixel) is the including file's
// business; everything after the load is here. The images are described in
// gemm_kernels.hip's header.
#pragma once
#include <type_traits>

#include "kernel_common.h"

// Device code that includes this header carries the no-packed-fp32-ops
// attribute; a function without it would stay a CALL from one with it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace mi355x {

namespace {

constexpr int kBM = 128, kBN = 128, kBK = 32;
constexpr int kGemmThreads = 256;

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

template <typename T>
struct Geo;
template <>
struct Geo<float> {
  static constexpr int E = 4;        // elements of a 16-byte chunk
  static constexpr int NP = 4;       // chunks a thread moves per operand
  static constexpr int PRK = 36;     // pitch of the straight image, words
  static constexpr int PKR = 144;    // pitch of the transposed image, words
  static constexpr int WORDS = 128 * 36;  // == 32 * 144
  static constexpr int RG = 8;       // row groups of a transposed load
};
template <>
struct Geo<__hip_bfloat16> {
  static constexpr int E = 8;
  static constexpr int NP = 2;
  static constexpr int PRK = 20;
  static constexpr int PKR = 20;     // transposed while storing: same image
  static constexpr int WORDS = 128 * 20;
  static constexpr int RG = 16;
};

__device__ __forceinline__ float as_f32(uint32_t u) {
  return __builtin_bit_cast(float, u);
}
// Two floats to two bf16, round to nearest even (v_cvt_pk_bf16_f32).
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
  const bf16x2 p = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, p);
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const __hip_bfloat16* p) {
  return as_f32((uint32_t)(*reinterpret_cast<const uint16_t*>(p)) << 16);
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(__hip_bfloat16* p, float v) {
  *reinterpret_cast<uint16_t*>(p) = (uint16_t)bf16_pack(v, 0.f);
}
// What a value becomes when it is stored as T and read back.
__device__ __forceinline__ float stored(float v, const float*) { return v; }
__device__ __forceinline__ float stored(float v, const __hip_bfloat16*) {
  return as_f32(bf16_pack(0.f, v) & 0xffff0000u);
}
// __syncthreads, spelled out.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Which chunks of an operand's 128 x 32 block a thread moves, and their way
// from registers into the LDS image. TR: the contraction index is the ROW of
// the source (a "transposed" operand); otherwise it is its contiguous
// dimension ("straight").
template <typename T, bool TR>
struct TileMap {
  using G = Geo<T>;
  static constexpr bool kBf16 = std::is_same<T, __hip_bfloat16>::value;
  static constexpr int kCpr = kBK / G::E;  // straight: chunks per image row

  int c;      // the thread's chunk column
  int rbase;  // its first row slot

  __device__ __forceinline__ void init(int tid) {
    if constexpr (!TR) {
      c = tid % kCpr, rbase = tid / kCpr;
    } else if constexpr (kBf16) {
      // four adjacent chunks per row and wave, 16 row pairs per wave: the
      // interleaved LDS stores of a wave then meet 32 banks (two-way)
      c = (tid >> 6) * 4 + (tid & 3), rbase = 2 * ((tid >> 2) & 15);
    } else {
      c = tid & 31, rbase = tid >> 5;
    }
  }
  // Slot j's row in the tile: an output (straight) or a contraction index.
  __device__ __forceinline__ int slot_row(int j) const {
    if constexpr (!TR) return rbase + j * (kGemmThreads / kCpr);
    else if constexpr (kBf16) return rbase + j;
    else return rbase + G::RG * j;
  }
  // The thread's chunks, already zero where the operand ends, to the image.
  // SUM (transposed only): add them into colacc[E], one sum per output of
  // the chunk.
  template <bool SUM>
  __device__ __forceinline__ void store(uint32_t* img,
                                        const u32x4 (&x)[G::NP],
                                        float* colacc) const {
    if constexpr (!TR) {
#pragma unroll
      for (int j = 0; j < G::NP; ++j)
        *reinterpret_cast<u32x4*>(&img[slot_row(j) * G::PRK + c * 4]) = x[j];
    } else if constexpr (!kBf16) {
#pragma unroll
      for (int j = 0; j < G::NP; ++j) {
        *reinterpret_cast<u32x4*>(&img[slot_row(j) * G::PKR + c * 4]) = x[j];
        if constexpr (SUM) {
#pragma unroll
          for (int e = 0; e < 4; ++e) colacc[e] += as_f32(x[j][e]);
        }
      }
    } else {
      const int p = rbase >> 1;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint32_t lo = x[0][w], hi = x[1][w];
        img[(8 * c + 2 * w) * G::PRK + p] = (lo & 0xffffu) | (hi << 16);
        img[(8 * c + 2 * w + 1) * G::PRK + p] =
            (lo >> 16) | (hi & 0xffff0000u);
        if constexpr (SUM) {
          colacc[2 * w] += as_f32(lo << 16) + as_f32(hi << 16);
          colacc[2 * w + 1] +=
              as_f32(lo & 0xffff0000u) + as_f32(hi & 0xffff0000u);
        }
      }
    }
  }
};

// The 16 MFMAs of one wave over one staged contraction block.
template <typename T, bool TA, bool TB>
__device__ __forceinline__ void multiply_block(const uint32_t* imgA,
                                               const uint32_t* imgB, int rowA,
                                               int rowB, int q,
                                               f32x4 (&acc)[4][4]) {
  using G = Geo<T>;
  if constexpr (std::is_same<T, __hip_bfloat16>::value) {
    bf16x8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const u32x4*>(
                      &imgA[(rowA + 16 * i) * G::PRK + 4 * q]));
      b[i] = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const u32x4*>(
                      &imgB[(rowB + 16 * i) * G::PRK + 4 * q]));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j],
                                                            acc[i][j], 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < kBK / 4; ++s) {
      const int k = 4 * s + q;
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = as_f32(TA ? imgA[k * G::PKR + rowA + 16 * i]
                         : imgA[(rowA + 16 * i) * G::PRK + k]);
        b[i] = as_f32(TB ? imgB[k * G::PKR + rowB + 16 * i]
                         : imgB[(rowB + 16 * i) * G::PRK + k]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j],
                                                           acc[i][j], 0, 0, 0);
    }
  }
}

inline bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
