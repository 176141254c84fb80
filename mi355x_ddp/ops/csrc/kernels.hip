// MI355X (gfx950, CDNA4) kernel pack for mi355x_ddp — written directly in
// HIP for CDNA4 (64-wide wavefronts, MFMA via __builtin_amdgcn_mfma_*,
// LDS staging). No CUDA compatibility paths, no hipify.
//
// Re-implements the native components the reference pulls in implicitly
// (SURVEY.md §2.2): N6 GEMM fwd/bwd for the toy Linear (reference
// single_gpu.py:23,25 / nn.Linear(20,1) at :50), N7 CE/MSE loss kernels
// (single_gpu.py:24, multinode_torchrun.py:46), N8 fused SGD
// (single_gpu.py:26), N9 zero_grad folded into the bucket lifecycle
// (single_gpu.py:22), and the reducer's bucket flatten/unflatten (N3).
//
// Dtypes: every kernel is templated on the STORAGE type (f32 or bf16;
// bf16 is the BASELINE.json config-2 capability). Matmul compute uses
// the exact-f32 MFMA `v_mfma_f32_16x16x4_f32` for f32 storage (no
// xf32/TF32 exists on gfx950 — cdna_hip_programming.md §3) and
// `v_mfma_f32_16x16x32_bf16` for bf16; the toy shapes are single-wave
// and latency-bound, so the MFMA path buys kernel-count and issue-slot
// economy, not FLOPs. The one exception is the fp32
// world-1 multi-step fast path (batch 32/64, K 20): `k_toy_multistep_chain`
// runs the same k-ordered fmaf chains the f32 MFMA evaluates, bit for bit,
// on the vector ALU — one row (forward) / one column (backward) per lane,
// cross-lane hand-offs by v_readlane broadcast, no LDS and no barrier —
// because those MFMA tiles discard 15/16 of their work on the serial
// critical path (3.6x faster in kernel, profiles r03a). The MFMA spec
// kernel stays selectable (set_toy_multistep_impl / MI355X_TOY_MULTISTEP).
//
// Beyond parity (design notes in docs/KERNELS.md): the multi-step
// trainers (`k_toy_multistep_spec`, `k_toy_multistep_bf16w`) run S
// sequential SGD steps per launch with LDS-resident weights; their MESH
// variants embed a per-step device-side xGMI all-reduce (p2p_mesh.h);
// `k_epoch_shard` fuses the epoch shuffle into one copy pass, and
// `k_epoch_shard_multi` gathers a whole BLOCK of epochs per launch so
// the engine's deferral spans epoch boundaries (profiles r01q).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "ops.h"
#include "p2p_mesh.h"

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

// ---------------------------------------------------------------------------
// Linear forward: Y[B,N] = X[B,K] @ W[N,K]^T + bias[N]
// One wave (64 lanes) per 16x16 output tile; K-loop of mfma_f32_16x16x4f32
// (storage loads upconvert bf16 -> f32; exact-f32 accumulate).
// Lane maps (cdna_hip_programming.md §3): A[l&15][k=l>>4], B[k=l>>4][l&15],
// C/D col=lane&15, row=(lane>>4)*4+reg.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_linear_fwd(const T* __restrict__ X, const T* __restrict__ W,
                             const T* __restrict__ bias, T* __restrict__ Y,
                             int B, int K, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;  // 4 waves/block, each one M-tile
  const int tile_m = blockIdx.x * 4 + wave;
  const int tile_n = blockIdx.y;
  if (tile_m * 16 >= B) return;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;   // A row for this lane
  const int n = tile_n * 16 + r;   // B column (j) for this lane
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + q;
    const float a = (m < B && k < K) ? ldf(&X[(size_t)m * K + k]) : 0.f;
    const float b = (n < N && k < K) ? ldf(&W[(size_t)n * K + k]) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int col = tile_n * 16 + r;
  if (col < N) {
    const float bv = bias ? ldf(&bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < B) stf(&Y[(size_t)row * N + col], acc[i] + bv);
    }
  }
}

// Split-K variant for small-M / large-K shapes (e.g. the ResNet-50 FC,
// 32x2048 @ 2048x1000): the 4 waves of a workgroup contract DISJOINT
// K-slices of the SAME 16x16 output tile and reduce partials through LDS —
// 4x the memory-level parallelism of the serial-K kernel on shapes where
// M-tiling alone cannot fill the chip.
template <typename T>
__global__ void k_linear_fwd_splitk(const T* __restrict__ X,
                                    const T* __restrict__ W,
                                    const T* __restrict__ bias,
                                    T* __restrict__ Y, int B, int K, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_m = blockIdx.x;
  const int tile_n = blockIdx.y;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;
  const int n = tile_n * 16 + r;
  const int kq = (((K + 3) / 4 + 3) / 4) * 4;  // K-slice per wave (mult of 4)
  const int k_lo = wave * kq, k_hi = min(K, (wave + 1) * kq);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k0 = k_lo; k0 < k_hi; k0 += 4) {
    const int k = k0 + q;
    const float a = (m < B && k < K) ? ldf(&X[(size_t)m * K + k]) : 0.f;
    const float b = (n < N && k < K) ? ldf(&W[(size_t)n * K + k]) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  __shared__ float red[4][64][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][lane][i] = acc[i];
  __syncthreads();
  if (wave == 0) {
    const int col = tile_n * 16 + r;
    const float bv = (bias && col < N) ? ldf(&bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < B && col < N) {
        const float v = red[0][lane][i] + red[1][lane][i] +
                        red[2][lane][i] + red[3][lane][i];
        stf(&Y[(size_t)row * N + col], v + bv);
      }
    }
  }
}

torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(x.is_cuda(), "x must be on device");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
              "shape mismatch for linear");
  TORCH_CHECK(x.scalar_type() == w.scalar_type(), "x/w dtype mismatch");
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = (int)xc.size(0), K = (int)xc.size(1), N = (int)wc.size(0);
  auto y = at::empty({B, N}, x.options());
  torch::Tensor bc;
  bool has_bias = bias.has_value();
  if (has_bias) bc = bias->contiguous();
  if (B < 64) {  // small-M: split the contraction across the block's waves
    dim3 grid(cdiv(B, 16), cdiv(N, 16));
    DISPATCH_F32_BF16(x.scalar_type(), "linear_fwd", {
      hipLaunchKernelGGL((k_linear_fwd_splitk<scalar_t>), grid, dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(xc), cdptr<scalar_t>(wc),
                         has_bias ? cdptr<scalar_t>(bc) : nullptr,
                         dptr<scalar_t>(y), B, K, N);
    });
    HIP_OK(hipGetLastError());
    return y;
  }
  dim3 grid(cdiv(B, 64), cdiv(N, 16));
  DISPATCH_F32_BF16(x.scalar_type(), "linear_fwd", {
    hipLaunchKernelGGL((k_linear_fwd<scalar_t>), grid, dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(xc), cdptr<scalar_t>(wc),
                       has_bias ? cdptr<scalar_t>(bc) : nullptr,
                       dptr<scalar_t>(y), B, K, N);
  });
  HIP_OK(hipGetLastError());
  return y;
}

// ---------------------------------------------------------------------------
// Linear weight/bias backward: dW[N,K] = dY[B,N]^T @ X[B,K]; db[N] = sum_i dY.
// Output tile (16 rows of N) x (16 cols of K) per wave; contraction over B.
// A[j][i] = dY[i][j]; B-operand[i][k] = X[i][k].
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_linear_bwd_w(const T* __restrict__ X,
                               const T* __restrict__ dY,
                               T* __restrict__ dW, T* __restrict__ dB,
                               int B, int K, int N, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_k = blockIdx.x * 4 + wave;  // K-tile (output cols)
  const int tile_n = blockIdx.y;             // N-tile (output rows)
  const int r = lane & 15;
  const int q = lane >> 4;
  const int j = tile_n * 16 + r;  // dY column for A operand
  const int k = tile_k * 16 + r;  // X column for B operand
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;  // partial db over this lane's i-chunk
  if (tile_k * 16 < K) {
    for (int i0 = 0; i0 < B; i0 += 4) {
      const int i = i0 + q;
      const float a = (i < B && j < N) ? ldf(&dY[(size_t)i * N + j]) : 0.f;
      const float b = (i < B && k < K) ? ldf(&X[(size_t)i * K + k]) : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
      if (tile_k == 0) bsum += a;  // reuse the loaded dY for db
    }
    const int col = tile_k * 16 + r;
    if (col < K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile_n * 16 + q * 4 + i;
        if (row < N) {
          T* out = &dW[(size_t)row * K + col];
          stf(out, acc[i] + (accumulate ? ldf(out) : 0.f));
        }
      }
    }
  } else if (tile_k == 0) {
    for (int i0 = 0; i0 < B; i0 += 4) {
      const int i = i0 + q;
      bsum += (i < B && j < N) ? ldf(&dY[(size_t)i * N + j]) : 0.f;
    }
  }
  if (tile_k == 0 && dB) {
    // combine the four q-chunks of lane-row r: lanes r, r+16, r+32, r+48
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (q == 0 && j < N) {
      stf(&dB[j], bsum + (accumulate ? ldf(&dB[j]) : 0.f));
    }
  }
}

void linear_bwd_weight(torch::Tensor x, torch::Tensor dy,
                       torch::Tensor dw, torch::Tensor db, bool accumulate) {
  auto xc = x.contiguous();
  auto dyc = dy.contiguous();
  TORCH_CHECK(dw.is_contiguous() && db.is_contiguous(), "grad views must be contiguous");
  const int B = (int)xc.size(0), K = (int)xc.size(1), N = (int)dyc.size(1);
  dim3 grid(cdiv(K, 64), cdiv(N, 16));
  DISPATCH_F32_BF16(x.scalar_type(), "linear_bwd_weight", {
    hipLaunchKernelGGL((k_linear_bwd_w<scalar_t>), grid, dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(xc), cdptr<scalar_t>(dyc),
                       dptr<scalar_t>(dw),
                       db.numel() ? dptr<scalar_t>(db) : nullptr,
                       B, K, N, accumulate ? 1 : 0);
  });
  HIP_OK(hipGetLastError());
}

// dX[B,K] = dY[B,N] @ W[N,K]
template <typename T>
__global__ void k_linear_bwd_x(const T* __restrict__ dY,
                               const T* __restrict__ W, T* __restrict__ dX,
                               int B, int K, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_m = blockIdx.x * 4 + wave;
  const int tile_k = blockIdx.y;
  if (tile_m * 16 >= B) return;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;   // dY row
  const int kc = tile_k * 16 + r;  // W column for B operand
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < N; j0 += 4) {
    const int j = j0 + q;
    const float a = (m < B && j < N) ? ldf(&dY[(size_t)m * N + j]) : 0.f;
    const float b = (j < N && kc < K) ? ldf(&W[(size_t)j * K + kc]) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int col = tile_k * 16 + r;
  if (col < K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < B) stf(&dX[(size_t)row * K + col], acc[i]);
    }
  }
}

// Split-N variant of dX (same rationale as k_linear_fwd_splitk: the
// contraction over N=1000+ is split across the block's 4 waves).
template <typename T>
__global__ void k_linear_bwd_x_splitk(const T* __restrict__ dY,
                                      const T* __restrict__ W,
                                      T* __restrict__ dX, int B, int K, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_m = blockIdx.x;
  const int tile_k = blockIdx.y;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;
  const int kc = tile_k * 16 + r;
  const int nq = (((N + 3) / 4 + 3) / 4) * 4;
  const int j_lo = wave * nq, j_hi = min(N, (wave + 1) * nq);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int j0 = j_lo; j0 < j_hi; j0 += 4) {
    const int j = j0 + q;
    const float a = (m < B && j < N) ? ldf(&dY[(size_t)m * N + j]) : 0.f;
    const float b = (j < N && kc < K) ? ldf(&W[(size_t)j * K + kc]) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  __shared__ float red[4][64][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][lane][i] = acc[i];
  __syncthreads();
  if (wave == 0) {
    const int col = tile_k * 16 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < B && col < K) {
        stf(&dX[(size_t)row * K + col],
            red[0][lane][i] + red[1][lane][i] +
            red[2][lane][i] + red[3][lane][i]);
      }
    }
  }
}

torch::Tensor linear_bwd_input(torch::Tensor dy, torch::Tensor w) {
  auto dyc = dy.contiguous();
  auto wc = w.contiguous();
  const int B = (int)dyc.size(0), N = (int)dyc.size(1), K = (int)wc.size(1);
  auto dx = at::empty({B, K}, dy.options());
  if (B < 64) {
    dim3 grid(cdiv(B, 16), cdiv(K, 16));
    DISPATCH_F32_BF16(dy.scalar_type(), "linear_bwd_input", {
      hipLaunchKernelGGL((k_linear_bwd_x_splitk<scalar_t>), grid, dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(dyc), cdptr<scalar_t>(wc),
                         dptr<scalar_t>(dx), B, K, N);
    });
    HIP_OK(hipGetLastError());
    return dx;
  }
  dim3 grid(cdiv(B, 64), cdiv(K, 16));
  DISPATCH_F32_BF16(dy.scalar_type(), "linear_bwd_input", {
    hipLaunchKernelGGL((k_linear_bwd_x<scalar_t>), grid, dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(dyc), cdptr<scalar_t>(wc),
                       dptr<scalar_t>(dx), B, K, N);
  });
  HIP_OK(hipGetLastError());
  return dx;
}

// ---------------------------------------------------------------------------
// Standalone bf16 MFMA GEMM: Y[B,N] = X[B,K] @ W[N,K]^T (+bias), f32
// accumulate via v_mfma_f32_16x16x32_bf16 (the gfx950 2xK form). One wave
// per 16x16 tile, K consumed 32 at a time, 8 bf16 per lane per operand.
// A: lane l holds A[l&15][(l>>4)*8 + j], j=0..7; B-op: W[l&15][(l>>4)*8+j];
// C/D: col=lane&15, row=(lane>>4)*4+reg (cdna_hip_programming.md §3).
// Used for larger HipLinear shapes in bf16 models; verified against torch
// in tests/test_kernels_gpu.py.
// ---------------------------------------------------------------------------
__global__ void k_gemm_bf16(const __hip_bfloat16* __restrict__ X,
                            const __hip_bfloat16* __restrict__ W,
                            const __hip_bfloat16* __restrict__ bias,
                            __hip_bfloat16* __restrict__ Y,
                            int B, int K, int N) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_m = blockIdx.x * 4 + wave;
  const int tile_n = blockIdx.y;
  if (tile_m * 16 >= B) return;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;
  const int n = tile_n * 16 + r;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    bf16x8 a{}, b{};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + q * 8 + j;
      a[j] = (m < B && k < K)
                 ? *reinterpret_cast<const __bf16*>(&X[(size_t)m * K + k])
                 : (__bf16)0.f;
      b[j] = (n < N && k < K)
                 ? *reinterpret_cast<const __bf16*>(&W[(size_t)n * K + k])
                 : (__bf16)0.f;
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  const int col = tile_n * 16 + r;
  if (col < N) {
    const float bv = bias ? ldf(&bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < B) stf(&Y[(size_t)row * N + col], acc[i] + bv);
    }
  }
}

torch::Tensor gemm_bf16(torch::Tensor x, torch::Tensor w,
                        c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = (int)xc.size(0), K = (int)xc.size(1), N = (int)wc.size(0);
  auto y = at::empty({B, N}, x.options());
  torch::Tensor bc;
  bool has_bias = bias.has_value();
  if (has_bias) bc = bias->contiguous();
  dim3 grid(cdiv(B, 64), cdiv(N, 16));
  hipLaunchKernelGGL(k_gemm_bf16, grid, dim3(256), 0, cur_stream(),
                     cdptr<__hip_bfloat16>(xc), cdptr<__hip_bfloat16>(wc),
                     has_bias ? cdptr<__hip_bfloat16>(bc) : nullptr,
                     dptr<__hip_bfloat16>(y), B, K, N);
  HIP_OK(hipGetLastError());
  return y;
}

// ---------------------------------------------------------------------------
// Cross-entropy with probability targets (torch semantics:
// loss = mean_i [ -sum_c t_ic * log_softmax(y_i)_c ]).
// One wave per row; lanes stride over C; wave shuffle reductions (wave=64).
// probs/tsum/loss are saved in f32 regardless of storage dtype.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_ce_fwd(const T* __restrict__ Y, const T* __restrict__ Tg,
                         float* __restrict__ P, float* __restrict__ tsum,
                         float* __restrict__ loss,  // pre-zeroed scalar
                         int B, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* y = Y + (size_t)row * C;
  const T* t = Tg + (size_t)row * C;
  float* p = P + (size_t)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, ldf(&y[c]));
  m = wave_max(m);
  float se = 0.f, ts = 0.f, ty = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float yv = ldf(&y[c]);
    const float tv = ldf(&t[c]);
    se += __expf(yv - m);
    ts += tv;
    ty += tv * yv;
  }
  se = wave_sum(se); ts = wave_sum(ts); ty = wave_sum(ty);
  const float inv_se = 1.f / se;
  for (int c = lane; c < C; c += 64) p[c] = __expf(ldf(&y[c]) - m) * inv_se;
  if (lane == 0) {
    tsum[row] = ts;
    const float logZ = m + __logf(se);
    atomicAdd(loss, (ts * logZ - ty) / (float)B);
  }
}

std::vector<torch::Tensor> ce_fwd(torch::Tensor y, torch::Tensor t) {
  auto yc = y.contiguous();
  auto tc = t.contiguous();
  TORCH_CHECK(tc.sizes() == yc.sizes(),
              "ce: probability targets must match the output shape (got ",
              tc.sizes(), " vs ", yc.sizes(), ")");
  const int B = (int)yc.size(0), C = (int)yc.size(1);
  auto f32opt = yc.options().dtype(at::kFloat);
  auto probs = at::empty({B, C}, f32opt);
  auto tsum = at::empty({B}, f32opt);
  auto loss = at::zeros({}, f32opt);
  dim3 grid(cdiv(B, 4));
  DISPATCH_F32_BF16(y.scalar_type(), "ce_fwd", {
    hipLaunchKernelGGL((k_ce_fwd<scalar_t>), grid, dim3(256), 0, cur_stream(),
                       cdptr<scalar_t>(yc), cdptr<scalar_t>(tc),
                       probs.data_ptr<float>(), tsum.data_ptr<float>(),
                       loss.data_ptr<float>(), B, C);
  });
  HIP_OK(hipGetLastError());
  return {loss, probs, tsum};
}

// dY = (tsum_row * p - t) * grad_scale / B
template <typename T>
__global__ void k_ce_bwd(const float* __restrict__ P, const T* __restrict__ Tg,
                         const float* __restrict__ tsum, T* __restrict__ dY,
                         float scale, int B, int C,
                         const float* __restrict__ gout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)B * C;
  if (i >= n) return;
  // gout: the incoming scalar grad (autograd's seed) read on-device —
  // folds the dy*gout elementwise multiply into this kernel (one fewer
  // launch per training step on the generic path)
  const float s = gout ? scale * *gout : scale;
  const int row = (int)(i / C);
  stf(&dY[i], (tsum[row] * P[i] - ldf(&Tg[i])) * s);
}

torch::Tensor ce_bwd(torch::Tensor probs, torch::Tensor t,
                     torch::Tensor tsum, double grad_scale,
                     c10::optional<torch::Tensor> gout) {
  const int B = (int)probs.size(0), C = (int)probs.size(1);
  auto tc = t.contiguous();
  auto dy = at::empty({B, C}, tc.options());
  const int64_t n = (int64_t)B * C;
  const float* gp = nullptr;
  if (gout.has_value()) {
    TORCH_CHECK(gout->is_cuda() && gout->numel() == 1 &&
                gout->scalar_type() == at::kFloat,
                "ce_bwd gout must be a device f32 scalar");
    gp = gout->data_ptr<float>();
  }
  DISPATCH_F32_BF16(tc.scalar_type(), "ce_bwd", {
    hipLaunchKernelGGL((k_ce_bwd<scalar_t>), dim3(cdiv(n, 256)), dim3(256), 0,
                       cur_stream(), probs.data_ptr<float>(),
                       cdptr<scalar_t>(tc), tsum.data_ptr<float>(),
                       dptr<scalar_t>(dy), (float)(grad_scale / B), B, C, gp);
  });
  HIP_OK(hipGetLastError());
  return dy;
}

// ---------------------------------------------------------------------------
// MSE: loss = mean((y - t)^2); dY = 2 (y - t) * grad_scale / numel
// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_mse_fwd(const T* __restrict__ Y, const T* __restrict__ Tg,
                          float* __restrict__ loss,  // pre-zeroed
                          int64_t n, float inv_n) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float d = ldf(&Y[i]) - ldf(&Tg[i]);
    acc += d * d;
  }
  acc = wave_sum(acc);
  __shared__ float warp_part[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) warp_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += warp_part[w];
    atomicAdd(loss, s * inv_n);
  }
}

torch::Tensor mse_fwd(torch::Tensor y, torch::Tensor t) {
  auto yc = y.contiguous();
  auto tc = t.contiguous();
  // Full-size equality, like ce_fwd: equal-NUMEL shape mismatches (e.g.
  // [B,1] vs [B]) would compute elementwise here while torch's
  // F.mse_loss broadcasts the pair to [B,B] — a silent numeric
  // divergence. The reference's usage always has matching shapes, so a
  // hard error is safe.
  TORCH_CHECK(tc.sizes() == yc.sizes(), "mse: target shape ", tc.sizes(),
              " != output shape ", yc.sizes());
  const int64_t n = yc.numel();
  auto loss = at::zeros({}, yc.options().dtype(at::kFloat));
  const int blocks = (int)std::min<int64_t>(cdiv(n, 256), 2048);
  DISPATCH_F32_BF16(y.scalar_type(), "mse_fwd", {
    hipLaunchKernelGGL((k_mse_fwd<scalar_t>), dim3(blocks), dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(yc), cdptr<scalar_t>(tc),
                       loss.data_ptr<float>(), n, 1.f / (float)n);
  });
  HIP_OK(hipGetLastError());
  return loss;
}

template <typename T>
__global__ void k_mse_bwd(const T* __restrict__ Y, const T* __restrict__ Tg,
                          T* __restrict__ dY, float scale, int64_t n,
                          const float* __restrict__ gout) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float s = gout ? scale * *gout : scale;  // see k_ce_bwd
  if (i < n) stf(&dY[i], (ldf(&Y[i]) - ldf(&Tg[i])) * s);
}

torch::Tensor mse_bwd(torch::Tensor y, torch::Tensor t, double grad_scale,
                      c10::optional<torch::Tensor> gout) {
  auto yc = y.contiguous();
  auto tc = t.contiguous();
  const int64_t n = yc.numel();
  auto dy = at::empty_like(yc);
  const float* gp = nullptr;
  if (gout.has_value()) {
    TORCH_CHECK(gout->is_cuda() && gout->numel() == 1 &&
                gout->scalar_type() == at::kFloat,
                "mse_bwd gout must be a device f32 scalar");
    gp = gout->data_ptr<float>();
  }
  DISPATCH_F32_BF16(y.scalar_type(), "mse_bwd", {
    hipLaunchKernelGGL((k_mse_bwd<scalar_t>), dim3(cdiv(n, 256)), dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(yc), cdptr<scalar_t>(tc),
                       dptr<scalar_t>(dy), (float)(2.0 * grad_scale / n), n,
                       gp);
  });
  HIP_OK(hipGetLastError());
  return dy;
}

// ---------------------------------------------------------------------------
// Fused SGD over a flat bucket (+ fold zero_grad): p -= lr * g; g = 0.
// 4 elements per lane (16 B for f32, 8 B for bf16); bucket lengths are
// padded to a multiple of 4 elements by the reducer.
// ---------------------------------------------------------------------------
__global__ void k_sgd_flat_f32(float4* __restrict__ p, float4* __restrict__ g,
                               float lr, int64_t n4, int zero) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 gv = g[i];
  float4 pv = p[i];
  pv.x -= lr * gv.x; pv.y -= lr * gv.y; pv.z -= lr * gv.z; pv.w -= lr * gv.w;
  p[i] = pv;
  if (zero) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// bf16 variant: 4 elements = one 8-byte ushort4 per lane (vectorized load;
// hipcc does not auto-vectorize scalar bf16 — guide G13)
__global__ void k_sgd_flat_bf16(ushort4* __restrict__ p, ushort4* __restrict__ g,
                                float lr, int64_t n4, int zero) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  ushort4 gv = g[i];
  ushort4 pv = p[i];
  unsigned short* gs = &gv.x;
  unsigned short* ps = &pv.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float pf = __bfloat162float(*reinterpret_cast<__hip_bfloat16*>(ps + j));
    const float gf = __bfloat162float(*reinterpret_cast<__hip_bfloat16*>(gs + j));
    const __hip_bfloat16 out = __float2bfloat16(pf - lr * gf);
    ps[j] = *reinterpret_cast<const unsigned short*>(&out);
  }
  p[i] = pv;
  if (zero) g[i] = make_ushort4(0, 0, 0, 0);
}

void sgd_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
              double lr, bool zero_grad) {
  TORCH_CHECK(param_flat.is_cuda() && param_flat.is_contiguous() &&
              grad_flat.is_contiguous(), "flat buffers must be contiguous");
  TORCH_CHECK(param_flat.numel() % 4 == 0,
              "bucket length must be padded to a multiple of 4");
  const int64_t n4 = param_flat.numel() / 4;
  const dim3 grid(cdiv(n4, 256));
  if (param_flat.scalar_type() == at::kFloat) {
    hipLaunchKernelGGL(k_sgd_flat_f32, grid, dim3(256), 0, cur_stream(),
                       reinterpret_cast<float4*>(param_flat.data_ptr()),
                       reinterpret_cast<float4*>(grad_flat.data_ptr()),
                       (float)lr, n4, zero_grad ? 1 : 0);
  } else if (param_flat.scalar_type() == at::kBFloat16) {
    hipLaunchKernelGGL(k_sgd_flat_bf16, grid, dim3(256), 0, cur_stream(),
                       reinterpret_cast<ushort4*>(param_flat.data_ptr()),
                       reinterpret_cast<ushort4*>(grad_flat.data_ptr()),
                       (float)lr, n4, zero_grad ? 1 : 0);
  } else {
    TORCH_CHECK(false, "sgd_flat: unsupported dtype");
  }
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Bucket flatten/unflatten: one launch per bucket moves all
// member tensors <-> their byte ranges of the flat bucket via a precomputed
// per-block copy plan. plan row (int64 x3): [src_addr_bytes,
// bucket_byte_offset, nbytes]. Offsets are 4-element aligned and torch
// allocations are 256-B aligned, so 8-byte vector moves cover whole chunks
// for both f32 and bf16; tails go bytewise.
// ---------------------------------------------------------------------------
static constexpr int64_t BYTES_PER_BLOCK = 8192;

template <bool INTO_BUCKET>
__global__ void k_bucket_copy(char* __restrict__ bucket,
                              const int64_t* __restrict__ plan,
                              int zero_src) {
  const int64_t* row = plan + (int64_t)blockIdx.x * 3;
  char* tp = reinterpret_cast<char*>(row[0]);  // tensor chunk
  char* bp = bucket + row[1];                  // bucket segment
  const int64_t n = row[2];
  char* src = INTO_BUCKET ? tp : bp;
  char* dst = INTO_BUCKET ? bp : tp;
  const int64_t n8 = n >> 3;
  uint64_t* s8 = reinterpret_cast<uint64_t*>(src);
  uint64_t* d8 = reinterpret_cast<uint64_t*>(dst);
  for (int64_t i = threadIdx.x; i < n8; i += blockDim.x) {
    d8[i] = s8[i];
    if (zero_src) s8[i] = 0;  // fold zero_grad into the gather
  }
  for (int64_t i = (n8 << 3) + threadIdx.x; i < n; i += blockDim.x) {
    dst[i] = src[i];
    if (zero_src) src[i] = 0;
  }
}

torch::Tensor build_copy_plan(const std::vector<torch::Tensor>& tensors,
                              const std::vector<int64_t>& offsets,
                              torch::Device device) {
  std::vector<int64_t> rows;
  for (size_t t = 0; t < tensors.size(); ++t) {
    TORCH_CHECK(tensors[t].is_contiguous(), "bucket members must be contiguous");
    const int64_t esz = tensors[t].element_size();
    const int64_t nbytes = tensors[t].numel() * esz;
    const int64_t addr = (int64_t)(uintptr_t)tensors[t].data_ptr();
    const int64_t byte_off = offsets[t] * esz;
    for (int64_t base = 0; base < nbytes; base += BYTES_PER_BLOCK) {
      rows.push_back(addr + base);
      rows.push_back(byte_off + base);
      rows.push_back(std::min(BYTES_PER_BLOCK, nbytes - base));
    }
  }
  auto plan = torch::from_blob(rows.data(), {(int64_t)rows.size() / 3, 3},
                               torch::kInt64).clone();
  return plan.to(device);
}

void flatten_into(torch::Tensor bucket, torch::Tensor plan,
                  int64_t total_blocks, bool zero_src) {
  hipLaunchKernelGGL((k_bucket_copy<true>), dim3((uint32_t)total_blocks),
                     dim3(256), 0, cur_stream(),
                     reinterpret_cast<char*>(bucket.data_ptr()),
                     plan.data_ptr<int64_t>(), zero_src ? 1 : 0);
  HIP_OK(hipGetLastError());
}

void unflatten_from(torch::Tensor bucket, torch::Tensor plan, int64_t total_blocks) {
  hipLaunchKernelGGL((k_bucket_copy<false>), dim3((uint32_t)total_blocks),
                     dim3(256), 0, cur_stream(),
                     reinterpret_cast<char*>(bucket.data_ptr()),
                     plan.data_ptr<int64_t>(), 0);
  HIP_OK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Epoch shard gather with an IN-KERNEL seeded permutation: dest row i of
// this rank's shard copies source row perm(seed, rank + i*world) of the
// device-resident dataset. perm is a seeded bijection on [0, n) (mix of
// add/odd-multiply/xorshift rounds on ceil-log2 bits with cycle-walking),
// so one linear copy pass replaces torch.randperm's radix sort + two
// index_select launches (~30 us -> ~3 us per epoch). Python mirror:
// mi355x_ddp.ops.perm_index (tested for permutation property + parity).
// ---------------------------------------------------------------------------
__device__ __host__ __forceinline__ uint32_t mix_bijection(
    uint32_t x, uint32_t k_mask, uint32_t n, uint32_t c0, uint32_t m0,
    uint32_t c1, uint32_t m1) {
  // each op is bijective on (k_mask+1)-space; cycle-walk back into [0, n)
  do {
    x = (x + c0) & k_mask;
    x = (x * m0) & k_mask;       // m0 odd
    x ^= x >> 3;
    x = (x + c1) & k_mask;
    x = (x * m1) & k_mask;       // m1 odd
    x ^= x >> 5;
  } while (x >= n);
  return x;
}

__device__ __host__ __forceinline__ void shard_consts(
    uint32_t seed, uint32_t* c0, uint32_t* m0, uint32_t* c1, uint32_t* m1) {
  uint32_t z = seed * 0x9E3779B9u + 0x7F4A7C15u;
  z ^= z >> 15; z *= 0x2C1B3C6Du; z ^= z >> 12;
  *c0 = z;
  *m0 = (z >> 8) | 1u;
  z = z * 0x297A2D39u + 0x68E31DA4u; z ^= z >> 16;
  *c1 = z;
  *m1 = (z >> 7) | 1u;
}

template <typename T>
__global__ void k_epoch_shard(const T* __restrict__ X, const T* __restrict__ Tg,
                              T* __restrict__ xs, T* __restrict__ ts,
                              int n, int K, int per_rank, int rank, int world,
                              uint32_t k_mask, uint32_t c0, uint32_t m0,
                              uint32_t c1, uint32_t m1) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int cols = K + 1;
  if (tid >= per_rank * cols) return;
  const int i = tid / cols;
  const int c = tid - i * cols;
  const uint32_t p = (uint32_t)(rank + (size_t)i * world);
  const uint32_t src = mix_bijection(p, k_mask, (uint32_t)n, c0, m0, c1, m1);
  if (c < K) xs[(size_t)i * K + c] = X[(size_t)src * K + c];
  else       ts[i] = Tg[src];
}

std::vector<torch::Tensor> epoch_shard(torch::Tensor X, torch::Tensor Tg,
                                       int64_t seed, int64_t rank,
                                       int64_t world) {
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && Tg.is_contiguous());
  const int n = (int)X.size(0), K = (int)X.size(1);
  TORCH_CHECK(Tg.size(0) == n && Tg.size(1) == 1, "targets must be [n,1]");
  const int per_rank = n / (int)world;
  auto xs = at::empty({per_rank, K}, X.options());
  auto ts = at::empty({per_rank, 1}, Tg.options());
  uint32_t k_mask = 1;
  while ((int64_t)k_mask + 1 < n) k_mask = (k_mask << 1) | 1u;
  uint32_t c0, m0, c1, m1;
  shard_consts((uint32_t)seed, &c0, &m0, &c1, &m1);
  const int total = per_rank * (K + 1);
  DISPATCH_F32_BF16(X.scalar_type(), "epoch_shard", {
    hipLaunchKernelGGL((k_epoch_shard<scalar_t>), dim3(cdiv(total, 256)),
                       dim3(256), 0, cur_stream(), cdptr<scalar_t>(X),
                       cdptr<scalar_t>(Tg), dptr<scalar_t>(xs),
                       dptr<scalar_t>(ts), n, K, per_rank, (int)rank,
                       (int)world, k_mask, c0, m0, c1, m1);
  });
  HIP_OK(hipGetLastError());
  return {xs, ts};
}

// Multi-EPOCH variant: one launch gathers `epochs` consecutive epoch
// shards (seeds seed0, seed0+1, …) into one contiguous buffer pair —
// block e of the output is bitwise-identical to epoch_shard(X, T,
// seed0+e)'s result. This is what lets the persistent-engine deferral
// span epoch boundaries (one multistep launch per ~max_defer steps
// instead of one per epoch) and, as a side effect, gives this gather
// kernel epochs× more workgroups to fill the 256 CUs with.
template <typename T>
__global__ void k_epoch_shard_multi(const T* __restrict__ X,
                                    const T* __restrict__ Tg,
                                    T* __restrict__ xs, T* __restrict__ ts,
                                    int n, int K, int per_rank, int rank,
                                    int world, uint32_t k_mask,
                                    uint32_t seed0, int epochs) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cols = K + 1;
  const long long per_epoch = (long long)per_rank * cols;
  if (tid >= per_epoch * epochs) return;
  const int e = (int)(tid / per_epoch);
  const int t = (int)(tid - (long long)e * per_epoch);
  const int i = t / cols;
  const int c = t - i * cols;
  uint32_t c0, m0, c1, m1;
  shard_consts(seed0 + (uint32_t)e, &c0, &m0, &c1, &m1);
  const uint32_t p = (uint32_t)(rank + (size_t)i * world);
  const uint32_t src = mix_bijection(p, k_mask, (uint32_t)n, c0, m0, c1, m1);
  const size_t o = (size_t)e * per_rank + i;
  if (c < K) xs[o * K + c] = X[(size_t)src * K + c];
  else       ts[o] = Tg[src];
}

std::vector<torch::Tensor> epoch_shard_multi(torch::Tensor X, torch::Tensor Tg,
                                             int64_t seed0, int64_t epochs,
                                             int64_t rank, int64_t world) {
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && Tg.is_contiguous());
  TORCH_CHECK(epochs >= 1 && epochs <= 1 << 20, "epochs out of range");
  const int n = (int)X.size(0), K = (int)X.size(1);
  TORCH_CHECK(Tg.size(0) == n && Tg.size(1) == 1, "targets must be [n,1]");
  const int per_rank = n / (int)world;
  auto xs = at::empty({epochs * per_rank, K}, X.options());
  auto ts = at::empty({epochs * per_rank, 1}, Tg.options());
  uint32_t k_mask = 1;
  while ((int64_t)k_mask + 1 < n) k_mask = (k_mask << 1) | 1u;
  const long long total = (long long)epochs * per_rank * (K + 1);
  DISPATCH_F32_BF16(X.scalar_type(), "epoch_shard_multi", {
    hipLaunchKernelGGL((k_epoch_shard_multi<scalar_t>),
                       dim3((uint32_t)((total + 255) / 256)), dim3(256), 0,
                       cur_stream(), cdptr<scalar_t>(X), cdptr<scalar_t>(Tg),
                       dptr<scalar_t>(xs), dptr<scalar_t>(ts), n, K, per_rank,
                       (int)rank, (int)world, k_mask, (uint32_t)seed0,
                       (int)epochs);
  });
  HIP_OK(hipGetLastError());
  return {xs, ts};
}

// ---------------------------------------------------------------------------
// Fused toy training step (fwd + loss-grad + bwd [+ SGD] in ONE kernel):
// the reference hot loop single_gpu.py:21-26 for model = Linear(K,1).
// Single workgroup, 64 threads (one wave): at 84 B of gradients the step is
// launch-latency bound, so one launch replaces five (SURVEY §7 hard-part 2).
// lr > 0: apply SGD in-kernel (world-1 path — no all-reduce exists);
// lr <= 0: write grads into the bucket for the all-reduce + sgd_flat path.
// Supports B <= 128, K <= 32.
// ---------------------------------------------------------------------------
// MT = M-tiles (ceil(B/16), compile-time), KT = K-tiles (ceil(K/16)).
// Structure: one coalesced LDS burst loads X, t, w, bias up front (one
// global round trip instead of per-MFMA dependent loads), then both MFMA
// phases run off LDS with the tile accumulators interleaved so the 40-cycle
// dependent-accumulator latency of v_mfma_f32_16x16x4_f32 hides behind the
// other tile's issue (cdna_hip_programming.md §3: >=2 independent
// accumulators reach the issue rate).
template <typename T, int MT, int KT>
__global__ void k_toy_fused(const T* __restrict__ X, const T* __restrict__ Tg,
                            T* __restrict__ param, T* __restrict__ grad,
                            float* __restrict__ loss_out,
                            int B, int K, int use_mse,
                            int w_off, int b_off, float lr) {
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  __shared__ float xs[128 * 32];   // X staged [B][K]
  __shared__ float ts[128];        // targets
  __shared__ float ws[33];         // w (K) + bias at ws[32]
  __shared__ float dy_s[128];

  {  // one coalesced staging burst (independent loads, one latency trip)
    const int total = B * K;
    for (int i = lane; i < total; i += 64) xs[i] = ldf(&X[i]);
    for (int i = lane; i < B; i += 64) ts[i] = ldf(&Tg[i]);
    if (lane < K) ws[lane] = ldf(&param[w_off + lane]);
    if (lane == K) ws[32] = ldf(&param[b_off]);
  }
  __syncthreads();

  // forward: y = X @ w + b; MT interleaved 16-row tiles, j=0 column only
  const float bterm = ws[32];
  const float inv2B = 2.f / (float)B;
  float loss_acc = 0.f;
  {
    f32x4 acc[MT];
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) acc[tm] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + q;
      const float b = (r == 0 && k < K) ? ws[k] : 0.f;  // B[k][j=0]
#pragma unroll
      for (int tm = 0; tm < MT; ++tm) {
        const int m = tm * 16 + r;
        const float a = (m < B && k < K) ? xs[m * K + k] : 0.f;
        acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tm], 0, 0, 0);
      }
    }
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) {
      if (r == 0) {  // lanes 0,16,32,48 hold col j=0; rows q*4+i
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = tm * 16 + q * 4 + i;
          if (row < B) {
            const float y = acc[tm][i] + bterm;
            float dy;
            if (use_mse) {
              const float d = y - ts[row];
              loss_acc += d * d;
              dy = d * inv2B;
            } else {
              // CE over one logit: log_softmax == 0 -> loss == 0, dY == 0
              // (the reference's degenerate loss).
              dy = 0.f;
            }
            dy_s[row] = dy;
          }
        }
      }
    }
  }
  __syncthreads();

  // backward: dw_k = sum_i dY_i X[i,k]; KT interleaved K-tiles; db = sum dY
  {
    f32x4 acc[KT];
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) acc[tk] = {0.f, 0.f, 0.f, 0.f};
    // db rides a FREE output column: when K is not a multiple of 16,
    // column K of the bwd tile multiplies dY against a constant-1 operand,
    // so the bias gradient falls out of the same MFMA chain — no LDS
    // re-read, no wave_sum of 6 dependent cross-lane shuffles per step.
    const bool mfma_db = (K & 15) != 0;
    for (int i0 = 0; i0 < B; i0 += 4) {
      const int i = i0 + q;
      const float a = (r == 0 && i < B) ? dy_s[i] : 0.f;  // A[j=0][i]
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) {
        const int k = tk * 16 + r;
        const float b = (i < B && k < K) ? xs[i * K + k]
                       : (i < B && k == K && mfma_db) ? 1.f : 0.f;
        acc[tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tk], 0, 0, 0);
      }
    }
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      // D row j=0 lives in reg 0 of lanes with q==0; col = k
      if (q == 0 && k < K) {
        if (lr > 0.f) stf(&param[w_off + k], ws[k] - lr * acc[tk][0]);
        else stf(&grad[w_off + k], acc[tk][0]);
      } else if (q == 0 && k == K && mfma_db) {
        if (lr > 0.f) stf(&param[b_off], bterm - lr * acc[tk][0]);
        else stf(&grad[b_off], acc[tk][0]);
      }
    }
    if (!mfma_db) {
      float dbp = 0.f;
      for (int i = lane; i < B; i += 64) dbp += dy_s[i];
      dbp = wave_sum(dbp);
      if (lane == 0) {
        if (lr > 0.f) stf(&param[b_off], bterm - lr * dbp);
        else stf(&grad[b_off], dbp);
      }
    }
  }
  if (use_mse && loss_out) loss_acc = wave_sum(loss_acc);
  if (lane == 0 && loss_out) *loss_out = use_mse ? loss_acc / (float)B : 0.f;
}

// ---------------------------------------------------------------------------
// Multi-step persistent toy trainer: S sequential SGD steps in ONE launch.
//
// The single-step kernel above executes in ~6 us wall: ~0.3 us of MFMA and
// ~5+ us of dispatch ramp + HBM round trips for 84 B of params re-read and
// re-written every launch. Since the epoch shard is device-resident and
// consecutive steps read consecutive [B,K] slices, this kernel keeps the
// weights in LDS across steps, double-buffers the next step's X/T tile
// through registers while MFMAing the current one, and only touches HBM
// for the streamed batches plus one final param write-back. Per-step
// arithmetic (MFMA tiling, update order, bf16 rounding of the stored
// params) is IDENTICAL to k_toy_fused, so S multi-steps == S single-step
// launches bitwise; tests/test_engine_gpu.py holds it to that.
//
// World-1 only (lr applied in-kernel; no collective exists). B<=128, K<=32.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float round_store(float v);
template <>
__device__ __forceinline__ float round_store<float>(float v) { return v; }
template <>
__device__ __forceinline__ float round_store<__hip_bfloat16>(float v) {
  return __bfloat162float(__float2bfloat16(v));
}

template <typename T, int MT, int KT>
__global__ void k_toy_multistep(const T* __restrict__ X,
                                const T* __restrict__ Tg,
                                T* __restrict__ param,
                                float* __restrict__ loss_out,
                                int B, int K, int S, int use_mse,
                                int w_off, int b_off, float lr) {
  constexpr int NR = (MT * 16 * KT * 16 + 63) / 64;  // X regs per lane
  constexpr int NT = (MT * 16 + 63) / 64;            // target regs per lane
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  __shared__ float xs2[2][128 * 32];
  __shared__ float ts2[2][128];
  __shared__ float ws[33];  // w (K) + bias at ws[32]; persists across steps
  __shared__ float dy_s[128];

  if (lane < K) ws[lane] = ldf(&param[w_off + lane]);
  if (lane == K) ws[32] = ldf(&param[b_off]);

  const int total = B * K;
  float xr[NR], tr[NT];
  // prologue: step 0 tile -> regs
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int i = lane + j * 64;
    if (i < total) xr[j] = ldf(&X[i]);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int i = lane + j * 64;
    if (i < B) tr[j] = ldf(&Tg[i]);
  }

  float loss_last = 0.f;
  for (int s = 0; s < S; ++s) {
    const int buf = s & 1;
    float* xs = xs2[buf];
    float* ts = ts2[buf];
    // stage this step's regs into LDS
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int i = lane + j * 64;
      if (i < total) xs[i] = xr[j];
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int i = lane + j * 64;
      if (i < B) ts[i] = tr[j];
    }
    __syncthreads();
    // issue next step's global loads: latency hides under this step's MFMAs
    if (s + 1 < S) {
      const T* Xn = X + (size_t)(s + 1) * total;
      const T* Tn = Tg + (size_t)(s + 1) * B;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int i = lane + j * 64;
        if (i < total) xr[j] = ldf(&Xn[i]);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int i = lane + j * 64;
        if (i < B) tr[j] = ldf(&Tn[i]);
      }
    }

    // ---- forward (identical tiling to k_toy_fused) ----
    const float bterm = ws[32];
    const float inv2B = 2.f / (float)B;
    float loss_acc = 0.f;
    {
      f32x4 acc[MT];
#pragma unroll
      for (int tm = 0; tm < MT; ++tm) acc[tm] = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + q;
        const float b = (r == 0 && k < K) ? ws[k] : 0.f;
#pragma unroll
        for (int tm = 0; tm < MT; ++tm) {
          const int m = tm * 16 + r;
          const float a = (m < B && k < K) ? xs[m * K + k] : 0.f;
          acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tm], 0, 0, 0);
        }
      }
#pragma unroll
      for (int tm = 0; tm < MT; ++tm) {
        if (r == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = tm * 16 + q * 4 + i;
            if (row < B) {
              const float y = acc[tm][i] + bterm;
              float dy;
              if (use_mse) {
                const float d = y - ts[row];
                loss_acc += d * d;
                dy = d * inv2B;
              } else {
                dy = 0.f;  // degenerate 1-logit CE
              }
              dy_s[row] = dy;
            }
          }
        }
      }
    }
    __syncthreads();  // dy_s visible to all lanes before the bwd MFMAs

    // ---- backward + in-LDS SGD update ----
    const bool mfma_db = (K & 15) != 0;  // free db column (as k_toy_fused)
    {
      f32x4 acc[KT];
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) acc[tk] = {0.f, 0.f, 0.f, 0.f};
      for (int i0 = 0; i0 < B; i0 += 4) {
        const int i = i0 + q;
        const float a = (r == 0 && i < B) ? dy_s[i] : 0.f;
#pragma unroll
        for (int tk = 0; tk < KT; ++tk) {
          const int k = tk * 16 + r;
          const float b = (i < B && k < K) ? xs[i * K + k]
                         : (i < B && k == K && mfma_db) ? 1.f : 0.f;
          acc[tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[tk], 0, 0, 0);
        }
      }
      __syncthreads();  // all ws reads of this step done before the update
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) {
        const int k = tk * 16 + r;
        if (q == 0 && k < K)
          ws[k] = round_store<T>(ws[k] - lr * acc[tk][0]);
        else if (q == 0 && k == K && mfma_db)
          ws[32] = round_store<T>(bterm - lr * acc[tk][0]);
      }
    }
    if (!mfma_db) {
      float dbp = 0.f;
      for (int i = lane; i < B; i += 64) dbp += dy_s[i];
      dbp = wave_sum(dbp);
      if (lane == 0) ws[32] = round_store<T>(bterm - lr * dbp);
    }
    if (use_mse && loss_out && s == S - 1) loss_last = wave_sum(loss_acc);
    __syncthreads();
  }

  // final param write-back (one HBM trip for the whole S-step run)
  if (lane < K) stf(&param[w_off + lane], ws[lane]);
  if (lane == K) stf(&param[b_off], ws[32]);
  if (lane == 0 && loss_out) *loss_out = use_mse ? loss_last / (float)B : 0.f;
}

// ---------------------------------------------------------------------------
// Compile-time-shape multi-step trainer for the canonical toy shape.
// All loop bounds are template constants so every MFMA operand lives in a
// REGISTER, prefetched from global memory in operand layout during the
// previous step's compute (the epoch shard is L2-resident after its
// gather, so the depth-1 prefetch covers the latency). LDS is used only
// where data must cross lanes: the w vector (updated by q==0 lanes, read
// by r==0 lanes) and the per-row dY exchange between the forward readout
// and the backward MFMA. Divisions are hoisted to one reciprocal
// (2/B is exact for the reference batch 32, so dy is bitwise-unchanged).

// In-kernel mesh exchange for the multi-step trainers: scatter this
// rank's 21-float gradient vector (held one value per q==0 lane per
// K-tile, db on the free column) into every rank's mailbox, publish a
// per-step sequence number, bounded-wait for all peers, and return the
// averaged value for this lane's tile. Returns false on timeout (caller
// must set the error flag and exit).
template <int KT>
__device__ __forceinline__ bool mesh_exchange(
    float (&gval)[KT], int K_, int lane, int r, int q,
    MeshSlot* const* __restrict__ peer_slots, MeshSlot* __restrict__ my_mb,
    int mworld, float minv_world, unsigned long long sq) {
  if (q == 0) {
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (k <= K_) {
        for (int p = 0; p < mworld; ++p) peer_slots[p]->data[k] = gval[tk];
      }
    }
  }
  __threadfence_system();
  __syncthreads();
  if (lane == 0) {
    for (int p = 0; p < mworld; ++p)
      __hip_atomic_store(&peer_slots[p]->seq, sq, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
  bool timed_out = false;
  if (lane < mworld) {
    const unsigned long long t0c = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(&my_mb[lane].seq, __ATOMIC_ACQUIRE,
                             __HIP_MEMORY_SCOPE_SYSTEM) < sq) {
      if (__builtin_amdgcn_s_memrealtime() - t0c > 500000000ull) {
        timed_out = true;
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
  if (__any(timed_out)) return false;
  // system-scope fence: subsequent data reads (by OTHER lanes than the
  // acquirers) must observe the remote ranks' mailbox writes
  __threadfence_system();
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (k <= K_) {
        float sum = 0.f;
        for (int p = 0; p < mworld; ++p) sum += my_mb[p].data[k];
        gval[tk] = sum * minv_world;
      }
    }
  }
  return true;
}

// ---------------------------------------------------------------------------
// bf16 wide-MFMA variant: the whole K (<=32) contraction of the forward and
// the whole B (=32) contraction of the backward are each ONE
// v_mfma_f32_16x16x32_bf16 per tile (4 MFMAs/step vs 26 in the f32 path),
// with operands kept as raw bf16x8 registers — no per-element up-convert.
// dY is rounded to bf16 before the backward MFMA (true bf16 compute), so
// this path matches the f32-MFMA path to bf16 accuracy, not bitwise
// (tests/test_engine_gpu.py uses allclose for bf16).
// Operand map (as k_gemm_bf16): A[l&15][(l>>4)*8+j]; B[(l>>4)*8+j][l&15];
// D col=l&15, row=(l>>4)*4+reg.
// ---------------------------------------------------------------------------
template <int B_, int K_, bool MESH = false>
__global__ void __launch_bounds__(64, 1)
k_toy_multistep_bf16w(const __hip_bfloat16* __restrict__ X,
                      const __hip_bfloat16* __restrict__ Tg,
                      __hip_bfloat16* __restrict__ param,
                      float* __restrict__ loss_out,
                      int S, int use_mse, int w_off, int b_off, float lr,
                      MeshSlot* const* __restrict__ peer_slots = nullptr,
                      MeshSlot* __restrict__ my_mb = nullptr,
                      int mworld = 1, float minv_world = 1.f,
                      unsigned long long seq0 = 0,
                      unsigned int* __restrict__ mesh_err = nullptr) {
  static_assert((B_ == 32 || B_ == 64) && K_ <= 32,
                "bf16 wide path: B in {32, 64}, K<=32");
  constexpr int MT = B_ / 16;          // fwd 16-row tiles
  constexpr int BT = B_ / 32;          // bwd contraction chunks (MFMA K=32)
  constexpr int KT = (K_ + 15) / 16;   // bwd 16-col tiles
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  __shared__ float ws[33];
  __shared__ float dy_s[B_];

  if (lane < K_) ws[lane] = ldf(&param[w_off + lane]);
  if (lane == K_) ws[32] = ldf(&param[b_off]);
  const float inv2B = 2.f / (float)B_;
  // write-only LDS update: updater lanes keep w in registers (see the
  // f32 spec kernel)
  float wreg[KT];
#pragma unroll
  for (int tk = 0; tk < KT; ++tk) {
    const int k = tk * 16 + r;
    wreg[tk] = (k < K_) ? ldf(&param[w_off + ((k < K_) ? k : 0)]) : 0.f;
  }

  // Two operand register sets, DISTANCE-2 prefetch: iteration s consumes
  // set s%2 and — at the same late, off-critical-path point as before —
  // issues the loads for step s+2 into that same set. The vmcnt wait for
  // a set therefore lands a FULL iteration after its loads issued (no
  // adopt-copies, no issue at the chain head — the two failure modes of
  // the earlier pipelining attempts, kept in git history).
  struct BSet {
    bf16x8 fa[MT];      // fwd A: X[tm*16+r][q*8+j] (raw, clamped)
    bf16x8 bb[BT][KT];  // bwd B: X[bt*32 + q*8+j][tk*16+r] (raw)
    float tR[MT][4];    // targets for rows tm*16+q*4+i
  };
  BSet setA, setB;

  auto prefetch = [&](BSet& R, int s) {
    const __hip_bfloat16* Xs = X + (size_t)s * (B_ * K_);
    const __hip_bfloat16* Ts = Tg + (size_t)s * B_;
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) {
      const int m = tm * 16 + r;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = q * 8 + j;
        const int kc = (k < K_) ? k : K_ - 1;
        R.fa[tm][j] = *reinterpret_cast<const __bf16*>(&Xs[(size_t)m * K_ + kc]);
      }
    }
#pragma unroll
    for (int bt = 0; bt < BT; ++bt)
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) {
        const int k = tk * 16 + r;
        const int kc = (k < K_) ? k : K_ - 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = bt * 32 + q * 8 + j;  // batch row of this chunk
          R.bb[bt][tk][j] =
              *reinterpret_cast<const __bf16*>(&Xs[(size_t)i * K_ + kc]);
        }
      }
#pragma unroll
    for (int tm = 0; tm < MT; ++tm)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        R.tR[tm][i] = ldf(&Ts[tm * 16 + q * 4 + i]);
  };

  prefetch(setA, 0);
  if (S > 1) prefetch(setB, 1);
  float loss_last = 0.f;
  auto body = [&](BSet& R, int s) {
    const bf16x8* cfa = R.fa;
    const auto& cbb = R.bb;
    const auto& ctR = R.tR;
    // forward B-operand: w as bf16 (stored values round-trip bf16 exactly),
    // zero-padded for k >= K_ so raw garbage in A contributes nothing
    bf16x8 b8{};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = q * 8 + j;
      const float v = ws[(k < K_) ? k : K_ - 1];
      b8[j] = (r == 0 && k < K_) ? (__bf16)v : (__bf16)0.f;
    }
    const float bterm = ws[32];

    f32x4 acc[MT];
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) {
      acc[tm] = {0.f, 0.f, 0.f, 0.f};
      acc[tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cfa[tm], b8,
                                                        acc[tm], 0, 0, 0);
    }

    float loss_acc = 0.f;
    if (r == 0) {
#pragma unroll
      for (int tm = 0; tm < MT; ++tm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = tm * 16 + q * 4 + i;
          float dy = 0.f;
          if (use_mse) {
            const float d = acc[tm][i] + bterm - ctR[tm][i];
            loss_acc += d * d;
            dy = d * inv2B;
          }
          dy_s[row] = dy;
        }
    }
    __syncthreads();  // dy_s visible to all lanes

    // backward A-operands: dY rounded to bf16, one 32-row chunk per BT
    // (j-th element of chunk bt = dy[bt*32 + q*8+j]); chunks accumulate
    // into the same f32 accumulator — the full B_ contraction.
    bf16x8 a8[BT];
#pragma unroll
    for (int bt = 0; bt < BT; ++bt)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = dy_s[bt * 32 + q * 8 + j];
        a8[bt][j] = (r == 0) ? (__bf16)v : (__bf16)0.f;
      }
    f32x4 gacc[KT];
    static_assert(K_ % 16 != 0, "free db column requires K_ % 16 != 0");
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      gacc[tk] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int bt = 0; bt < BT; ++bt) {
        // db rides output column K_: constant-1 B operand on that lane
        bf16x8 bb = cbb[bt][tk];
        if (tk * 16 + r == K_) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bb[j] = (__bf16)1.f;
        }
        gacc[tk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8[bt], bb,
                                                           gacc[tk], 0, 0, 0);
      }
    }

    if (s + 2 < S) prefetch(R, s + 2);  // this set's regs dead from here

    if (use_mse && loss_out && s == S - 1) loss_last = wave_sum(loss_acc);

    if constexpr (MESH) {
      float gval[KT];
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) gval[tk] = gacc[tk][0];
      if (!mesh_exchange<KT>(gval, K_, lane, r, q, peer_slots, my_mb,
                             mworld, minv_world,
                             seq0 + (unsigned long long)s)) {
        if (lane == 0) *mesh_err = 1u;
        return false;
      }
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) gacc[tk][0] = gval[tk];
    }

#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (q == 0 && k < K_) {
        wreg[tk] = round_store<__hip_bfloat16>(wreg[tk] - lr * gacc[tk][0]);
        ws[k] = wreg[tk];
      } else if (q == 0 && k == K_) {
        ws[32] = round_store<__hip_bfloat16>(bterm - lr * gacc[tk][0]);
      }
    }
    __syncthreads();  // ws update visible before next iteration's forward
    return true;
  };

  int s = 0;
  for (; s + 2 <= S; s += 2) {
    if (!body(setA, s)) return;
    if (!body(setB, s + 1)) return;
  }
  if (s < S && !body(setA, s)) return;

  if (lane < K_) stf(&param[w_off + lane], ws[lane]);
  if (lane == K_) stf(&param[b_off], ws[32]);
  if (lane == 0 && loss_out) *loss_out = use_mse ? loss_last / (float)B_ : 0.f;
}

template <typename T, int B_, int K_, bool MESH = false>
__global__ void __launch_bounds__(64, 1)
k_toy_multistep_spec(const T* __restrict__ X, const T* __restrict__ Tg,
                     T* __restrict__ param, float* __restrict__ loss_out,
                     int S, int use_mse, int w_off, int b_off, float lr,
                     MeshSlot* const* __restrict__ peer_slots = nullptr,
                     MeshSlot* __restrict__ my_mb = nullptr,
                     int mworld = 1, float minv_world = 1.f,
                     unsigned long long seq0 = 0,
                     unsigned int* __restrict__ mesh_err = nullptr) {
  constexpr int MT = (B_ + 15) / 16;   // fwd 16-row tiles
  constexpr int KT = (K_ + 15) / 16;   // bwd 16-col tiles
  constexpr int KS = (K_ + 3) / 4;     // fwd k-steps
  constexpr int BS = (B_ + 3) / 4;     // bwd i-steps
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  __shared__ float ws[33];             // w (K_) + bias at ws[32]
  __shared__ float dy_s[MT * 16];

  if (lane < K_) ws[lane] = ldf(&param[w_off + lane]);
  if (lane == K_) ws[32] = ldf(&param[b_off]);
  const float inv2B = 2.f / (float)B_;
  // updater lanes (q==0) also keep their w values in registers so the
  // end-of-iteration update is WRITE-only to LDS (no dependent LDS read
  // on the critical path); readers still take w from LDS
  float wreg[KT];
#pragma unroll
  for (int tk = 0; tk < KT; ++tk) {
    const int k = tk * 16 + r;
    wreg[tk] = (k < K_) ? ldf(&param[w_off + ((k < K_) ? k : 0)]) : 0.f;
  }

  // Per-lane operand registers, software-pipelined: `c*` hold the step
  // being computed, `n*` receive the next step's loads (issued at the top
  // of the iteration, consumed — behind one vmcnt wait — at its end).
  // All loads are UNCONDITIONAL with clamped addresses + value selects:
  // ternary-guarded loads compile to exec-masked branch-per-element code
  // that serializes the burst (seen in the r01b ISA), selects do not.
  float cfA[MT][KS];  // fwd A: X[tm*16+r][4*kk+q]
  float cbB[KT][BS];  // bwd B: X[4*ii+q][tk*16+r]
  float ctR[MT][4];   // targets for rows tm*16+q*4+i

  auto prefetch = [&](int s) {
    const T* Xs = X + (size_t)s * (B_ * K_);
    const T* Ts = Tg + (size_t)s * B_;
    // Loads are raw (address-clamped, no value select): out-of-range
    // lanes load in-bounds garbage whose products are either multiplied
    // by a zeroed LDS-side operand (wv/av) or discarded by the guarded
    // ws/dy writes — so no per-load mask, and therefore no vmcnt wait
    // until the next iteration's first MFMA use.
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) {
      const int m = tm * 16 + r;
      const int mc = (m < B_) ? m : B_ - 1;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const int k = 4 * kk + q;
        const int kc = (k < K_) ? k : K_ - 1;
        cfA[tm][kk] = ldf(&Xs[mc * K_ + kc]);
      }
    }
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      const int kc = (k < K_) ? k : K_ - 1;
#pragma unroll
      for (int ii = 0; ii < BS; ++ii) {
        const int i = 4 * ii + q;
        const int ic = (i < B_) ? i : B_ - 1;
        cbB[tk][ii] = ldf(&Xs[ic * K_ + kc]);
      }
    }
#pragma unroll
    for (int tm = 0; tm < MT; ++tm)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tm * 16 + q * 4 + i;
        ctR[tm][i] = ldf(&Ts[(row < B_) ? row : B_ - 1]);
      }
  };

  prefetch(0);
  float loss_last = 0.f;
  for (int s = 0; s < S; ++s) {
    // batch the w reads (LDS; one unconditional read + select per kk)
    float wv[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      const int k = 4 * kk + q;
      const float v = ws[(k < K_) ? k : K_ - 1];
      wv[kk] = (r == 0 && k < K_) ? v : 0.f;
    }
    const float bterm = ws[32];

    // ---- forward: y = X @ w + b ----
    f32x4 acc[MT];
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) acc[tm] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
      for (int tm = 0; tm < MT; ++tm)
        acc[tm] = __builtin_amdgcn_mfma_f32_16x16x4f32(cfA[tm][kk], wv[kk],
                                                       acc[tm], 0, 0, 0);

    // ---- loss grad (rows live on r==0 lanes) + dY exchange ----
    float loss_acc = 0.f;
    if (r == 0) {
#pragma unroll
      for (int tm = 0; tm < MT; ++tm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = tm * 16 + q * 4 + i;
          float dy = 0.f;
          if (row < B_ && use_mse) {
            const float d = acc[tm][i] + bterm - ctR[tm][i];
            loss_acc += d * d;
            dy = d * inv2B;
          }
          if (row < B_) dy_s[row] = dy;
        }
    }
    __syncthreads();  // dy_s visible to all lanes

    // ---- backward: dw_k = sum_i dY_i X[i,k] ----
    float av[BS];
#pragma unroll
    for (int ii = 0; ii < BS; ++ii) {
      const int i = 4 * ii + q;
      const float v = dy_s[(i < B_) ? i : B_ - 1];
      av[ii] = (r == 0 && i < B_) ? v : 0.f;
    }
    f32x4 gacc[KT];
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) gacc[tk] = {0.f, 0.f, 0.f, 0.f};
    // db rides output column K_ of the bwd tile against a constant-1
    // B-operand (K_ % 16 != 0 guarantees the free column) — same MFMA
    // chain order as the single-step kernel, so history stays bitwise.
    static_assert(K_ % 16 != 0, "free db column requires K_ % 16 != 0");
#pragma unroll
    for (int ii = 0; ii < BS; ++ii)
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) {
        const int k = tk * 16 + r;
        const float bop = (k == K_) ? 1.f : cbB[tk][ii];
        gacc[tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ii], bop,
                                                        gacc[tk], 0, 0, 0);
      }

    // cur regs are dead from here: load next step's operands straight into
    // them — the vmcnt wait attaches to their first use (next iteration's
    // forward MFMA), shadowed by the update/barrier below
    if (s + 1 < S) prefetch(s + 1);

    if (use_mse && loss_out && s == S - 1) loss_last = wave_sum(loss_acc);

    if constexpr (MESH) {
      float gval[KT];
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) gval[tk] = gacc[tk][0];
      if (!mesh_exchange<KT>(gval, K_, lane, r, q, peer_slots, my_mb,
                             mworld, minv_world,
                             seq0 + (unsigned long long)s)) {
        if (lane == 0) *mesh_err = 1u;
        return;
      }
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) gacc[tk][0] = gval[tk];
    }

    // no barrier needed here: the dy_s barrier above already ordered this
    // step's ws READS (forward) before these writes
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (q == 0 && k < K_) {
        wreg[tk] = round_store<T>(wreg[tk] - lr * gacc[tk][0]);
        ws[k] = wreg[tk];
      } else if (q == 0 && k == K_) {
        ws[32] = round_store<T>(bterm - lr * gacc[tk][0]);
      }
    }
    __syncthreads();  // ws update visible before next iteration's forward
  }

  if (lane < K_) stf(&param[w_off + lane], ws[lane]);
  if (lane == K_) stf(&param[b_off], ws[32]);
  if (lane == 0 && loss_out) *loss_out = use_mse ? loss_last / (float)B_ : 0.f;
}

// ---------------------------------------------------------------------------
// Lane-parallel fmaf-chain form of the fp32 multi-step trainer (the world-1
// default for batch 32/64, K 20). The f32-input MFMA result is bit-for-bit
// a k-ordered f32 fmaf chain with one rounding per product
// (cdna_hip_programming.md §3), and the spec kernel above uses ONE column
// (forward) / ONE row (backward) of each 16x16 MFMA tile — so the same
// bits come off the vector ALU with only the useful work and no LDS:
//   forward   lane m owns row m of X:  y = fmaf(x[m][k], w[k], y), k = 0..K-1
//   loss grad all rows at once:        dy = ((y + b) - t) * (2/B)
//   backward  lane k owns column k:    g = fmaf(dy[i], x[i][k], g), i = 0..B-1
//             lane K_ multiplies by a constant 1 (the db column)
//   update    w[k] stays in lane k's register for the whole launch
//             (bias in lane K_): w -= lr * g
// B_ = 8x4 (or 16x4) and K_ = 5x4 fill the MFMA k-groups exactly, so the
// MFMA chain order is the plain index order with no padding terms. The two
// cross-lane hand-offs are broadcasts of wave-uniform values (w[k] to the
// row lanes, dy[i] to the column lanes): v_readlane_b32 with a constant
// lane puts each in an SGPR the v_fma reads directly — no LDS, no barrier.
// Operands stream through a ring of D register sets (distance-D prefetch,
// unrolled by D like the bf16 kernel's setA/setB): rows as 16-byte loads
// when VEC4 (tile base 16-byte aligned; rows are 80 B), columns as dwords.
// Loads are unconditional with clamped addresses and never pass tile S-1.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __int_as_float(
      __builtin_amdgcn_readlane(__float_as_int(v), src_lane));
}

// A tile of ones with the X tile's row pitch: the db lane (and the idle
// lanes above it) stream their backward operand from here with the same
// immediate offsets as a real column, so the constant-1 column costs no
// per-term select on the chain. Deliberately not `const`: a const device
// variable lands in the constant address space, and a pointer select
// between it and the global X pointer degrades every column load to a FLAT
// load, whose out-of-order return forces full vmcnt(0) drains.
template <int N>
struct OnesTile {
  float v[N];
  constexpr OnesTile() : v() {
    for (int i = 0; i < N; ++i) v[i] = 1.f;
  }
};
__device__ OnesTile<64 * 20> k_ones_tile{};

template <int B_, int K_, int D, bool VEC4>
__global__ void __launch_bounds__(64, 1)
k_toy_multistep_chain(const float* __restrict__ X,
                      const float* __restrict__ Tg,
                      float* __restrict__ param, float* __restrict__ loss_out,
                      int S, int use_mse, int w_off, int b_off, float lr) {
  static_assert((B_ == 32 || B_ == 64) && K_ == 20 && D >= 1,
                "chain path: B in {32, 64}, K = 20 (k_ones_tile pitch)");
  const int lane = threadIdx.x;
  const int mr = lane & (B_ - 1);  // row owned in the forward
  const float inv2B = 2.f / (float)B_;
  // w[k] in lane k, bias in lane K_ (lanes above hold an unused copy)
  float wv = param[(lane < K_) ? w_off + lane : b_off];
  // backward operand stream: column `lane` of X for lanes < K_, advancing
  // one tile per step; the ones tile (never advancing) for lane K_ and up
  const float* colp = (lane < K_) ? X + lane : k_ones_tile.v;
  const size_t cstep = (lane < K_) ? (size_t)(B_ * K_) : 0;

  struct CSet {
    float xr[K_];  // fwd: X[mr][0..K_)
    float xc[B_];  // bwd: X[0..B_)[lane] (ones on the db lane)
    float t;       // target of row mr
  };
  CSet ring[D];

  // Unconditional loads; the step index is clamped to the last tile, so
  // the D prefetches past the end re-read tile S-1 and nothing beyond it.
  auto prefetch = [&](CSet& R, int s_raw) {
    const int s = (s_raw < S) ? s_raw : S - 1;
    const float* rowp = X + (size_t)s * (B_ * K_) + mr * K_;
    if constexpr (VEC4) {
#pragma unroll
      for (int j = 0; j < K_ / 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(rowp + 4 * j);
        R.xr[4 * j + 0] = v.x;
        R.xr[4 * j + 1] = v.y;
        R.xr[4 * j + 2] = v.z;
        R.xr[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < K_; ++k) R.xr[k] = rowp[k];
    }
    R.t = Tg[(size_t)s * B_ + mr];
    const float* cp = colp + (size_t)s * cstep;
#pragma unroll
    for (int i = 0; i < B_; ++i) R.xc[i] = cp[i * K_];
  };

  float d_last = 0.f;
  auto body = [&](CSet& R, int s) {
    // ---- forward: y = X @ w, k-ordered chain from +0 ----
    float wk[K_ + 1];
#pragma unroll
    for (int k = 0; k <= K_; ++k) wk[k] = lane_bcast(wv, k);
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < K_; ++k) y = __builtin_fmaf(R.xr[k], wk[k], y);
    const float bterm = wk[K_];

    // ---- loss grad: one row per lane ----
    const float d = y + bterm - R.t;
    const float dy = use_mse ? d * inv2B : 0.f;
    d_last = d;

    // ---- backward: dw_k = sum_i dY_i X[i,k]; db on the ones lane ----
    float dyi[B_];
#pragma unroll
    for (int i = 0; i < B_; ++i) dyi[i] = lane_bcast(dy, i);
    float g = 0.f;
#pragma unroll
    for (int i = 0; i < B_; ++i) g = __builtin_fmaf(dyi[i], R.xc[i], g);

    // this set's regs are dead from here: refill them for step s + D
    prefetch(R, s + D);

    wv = wv - lr * g;
    // compiler-only ordering point between steps (one wave, no LDS)
    __builtin_amdgcn_wave_barrier();
  };

#pragma unroll
  for (int j = 0; j < D; ++j) prefetch(ring[j], j);
  int s = 0;
  for (; s + D <= S; s += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) body(ring[j], s + j);
  }
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (s + j < S) body(ring[j], s + j);

  if (lane < K_) param[w_off + lane] = wv;
  if (lane == K_) param[b_off] = wv;
  if (loss_out) {
    float loss_last = 0.f;
    if (use_mse) {
      // the spec kernel's reduction over the last step's residuals: four
      // partial sums on lanes 0/16/32/48, rows tm*16 + q*4 + i accumulated
      // in (tm, i) order, zeros elsewhere, then the same butterfly
      const int r = lane & 15, q = lane >> 4;
      float loss_acc = 0.f;
#pragma unroll
      for (int tm = 0; tm < B_ / 16; ++tm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dd = __shfl(d_last, tm * 16 + q * 4 + i, 64);
          // explicit fma: the spec kernel's `loss_acc += d * d` compiles
          // to one contracted v_fma per row; here the same source form
          // gets SLP-vectorized into v_pk_mul + separate adds instead
          if (r == 0) loss_acc = __builtin_fmaf(dd, dd, loss_acc);
        }
      loss_last = wave_sum(loss_acc);
    }
    if (lane == 0) *loss_out = use_mse ? loss_last / (float)B_ : 0.f;
  }
}

// Process-wide implementation selector for the fp32 (32|64, 20) multi-step
// fast path: the chain kernel by default, the MFMA spec kernel on request
// (tests and A/B runs need both). Initialised once from
// MI355X_TOY_MULTISTEP (chain | mfma).
enum : int { kImplChain = 0, kImplMfma = 1 };
static int impl_from_env() {
  const char* e = std::getenv("MI355X_TOY_MULTISTEP");
  if (e == nullptr || *e == '\0' || std::string(e) == "chain") return kImplChain;
  TORCH_CHECK(std::string(e) == "mfma",
              "MI355X_TOY_MULTISTEP must be 'chain' or 'mfma', got '", e, "'");
  return kImplMfma;
}
static std::atomic<int>& multistep_impl() {
  static std::atomic<int> impl{impl_from_env()};
  return impl;
}
static std::atomic<int> g_chain_depth{0};  // 0 = measured default

void set_toy_multistep_impl(const std::string& name) {
  TORCH_CHECK(name == "chain" || name == "mfma",
              "toy multistep impl must be 'chain' or 'mfma', got '", name, "'");
  multistep_impl().store(name == "chain" ? kImplChain : kImplMfma);
}
std::string get_toy_multistep_impl() {
  return multistep_impl().load() == kImplChain ? "chain" : "mfma";
}
void set_toy_multistep_chain_depth(int64_t depth) {
  TORCH_CHECK(depth == 0 || (depth >= 2 && depth <= 4),
              "chain prefetch depth must be 0 (default), 2, 3 or 4");
  g_chain_depth.store((int)depth);
}

// measured at S = 1024 on fresh tiles: D = 2 / 3 / 4 -> 335 / 329 / 319 ns/step
static constexpr int kChainDefaultDepth = 4;

template <int B_>
static void launch_toy_multistep_chain(const float* xp, const float* tp,
                                       float* pp, float* lossp, bool use_mse,
                                       int w_off, int b_off, float lr, int S) {
  int depth = g_chain_depth.load();
  if (depth == 0) depth = kChainDefaultDepth;
  // rows are 80 B, so every row start is 16-byte aligned iff the base is
  const bool vec4 = (reinterpret_cast<uintptr_t>(xp) & 15u) == 0;
  auto go = [&](auto kptr) {
    hipLaunchKernelGGL(kptr, dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp,
                       lossp, S, use_mse ? 1 : 0, w_off, b_off, lr);
  };
  auto by_depth = [&](auto vec) {
    constexpr bool V = decltype(vec)::value;
    if constexpr (B_ == 64) {
      // 85 operand registers per set: a third set spills into AGPR copies
      go(k_toy_multistep_chain<64, 20, 2, V>);
    } else {
      if (depth == 2) go(k_toy_multistep_chain<B_, 20, 2, V>);
      else if (depth == 3) go(k_toy_multistep_chain<B_, 20, 3, V>);
      else go(k_toy_multistep_chain<B_, 20, 4, V>);
    }
  };
  if (vec4) by_depth(std::true_type{});
  else by_depth(std::false_type{});
}

template <typename T>
static void launch_toy_multistep(const torch::Tensor& x, const torch::Tensor& t,
                                 torch::Tensor& param_flat, float* lossp,
                                 bool use_mse, int w_off, int b_off, float lr,
                                 int B, int K, int S) {
  const T* xp = cdptr<T>(x);
  const T* tp = cdptr<T>(t);
  T* pp = dptr<T>(param_flat);
  if constexpr (std::is_same<T, float>::value) {
    if ((B == 32 || B == 64) && K == 20 &&
        multistep_impl().load() == kImplChain) {
      if (B == 32)
        launch_toy_multistep_chain<32>(xp, tp, pp, lossp, use_mse, w_off,
                                       b_off, lr, S);
      else
        launch_toy_multistep_chain<64>(xp, tp, pp, lossp, use_mse, w_off,
                                       b_off, lr, S);
      return;
    }
  }
  if (B == 32 && K == 20) {  // the reference shape: compile-time fast path
    if constexpr (std::is_same<T, __hip_bfloat16>::value) {
      // native bf16 MFMA (16x16x32): whole contraction in one MFMA/tile
      hipLaunchKernelGGL((k_toy_multistep_bf16w<32, 20>), dim3(1), dim3(64),
                         0, cur_stream(), xp, tp, pp, lossp, S,
                         use_mse ? 1 : 0, w_off, b_off, lr);
    } else {
      hipLaunchKernelGGL((k_toy_multistep_spec<T, 32, 20>), dim3(1), dim3(64),
                         0, cur_stream(), xp, tp, pp, lossp, S,
                         use_mse ? 1 : 0, w_off, b_off, lr);
    }
    return;
  }
  if (B == 64 && K == 20) {  // batch-64 variant of the fast path
    if constexpr (std::is_same<T, __hip_bfloat16>::value) {
      // wide bf16 MFMA, backward contraction as two chained 16x16x32
      // chunks (close the fast-path matrix)
      hipLaunchKernelGGL((k_toy_multistep_bf16w<64, 20>), dim3(1), dim3(64),
                         0, cur_stream(), xp, tp, pp, lossp, S,
                         use_mse ? 1 : 0, w_off, b_off, lr);
    } else {
      hipLaunchKernelGGL((k_toy_multistep_spec<T, 64, 20>), dim3(1), dim3(64),
                         0, cur_stream(), xp, tp, pp, lossp, S,
                         use_mse ? 1 : 0, w_off, b_off, lr);
    }
    return;
  }
  auto go = [&](auto mt, auto kt) {
    hipLaunchKernelGGL((k_toy_multistep<T, decltype(mt)::value, decltype(kt)::value>),
                       dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp, lossp,
                       B, K, S, use_mse ? 1 : 0, w_off, b_off, lr);
  };
  using c1 = std::integral_constant<int, 1>;
  using c2 = std::integral_constant<int, 2>;
  using c4 = std::integral_constant<int, 4>;
  using c8 = std::integral_constant<int, 8>;
  const int mt = (B + 15) / 16, kt = (K + 15) / 16;
  if (kt <= 1) {
    if (mt <= 1) go(c1{}, c1{});
    else if (mt <= 2) go(c2{}, c1{});
    else if (mt <= 4) go(c4{}, c1{});
    else go(c8{}, c1{});
  } else {
    if (mt <= 1) go(c1{}, c2{});
    else if (mt <= 2) go(c2{}, c2{});
    else if (mt <= 4) go(c4{}, c2{});
    else go(c8{}, c2{});
  }
}

void toy_multistep(torch::Tensor x, torch::Tensor t, torch::Tensor param_flat,
                   torch::Tensor loss_out, bool use_mse,
                   int64_t w_off, int64_t b_off, double lr, int64_t batch) {
  const int B = (int)batch, K = (int)x.size(1);
  TORCH_CHECK(B <= 128 && K <= 32, "toy multistep supports B<=128, K<=32");
  TORCH_CHECK(x.is_contiguous() && t.is_contiguous());
  TORCH_CHECK(x.size(0) % B == 0, "x rows must be a multiple of batch");
  TORCH_CHECK(t.size(0) == x.size(0), "t rows must match x rows");
  TORCH_CHECK(lr > 0.0, "toy_multistep is the world-1 in-kernel-SGD path");
  const int S = (int)(x.size(0) / B);
  if (S == 0) return;
  float* lossp = nullptr;
  if (loss_out.defined() && loss_out.numel()) {
    TORCH_CHECK(loss_out.scalar_type() == at::kFloat, "loss_out must be f32");
    lossp = loss_out.data_ptr<float>();
  }
  DISPATCH_F32_BF16(x.scalar_type(), "toy_multistep", {
    launch_toy_multistep<scalar_t>(x, t, param_flat, lossp, use_mse,
                                   (int)w_off, (int)b_off, (float)lr, B, K, S);
  });
  HIP_OK(hipGetLastError());
}

void toy_multistep_mesh(torch::Tensor x, torch::Tensor t,
                        torch::Tensor param_flat, torch::Tensor loss_out,
                        bool use_mse, int64_t w_off, int64_t b_off, double lr,
                        int64_t batch, P2pMesh& mesh) {
  const int B = (int)batch, K = (int)x.size(1);
  TORCH_CHECK((B == 32 || B == 64) && K == 20,
              "mesh multistep supports the fast-path shapes "
              "(batch 32 or 64, K 20)");
  TORCH_CHECK(x.is_contiguous() && t.is_contiguous());
  TORCH_CHECK(x.size(0) % B == 0 && t.size(0) == x.size(0));
  TORCH_CHECK(lr > 0.0, "mesh multistep applies SGD in-kernel");
  const int S = (int)(x.size(0) / B);
  if (S == 0) return;
  float* lossp = nullptr;
  if (loss_out.defined() && loss_out.numel()) {
    TORCH_CHECK(loss_out.scalar_type() == at::kFloat, "loss_out must be f32");
    lossp = loss_out.data_ptr<float>();
  }
  const unsigned long long seq0 = mesh.alloc_seq((unsigned long long)S);
  const float inv = 1.f / (float)mesh.world();
  if (x.scalar_type() == at::kFloat) {
    auto go = [&](auto kptr) {
      hipLaunchKernelGGL(kptr, dim3(1), dim3(64), 0, cur_stream(),
                         cdptr<float>(x), cdptr<float>(t),
                         dptr<float>(param_flat), lossp, S,
                         use_mse ? 1 : 0, (int)w_off, (int)b_off, (float)lr,
                         mesh.peer_slots(), mesh.my_mb(), mesh.world(), inv,
                         seq0, mesh.err_flag());
    };
    if (B == 32) go(k_toy_multistep_spec<float, 32, 20, true>);
    else go(k_toy_multistep_spec<float, 64, 20, true>);
  } else if (x.scalar_type() == at::kBFloat16) {
    auto go = [&](auto kptr) {
      hipLaunchKernelGGL(kptr, dim3(1), dim3(64), 0, cur_stream(),
                         cdptr<__hip_bfloat16>(x), cdptr<__hip_bfloat16>(t),
                         dptr<__hip_bfloat16>(param_flat), lossp, S,
                         use_mse ? 1 : 0, (int)w_off, (int)b_off, (float)lr,
                         mesh.peer_slots(), mesh.my_mb(), mesh.world(), inv,
                         seq0, mesh.err_flag());
    };
    if (B == 32) go(k_toy_multistep_bf16w<32, 20, true>);
    else go(k_toy_multistep_bf16w<64, 20, true>);
  } else {
    TORCH_CHECK(false, "mesh multistep: dtype must be f32 or bf16");
  }
  HIP_OK(hipGetLastError());
}

template <typename T>
static void launch_toy_fused(const torch::Tensor& x, const torch::Tensor& t,
                             torch::Tensor& param_flat, torch::Tensor& grad_flat,
                             float* lossp, bool use_mse, int w_off, int b_off,
                             float lr, int B, int K) {
  const T* xp = cdptr<T>(x);
  const T* tp = cdptr<T>(t);
  T* pp = dptr<T>(param_flat);
  T* gp = dptr<T>(grad_flat);
  auto go = [&](auto mt, auto kt) {
    hipLaunchKernelGGL((k_toy_fused<T, decltype(mt)::value, decltype(kt)::value>),
                       dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp, gp,
                       lossp, B, K, use_mse ? 1 : 0, w_off, b_off, lr);
  };
  using c1 = std::integral_constant<int, 1>;
  using c2 = std::integral_constant<int, 2>;
  using c4 = std::integral_constant<int, 4>;
  using c8 = std::integral_constant<int, 8>;
  const int mt = (B + 15) / 16, kt = (K + 15) / 16;
  if (kt <= 1) {
    if (mt <= 1) go(c1{}, c1{});
    else if (mt <= 2) go(c2{}, c1{});
    else if (mt <= 4) go(c4{}, c1{});
    else go(c8{}, c1{});
  } else {
    if (mt <= 1) go(c1{}, c2{});
    else if (mt <= 2) go(c2{}, c2{});
    else if (mt <= 4) go(c4{}, c2{});
    else go(c8{}, c2{});
  }
}

void toy_fused_fwd_bwd(torch::Tensor x, torch::Tensor t,
                       torch::Tensor param_flat, torch::Tensor grad_flat,
                       torch::Tensor loss_out, bool use_mse,
                       int64_t w_off, int64_t b_off, double lr) {
  const int B = (int)x.size(0), K = (int)x.size(1);
  TORCH_CHECK(B <= 128 && K <= 32, "toy fused kernel supports B<=128, K<=32");
  TORCH_CHECK(x.is_contiguous() && t.is_contiguous());
  float* lossp = nullptr;
  if (loss_out.defined() && loss_out.numel()) {
    TORCH_CHECK(loss_out.scalar_type() == at::kFloat, "loss_out must be f32");
    lossp = loss_out.data_ptr<float>();
  }
  DISPATCH_F32_BF16(x.scalar_type(), "toy_fused_fwd_bwd", {
    launch_toy_fused<scalar_t>(x, t, param_flat, grad_flat, lossp, use_mse,
                               (int)w_off, (int)b_off, (float)lr, B, K);
  });
  HIP_OK(hipGetLastError());
}

}  // namespace mi355x
