// Fused short-sequence self-attention for gfx950 (MI355X), forward and
// backward, over the PACKED in-projection output.
//
//   qkv  [B, N, 3E]  columns [0,E) Q, [E,2E) K, [2E,3E) V; head h is columns
//                    h*D .. h*D+D-1 of each third, E = H*D
//   out  [B, N, E]   softmax(Q K^T / sqrt(D)) V, ready for the out-projection
//   stats [B, H, N, 2] f32 per row: the max of the raw scores and the
//                    reciprocal of the row's sum of exponentials
//   dqkv [B, N, 3E]  the three gradients in qkv's own layout
//
// 1 <= N <= 64, D in {16, 32, 64}; no mask, no dropout. A whole (batch, head)
// problem is smaller than one flash-attention tile, so ONE workgroup of four
// waves holds all of it in LDS: no online softmax, no split over keys, no
// atomics, and no [B, H, N, D] copy on either side of the kernel.
//
// Work split. N is padded to NT = ceil(N/16) tiles of 16. Wave w owns the
// 16 QUERY rows of tile w in every product whose rows are queries (S, P, O,
// dP, dS, dQ) and the 16 KEY rows of tile w where the rows are keys (dK, dV).
// A wave's score strip (16 x NT*16) therefore sits in its own registers: the
// softmax never leaves the wave, and P (forward) is written over the wave's
// own Q rows, which nobody else reads. Waves w >= NT only help staging.
//
// Arithmetic. LDS holds f32 whatever the storage dtype (loads widen bf16,
// as k_linear_tile does) and every product is v_mfma_f32_16x16x4_f32, the
// project's exact-fp32 policy: one code path, and bf16 storage pays two
// roundings in all (its operands, its result). Lane maps of that MFMA
// (r = lane & 15, q = lane >> 4): A[m = r][k = q], B[k = q][n = r],
// C/D col = r, row = 4q + reg.
//
// LDS. An operand is read in one of two patterns: "rk" — the lane's row is
// r, the contraction runs along the columns (address r*pitch + k0 + q) — and
// "kr" — the contraction runs along the rows ((k0 + q)*pitch + r). Over 64
// four-byte banks rk is conflict-free at pitch = 4 (mod 64) and kr at
// pitch = 16 (mod 64). The forward reads Q, P and K only as rk (pitch 68)
// and V only as kr (pitch 80). The backward reads every image both ways and
// takes pitch 72, a two-way conflict in either pattern. Both kernels stay at
// three images (54 KB), below the 64 KB a launch is sure to get; two
// workgroups fit a CU's 160 KB, which is all ViT-L/32 at batch 32 offers
// (512 workgroups on 256 CUs).
//
// Masking. Rows >= N of every staged image are zero-filled, never read from
// global memory and never stored. Key columns >= N are set to -inf before the
// row max (forward) and their P to zero (backward), so no padded key reaches
// a sum; padded query rows carry zeros throughout.
#include <cmath>

#include "kernel_common.h"
#include "ops.h"

// No packed-fp32 VALU forms (v_pk_*_f32) in this file's device code.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace mi355x {

namespace {

constexpr int kAttnMaxN = 64;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ void load4(const float* p, float v[4]) {
  const float4 x = *reinterpret_cast<const float4*>(p);
  v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
}
__device__ __forceinline__ void load4(const __hip_bfloat16* p, float v[4]) {
  const uint2 x = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(x.x << 16), v[1] = __uint_as_float(x.x & 0xffff0000u);
  v[2] = __uint_as_float(x.y << 16), v[3] = __uint_as_float(x.y & 0xffff0000u);
}

// Stage rows [0, NP) x D of one head slice (row stride ld elements) into an
// f32 LDS image: 4 elements per thread and trip, rows >= N zero-filled.
template <typename T, int D>
__device__ __forceinline__ void stage(float* img, int pitch, const T* src,
                                      size_t ld, int N, int NP) {
  constexpr int CH = D / 4;
  for (int idx = threadIdx.x; idx < NP * CH; idx += 256) {
    const int row = idx / CH, c = (idx % CH) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < N) load4(src + (size_t)row * ld + c, v);
    *reinterpret_cast<float4*>(&img[row * pitch + c]) =
        make_float4(v[0], v[1], v[2], v[3]);
  }
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One wave's strip of up to four 16x16 score-shaped tiles: acc[j] +=
// A(row0 + r, :) . Bimg(j*16 + r, :) over a contraction of D, both rk.
// `a` is the lane's A operand per step, already in registers.
template <int D>
__device__ __forceinline__ void strip_rk(f32x4 acc[4], const float a[D / 4],
                                         const float* bimg, int pb, int NT,
                                         int r, int q) {
#pragma unroll
  for (int s = 0; s < D / 4; ++s) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < NT)
        acc[j] = mfma4(a[s], bimg[(j * 16 + r) * pb + s * 4 + q], acc[j]);
  }
}

// One wave's strip of D/16 output tiles over a contraction of NP rows:
// acc[t] += sum_k A(k) * Bimg[k][t*16 + r] (B read kr). The A operand is
// aimg[(row0 + r)*pa + k] (rk) or, A_KR, aimg[k*pa + row0 + r]: the
// transposed use of the same image.
template <int D, bool A_KR>
__device__ __forceinline__ void strip_out(f32x4 acc[D / 16], const float* aimg,
                                          int pa, int row0, const float* bimg,
                                          int pb, int NP, int r, int q) {
  for (int k0 = 0; k0 < NP; k0 += 4) {
    const int k = k0 + q;
    const float a = A_KR ? aimg[k * pa + row0 + r] : aimg[(row0 + r) * pa + k];
#pragma unroll
    for (int t = 0; t < D / 16; ++t)
      acc[t] = mfma4(a, bimg[k * pb + t * 16 + r], acc[t]);
  }
}

// Store a strip of D/16 D-fragments, times `mul`, into rows row0.. of one
// head slice; rows >= N stay unwritten. 16 lanes cover 16 adjacent columns.
template <typename T, int D>
__device__ __forceinline__ void store_strip(T* dst, size_t ld,
                                            const f32x4 acc[D / 16], int row0,
                                            int N, const float mul[4], int r,
                                            int q) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + q * 4 + i;
    if (row < N) {
#pragma unroll
      for (int t = 0; t < D / 16; ++t)
        stf(&dst[(size_t)row * ld + t * 16 + r], acc[t][i] * mul[i]);
    }
  }
}

// Reduce over the 16 lanes that share q (one fragment row's 16 columns).
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---------------------------------------------------------------------------
// Forward. Images: QP (Q, then this wave's P over its own Q rows), K, V.
// ---------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_fwd(const T* __restrict__ qkv,
                                                  T* __restrict__ out,
                                                  float2* __restrict__ stats,
                                                  int N, int H, float scale) {
  constexpr int PQ = 68, PK = 68, PV = 80;
  __shared__ float sQP[kAttnMaxN * PQ];
  __shared__ float sK[kAttnMaxN * PK];
  __shared__ float sV[kAttnMaxN * PV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int NT = (N + 15) >> 4, NP = NT * 16;
  const size_t E = (size_t)H * D;
  const T* src = qkv + (size_t)b * N * 3 * E + (size_t)h * D;
  stage<T, D>(sQP, PQ, src, 3 * E, N, NP);
  stage<T, D>(sK, PK, src + E, 3 * E, N, NP);
  stage<T, D>(sV, PV, src + 2 * E, 3 * E, N, NP);
  __syncthreads();

  const int row0 = wave * 16;
  const bool active = wave < NT;
  float l[4] = {1.f, 1.f, 1.f, 1.f};
  if (active) {
    float a[D / 4];
#pragma unroll
    for (int s = 0; s < D / 4; ++s) a[s] = sQP[(row0 + r) * PQ + s * 4 + q];
    f32x4 s4[4] = {};
    strip_rk<D>(s4, a, sK, PK, NT, r, q);
    // softmax on the fragments: row = row0 + 4q + i, column = 16j + r
    const float c = scale * kLog2e;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= NT || j * 16 + r >= N) s4[j][i] = -INFINITY;
        m = fmaxf(m, s4[j][i]);
      }
      m = row16_max(m);  // finite: column 0 is always a key
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __builtin_amdgcn_exp2f((s4[j][i] - m) * c);
        s4[j][i] = p;
        sum += p;
      }
      sum = row16_sum(sum);
      l[i] = 1.f / sum;
      const int row = row0 + q * 4 + i;
      if (r == 0 && row < N)
        stats[((size_t)b * H + h) * N + row] = make_float2(m, l[i]);
    }
    // unnormalised P over this wave's Q rows (its A operand is in registers
    // and no other wave reads these rows)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          sQP[(row0 + q * 4 + i) * PQ + j * 16 + r] = s4[j][i];
      }
  }
  __syncthreads();
  if (active) {
    f32x4 o[D / 16] = {};
    strip_out<D, false>(o, sQP, PQ, row0, sV, PV, NP, r, q);
    store_strip<T, D>(out + (size_t)b * N * E + (size_t)h * D, E, o, row0, N,
                      l, r, q);
  }
}

// ---------------------------------------------------------------------------
// Backward. Images X, Y, Z hold in turn
//   phase 1: Q, K, V     S = Q K^T and dP = dO V^T strips -> P, dS registers
//   phase 2: Q, K, dS    dQ = dS K (query strip), dK = dS^T Q (key strip)
//   phase 3: dO, K, P    dV = P^T dO (key strip)
// The wave's dO rows for dP come straight from global memory into A-operand
// registers; delta = rowsum(dO * O) is taken as rowsum(P * dP), the same
// number, from the fragments at hand, so `out` is not read at all.
// ---------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(256) void k_attn_bwd(const T* __restrict__ qkv,
                                                  const T* __restrict__ dout,
                                                  const float2* __restrict__ stats,
                                                  T* __restrict__ dqkv, int N,
                                                  int H, float scale) {
  constexpr int P = 72;
  __shared__ float sX[kAttnMaxN * P];
  __shared__ float sY[kAttnMaxN * P];
  __shared__ float sZ[kAttnMaxN * P];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int NT = (N + 15) >> 4, NP = NT * 16;
  const size_t E = (size_t)H * D;
  const size_t hq = (size_t)b * N * 3 * E + (size_t)h * D;
  const T* dO = dout + (size_t)b * N * E + (size_t)h * D;
  const int row0 = wave * 16;
  const bool active = wave < NT;
  const float one[4] = {1.f, 1.f, 1.f, 1.f};

  float a_do[D / 4];
  if (active) {
    const int row = row0 + r;
#pragma unroll
    for (int s = 0; s < D / 4; ++s)
      a_do[s] = row < N ? ldf(&dO[(size_t)row * E + s * 4 + q]) : 0.f;
  }
  stage<T, D>(sX, P, qkv + hq, 3 * E, N, NP);
  stage<T, D>(sY, P, qkv + hq + E, 3 * E, N, NP);
  stage<T, D>(sZ, P, qkv + hq + 2 * E, 3 * E, N, NP);
  __syncthreads();

  f32x4 p4[4] = {}, ds4[4] = {};
  if (active) {
    float a[D / 4];
#pragma unroll
    for (int s = 0; s < D / 4; ++s) a[s] = sX[(row0 + r) * P + s * 4 + q];
    strip_rk<D>(p4, a, sY, P, NT, r, q);     // S
    strip_rk<D>(ds4, a_do, sZ, P, NT, r, q); // dP
    const float c = scale * kLog2e;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + q * 4 + i;
      const float2 st = row < N ? stats[((size_t)b * H + h) * N + row]
                                : make_float2(0.f, 0.f);
      float delta = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = j < NT && j * 16 + r < N && row < N;
        const float p =
            live ? __builtin_amdgcn_exp2f((p4[j][i] - st.x) * c) * st.y : 0.f;
        p4[j][i] = p;
        delta += p * ds4[j][i];
      }
      delta = row16_sum(delta);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        ds4[j][i] = p4[j][i] * (ds4[j][i] - delta) * scale;
    }
  }
  __syncthreads();  // V and the rk reads of Q, K are done: Z <- dS
  if (active) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          sZ[(row0 + q * 4 + i) * P + j * 16 + r] = ds4[j][i];
      }
  }
  __syncthreads();
  if (active) {
    f32x4 dq[D / 16] = {}, dk[D / 16] = {};
    strip_out<D, false>(dq, sZ, P, row0, sY, P, NP, r, q);
    store_strip<T, D>(dqkv + hq, 3 * E, dq, row0, N, one, r, q);
    strip_out<D, true>(dk, sZ, P, row0, sX, P, NP, r, q);
    store_strip<T, D>(dqkv + hq + E, 3 * E, dk, row0, N, one, r, q);
  }
  __syncthreads();  // dS and Q are done: Z <- P, X <- dO
  if (active) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < NT) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          sZ[(row0 + q * 4 + i) * P + j * 16 + r] = p4[j][i];
      }
  }
  stage<T, D>(sX, P, dO, E, N, NP);
  __syncthreads();
  if (active) {
    f32x4 dv[D / 16] = {};
    strip_out<D, true>(dv, sZ, P, row0, sX, P, NP, r, q);
    store_strip<T, D>(dqkv + hq + 2 * E, 3 * E, dv, row0, N, one, r, q);
  }
}

struct AttnDims {
  int64_t B, N, H, D;
};

// The argument check shared by attn_fwd and attn_bwd, complete before any
// launch.
AttnDims attn_check_args(const char* who, const torch::Tensor& qkv,
                         int64_t heads) {
  TORCH_CHECK(qkv.defined() && qkv.is_cuda(), who, ": qkv must be on a GPU");
  const auto dt = qkv.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(), who,
              ": qkv must be [B, N, 3*E] and contiguous");
  TORCH_CHECK(heads >= 1 && qkv.size(2) % (3 * heads) == 0, who,
              ": the last dimension (", qkv.size(2),
              ") must be 3 * heads * D with heads = ", heads);
  const int64_t B = qkv.size(0), N = qkv.size(1);
  const int64_t D = qkv.size(2) / (3 * heads);
  TORCH_CHECK(D == 16 || D == 32 || D == 64, who,
              " supports head sizes 16, 32 and 64, got D = ", D);
  TORCH_CHECK(N >= 1 && N <= kAttnMaxN, who, " supports 1 <= N <= ", kAttnMaxN,
              " tokens, got N = ", N);
  TORCH_CHECK(B * heads <= INT32_MAX, who, ": B * heads exceeds the grid");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, who,
              ": qkv must be 16-byte aligned");
  return {B, N, heads, D};
}

// A caller's preallocated result, checked, or a fresh one.
torch::Tensor attn_result(const char* who, const char* name,
                          const c10::optional<torch::Tensor>& given,
                          at::IntArrayRef shape, at::TensorOptions opts) {
  if (!given.has_value()) return torch::empty(shape, opts);
  TORCH_CHECK(given->device() == opts.device() &&
                  given->scalar_type() ==
                      c10::typeMetaToScalarType(opts.dtype()) &&
                  given->is_contiguous() && given->sizes() == shape &&
                  reinterpret_cast<uintptr_t>(given->data_ptr()) % 16 == 0,
              who, ": ", name, " must be contiguous, 16-byte aligned, ",
              opts.dtype(), " ", shape, " on qkv's device");
  return *given;
}

template <typename F>
void with_head_dim(int64_t D, F&& f) {
  if (D == 16) f(std::integral_constant<int, 16>{});
  else if (D == 32) f(std::integral_constant<int, 32>{});
  else f(std::integral_constant<int, 64>{});
}

}  // namespace

std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t heads,
                                    c10::optional<torch::Tensor> out_,
                                    c10::optional<torch::Tensor> row_stats_) {
  const AttnDims d = attn_check_args("attn_fwd", qkv, heads);
  auto out = attn_result("attn_fwd", "out", out_, {d.B, d.N, d.H * d.D},
                         qkv.options());
  auto stats = attn_result("attn_fwd", "row_stats", row_stats_,
                           {d.B, d.H, d.N, 2},
                           qkv.options().dtype(at::kFloat));
  if (d.B == 0) return {out, stats};
  const float scale = 1.f / std::sqrt((float)d.D);
  DISPATCH_F32_BF16(qkv.scalar_type(), "attn_fwd", {
    with_head_dim(d.D, [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      hipLaunchKernelGGL((k_attn_fwd<scalar_t, D>), dim3(d.B * d.H), dim3(256),
                         0, cur_stream(), cdptr<scalar_t>(qkv),
                         dptr<scalar_t>(out), dptr<float2>(stats), (int)d.N,
                         (int)d.H, scale);
    });
  });
  HIP_OK(hipGetLastError());
  return {out, stats};
}

torch::Tensor attn_bwd(torch::Tensor dout, torch::Tensor qkv,
                       torch::Tensor row_stats, int64_t heads,
                       c10::optional<torch::Tensor> dqkv_) {
  const char* who = "attn_bwd";
  const AttnDims d = attn_check_args(who, qkv, heads);
  TORCH_CHECK(dout.defined() && dout.device() == qkv.device() &&
                  dout.scalar_type() == qkv.scalar_type(),
              who, ": dout must have qkv's dtype and device");
  TORCH_CHECK(dout.dim() == 3 && dout.is_contiguous() &&
                  dout.size(0) == d.B && dout.size(1) == d.N &&
                  dout.size(2) == d.H * d.D,
              who, ": dout must be [B, N, E] = [", d.B, ", ", d.N, ", ",
              d.H * d.D, "] and contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dout.data_ptr()) % 16 == 0, who,
              ": dout must be 16-byte aligned");
  TORCH_CHECK(row_stats.defined() && row_stats.device() == qkv.device() &&
                  row_stats.scalar_type() == at::kFloat &&
                  row_stats.is_contiguous() && row_stats.dim() == 4 &&
                  row_stats.size(0) == d.B && row_stats.size(1) == d.H &&
                  row_stats.size(2) == d.N && row_stats.size(3) == 2,
              who, ": row_stats must be attn_fwd's f32 [B, H, N, 2] = [", d.B,
              ", ", d.H, ", ", d.N, ", 2] on qkv's device");
  auto dqkv = attn_result(who, "dqkv", dqkv_, qkv.sizes(), qkv.options());
  if (d.B == 0) return dqkv;
  const float scale = 1.f / std::sqrt((float)d.D);
  DISPATCH_F32_BF16(qkv.scalar_type(), who, {
    with_head_dim(d.D, [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      hipLaunchKernelGGL((k_attn_bwd<scalar_t, D>), dim3(d.B * d.H), dim3(256),
                         0, cur_stream(), cdptr<scalar_t>(qkv),
                         cdptr<scalar_t>(dout), cdptr<float2>(row_stats),
                         dptr<scalar_t>(dqkv), (int)d.N, (int)d.H, scale);
    });
  });
  HIP_OK(hipGetLastError());
  return dqkv;
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
