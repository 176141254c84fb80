// Fused LayerNorm and residual-add LayerNorm for gfx950 (MI355X), forward and
// backward, over the last dimension of a contiguous tensor.
//
//   x, residual, s, y, dy, ds, dx   [R, E]  rows are the flattened leading
//                                           dimensions, storage T (f32 | bf16)
//   weight, bias, dgamma, dbeta     [E]     storage T
//   row_stats                       [R, 2]  f32 (mean, rstd) of the LN input
//   partials                        [g, 2, E] f32 workspace, g = the grid
//
// E % 4 == 0, 4 <= E <= 2048. All arithmetic is f32.
//
// Work split. ONE WAVE owns one row at a time; a 256-thread workgroup is four
// independent waves and the waves of the grid stride over the rows. Lane l
// holds vectors l + 64 j (j < NV) of four adjacent elements of its row in
// registers: one 16-byte (f32) or 8-byte (bf16) load per j, a wave reading
// 1 KB / 512 B of one row per j. NV in {1, 2, 4, 8} is a template constant
// picked from E; vectors at or past E/4 are masked (never loaded, never
// stored, zero in every sum). A row is read once and never touches LDS; the
// row reductions are ds_bpermute butterflies inside the wave.
//
// Grid. min(kLnGridCap, ceil(R / 4)) workgroups. The cap is a compile-time
// constant, not a device query, so a launch recorded into a graph and the
// eager launch of the same shape are the same launch, and the backward's
// workspace has a size known from the shape alone.
//
// Forward. gamma and beta go into registers once per wave (at E = 1024 they
// are as many bytes as a row). Per row: mean = wave_sum(x) / E; d = x - mean
// stays in registers; var = wave_sum(d * d) / E, two passes over registers,
// never E[x^2] - mean^2; rstd = 1 / sqrt(var + eps); y = d * rstd * gamma +
// beta, rounded once. With ADD, s = x + residual is formed in f32, rounded to
// T and stored, and the row that is normalised is that ROUNDED s: y is LN of
// the tensor the caller gets, and the backward, which re-reads s, sees the
// numbers the forward saw.
//
// Backward. Per row: xhat = (x - mean) * rstd from the saved input and
// statistics, g = dy * gamma, c1 = mean(g * xhat) and c2 = mean(g) in one
// two-value butterfly, dx = rstd * (g - c2 - xhat * c1) (+ ds with ADD),
// stored once. Each lane accumulates dgamma += dy * xhat and dbeta += dy of
// its own columns over every row its wave visits. At the end waves 1..3 hand
// their accumulators to wave 0 through LDS (3 x 2 x NV*256 f32, 48 KB at
// NV = 8), wave 0 adds them in wave order and stores the workgroup's [2, E]
// slice of `partials`. Every workgroup of the grid stores its slice (zeros
// where a wave saw no row), so nothing is pre-zeroed and there are no atomics.
//
// k_ln_bwd_params sums partials over the g slices: a workgroup of 16 waves
// owns 64 adjacent columns of the [g, 2E] matrix, wave w adds slices w,
// w + 16, ... in order (a 256-byte coalesced read per slice), the 16 sums
// meet in LDS and wave 0 adds them in wave order, rounds once and stores.
// The order is fixed by (g, E) alone: the gradients are reproducible.
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

constexpr int kLnGridCap = 512;   // workgroups; see ln_grid_cap()
constexpr int kLnMaxE = 2048;
constexpr int kParamWaves = 16;   // k_ln_bwd_params: waves per workgroup

// The helpers below use clang's vector types and builtins only. A function
// of the HIP headers (make_float4, __uint_as_float, __shfl_xor,
// __syncthreads, __float2bfloat16) does not carry this file's target
// attribute, so it is not inlined into these kernels and stays a CALL.
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

__device__ __forceinline__ float as_f32(uint32_t u) {
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ void ld4(const float* p, float v[4]) {
  const f32x4 x = *reinterpret_cast<const f32x4*>(p);
  v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
}
__device__ __forceinline__ void ld4(const __hip_bfloat16* p, float v[4]) {
  const u32x2 x = *reinterpret_cast<const u32x2*>(p);
  v[0] = as_f32(x[0] << 16), v[1] = as_f32(x[0] & 0xffff0000u);
  v[2] = as_f32(x[1] << 16), v[3] = as_f32(x[1] & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float v[4]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
}
// Two floats to two bf16, round to nearest even (v_cvt_pk_bf16_f32).
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
  const bf16x2 p = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, p);
}
__device__ __forceinline__ void st4(__hip_bfloat16* p, const float v[4]) {
  *reinterpret_cast<u32x2*>(p) =
      u32x2{bf16_pack(v[0], v[1]), bf16_pack(v[2], v[3])};
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

// v of lane (lane ^ off): one ds_bpermute_b32.
__device__ __forceinline__ float xor_lane(float v, int lane, int off) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                          __builtin_bit_cast(int, v)));
}
// Butterfly sums over the 64 lanes; every lane ends with the same bits. The
// two-value form reduces both in one pass: the second's shuffles hide in
// the first's.
__device__ __forceinline__ float lane_sum(float a, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += xor_lane(a, lane, off);
  return a;
}
__device__ __forceinline__ void lane_sum2(float& a, float& b, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ta = xor_lane(a, lane, off), tb = xor_lane(b, lane, off);
    a += ta, b += tb;
  }
}
// __syncthreads, spelled out.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <typename T, int NV, bool ADD>
__global__ __launch_bounds__(256) void k_ln_fwd(
    const T* __restrict__ x, const T* __restrict__ res,
    const T* __restrict__ gamma, const T* __restrict__ beta,
    T* __restrict__ s, T* __restrict__ y, f32x2* __restrict__ stats,
    int64_t R, int E, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = E >> 2;
  float gm[NV][4], bt[NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) ld4(gamma + 4 * v, gm[j]), ld4(beta + 4 * v, bt[j]);
  }
  const float inv_e = 1.f / (float)E;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R;
       row += (int64_t)gridDim.x * 4) {
    const int64_t base = row * E;
    float d[NV][4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
        ld4(x + base + 4 * v, d[j]);
        if (ADD) {
          float r[4];
          ld4(res + base + 4 * v, r);
#pragma unroll
          for (int i = 0; i < 4; ++i) d[j][i] = stored(d[j][i] + r[i], s);
          st4(s + base + 4 * v, d[j]);
        }
        sum += (d[j][0] + d[j][1]) + (d[j][2] + d[j][3]);
      }
    }
    const float mean = lane_sum(sum, lane) / (float)E;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (lane + 64 * j < nvec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d[j][i] -= mean;
          sq = fmaf(d[j][i], d[j][i], sq);
        }
      }
    }
    const float rstd = 1.f / sqrtf(lane_sum(sq, lane) * inv_e + eps);
    if (lane == 0) stats[row] = f32x2{mean, rstd};
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[i] = fmaf(d[j][i] * rstd, gm[j][i], bt[j][i]);
        st4(y + base + 4 * v, o);
      }
    }
  }
}

template <typename T, int NV, bool ADD>
__global__ __launch_bounds__(256) void k_ln_bwd(
    const T* __restrict__ dy, const T* __restrict__ xin,
    const f32x2* __restrict__ stats, const T* __restrict__ gamma,
    const T* __restrict__ ds, T* __restrict__ dx,
    float* __restrict__ partials, int64_t R, int E) {
  __shared__ float hand[3][2][NV * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = E >> 2;
  float gm[NV][4], dg[NV][4], db[NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int v = lane + 64 * j;
    if (v < nvec) ld4(gamma + 4 * v, gm[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) dg[j][i] = 0.f, db[j][i] = 0.f;
  }
  const float inv_e = 1.f / (float)E;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < R;
       row += (int64_t)gridDim.x * 4) {
    const int64_t base = row * E;
    const f32x2 st = stats[row];
    const float mean = st[0], rstd = st[1];
    float xh[NV][4], g[NV][4];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
        float d[4];
        ld4(xin + base + 4 * v, xh[j]);
        ld4(dy + base + 4 * v, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xh[j][i] = (xh[j][i] - mean) * rstd;
          g[j][i] = d[i] * gm[j][i];
          c1 = fmaf(g[j][i], xh[j][i], c1);
          c2 += g[j][i];
          dg[j][i] = fmaf(d[i], xh[j][i], dg[j][i]);
          db[j][i] += d[i];
        }
      }
    }
    lane_sum2(c1, c2, lane);
    c1 *= inv_e, c2 *= inv_e;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[i] = rstd * ((g[j][i] - c2) - xh[j][i] * c1);
        if (ADD && ds != nullptr) {
          float a[4];
          ld4(ds + base + 4 * v, a);
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] += a[i];
        }
        st4(dx + base + 4 * v, o);
      }
    }
  }
  // waves 1..3 -> LDS -> wave 0, added in wave order
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      st4(&hand[wave - 1][0][(lane + 64 * j) * 4], dg[j]);
      st4(&hand[wave - 1][1][(lane + 64 * j) * 4], db[j]);
    }
  }
  block_sync();
  if (wave == 0) {
    float* slice = partials + (int64_t)blockIdx.x * 2 * E;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < nvec) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
          float a[4], b[4];
          ld4(&hand[w][0][v * 4], a);
          ld4(&hand[w][1][v * 4], b);
#pragma unroll
          for (int i = 0; i < 4; ++i) dg[j][i] += a[i], db[j][i] += b[i];
        }
        st4(slice + 4 * v, dg[j]);
        st4(slice + E + 4 * v, db[j]);
      }
    }
  }
}

// partials [g, 2E] -> dgamma | dbeta. 16 waves x 64 columns per workgroup.
template <typename T>
__global__ __launch_bounds__(kParamWaves * 64) void k_ln_bwd_params(
    const float* __restrict__ partials, T* __restrict__ dgamma,
    T* __restrict__ dbeta, int g, int E) {
  __shared__ float part[kParamWaves][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane, C = 2 * E;
  float acc = 0.f;
  if (col < C) {
    const float* p = partials + col;
    int k = wave;
    for (; k + 3 * kParamWaves < g; k += 4 * kParamWaves) {
      // four loads in flight, added in slice order
      const float a0 = p[(int64_t)k * C];
      const float a1 = p[(int64_t)(k + kParamWaves) * C];
      const float a2 = p[(int64_t)(k + 2 * kParamWaves) * C];
      const float a3 = p[(int64_t)(k + 3 * kParamWaves) * C];
      acc = (((acc + a0) + a1) + a2) + a3;
    }
    for (; k < g; k += kParamWaves) acc += p[(int64_t)k * C];
  }
  part[wave][lane] = acc;
  block_sync();
  if (wave == 0 && col < C) {
    float t = part[0][lane];
#pragma unroll
    for (int w = 1; w < kParamWaves; ++w) t += part[w][lane];
    if (col < E) st1(&dgamma[col], t);
    else st1(&dbeta[col - E], t);
  }
}

struct LnDims {
  int64_t R, E;
};

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// An operand of x's dtype and device, contiguous, 16-byte aligned, of `shape`.
void ln_check_like(const char* who, const char* name, const torch::Tensor& t,
                   const torch::Tensor& x, at::IntArrayRef shape) {
  TORCH_CHECK(t.defined() && t.device() == x.device() &&
                  t.scalar_type() == x.scalar_type(),
              who, ": ", name, " must have x's dtype and device");
  TORCH_CHECK(t.sizes() == shape && t.is_contiguous() && aligned16(t), who,
              ": ", name, " must be contiguous, 16-byte aligned and of shape ",
              shape, ", got ", t.sizes());
}

// The argument check shared by ln_fwd and ln_bwd, complete before any launch.
// `x` is the LN input (x, or s); `same` are the optional operands of x's shape
// (residual; dy and ds), `stats` the backward's row_stats.
LnDims ln_check_args(const char* who, const torch::Tensor& x,
                     const torch::Tensor& weight, const torch::Tensor* bias,
                     double eps,
                     std::initializer_list<
                         std::pair<const char*, const torch::Tensor*>> same,
                     const torch::Tensor* stats) {
  TORCH_CHECK(x.defined() && x.is_cuda(), who, ": x must be on a GPU");
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  TORCH_CHECK(x.dim() >= 1 && x.is_contiguous() && aligned16(x), who,
              ": x must be contiguous and 16-byte aligned");
  const int64_t E = x.size(-1);
  TORCH_CHECK(E % 4 == 0 && E >= 4 && E <= kLnMaxE, who,
              " supports a last dimension that is a multiple of 4 in [4, ",
              kLnMaxE, "], got E = ", E);
  ln_check_like(who, "weight", weight, x, {E});
  if (bias) ln_check_like(who, "bias", *bias, x, {E});
  for (const auto& [name, t] : same)
    if (t) ln_check_like(who, name, *t, x, x.sizes());
  TORCH_CHECK(eps >= 0, who, ": eps must be >= 0, got ", eps);
  const int64_t R = x.numel() / E;
  if (stats)
    TORCH_CHECK(stats->defined() && stats->device() == x.device() &&
                    stats->scalar_type() == at::kFloat &&
                    stats->is_contiguous() && stats->dim() == 2 &&
                    stats->size(0) == R && stats->size(1) == 2 &&
                    aligned16(*stats),
                who, ": row_stats must be ln_fwd's f32 [R, 2] = [", R,
                ", 2] on x's device");
  return {R, E};
}

// A caller's preallocated result, checked, or a fresh one.
torch::Tensor ln_result(const char* who, const char* name,
                        const c10::optional<torch::Tensor>& given,
                        at::IntArrayRef shape, at::TensorOptions opts) {
  if (!given.has_value()) return torch::empty(shape, opts);
  TORCH_CHECK(given->device() == opts.device() &&
                  given->scalar_type() ==
                      c10::typeMetaToScalarType(opts.dtype()) &&
                  given->is_contiguous() && given->sizes() == shape &&
                  aligned16(*given),
              who, ": ", name, " must be contiguous, 16-byte aligned, ",
              opts.dtype(), " ", shape, " on x's device");
  return *given;
}

const torch::Tensor* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? &*t : nullptr;
}

int ln_grid(int64_t R) {
  return (int)std::min<int64_t>(kLnGridCap, (R + 3) / 4);
}

// f(NV, ADD) as integral constants, NV the smallest of 1, 2, 4, 8 with
// 64 * NV >= E / 4.
template <typename F>
void with_ln_variant(int64_t E, bool add, F&& f) {
  auto with_add = [&](auto nv) {
    if (add) f(nv, std::true_type{});
    else f(nv, std::false_type{});
  };
  if (E <= 256) with_add(std::integral_constant<int, 1>{});
  else if (E <= 512) with_add(std::integral_constant<int, 2>{});
  else if (E <= 1024) with_add(std::integral_constant<int, 4>{});
  else with_add(std::integral_constant<int, 8>{});
}

}  // namespace

int64_t ln_grid_cap() { return kLnGridCap; }

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor weight,
                                  torch::Tensor bias, double eps,
                                  c10::optional<torch::Tensor> residual,
                                  c10::optional<torch::Tensor> y_,
                                  c10::optional<torch::Tensor> row_stats_,
                                  c10::optional<torch::Tensor> s_) {
  const char* who = "ln_fwd";
  const LnDims d = ln_check_args(who, x, weight, &bias, eps,
                                 {{"residual", opt_ptr(residual)}}, nullptr);
  const bool add = residual.has_value();
  TORCH_CHECK(add || !s_.has_value(), who, ": s needs a residual");
  auto y = ln_result(who, "y", y_, x.sizes(), x.options());
  auto stats = ln_result(who, "row_stats", row_stats_, {d.R, 2},
                         x.options().dtype(at::kFloat));
  torch::Tensor s;
  if (add) s = ln_result(who, "s", s_, x.sizes(), x.options());
  if (d.R > 0) {
    DISPATCH_F32_BF16(x.scalar_type(), who, {
      with_ln_variant(d.E, add, [&](auto nv, auto ad) {
        constexpr int NV = decltype(nv)::value;
        constexpr bool ADD = decltype(ad)::value;
        hipLaunchKernelGGL(
            (k_ln_fwd<scalar_t, NV, ADD>), dim3(ln_grid(d.R)), dim3(256), 0,
            cur_stream(), cdptr<scalar_t>(x),
            ADD ? cdptr<scalar_t>(*residual) : nullptr,
            cdptr<scalar_t>(weight), cdptr<scalar_t>(bias),
            ADD ? dptr<scalar_t>(s) : nullptr, dptr<scalar_t>(y),
            dptr<f32x2>(stats), d.R, (int)d.E, (float)eps);
      });
    });
    HIP_OK(hipGetLastError());
  }
  if (add) return {s, y, stats};
  return {y, stats};
}

std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor ln_input,
                                  torch::Tensor row_stats,
                                  torch::Tensor weight,
                                  c10::optional<torch::Tensor> ds,
                                  c10::optional<torch::Tensor> dx_,
                                  c10::optional<torch::Tensor> dgamma_,
                                  c10::optional<torch::Tensor> dbeta_) {
  const char* who = "ln_bwd";
  const LnDims d =
      ln_check_args(who, ln_input, weight, nullptr, 0.0,
                    {{"dy", &dy}, {"ds", opt_ptr(ds)}}, &row_stats);
  auto dx = ln_result(who, "dx", dx_, ln_input.sizes(), ln_input.options());
  auto dgamma = ln_result(who, "dgamma", dgamma_, {d.E}, weight.options());
  auto dbeta = ln_result(who, "dbeta", dbeta_, {d.E}, weight.options());
  if (d.R == 0) {
    dgamma.zero_(), dbeta.zero_();
    return {dx, dgamma, dbeta};
  }
  const int g = ln_grid(d.R);
  auto partials =
      torch::empty({g, 2, d.E}, ln_input.options().dtype(at::kFloat));
  const bool add = ds.has_value();
  DISPATCH_F32_BF16(ln_input.scalar_type(), who, {
    with_ln_variant(d.E, add, [&](auto nv, auto ad) {
      constexpr int NV = decltype(nv)::value;
      constexpr bool ADD = decltype(ad)::value;
      hipLaunchKernelGGL((k_ln_bwd<scalar_t, NV, ADD>), dim3(g), dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(dy),
                         cdptr<scalar_t>(ln_input), cdptr<f32x2>(row_stats),
                         cdptr<scalar_t>(weight),
                         ADD ? cdptr<scalar_t>(*ds) : nullptr,
                         dptr<scalar_t>(dx), dptr<float>(partials), d.R,
                         (int)d.E);
    });
    hipLaunchKernelGGL((k_ln_bwd_params<scalar_t>), dim3(cdiv(2 * d.E, 64)),
                       dim3(kParamWaves * 64), 0, cur_stream(),
                       cdptr<float>(partials), dptr<scalar_t>(dgamma),
                       dptr<scalar_t>(dbeta), g, (int)d.E);
  });
  HIP_OK(hipGetLastError());
  return {dx, dgamma, dbeta};
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
