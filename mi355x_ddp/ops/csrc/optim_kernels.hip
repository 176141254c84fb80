// Optimizers over one flat bucket: plain SGD, momentum SGD and AdamW.
//
// All are memory-bound streaming kernels in one layout: 4 elements per lane
// (one float4, or one ushort4 of bf16; bucket lengths are padded to a
// multiple of 4 by the reducer), int64 indexing. Plain SGD takes one vector
// per thread on an uncapped grid; the stateful kernels cap the grid at
// kMaxBlocks and walk a grid-stride loop (guide G11).
// Parameters and gradients are f32 or bf16; optimizer state is always f32.
// bf16 does the arithmetic in f32 and rounds to nearest once, on the
// parameter store — there are no f32 master weights.
//
// Rounding follows torch's single-tensor optimizers as they run ON THE
// DEVICE, operation by operation, so that a model moved from torch.optim to
// these kernels keeps its trajectory bit for bit: a fused multiply-add
// exactly where torch's device add(alpha)/lerp/addcmul/addcdiv kernels
// contract one, separate roundings everywhere else, IEEE divide and sqrt,
// the division by the scalar sqrt(bc2) as a multiplication by its
// reciprocal. (torch's CPU kernels, which ops.sgd_momentum_flat_ /
// ops.adamw_flat_ mirror on the host, place three of AdamW's roundings
// differently; momentum SGD is the same sequence on both.) Contraction is
// therefore switched off for the file and every fma below is explicit.
//
// Bucket padding (p == g == 0, state 0) stays exactly 0 under both kernels:
// every term of both updates is a product with p, g or the state.
//
// Global grad-norm clipping rides on the same layout: k_sumsq_flat reads a
// bucket's gradient once and leaves one double per block, k_clip_coef folds
// every bucket's partials into (total_norm, coef), and the SCALED form of
// the three update kernels multiplies each loaded gradient by coef — what
// torch's clip_grad_norm_ does with grad.mul_(coef), without the extra
// read and write of g. SCALED = false is the unclipped kernel unchanged.
#include "kernel_common.h"
#include "ops.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace mi355x {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

struct F4 {
  float v[4];
};

__device__ __forceinline__ F4 ld4(const float* p, int64_t i) {
  const float4 t = reinterpret_cast<const float4*>(p)[i];
  return {{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ F4 ld4(const __hip_bfloat16* p, int64_t i) {
  const ushort4 t = reinterpret_cast<const ushort4*>(p)[i];
  return {{__uint_as_float((uint32_t)t.x << 16),
           __uint_as_float((uint32_t)t.y << 16),
           __uint_as_float((uint32_t)t.z << 16),
           __uint_as_float((uint32_t)t.w << 16)}};
}
__device__ __forceinline__ void st4(float* p, int64_t i, const F4& f) {
  reinterpret_cast<float4*>(p)[i] =
      make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
}
__device__ __forceinline__ unsigned short bf16_bits(float f) {
  const __hip_bfloat16 h = __float2bfloat16(f);  // round to nearest even
  return *reinterpret_cast<const unsigned short*>(&h);
}
__device__ __forceinline__ void st4(__hip_bfloat16* p, int64_t i,
                                    const F4& f) {
  reinterpret_cast<ushort4*>(p)[i] =
      make_ushort4(bf16_bits(f.v[0]), bf16_bits(f.v[1]), bf16_bits(f.v[2]),
                   bf16_bits(f.v[3]));
}
__device__ __forceinline__ void zero4(float* p, int64_t i) {
  reinterpret_cast<float4*>(p)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void zero4(__hip_bfloat16* p, int64_t i) {
  reinterpret_cast<ushort4*>(p)[i] = make_ushort4(0, 0, 0, 0);
}

// g *= coef as grad.mul_(coef) would have stored it: one f32 multiply, and
// for bf16 the rounding of that store (then widened again for the update).
template <typename T>
__device__ __forceinline__ void scale4(F4& f, float coef) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float s = f.v[j] * coef;
    if constexpr (std::is_same<T, float>::value)
      f.v[j] = s;
    else
      f.v[j] = __uint_as_float((uint32_t)bf16_bits(s) << 16);
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace

// Plain SGD (+ fold zero_grad): p -= lr*g as one fma; g = 0.
// SCALED (all three update kernels): g is taken as g * gscale[0], the
// clip coefficient k_clip_coef left on the device; g itself is not
// rewritten (it is zeroed, or with zero == 0 left unscaled).
template <typename T, bool SCALED = false>
__global__ void k_sgd_flat(T* __restrict__ p, T* __restrict__ g, float lr,
                           int64_t n4, int zero,
                           const float* __restrict__ gscale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  F4 gv = ld4(g, i);
  if constexpr (SCALED) scale4<T>(gv, gscale[0]);
  F4 pv = ld4(p, i);
#pragma unroll
  for (int j = 0; j < 4; ++j) pv.v[j] = __builtin_fmaf(-lr, gv.v[j], pv.v[j]);
  st4(p, i, pv);
  if (zero) zero4(g, i);
}

// d = g + wd*p; buf = mu*buf + d; d = nesterov ? d + mu*buf : buf;
// p -= lr*d. buf == nullptr is momentum 0 (weight decay only).
template <typename T, bool SCALED = false>
__global__ void __launch_bounds__(kThreads)
k_sgd_momentum_flat(T* __restrict__ p, T* __restrict__ g,
                    float* __restrict__ buf, float neg_lr, float mu, float wd,
                    int nesterov, int zero, int64_t n4,
                    const float* __restrict__ gscale) {
  float coef = 1.f;
  if constexpr (SCALED) coef = gscale[0];
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4;
       i += stride) {
    F4 pv = ld4(p, i);
    F4 gv = ld4(g, i);
    if constexpr (SCALED) scale4<T>(gv, coef);
    F4 bv = {{0.f, 0.f, 0.f, 0.f}};
    if (buf) bv = ld4(buf, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d = gv.v[j];
      if (wd != 0.f) d = __builtin_fmaf(pv.v[j], wd, d);
      if (buf) {
        const float b = bv.v[j] * mu + d;
        bv.v[j] = b;
        d = nesterov ? __builtin_fmaf(b, mu, d) : b;
      }
      pv.v[j] = __builtin_fmaf(d, neg_lr, pv.v[j]);
    }
    st4(p, i, pv);
    if (buf) st4(buf, i, bv);
    if (zero) zero4(g, i);
  }
}

// Advances the device-resident step count and derives the two bias-
// correction scalars the bucket kernels need, in double so they round to
// the same f32 as torch's Python-double values:
//   state[0] = t (int32), state[1] = bits of -(lr / (1 - b1^t)),
//   state[2] = bits of 1 / sqrt(1 - b2^t).
// One thread, launched once per optimizer step AHEAD of the bucket
// kernels on the same stream: no bucket block can see a half-advanced
// count, and a captured graph replays the increment.
__global__ void k_adamw_tick(int32_t* __restrict__ state, double lr,
                             double beta1, double beta2) {
  const int32_t t = state[0] + 1;
  const double bc1 = 1.0 - pow(beta1, (double)t);
  const double bc2 = 1.0 - pow(beta2, (double)t);
  state[0] = t;
  state[1] = __float_as_int((float)(-(lr / bc1)));
  state[2] = __float_as_int((float)(1.0 / sqrt(bc2)));
}

// torch's AdamW step (decoupled decay), t and the bias corrections read
// from `state`:
//   p *= 1 - lr*wd             (groups whose mask byte is non-zero)
//   m += (1-b1) * (g - m)      (lerp, as torch computes b1*m + (1-b1)*g)
//   v  = b2*v + (1-b2)*g*g
//   p += -(lr/bc1) * (m / (sqrt(v) * (1/sqrt(bc2)) + eps))
// mask: one byte per 4-element group (== per lane), nullptr = decay all.
template <typename T, bool SCALED = false>
__global__ void __launch_bounds__(kThreads)
k_adamw_flat(T* __restrict__ p, T* __restrict__ g, float* __restrict__ m,
             float* __restrict__ v, const int32_t* __restrict__ state,
             float decay, float w1, float beta2, float w2, float eps,
             const uint8_t* __restrict__ mask, int zero, int64_t n4,
             const float* __restrict__ gscale) {
  const float neg_step = __int_as_float(state[1]);
  const float inv_bc2_sqrt = __int_as_float(state[2]);
  float coef = 1.f;
  if constexpr (SCALED) coef = gscale[0];
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4;
       i += stride) {
    F4 pv = ld4(p, i);
    F4 gv = ld4(g, i);
    if constexpr (SCALED) scale4<T>(gv, coef);
    F4 mv = ld4(m, i);
    F4 vv = ld4(v, i);
    const bool decays = decay != 1.f && (mask == nullptr || mask[i] != 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = gv.v[j];
      float pj = pv.v[j];
      if (decays) pj = pj * decay;
      // torch's lerp picks the form by weight: m + w*(g-m) below 0.5,
      // g - (g-m)*(1-w) from there on
      const float mj = w1 < 0.5f
                           ? __builtin_fmaf(w1, gj - mv.v[j], mv.v[j])
                           : __builtin_fmaf(w1 - 1.f, gj - mv.v[j], gj);
      const float vj = __builtin_fmaf(w2, gj * gj, vv.v[j] * beta2);
      const float denom = sqrtf(vj) * inv_bc2_sqrt + eps;
      pv.v[j] = __builtin_fmaf(neg_step, mj / denom, pj);
      mv.v[j] = mj;
      vv.v[j] = vj;
    }
    st4(p, i, pv);
    st4(m, i, mv);
    st4(v, i, vv);
    if (zero) zero4(g, i);
  }
}

// Sum of squares of one flat gradient bucket, for the global grad norm.
// Same layout as the update kernels. A lane squares and adds in f32 (at
// most 4 * ceil(n4 / (kMaxBlocks * kThreads)) terms), everything after
// that is double: the wave by shuffles, the block's 4 waves through LDS.
// Thread 0 stores the block's sum into partials[blockIdx.x] — every one of
// the bucket's gridDim.x slots is overwritten on every call, nothing is
// accumulated or pre-zeroed, so the result is deterministic and a captured
// graph replays it.
template <typename T>
__global__ void __launch_bounds__(kThreads)
k_sumsq_flat(const T* __restrict__ g, double* __restrict__ partials,
             int64_t n4) {
  __shared__ double wave_part[kThreads / 64];
  float acc = 0.f;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4;
       i += stride) {
    const F4 gv = ld4(g, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += gv.v[j] * gv.v[j];
  }
  const double w = wave_sum((double)acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_part[0];
#pragma unroll
    for (int k = 1; k < kThreads / 64; ++k) s += wave_part[k];
    partials[blockIdx.x] = s;
  }
}

// One block: total_norm = sqrt(sum of all partials), summed in double in
// a fixed order (thread-strided, then an LDS tree), and torch's
// clip_grad_norm_ coefficient from it, operation for operation in f32:
// max_norm / (norm + 1e-6) as reciprocal * max_norm, then clamp(max=1),
// which lets a NaN through.
//   clip_state[0] = total_norm, clip_state[1] = coef.
__global__ void __launch_bounds__(kThreads)
k_clip_coef(const double* __restrict__ partials, int64_t nslots,
            float* __restrict__ clip_state, float max_norm) {
  __shared__ double tree[kThreads];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nslots; i += kThreads) s += partials[i];
  tree[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) tree[threadIdx.x] += tree[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total_norm = (float)sqrt(tree[0]);
    const float c = (1.0f / (total_norm + 1e-6f)) * max_norm;
    clip_state[0] = total_norm;
    clip_state[1] = c > 1.0f ? 1.0f : c;  // NaN stays NaN
  }
}

namespace {

int64_t check_flat(const torch::Tensor& param, const torch::Tensor& grad,
                   const char* name) {
  TORCH_CHECK(param.is_cuda() && grad.is_cuda(), name,
              ": flat buffers must be device tensors");
  TORCH_CHECK(param.is_contiguous() && grad.is_contiguous(), name,
              ": flat buffers must be contiguous");
  TORCH_CHECK(grad.scalar_type() == param.scalar_type() &&
                  grad.numel() == param.numel() &&
                  grad.device() == param.device(),
              name, ": grad must match param in dtype, length and device");
  TORCH_CHECK(param.numel() % 4 == 0, name,
              ": bucket length must be padded to a multiple of 4");
  // one 4-element vector access per lane: 16 B (f32) / 8 B (bf16) aligned
  const uintptr_t align = 4 * param.element_size();
  TORCH_CHECK(reinterpret_cast<uintptr_t>(param.data_ptr()) % align == 0 &&
                  reinterpret_cast<uintptr_t>(grad.data_ptr()) % align == 0,
              name, ": flat buffers must be aligned to 4 elements");
  return param.numel() / 4;
}

void check_state(const torch::Tensor& s, const torch::Tensor& param,
                 const char* name, const char* what) {
  TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                  s.scalar_type() == at::kFloat &&
                  s.numel() == param.numel() &&
                  s.device() == param.device() &&
                  reinterpret_cast<uintptr_t>(s.data_ptr()) % 16 == 0,
              name, ": ", what,
              " must be a contiguous, 16 B aligned f32 device tensor of the "
              "bucket's length");
}

dim3 flat_grid(int64_t n4) {
  const int64_t blocks = (n4 + kThreads - 1) / kThreads;
  return dim3((unsigned)std::min<int64_t>(std::max<int64_t>(blocks, 1),
                                          kMaxBlocks));
}

// The optional clip coefficient of the update ops -> its device pointer,
// nullptr when absent (the unscaled kernel runs).
const float* check_scale(const c10::optional<torch::Tensor>& s,
                         const torch::Tensor& param, const char* name) {
  if (!s.has_value() || !s->defined()) return nullptr;
  TORCH_CHECK(s->is_cuda() && s->is_contiguous() &&
                  s->scalar_type() == at::kFloat && s->numel() == 1 &&
                  s->device() == param.device(),
              name, ": grad_scale must be an f32 device tensor of 1 element "
              "on the bucket's device");
  return s->data_ptr<float>();
}

// Calls launch(std::true_type) with a clip coefficient, (false_type) without:
// the kernel's SCALED instantiation is chosen on the host.
template <typename F>
void with_scaled(bool scaled, F&& launch) {
  if (scaled)
    launch(std::true_type{});
  else
    launch(std::false_type{});
}

}  // namespace

int64_t sumsq_slots(int64_t numel) {
  TORCH_CHECK(numel >= 0 && numel % 4 == 0,
              "sumsq_slots: bucket length must be padded to a multiple of 4");
  return flat_grid(numel / 4).x;
}

void grad_sumsq_flat(torch::Tensor grad_flat, torch::Tensor partials) {
  TORCH_CHECK(grad_flat.is_cuda() && grad_flat.is_contiguous(),
              "grad_sumsq_flat: grad must be a contiguous device tensor");
  TORCH_CHECK(grad_flat.numel() % 4 == 0,
              "grad_sumsq_flat: bucket length must be padded to a multiple "
              "of 4");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(grad_flat.data_ptr()) %
                      (4 * grad_flat.element_size()) == 0,
              "grad_sumsq_flat: grad must be aligned to 4 elements");
  const int64_t n4 = grad_flat.numel() / 4;
  const dim3 grid = flat_grid(n4);
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == at::kDouble &&
                  partials.device() == grad_flat.device() &&
                  partials.numel() == (int64_t)grid.x,
              "grad_sumsq_flat: partials must be a contiguous f64 device "
              "tensor of exactly sumsq_slots(numel) = ", grid.x, " elements");
  // n4 == 0 still launches: the one slot must be rewritten (with 0)
  DISPATCH_F32_BF16(grad_flat.scalar_type(), "grad_sumsq_flat", {
    hipLaunchKernelGGL((k_sumsq_flat<scalar_t>), grid, dim3(kThreads), 0,
                       cur_stream(), cdptr<scalar_t>(grad_flat),
                       partials.data_ptr<double>(), n4);
  });
  HIP_OK(hipGetLastError());
}

void clip_coef(torch::Tensor partials, torch::Tensor clip_state,
               double max_norm) {
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
                  partials.scalar_type() == at::kDouble,
              "clip_coef: partials must be a contiguous f64 device tensor");
  TORCH_CHECK(clip_state.is_cuda() && clip_state.is_contiguous() &&
                  clip_state.scalar_type() == at::kFloat &&
                  clip_state.numel() == 2 &&
                  clip_state.device() == partials.device(),
              "clip_coef: clip_state must be an f32[2] tensor on the "
              "partials' device");
  hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(kThreads), 0, cur_stream(),
                     partials.data_ptr<double>(), partials.numel(),
                     clip_state.data_ptr<float>(), (float)max_norm);
  HIP_OK(hipGetLastError());
}

void sgd_flat(torch::Tensor param_flat, torch::Tensor grad_flat, double lr,
              bool zero_grad, c10::optional<torch::Tensor> grad_scale) {
  const int64_t n4 = check_flat(param_flat, grad_flat, "sgd_flat");
  const float* sp = check_scale(grad_scale, param_flat, "sgd_flat");
  if (n4 == 0) return;
  DISPATCH_F32_BF16(param_flat.scalar_type(), "sgd_flat", {
    with_scaled(sp != nullptr, [&](auto scaled) {
      hipLaunchKernelGGL((k_sgd_flat<scalar_t, decltype(scaled)::value>),
                         dim3(cdiv(n4, kThreads)), dim3(kThreads), 0,
                         cur_stream(), dptr<scalar_t>(param_flat),
                         dptr<scalar_t>(grad_flat), (float)lr, n4,
                         zero_grad ? 1 : 0, sp);
    });
  });
  HIP_OK(hipGetLastError());
}

void sgd_momentum_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
                       c10::optional<torch::Tensor> buf, double lr,
                       double momentum, double weight_decay, bool nesterov,
                       bool zero_grad,
                       c10::optional<torch::Tensor> grad_scale) {
  const int64_t n4 = check_flat(param_flat, grad_flat, "sgd_momentum_flat");
  const float* sp = check_scale(grad_scale, param_flat, "sgd_momentum_flat");
  float* bp = nullptr;
  if (buf.has_value() && buf->defined()) {
    check_state(*buf, param_flat, "sgd_momentum_flat", "buf");
    bp = buf->data_ptr<float>();
  }
  TORCH_CHECK(bp != nullptr || (momentum == 0.0 && !nesterov),
              "sgd_momentum_flat: momentum needs a buffer");
  if (n4 == 0) return;
  DISPATCH_F32_BF16(param_flat.scalar_type(), "sgd_momentum_flat", {
    with_scaled(sp != nullptr, [&](auto scaled) {
      hipLaunchKernelGGL(
          (k_sgd_momentum_flat<scalar_t, decltype(scaled)::value>),
          flat_grid(n4), dim3(kThreads), 0, cur_stream(),
          dptr<scalar_t>(param_flat), dptr<scalar_t>(grad_flat), bp,
          (float)(-lr), (float)momentum, (float)weight_decay,
          nesterov ? 1 : 0, zero_grad ? 1 : 0, n4, sp);
    });
  });
  HIP_OK(hipGetLastError());
}

void adamw_tick(torch::Tensor step_state, double lr, double beta1,
                double beta2) {
  TORCH_CHECK(step_state.is_cuda() && step_state.is_contiguous() &&
                  step_state.scalar_type() == at::kInt &&
                  step_state.numel() >= 3,
              "adamw_tick: step_state must be an int32 device tensor [>=3]");
  hipLaunchKernelGGL(k_adamw_tick, dim3(1), dim3(1), 0, cur_stream(),
                     step_state.data_ptr<int32_t>(), lr, beta1, beta2);
  HIP_OK(hipGetLastError());
}

void adamw_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
                torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                torch::Tensor step_state, double lr, double beta1,
                double beta2, double eps, double weight_decay,
                c10::optional<torch::Tensor> decay_mask, bool zero_grad,
                c10::optional<torch::Tensor> grad_scale) {
  const int64_t n4 = check_flat(param_flat, grad_flat, "adamw_flat");
  const float* sp = check_scale(grad_scale, param_flat, "adamw_flat");
  check_state(exp_avg, param_flat, "adamw_flat", "exp_avg");
  check_state(exp_avg_sq, param_flat, "adamw_flat", "exp_avg_sq");
  TORCH_CHECK(step_state.is_cuda() && step_state.is_contiguous() &&
                  step_state.scalar_type() == at::kInt &&
                  step_state.numel() >= 3 &&
                  step_state.device() == param_flat.device(),
              "adamw_flat: step_state must be an int32 device tensor [>=3]");
  const uint8_t* mp = nullptr;
  if (decay_mask.has_value() && decay_mask->defined()) {
    TORCH_CHECK(decay_mask->is_cuda() && decay_mask->is_contiguous() &&
                    decay_mask->scalar_type() == at::kByte &&
                    decay_mask->numel() == n4 &&
                    decay_mask->device() == param_flat.device(),
                "adamw_flat: decay_mask must be a uint8 device tensor with "
                "one byte per 4-element group");
    mp = decay_mask->data_ptr<uint8_t>();
  }
  if (n4 == 0) return;
  DISPATCH_F32_BF16(param_flat.scalar_type(), "adamw_flat", {
    with_scaled(sp != nullptr, [&](auto scaled) {
      hipLaunchKernelGGL(
          (k_adamw_flat<scalar_t, decltype(scaled)::value>), flat_grid(n4),
          dim3(kThreads), 0, cur_stream(), dptr<scalar_t>(param_flat),
          dptr<scalar_t>(grad_flat), exp_avg.data_ptr<float>(),
          exp_avg_sq.data_ptr<float>(), step_state.data_ptr<int32_t>(),
          (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1),
          (float)beta2, (float)(1.0 - beta2), (float)eps, mp,
          zero_grad ? 1 : 0, n4, sp);
    });
  });
  HIP_OK(hipGetLastError());
}

}  // namespace mi355x
