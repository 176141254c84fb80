// MI355X (gfx950, CDNA4) kernel pack for mi355x_ddp — written directly in
// HIP for CDNA4 (64-wide wavefronts, MFMA via __builtin_amdgcn_mfma_*,
// LDS staging). No CUDA compatibility paths, no hipify.
//
// Re-implements the native components the reference pulls in implicitly
// (SURVEY.md §2.2): N6 GEMM fwd/bwd for the toy Linear (reference
// single_gpu.py:23,25 / nn.Linear(20,1) at :50), N7 CE/MSE loss kernels
// (single_gpu.py:24, multinode_torchrun.py:46), N9 zero_grad folded into
// the bucket lifecycle (single_gpu.py:22), and the reducer's bucket
// flatten/unflatten (N3). N8, the fused SGD (single_gpu.py:26), is in
// optim_kernels.hip with the other flat-bucket optimizers.
//
// Dtypes: every kernel is templated on the STORAGE type (f32 or bf16;
// bf16 is the BASELINE.json config-2 capability). Matmul compute uses
// the exact-f32 MFMA `v_mfma_f32_16x16x4_f32` for f32 storage (no
// xf32/TF32 exists on gfx950 — cdna_hip_programming.md §3) and
// `v_mfma_f32_16x16x32_bf16` for bf16; the toy shapes are single-wave
// and latency-bound, so the MFMA path buys kernel-count and issue-slot
// economy, not FLOPs.
//
// This file holds the general-purpose kernels: the linear tile kernel
// `k_linear_tile` (forward and dX, serial and split), `k_linear_bwd_w`, the
// bf16 GEMM `k_gemm_bf16`, CE/MSE (`k_ce_*`, `k_mse_*`), the bucket copy
// `k_bucket_copy`, and the epoch shard gather `k_epoch_shard_multi`, which
// fuses the epoch shuffle into one copy pass over a whole BLOCK of epochs.
// The fused toy training-step family lives in toy_kernels.hip.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kernel_common.h"
#include "ops.h"

namespace mi355x {

// ---------------------------------------------------------------------------
// Linear tile kernel: C[M,Nc] = A[M,Kc] @ Bop[Kc,Nc].
//   forward (B_T):  Y = X @ W^T + b, Bop[k][n] = W[n*Kc + k], W is [Nc,Kc]
//   dX     (!B_T):  dX = dY @ W,     Bop[k][n] = W[k*Nc + n], W is [Kc,Nc]
// Only the forward adds a bias (bias may be null); dX ignores the argument
// and stores the accumulator as it is — adding a run-time zero instead cost
// the serial dX 0.4% (profiles r05a).
// One wave (64 lanes) per 16x16 output tile; K-loop of mfma_f32_16x16x4f32
// (storage loads upconvert bf16 -> f32; exact-f32 accumulate).
// Lane maps (cdna_hip_programming.md §3): A[l&15][k=l>>4], B[k=l>>4][l&15],
// C/D col=lane&15, row=(lane>>4)*4+reg.
// !SPLIT: the 4 waves of a workgroup take 4 consecutive M-tiles.
// SPLIT, for small-M / long-contraction shapes (e.g. the ResNet-50 FC,
// 32x2048 @ 2048x1000, and its dX): the 4 waves contract DISJOINT slices of
// the SAME output tile and reduce partials through LDS — 4x the
// memory-level parallelism on shapes where M-tiling cannot fill the chip.
// ---------------------------------------------------------------------------
template <typename T, bool B_T, bool SPLIT>
__global__ void k_linear_tile(const T* __restrict__ A, const T* __restrict__ W,
                              const T* __restrict__ bias, T* __restrict__ C,
                              int M, int Kc, int Nc) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int tile_m = SPLIT ? blockIdx.x : blockIdx.x * 4 + wave;
  const int tile_n = blockIdx.y;
  if (!SPLIT && tile_m * 16 >= M) return;
  const int r = lane & 15;
  const int q = lane >> 4;
  const int m = tile_m * 16 + r;  // A row for this lane
  const int n = tile_n * 16 + r;  // Bop column for this lane
  int k_lo = 0, k_hi = Kc;
  if constexpr (SPLIT) {
    const int kq = (((Kc + 3) / 4 + 3) / 4) * 4;  // slice per wave (mult of 4)
    k_lo = wave * kq;
    k_hi = min(Kc, (wave + 1) * kq);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = k_lo; k0 < k_hi; k0 += 4) {
    const int k = k0 + q;
    const float a = (m < M && k < Kc) ? ldf(&A[(size_t)m * Kc + k]) : 0.f;
    const size_t wi = B_T ? (size_t)n * Kc + k : (size_t)k * Nc + n;
    const float b = (n < Nc && k < Kc) ? ldf(&W[wi]) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int col = tile_n * 16 + r;
  if constexpr (SPLIT) {
    __shared__ float red[4][64][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][lane][i] = acc[i];
    __syncthreads();
    if (wave == 0) {
      const float bv = (B_T && bias && col < Nc) ? ldf(&bias[col]) : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile_m * 16 + q * 4 + i;
        if (row < M && col < Nc) {
          const float v = red[0][lane][i] + red[1][lane][i] +
                          red[2][lane][i] + red[3][lane][i];
          stf(&C[(size_t)row * Nc + col], B_T ? v + bv : v);
        }
      }
    }
  } else if (col < Nc) {
    const float bv = (B_T && bias) ? ldf(&bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = tile_m * 16 + q * 4 + i;
      if (row < M)
        stf(&C[(size_t)row * Nc + col], B_T ? acc[i] + bv : acc[i]);
    }
  }
}

// Picks the split form for M < 64, the serial one otherwise.
template <bool B_T>
static torch::Tensor linear_tile(const torch::Tensor& a, const torch::Tensor& w,
                                 const c10::optional<torch::Tensor>& bias,
                                 const char* name) {
  TORCH_CHECK(a.is_cuda() && w.device() == a.device(), name,
              ": operands must be on one device");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2 &&
                  a.size(1) == w.size(B_T ? 1 : 0),
              name, ": shape mismatch");
  TORCH_CHECK(a.scalar_type() == w.scalar_type(), name, ": dtype mismatch");
  auto ac = a.contiguous();
  auto wc = w.contiguous();
  const int M = (int)ac.size(0), Kc = (int)ac.size(1);
  const int Nc = (int)wc.size(B_T ? 0 : 1);
  torch::Tensor bc;
  if (bias.has_value()) {
    TORCH_CHECK(bias->device() == a.device() &&
                    bias->scalar_type() == a.scalar_type() &&
                    bias->dim() == 1 && bias->size(0) == Nc,
                name, ": bias must be a [", Nc, "] tensor of the operands' ",
                "dtype and device");
    bc = bias->contiguous();
  }
  auto c = at::empty({M, Nc}, a.options());
  if (M == 0 || Nc == 0) return c;  // nothing to compute: no zero-block grid
  const bool split = M < 64;
  const dim3 grid(cdiv(M, split ? 16 : 64), cdiv(Nc, 16));
  DISPATCH_F32_BF16(a.scalar_type(), name, {
    auto kernel = split ? k_linear_tile<scalar_t, B_T, true>
                        : k_linear_tile<scalar_t, B_T, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, cur_stream(),
                       cdptr<scalar_t>(ac), cdptr<scalar_t>(wc),
                       bc.defined() ? cdptr<scalar_t>(bc) : nullptr,
                       dptr<scalar_t>(c), M, Kc, Nc);
  });
  HIP_OK(hipGetLastError());
  return c;
}

torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias) {
  return linear_tile<true>(x, w, bias, "linear_fwd");
}

// dX[B,K] = dY[B,N] @ W[N,K]
torch::Tensor linear_bwd_input(torch::Tensor dy, torch::Tensor w) {
  return linear_tile<false>(dy, w, c10::nullopt, "linear_bwd_input");
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
  const char* name = "linear_bwd_weight";
  TORCH_CHECK(x.is_cuda() && dy.device() == x.device() &&
                  dw.device() == x.device() && db.device() == x.device(),
              name, ": x, dy, dw and db must be on one device");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() &&
                  dw.scalar_type() == x.scalar_type() &&
                  db.scalar_type() == x.scalar_type(),
              name, ": dtype mismatch (x ", x.scalar_type(), ", dy ",
              dy.scalar_type(), ", dw ", dw.scalar_type(), ", db ",
              db.scalar_type(), ")");
  TORCH_CHECK(x.dim() == 2 && dy.dim() == 2 && dy.size(0) == x.size(0), name,
              ": shape mismatch, x must be [B,K] and dy [B,N]");
  TORCH_CHECK(dw.dim() == 2 && dw.size(0) == dy.size(1) &&
                  dw.size(1) == x.size(1),
              name, ": dw must be [N,K] = [", dy.size(1), ",", x.size(1), "]");
  // an empty db means: no bias gradient wanted
  TORCH_CHECK(db.numel() == 0 || (db.dim() == 1 && db.size(0) == dy.size(1)),
              name, ": db must be empty or [N] = [", dy.size(1), "]");
  auto xc = x.contiguous();
  auto dyc = dy.contiguous();
  TORCH_CHECK(dw.is_contiguous() && db.is_contiguous(), "grad views must be contiguous");
  const int B = (int)xc.size(0), K = (int)xc.size(1), N = (int)dyc.size(1);
  if (B == 0 || K == 0 || N == 0) {  // an empty contraction or an empty dW
    if (!accumulate) {
      dw.zero_();
      db.zero_();
    }
    return;
  }
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

// ---------------------------------------------------------------------------
// Standalone bf16 MFMA GEMM: Y[B,N] = X[B,K] @ W[N,K]^T (+bias), f32
// accumulate via v_mfma_f32_16x16x32_bf16 (the gfx950 2xK form). One wave
// per 16x16 tile, K consumed 32 at a time, 8 bf16 per lane per operand.
// A: lane l holds A[l&15][(l>>4)*8 + j], j=0..7; B-op: W[l&15][(l>>4)*8+j];
// C/D: col=lane&15, row=(lane>>4)*4+reg (cdna_hip_programming.md §3).
// No model path routes here (HipLinear takes k_linear_tile or rocBLAS); it
// is bound as ops.ext().gemm_bf16, verified against torch in
// tests/test_bf16_gpu.py and timed by tools/bench_kernels.py.
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
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "gemm_bf16: x must be a device bf16 tensor");
  TORCH_CHECK(w.device() == x.device() && w.scalar_type() == at::kBFloat16,
              "gemm_bf16: w must be bf16 on x's device");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
              "gemm_bf16: shape mismatch, x must be [B,K] and w [N,K]");
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  const int B = (int)xc.size(0), K = (int)xc.size(1), N = (int)wc.size(0);
  torch::Tensor bc;
  bool has_bias = bias.has_value();
  if (has_bias) {
    TORCH_CHECK(bias->device() == x.device() &&
                    bias->scalar_type() == at::kBFloat16 &&
                    bias->dim() == 1 && bias->size(0) == N,
                "gemm_bf16: bias must be a bf16 [", N, "] tensor on x's device");
    bc = bias->contiguous();
  }
  auto y = at::empty({B, N}, x.options());
  if (B == 0 || N == 0) return y;
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
    ty += tv * (yv - m);
  }
  se = wave_sum(se); ts = wave_sum(ts); ty = wave_sum(ty);
  const float inv_se = 1.f / se;
  for (int c = lane; c < C; c += 64) p[c] = __expf(ldf(&y[c]) - m) * inv_se;
  if (lane == 0) {
    tsum[row] = ts;
    // -sum_c t_c * log_softmax(y)_c with the row max taken out of BOTH
    // terms: ts * (m + log se) - sum t*y cancels catastrophically once the
    // logits share a large offset (an f32 ulp at 1e4 is 1e-3)
    atomicAdd(loss, (ts * __logf(se) - ty) / (float)B);
  }
}

std::vector<torch::Tensor> ce_fwd(torch::Tensor y, torch::Tensor t) {
  TORCH_CHECK(y.is_cuda() && t.device() == y.device(),
              "ce_fwd: output and targets must be on one device");
  TORCH_CHECK(y.dim() == 2, "ce_fwd: the output must be [B,C]");
  TORCH_CHECK(t.scalar_type() == y.scalar_type(), "ce_fwd: dtype mismatch (",
              y.scalar_type(), " output, ", t.scalar_type(), " targets)");
  auto yc = y.contiguous();
  auto tc = t.contiguous();
  TORCH_CHECK(tc.sizes() == yc.sizes(),
              "ce: probability targets must match the output shape (got ",
              tc.sizes(), " vs ", yc.sizes(), ")");
  const int B = (int)yc.size(0), C = (int)yc.size(1);
  auto f32opt = yc.options().dtype(at::kFloat);
  if (B == 0 || C == 0) {  // torch: the mean over nothing is nan
    return {at::full({}, NAN, f32opt), at::empty({B, C}, f32opt),
            at::zeros({B}, f32opt)};
  }
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

// The optional incoming scalar grad of ce_bwd / mse_bwd, as a device pointer.
static const float* gout_ptr(const c10::optional<torch::Tensor>& gout,
                             const char* name) {
  if (!gout.has_value()) return nullptr;
  TORCH_CHECK(gout->is_cuda() && gout->numel() == 1 &&
                  gout->scalar_type() == at::kFloat,
              name, " gout must be a device f32 scalar");
  return gout->data_ptr<float>();
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
  TORCH_CHECK(t.is_cuda() && probs.device() == t.device() &&
                  tsum.device() == t.device(),
              "ce_bwd: probs, targets and tsum must be on one device");
  TORCH_CHECK(probs.scalar_type() == at::kFloat &&
                  tsum.scalar_type() == at::kFloat,
              "ce_bwd: probs and tsum are the f32 outputs of ce_fwd");
  TORCH_CHECK(probs.dim() == 2 && probs.is_contiguous() &&
                  t.sizes() == probs.sizes(),
              "ce_bwd: probs must be contiguous [B,C] and match the targets");
  TORCH_CHECK(tsum.dim() == 1 && tsum.size(0) == probs.size(0) &&
                  tsum.is_contiguous(),
              "ce_bwd: tsum must be contiguous [B]");
  const int B = (int)probs.size(0), C = (int)probs.size(1);
  auto tc = t.contiguous();
  auto dy = at::empty({B, C}, tc.options());
  const int64_t n = (int64_t)B * C;
  const float* gp = gout_ptr(gout, "ce_bwd");
  if (n == 0) return dy;
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
  TORCH_CHECK(y.is_cuda() && t.device() == y.device(),
              "mse_fwd: output and target must be on one device");
  TORCH_CHECK(t.scalar_type() == y.scalar_type(), "mse_fwd: dtype mismatch (",
              y.scalar_type(), " output, ", t.scalar_type(), " target)");
  const int64_t n = yc.numel();
  if (n == 0)  // torch: the mean over nothing is nan
    return at::full({}, NAN, yc.options().dtype(at::kFloat));
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
  TORCH_CHECK(y.is_cuda() && t.device() == y.device(),
              "mse_bwd: output and target must be on one device");
  TORCH_CHECK(t.scalar_type() == y.scalar_type(), "mse_bwd: dtype mismatch (",
              y.scalar_type(), " output, ", t.scalar_type(), " target)");
  TORCH_CHECK(t.sizes() == y.sizes(), "mse: target shape ", t.sizes(),
              " != output shape ", y.sizes());
  auto yc = y.contiguous();
  auto tc = t.contiguous();
  const int64_t n = yc.numel();
  auto dy = at::empty_like(yc);
  const float* gp = gout_ptr(gout, "mse_bwd");
  if (n == 0) return dy;
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

// The plan rows are raw addresses: all that can be checked here is that the
// launch reads no more rows than the plan has.
static void check_copy_plan(const torch::Tensor& bucket,
                            const torch::Tensor& plan, int64_t total_blocks,
                            const char* name) {
  TORCH_CHECK(bucket.is_cuda() && plan.device() == bucket.device(), name,
              ": bucket and plan must be on one device");
  TORCH_CHECK(plan.scalar_type() == at::kLong && plan.is_contiguous() &&
                  plan.dim() == 2 && plan.size(1) == 3,
              name, ": plan must be a contiguous int64 [blocks,3] tensor");
  TORCH_CHECK(total_blocks >= 0 && total_blocks <= plan.size(0), name,
              ": total_blocks ", total_blocks, " outside the plan's ",
              plan.size(0), " rows");
}

void flatten_into(torch::Tensor bucket, torch::Tensor plan,
                  int64_t total_blocks, bool zero_src) {
  check_copy_plan(bucket, plan, total_blocks, "flatten_into");
  if (total_blocks == 0) return;  // an empty plan copies nothing
  hipLaunchKernelGGL((k_bucket_copy<true>), dim3((uint32_t)total_blocks),
                     dim3(256), 0, cur_stream(),
                     reinterpret_cast<char*>(bucket.data_ptr()),
                     plan.data_ptr<int64_t>(), zero_src ? 1 : 0);
  HIP_OK(hipGetLastError());
}

void unflatten_from(torch::Tensor bucket, torch::Tensor plan, int64_t total_blocks) {
  check_copy_plan(bucket, plan, total_blocks, "unflatten_from");
  if (total_blocks == 0) return;
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
//
// One launch gathers `epochs` consecutive epoch shards (seeds seed0,
// seed0+1, …) into one contiguous buffer pair; block e is what a
// single-epoch launch with seed0+e writes. This is what lets the
// persistent-engine deferral span epoch boundaries (one multistep launch
// per ~max_defer steps instead of one per epoch, profiles r01q) and, as a
// side effect, gives this gather kernel epochs× more workgroups to fill the
// 256 CUs with.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix_bijection(
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

__device__ __forceinline__ void shard_consts(
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
  TORCH_CHECK(X.is_cuda() && Tg.is_cuda() && X.is_contiguous() &&
              Tg.is_contiguous());
  TORCH_CHECK(Tg.device() == X.device() &&
                  Tg.scalar_type() == X.scalar_type(),
              "epoch_shard: X and T must share a device and a dtype");
  TORCH_CHECK(epochs >= 1 && epochs <= 1 << 20, "epochs out of range");
  TORCH_CHECK(X.dim() == 2 && Tg.dim() == 2, "epoch_shard: X must be [n,K] ",
              "and T [n,1]");
  const int n = (int)X.size(0), K = (int)X.size(1);
  TORCH_CHECK(Tg.size(0) == n && Tg.size(1) == 1, "targets must be [n,1]");
  TORCH_CHECK(world >= 1 && rank >= 0 && rank < world,
              "epoch_shard: rank ", rank, " outside world ", world);
  TORCH_CHECK(world <= n, "epoch_shard: world ", world, " exceeds the ", n,
              " dataset rows, every shard would be empty");
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

std::vector<torch::Tensor> epoch_shard(torch::Tensor X, torch::Tensor Tg,
                                       int64_t seed, int64_t rank,
                                       int64_t world) {
  return epoch_shard_multi(X, Tg, seed, 1, rank, world);
}

}  // namespace mi355x
