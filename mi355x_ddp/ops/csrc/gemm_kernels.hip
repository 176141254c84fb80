// LDS-tiled, register-blocked MFMA GEMMs for transformer-sized linear layers
// on gfx950 (MI355X), in the three orientations a linear layer needs, with
// the elementwise work of an MLP in their epilogues.
//
//   NT  C[M,N] = A[M,K] . B[N,K]^T   forward    (+ bias; + GELU, two outputs)
//   NN  C[M,K] = A[M,N] . B[N,K]     dX         (x gelu'(h): dh from dA)
//   TN  C[N,K] = A[M,N]^T . B[M,K]   dW, and db[n] = sum_m A[m][n]
//
// Storage T is f32 or bf16, alike for all operands of a call; operands are
// contiguous, 2-D and 16-byte aligned; every feature dimension is a multiple
// of 16, the row count (M) is any number. Accumulation is f32.
//
// One kernel, k_gemm_tile<T, TA, TB, EPI>. The output is C[I, J] and the
// contraction has length Kc; an operand is "straight" (its contraction index
// is the contiguous dimension of its source: element (i, k) at src[i*Kc + k])
// or "transposed" (TA / TB: the contraction index is the ROW of its source:
// element (i, k) at src[k*I + i]). NT = straight x straight, NN = straight x
// transposed, TN = transposed x transposed.
//
// Work split. 256 threads own a BM x BN = 128 x 128 tile of C and walk the
// contraction in blocks of BK = 32. The four waves sit 2 x 2 on the tile; a
// wave owns 64 x 64 = 4 x 4 MFMA tiles of 16 x 16, 16 accumulators of four
// f32 (64 registers). Per block a wave reads four A and four B fragments
// from LDS and issues 16 MFMAs: every fragment feeds four of them.
// No split-K, no atomics.
//
// Data movement. Global to registers in 16-byte loads (8 bf16 / 4 f32 per
// lane), registers to LDS, LDS to MFMA operands. The loads of block k+1 are
// issued before the MFMAs of block k and land in registers while they run;
// there is one LDS stage and two barriers per block. Loads are branch-free:
// a row or chunk outside the operand has its ADDRESS clamped into it and its
// value replaced by zero (a select) on the way into LDS. Feature dimensions
// are multiples of 16, so a 16-byte chunk is inside or outside as a whole;
// the row count is arbitrary and is masked per row.
//
// LDS images (one per operand, words of four bytes):
//   bf16, any orientation  [128 outputs][32 k], pitch 20 words (40 bf16).
//       An MFMA operand (v_mfma_f32_16x16x32_bf16: lane (r, q) holds k =
//       8q..8q+7 of output r) is ONE ds_read_b128 at (row0 + r)*20 + 4q.
//       A straight operand is stored as loaded (ds_write_b128). A transposed
//       operand is TRANSPOSED WHILE STORING: a thread loads the same 8
//       outputs of two adjacent contraction rows 2p, 2p+1, interleaves them
//       into 8 words (k = 2p in the low half) and stores word (8c + i)*20 + p
//       for i < 8: every read stays a ds_read_b128, whatever the orientation.
//   f32 straight    "rk" [128 outputs][32 k], pitch 36: the lane's operand of
//       v_mfma_f32_16x16x4_f32 is the word (row0 + r)*36 + k0 + q; over 64
//       banks 36 r + q is a bijection (conflict-free).
//   f32 transposed  "kr" [32 k][128 outputs], pitch 144, stored as loaded;
//       the operand is the word (k0 + q)*144 + col0 + r, conflict-free at
//       pitch = 16 (mod 64). One word per lane: no transposition needed.
// bf16: 2 x 10240 B; f32: 2 x 18432 B. Both under the 64 KB every launch gets.
//
// Epilogues, on the f32 accumulators before the single rounding to T:
//   kPlain     + bias[col] when a bias is given (NT), else nothing
//   kGelu      h = acc + bias rounded to T and stored; a = gelu(h) of that
//              ROUNDED h (exact erf form), stored to C
//   kGeluGrad  acc * gelu'(h), h read from a [I, J] tensor of T,
//              gelu'(h) = Phi(h) + h phi(h)
//   kColSum    C as it is; also colsum[i] = sum_k A(i, k) (TN: db). In the
//              workgroups of output-column tile 0, and only there, every
//              thread adds the A chunks it stages anyway into registers;
//              they are reduced through LDS in a fixed order and stored. No atomics, nothing pre-zeroed: the
//              same bits run to run.
#include <algorithm>
#include <type_traits>

#include "gemm_tile.h"
#include "ops.h"

// No packed-fp32 VALU forms (v_pk_*_f32) in this file's device code. Header
// functions do not carry the attribute and would become calls: the device
// code below uses clang vector types and builtins only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace mi355x {

namespace {

enum GemmEpi { kPlain = 0, kGelu = 1, kGeluGrad = 2, kColSum = 3 };

constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;
// erf in f32 without a library call (the device library's erf would stay a
// CALL under this file's target attribute). |x| <= 1: x P(x^2), a degree-7
// fit of erf(sqrt t)/sqrt t on [0, 1]; 1 < |x| <= 4: 1 - exp(R(|x|)), R a
// degree-10 fit of log erfc on [1, 4]; beyond 4 erf is 1 in f32. Both fits
// are Chebyshev-node least squares against fp64 erf/erfc, 3e-11 and 3e-10
// off in exact arithmetic; evaluated in f32 the worst absolute error over
// [-6, 6] is 1.5e-7 (2.5 ulp of erf near |x| = 1). The bound is ABSOLUTE:
// 1 + erf(x) for x below about -2 keeps few significant digits, so Phi(h),
// gelu(h) and gelu'(h) in the negative tail are small and absolutely
// accurate, not relatively.
__device__ __forceinline__ float erf_f32(float x) {
  const float ax = __builtin_fabsf(x);
  float r;
  if (ax <= 1.f) {
    const float t = ax * ax;
    float p = -9.67359028e-06f;
    p = __builtin_fmaf(p, t, 0.000112682537f);
    p = __builtin_fmaf(p, t, -0.000848439639f);
    p = __builtin_fmaf(p, t, 0.00522105349f);
    p = __builtin_fmaf(p, t, -0.0268654376f);
    p = __builtin_fmaf(p, t, 0.112837829f);
    p = __builtin_fmaf(p, t, -0.376126379f);
    p = __builtin_fmaf(p, t, 1.12837923f);
    r = ax * p;
  } else {
    const float u = ax < 4.f ? ax : 4.f;
    float s = -4.10484944e-08f;
    s = __builtin_fmaf(s, u, 9.60383773e-07f);
    s = __builtin_fmaf(s, u, -8.2187853e-06f);
    s = __builtin_fmaf(s, u, 1.22791607e-05f);
    s = __builtin_fmaf(s, u, 0.000376564247f);
    s = __builtin_fmaf(s, u, -0.00420608418f);
    s = __builtin_fmaf(s, u, 0.0254840702f);
    s = __builtin_fmaf(s, u, -0.109025255f);
    s = __builtin_fmaf(s, u, -0.63258183f);
    s = __builtin_fmaf(s, u, -1.12992203f);
    s = __builtin_fmaf(s, u, 0.000264003844f);
    r = 1.f - __builtin_expf(s);
  }
  return __builtin_copysignf(r, x);
}
// nn.GELU(): x Phi(x), Phi by erf.
__device__ __forceinline__ float gelu(float h) {
  return 0.5f * h * (1.f + erf_f32(h * kRsqrt2));
}
// Phi(h) + h phi(h)
__device__ __forceinline__ float gelu_grad(float h) {
  const float cdf = 0.5f * (1.f + erf_f32(h * kRsqrt2));
  const float pdf = __builtin_expf(-0.5f * h * h) * kRsqrt2Pi;
  return __builtin_fmaf(h, pdf, cdf);
}

// One operand's way from global memory to its LDS image. `n_out` outputs
// (rows of C for A, columns of C for B), `n_k` contraction indices, `out0`
// the tile's first output. TR: the contraction index is the source's row.
// Which chunks the thread moves and how they reach LDS: TileMap.
template <typename T, bool TR>
struct Operand {
  using G = Geo<T>;

  const T* src;
  int n_out, n_k, out0;
  TileMap<T, TR> m;
  u32x4 v[G::NP];

  __device__ __forceinline__ void init(const T* s, int nout, int nk, int o0,
                                       int tid) {
    src = s, n_out = nout, n_k = nk, out0 = o0;
    m.init(tid);
  }
  __device__ __forceinline__ bool inside(int j, int k0) const {
    if constexpr (!TR)
      return out0 + m.slot_row(j) < n_out && k0 + m.c * G::E < n_k;
    else
      return k0 + m.slot_row(j) < n_k && out0 + m.c * G::E < n_out;
  }
  // Issue the 16-byte loads of contraction block k0; addresses clamped.
  __device__ __forceinline__ void load(int k0) {
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      int row, col, ld;
      if constexpr (!TR) {
        row = out0 + m.slot_row(j), row = row < n_out ? row : n_out - 1;
        col = k0 + m.c * G::E, col = col < n_k ? col : 0, ld = n_k;
      } else {
        row = k0 + m.slot_row(j), row = row < n_k ? row : n_k - 1;
        col = out0 + m.c * G::E, col = col < n_out ? col : 0, ld = n_out;
      }
      v[j] = *reinterpret_cast<const u32x4*>(src + (int64_t)row * ld + col);
    }
  }
  // Registers to the LDS image, zero where the operand ends.
  template <bool SUM>
  __device__ __forceinline__ void store(uint32_t* img, int k0,
                                        float* colacc) {
    u32x4 x[G::NP];
#pragma unroll
    for (int j = 0; j < G::NP; ++j)
      x[j] = inside(j, k0) ? v[j] : u32x4{0u, 0u, 0u, 0u};
    m.template store<SUM>(img, x, colacc);
  }
};

// C[I, J] = A (I x Kc) . B (J x Kc)^T in the orientations of the header.
// aux: kGelu the h output, kGeluGrad the h input ([I, J] like C); colsum [I].
template <typename T, bool TA, bool TB, int EPI>
__global__ __launch_bounds__(kGemmThreads) void k_gemm_tile(
    const T* __restrict__ A, const T* __restrict__ B, T* __restrict__ C,
    const T* __restrict__ bias, T* __restrict__ aux, T* __restrict__ colsum,
    int I, int J, int Kc) {
  using G = Geo<T>;
  __shared__ __attribute__((aligned(16))) uint32_t smem[2 * G::WORDS];
  uint32_t* imgA = smem;
  uint32_t* imgB = smem + G::WORDS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.x * kBM, j0 = blockIdx.y * kBN;
  const int rowA = (wave >> 1) * 64 + r, rowB = (wave & 1) * 64 + r;

  Operand<T, TA> opA;
  Operand<T, TB> opB;
  opA.init(A, I, Kc, i0, tid);
  opB.init(B, J, Kc, j0, tid);
  float colacc[G::E];
#pragma unroll
  for (int e = 0; e < G::E; ++e) colacc[e] = 0.f;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  opA.load(0), opB.load(0);
  for (int k0 = 0; k0 < Kc; k0 += kBK) {
    if (EPI == kColSum && blockIdx.y == 0)  // uniform: only tile 0 sums
      opA.template store<EPI == kColSum>(imgA, k0, colacc);
    else
      opA.template store<false>(imgA, k0, nullptr);
    opB.template store<false>(imgB, k0, nullptr);
    block_sync();
    if (k0 + kBK < Kc) opA.load(k0 + kBK), opB.load(k0 + kBK);
    multiply_block<T, TA, TB>(imgA, imgB, rowA, rowB, q, acc);
    block_sync();
  }

  if constexpr (EPI == kColSum) {
    if (blockIdx.y == 0) {  // the images are free: [RG][128] partial sums
      float* part = reinterpret_cast<float*>(smem);
      const int g = std::is_same<T, float>::value ? opA.m.rbase : opA.m.rbase >> 1;
#pragma unroll
      for (int e = 0; e < G::E; ++e)
        part[g * kBM + opA.m.c * G::E + e] = colacc[e];
      block_sync();
      if (tid < kBM && i0 + tid < I) {
        float t = part[tid];
#pragma unroll
        for (int k = 1; k < G::RG; ++k) t += part[k * kBM + tid];
        st1(&colsum[i0 + tid], t);
      }
    }
  }

#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = j0 + rowB + 16 * j;
    if (col >= J) continue;
    float bv = 0.f;
    if constexpr (EPI == kPlain || EPI == kGelu)
      if (bias != nullptr) bv = ld1(&bias[col]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = i0 + (wave >> 1) * 64 + 16 * i + 4 * q + e;
        if (row >= I) continue;
        const int64_t off = (int64_t)row * J + col;
        float val = acc[i][j][e];
        if constexpr (EPI == kPlain) {
          val += bv;
        } else if constexpr (EPI == kGelu) {
          const float h = stored(val + bv, C);
          st1(&aux[off], h);
          val = gelu(h);
        } else if constexpr (EPI == kGeluGrad) {
          val *= gelu_grad(ld1(&aux[off]));
        }
        st1(&C[off], val);
      }
    }
  }
}

// dh = da * gelu'(h) over n / E chunks of 16 bytes, grid-stride.
template <typename T>
__global__ __launch_bounds__(kGemmThreads) void k_gelu_grad_mul(
    const T* __restrict__ da, const T* __restrict__ h, T* __restrict__ dh,
    int64_t chunks) {
  constexpr int E = Geo<T>::E;
  for (int64_t i = (int64_t)blockIdx.x * kGemmThreads + threadIdx.x;
       i < chunks; i += (int64_t)gridDim.x * kGemmThreads) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(da + i * E);
    const u32x4 x = *reinterpret_cast<const u32x4*>(h + i * E);
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if constexpr (E == 4) {
        o[w] = __builtin_bit_cast(uint32_t,
                                  as_f32(a[w]) * gelu_grad(as_f32(x[w])));
      } else {
        o[w] = bf16_pack(
            as_f32(a[w] << 16) * gelu_grad(as_f32(x[w] << 16)),
            as_f32(a[w] & 0xffff0000u) * gelu_grad(as_f32(x[w] & 0xffff0000u)));
      }
    }
    *reinterpret_cast<u32x4*>(dh + i * E) = o;
  }
}

// The argument check shared by gemm_nt, gemm_nn and gemm_tn, complete before
// any launch. `mats`: the 2-D operands and preallocated results with the
// shapes they must have (the first one, the reference operand, fixes dtype
// and device); `vecs`: the same for the 1-D ones; `features`: the dimensions
// that must be multiples of 16.
struct GemmArg {
  const char* name;
  const torch::Tensor* t;  // nullptr: not given
  std::vector<int64_t> shape;
};
void gemm_check_args(const char* who, std::initializer_list<GemmArg> args,
                     std::initializer_list<int64_t> features) {
  const torch::Tensor& ref = *args.begin()->t;
  TORCH_CHECK(ref.defined() && ref.is_cuda(), who, ": ", args.begin()->name,
              " must be on a GPU");
  const auto dt = ref.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  for (const int64_t f : features)
    TORCH_CHECK(f >= 0 && f % 16 == 0 && f < (int64_t(1) << 31), who,
                ": every feature dimension must be a multiple of 16, got ",
                f);
  for (const auto& a : args) {
    if (a.t == nullptr) continue;
    TORCH_CHECK(a.t->defined() && a.t->device() == ref.device() &&
                    a.t->scalar_type() == dt,
                who, ": ", a.name, " must have ", args.begin()->name,
                "'s dtype and device");
    TORCH_CHECK(a.t->sizes() == at::IntArrayRef(a.shape) &&
                    a.t->is_contiguous() && aligned16(*a.t),
                who, ": ", a.name,
                " must be contiguous, 16-byte aligned and of shape ",
                at::IntArrayRef(a.shape), ", got ", a.t->sizes());
  }
  TORCH_CHECK(ref.size(0) < (int64_t(1) << 31), who, ": too many rows");
}

const torch::Tensor* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? &*t : nullptr;
}
torch::Tensor result(const c10::optional<torch::Tensor>& given,
                     at::IntArrayRef shape, const torch::Tensor& like) {
  return given.has_value() ? *given : torch::empty(shape, like.options());
}

template <typename T, bool TA, bool TB, int EPI>
void launch_gemm(const torch::Tensor& a, const torch::Tensor& b,
                 torch::Tensor& c, const torch::Tensor* bias,
                 torch::Tensor* aux, torch::Tensor* colsum, int64_t I,
                 int64_t J, int64_t Kc) {
  hipLaunchKernelGGL((k_gemm_tile<T, TA, TB, EPI>),
                     dim3(cdiv(I, kBM), cdiv(J, kBN)), dim3(kGemmThreads), 0,
                     cur_stream(), cdptr<T>(a), cdptr<T>(b), dptr<T>(c),
                     bias ? cdptr<T>(*bias) : nullptr,
                     aux ? dptr<T>(*aux) : nullptr,
                     colsum ? dptr<T>(*colsum) : nullptr, (int)I, (int)J,
                     (int)Kc);
  HIP_OK(hipGetLastError());
}

}  // namespace

std::vector<int64_t> gemm_tile_shape() { return {kBM, kBN, kBK}; }

std::vector<torch::Tensor> gemm_nt(torch::Tensor x, torch::Tensor w,
                                   c10::optional<torch::Tensor> bias,
                                   bool gelu,
                                   c10::optional<torch::Tensor> y_,
                                   c10::optional<torch::Tensor> h_) {
  const char* who = "gemm_nt";
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, who, ": x and w must be 2-D");
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(gelu || !h_.has_value(), who, ": h needs gelu=True");
  gemm_check_args(who,
                  {{"x", &x, {M, K}},
                   {"w", &w, {N, K}},
                   {"bias", opt_ptr(bias), {N}},
                   {"y", opt_ptr(y_), {M, N}},
                   {"h", opt_ptr(h_), {M, N}}},
                  {K, N});
  auto y = result(y_, {M, N}, x);
  torch::Tensor h;
  if (gelu) h = result(h_, {M, N}, x);
  if (M > 0 && N > 0) {
    if (K == 0) {  // an empty contraction: the bias alone
      auto& lin = gelu ? h : y;
      lin.zero_();
      if (bias.has_value()) lin.add_(*bias);
      if (gelu) y.copy_(torch::gelu(h));
    } else {
      DISPATCH_F32_BF16(x.scalar_type(), who, {
        if (gelu)
          launch_gemm<scalar_t, false, false, kGelu>(x, w, y, opt_ptr(bias),
                                                     &h, nullptr, M, N, K);
        else
          launch_gemm<scalar_t, false, false, kPlain>(
              x, w, y, opt_ptr(bias), nullptr, nullptr, M, N, K);
      });
    }
  }
  if (gelu) return {h, y};
  return {y};
}

torch::Tensor gemm_nn(torch::Tensor dy, torch::Tensor w,
                      c10::optional<torch::Tensor> gelu_grad_of,
                      c10::optional<torch::Tensor> dx_) {
  const char* who = "gemm_nn";
  TORCH_CHECK(dy.dim() == 2 && w.dim() == 2, who, ": dy and w must be 2-D");
  const int64_t M = dy.size(0), N = dy.size(1), K = w.size(1);
  gemm_check_args(who,
                  {{"dy", &dy, {M, N}},
                   {"w", &w, {N, K}},
                   {"gelu_grad_of", opt_ptr(gelu_grad_of), {M, K}},
                   {"dx", opt_ptr(dx_), {M, K}}},
                  {N, K});
  auto dx = result(dx_, {M, K}, dy);
  if (M > 0 && K > 0) {
    if (N == 0) {
      dx.zero_();
    } else {
      DISPATCH_F32_BF16(dy.scalar_type(), who, {
        if (gelu_grad_of.has_value())
          launch_gemm<scalar_t, false, true, kGeluGrad>(
              dy, w, dx, nullptr, &*gelu_grad_of, nullptr, M, K, N);
        else
          launch_gemm<scalar_t, false, true, kPlain>(dy, w, dx, nullptr,
                                                     nullptr, nullptr, M, K,
                                                     N);
      });
    }
  }
  return dx;
}

std::vector<torch::Tensor> gemm_tn(torch::Tensor dy, torch::Tensor x,
                                   c10::optional<torch::Tensor> dw_,
                                   c10::optional<torch::Tensor> db_) {
  const char* who = "gemm_tn";
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2, who, ": dy and x must be 2-D");
  const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
  gemm_check_args(who,
                  {{"dy", &dy, {M, N}},
                   {"x", &x, {M, K}},
                   {"dw", opt_ptr(dw_), {N, K}},
                   {"db", opt_ptr(db_), {N}}},
                  {N, K});
  auto dw = result(dw_, {N, K}, dy);
  auto db = result(db_, {N}, dy);
  if (N > 0) {
    if (M == 0) {
      dw.zero_(), db.zero_();
    } else if (K == 0) {  // no weight tile to ride on
      db.copy_(dy.sum(0));
    } else {
      DISPATCH_F32_BF16(dy.scalar_type(), who, {
        launch_gemm<scalar_t, true, true, kColSum>(dy, x, dw, nullptr,
                                                   nullptr, &db, N, K, M);
      });
    }
  }
  return {dw, db};
}

torch::Tensor gelu_grad_mul(torch::Tensor da, torch::Tensor h) {
  const char* who = "gelu_grad_mul";
  TORCH_CHECK(da.dim() == 2, who, ": da must be 2-D");
  const int64_t M = da.size(0), N = da.size(1);
  gemm_check_args(who, {{"da", &da, {M, N}}, {"h", &h, {M, N}}}, {N});
  auto dh = torch::empty_like(da);
  const int64_t n = M * N;
  if (n > 0) {
    DISPATCH_F32_BF16(da.scalar_type(), who, {
      const int64_t chunks = n / Geo<scalar_t>::E;
      hipLaunchKernelGGL((k_gelu_grad_mul<scalar_t>),
                         dim3((int)std::min<int64_t>(
                             4096, (chunks + kGemmThreads - 1) / kGemmThreads)),
                         dim3(kGemmThreads), 0, cur_stream(),
                         cdptr<scalar_t>(da), cdptr<scalar_t>(h),
                         dptr<scalar_t>(dh), chunks);
    });
    HIP_OK(hipGetLastError());
  }
  return dh;
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
