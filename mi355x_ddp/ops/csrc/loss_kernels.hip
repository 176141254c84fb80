// Fused cross-entropy on integer class labels for gfx950 (MI355X), forward and
// backward, with label smoothing, ignore_index and the three reductions.
//
//   logits, dlogits  [B, C]     rows are the flattened leading dimensions,
//                               storage T (f32 | bf16), 16-byte aligned base
//   labels           [B]        int64 | int32
//   workspace        [B, S, 4]  f32, one record per (row, column segment)
//   row_stats        [B, 2]     f32 (M, 1/L): the row maximum and the
//                               reciprocal of sum_c exp(y_c - M)
//   loss             [] | [B]   f32
//   inv_count        [1]        f32: 1 ("sum", "none") or 1 / #non-ignored rows
//
// All arithmetic is f32; bf16 is widened on load and dlogits rounded once.
// Exponentials are v_exp_f32 on (y - m) * log2(e).
//
// Vectors and misaligned rows. The unit of a load is four adjacent elements
// (16 bytes f32, 8 bytes bf16), as in the LayerNorm kernels. Row r begins at
// element r * C, which is no multiple of four when C is not, so every span of
// columns (a row, or a segment of one) is cut into a scalar HEAD of 0..3
// elements up to the next multiple of four of the element index, a BODY of
// aligned vectors, and a scalar TAIL of 0..3. Head and tail elements are
// taken by lanes 0..2 and 32..34 of the span's first wave, one scalar each.
// Nothing outside [r * C, (r + 1) * C) is ever addressed.
//
// Segmentation (cei_plan) is a function of (B, C) alone, never of a device
// query: the launch recorded into a graph is the eager launch and the
// workspace has a size known from the shape (kLnGridCap's argument).
//   C <= kCeiRowMaxC:  S = 1, the ROW kernels: one wave owns one row, held in
//     registers as NV vectors per lane, four rows per 256-thread workgroup,
//     min(kCeiGridCap, ceil(B / 4)) workgroups whose waves stride the rows.
//   above:  the SEGMENT kernels: a 256-thread workgroup owns one contiguous
//     segment of L columns of one row, grid B * S.
//       S = min(ceil(kCeiTargetGrid / B), max(1, C / kCeiMinSeg)),
//       L = ceil(C / S) rounded up to a multiple of 4, S = ceil(C / L):
//     a row is split when B alone gives too few workgroups for 256 CUs, but
//     never into segments shorter than kCeiMinSeg columns. (32, 21843) runs
//     on 320 workgroups of 2188 columns (the last 2151).
//
// k_cei_fwd_row: max over the registers first, then sum exp(y - m): no
//   rescale. k_cei_fwd_seg streams its segment in chunks of kCeiChunk vectors
//   per lane with a running (m, l) per lane; l is rescaled by ONE exp2 per
//   chunk, not per element. Lanes merge in a ds_bpermute butterfly, the four
//   waves through LDS in wave order. Both store one record per span:
//     [0] m            the span's maximum
//     [1] l            sum exp(y - m)
//     [2] sum (y - m)  for the smoothing term (see below)
//     [3] y[t] - m     if the label's column lies in the span, else 0;
//                      one lane, one guarded load
//   The third word is sum (y - m) and not sum y: with logits of 1000 + noise
//   the plain sum of C = 1000 of them is 1e6 with an ulp of 0.06, and the
//   smoothing term log L + M - sum_y / C would lose four digits. The streamed
//   kernel sums y - r against a reference r that cannot move while it
//   streams (the segment's first element, 0 if that is not finite) and
//   rebases once at the end: sum (y - m) = sum (y - r) + n (r - m).
//
// k_cei_finish: one workgroup; threads stride the rows. Each merges its
//   row's S records in segment order, M = max m_s,
//   L = sum l_s exp2((m_s - M) log2e), forms
//     nll    = log L - (y_t - M)           (the maximum is taken out BEFORE
//     smooth = log L - sum (y - M) / C      the subtraction: k_ce_fwd's rule)
//     loss   = (1 - eps) nll + eps smooth
//   stores row_stats and, for "none", the row loss; then the loss sum and the
//   non-ignored count are reduced in a fixed order (a thread's rows in row
//   order, a butterfly, four waves through LDS in wave order): no atomics,
//   nothing pre-zeroed, the same bits run to run.
//
// k_cei_bwd_row / k_cei_bwd_seg: one read of the logits, one store:
//     p = exp2((y - M) log2e) (1/L),
//     dy = (p - eps/C - (1 - eps) [c == t]) g,   g = incoming grad * inv_count
//   with g read on the device. Ignored rows store zeros without reading.
//
// Labels. A label equal to ignore_index drops the row: loss 0, gradient 0,
// not counted by "mean". Any other label outside [0, C) is INVALID: it is
// never used as an address; the row's loss and its dlogits row are NaN, the
// row counts as non-ignored, other rows are untouched. (torch asserts on the
// device instead.) Nothing is read back to the host, so the call can be
// captured into a graph.
#include <cmath>
#include <limits>

#include "kernel_common.h"
#include "ops.h"

// No packed-fp32 VALU forms (v_pk_*_f32) in this file's device code.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace mi355x {

namespace {

constexpr int kCeiRowMaxC = 2048;     // widest register-resident row
constexpr int kCeiGridCap = 512;      // row kernels: workgroups
constexpr int kCeiTargetGrid = 1024;  // segment kernels: four per CU
constexpr int kCeiMinSeg = 2048;      // columns; no shorter segment is cut
constexpr int kCeiChunk = 4;          // vectors per lane and rescale
constexpr int64_t kCeiMaxC = int64_t(1) << 30;
constexpr float kLog2e = 1.4426950408889634f;

enum Reduction : int { kMean = 0, kSum = 1, kNone = 2 };

// clang vector types and builtins only: a function of the HIP headers does
// not carry this file's target attribute and would stay a CALL (see
// layernorm_kernels.hip).
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
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const __hip_bfloat16* p) {
  return as_f32((uint32_t)*reinterpret_cast<const uint16_t*>(p) << 16);
}
// Two floats to two bf16, round to nearest even (v_cvt_pk_bf16_f32).
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
  const bf16x2 p = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, p);
}
__device__ __forceinline__ void st4(float* p, const float v[4]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ void st4(__hip_bfloat16* p, const float v[4]) {
  *reinterpret_cast<u32x2*>(p) =
      u32x2{bf16_pack(v[0], v[1]), bf16_pack(v[2], v[3])};
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(__hip_bfloat16* p, float v) {
  *reinterpret_cast<uint16_t*>(p) = (uint16_t)bf16_pack(v, 0.f);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ float ex2(float x) {
  return __builtin_amdgcn_exp2f(x);
}
// A maximum to subtract: 0 in place of -inf (a span of -inf logits), so that
// y - m is -inf and not NaN there.
__device__ __forceinline__ float finite_max(float m) {
  return m == -__builtin_inff() ? 0.f : m;
}
__device__ __forceinline__ float max4(float m, const float v[4]) {
  return __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fmaxf(v[0], v[1])),
                         __builtin_fmaxf(v[2], v[3]));
}

// v of lane (lane ^ off): one ds_bpermute_b32.
__device__ __forceinline__ float xor_lane(float v, int lane, int off) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ off) << 2,
                                          __builtin_bit_cast(int, v)));
}
// Butterflies over the 64 lanes; every lane ends with the same bits.
__device__ __forceinline__ float lane_max(float a, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    a = __builtin_fmaxf(a, xor_lane(a, lane, off));
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

__device__ __forceinline__ int64_t label_at(const void* labels, int label64,
                                            int64_t row) {
  return label64 ? static_cast<const int64_t*>(labels)[row]
                 : (int64_t) static_cast<const int32_t*>(labels)[row];
}

// A span of `len` columns that begins at element index `first` of a 16-byte
// aligned tensor: h head scalars, nvec aligned vectors, tail scalars.
struct Span {
  int h, nvec, tail;
};
__device__ __forceinline__ Span span_of(int64_t first, int len) {
  Span s;
  s.h = (int)((4 - (first & 3)) & 3);
  if (s.h > len) s.h = len;
  s.nvec = (len - s.h) >> 2;
  s.tail = len - s.h - 4 * s.nvec;
  return s;
}
// The head or tail column (relative to the span) that thread `tid` of the
// span's first wave takes, or -1.
__device__ __forceinline__ int edge_col(const Span& s, int tid) {
  if (tid < s.h) return tid;
  if (tid >= 32 && tid < 32 + s.tail) return s.h + 4 * s.nvec + (tid - 32);
  return -1;
}

// The record's fourth word: y[t] - m when column t is in [c0, c0 + len).
template <typename T>
__device__ __forceinline__ float target_logit(const T* span, int64_t t,
                                              int64_t ignore, int c0, int len,
                                              float m) {
  if (t == ignore || t < c0 || t >= (int64_t)c0 + len) return 0.f;
  return ld1(span + (t - c0)) - finite_max(m);
}

template <typename T, int NV>
__global__ __launch_bounds__(256) void k_cei_fwd_row(
    const T* __restrict__ y, const void* __restrict__ labels, int label64,
    f32x4* __restrict__ ws, int64_t B, int C, int64_t ignore) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < B;
       row += (int64_t)gridDim.x * 4) {
    const T* p = y + row * C;
    const Span sp = span_of(row * C, C);
    const T* body = p + sp.h;
    const int ec = edge_col(sp, lane);
    float d[NV][4];
    float e = 0.f, m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = lane + 64 * j;
      if (v < sp.nvec) {
        ld4(body + 4 * v, d[j]);
        m = max4(m, d[j]);
      }
    }
    if (ec >= 0) {
      e = ld1(p + ec);
      m = __builtin_fmaxf(m, e);
    }
    m = lane_max(m, lane);
    const float ms = finite_max(m);
    float l = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (lane + 64 * j < sp.nvec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float c = d[j][i] - ms;
          l += ex2(c * kLog2e);
          sy += c;
        }
      }
    }
    if (ec >= 0) {
      l += ex2((e - ms) * kLog2e);
      sy += e - ms;
    }
    lane_sum2(l, sy, lane);
    if (lane == 0) {
      const int64_t t = label_at(labels, label64, row);
      ws[row] = f32x4{m, l, sy, target_logit(p, t, ignore, 0, C, m)};
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_cei_fwd_seg(
    const T* __restrict__ y, const void* __restrict__ labels, int label64,
    f32x4* __restrict__ ws, int C, int S, int L, int64_t ignore) {
  __shared__ float part[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x / S;
  const int seg = (int)(blockIdx.x - row * S);
  const int c0 = seg * L, len = imin(L, C - c0);
  const T* p = y + row * C + c0;
  const Span sp = span_of(row * C + c0, len);
  const T* body = p + sp.h;
  const float r0 = ld1(p);  // the reference of this segment's sum (y - r)
  const float r = __builtin_fabsf(r0) < __builtin_inff() ? r0 : 0.f;
  float m = -__builtin_inff(), l = 0.f, sy = 0.f;
  for (int v0 = tid; v0 < sp.nvec; v0 += 256 * kCeiChunk) {
    float d[kCeiChunk][4];
    float cm = m;
#pragma unroll
    for (int k = 0; k < kCeiChunk; ++k) {
      const int v = v0 + 256 * k;
      if (v < sp.nvec) {
        ld4(body + 4 * v, d[k]);
        cm = max4(cm, d[k]);
      }
    }
    // one rescale per chunk; from m = -inf the factor is exp2(-inf) = 0
    const float ms = finite_max(cm);
    l *= ex2((m - ms) * kLog2e);
    m = cm;
#pragma unroll
    for (int k = 0; k < kCeiChunk; ++k) {
      if (v0 + 256 * k < sp.nvec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          l += ex2((d[k][i] - ms) * kLog2e);
          sy += d[k][i] - r;
        }
      }
    }
  }
  const int ec = edge_col(sp, tid);
  if (ec >= 0) {
    const float e = ld1(p + ec);
    const float cm = __builtin_fmaxf(m, e), ms = finite_max(cm);
    l = l * ex2((m - ms) * kLog2e) + ex2((e - ms) * kLog2e);
    sy += e - r;
    m = cm;
  }
  // lanes -> wave
  const float mw = lane_max(m, lane);
  l *= ex2((m - finite_max(mw)) * kLog2e);
  lane_sum2(l, sy, lane);
  if (lane == 0) part[wave][0] = mw, part[wave][1] = l, part[wave][2] = sy;
  block_sync();
  if (tid == 0) {  // waves -> segment, in wave order
    float M = part[0][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = __builtin_fmaxf(M, part[w][0]);
    const float Ms = finite_max(M);
    float Lsum = 0.f, SY = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      Lsum += part[w][1] * ex2((part[w][0] - Ms) * kLog2e);
      SY += part[w][2];
    }
    SY = __builtin_fmaf((float)len, r - Ms, SY);  // sum (y - r) -> sum (y - m)
    const int64_t t = label_at(labels, label64, row);
    ws[blockIdx.x] = f32x4{M, Lsum, SY, target_logit(p, t, ignore, c0, len, M)};
  }
}

__global__ __launch_bounds__(256) void k_cei_finish(
    const f32x4* __restrict__ ws, const void* __restrict__ labels, int label64,
    f32x2* __restrict__ stats, float* __restrict__ out,
    float* __restrict__ inv_count, int64_t B, int C, int S, int L,
    int64_t ignore, float eps, int reduction) {
  __shared__ float wsum[4];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_c = 1.f / (float)C;
  float sum = 0.f;
  int cnt = 0;
  for (int64_t row = tid; row < B; row += 256) {
    const f32x4* rec = ws + row * S;
    float M = rec[0][0];
    for (int s = 1; s < S; ++s) M = __builtin_fmaxf(M, rec[s][0]);
    const float Ms = finite_max(M);
    float Lsum = 0.f, SY = 0.f;
    for (int s = 0; s < S; ++s) {
      const f32x4 w = rec[s];
      const float ms = finite_max(w[0]);
      const int n = imin(L, C - s * L);
      Lsum += w[1] * ex2((w[0] - Ms) * kLog2e);
      // sum (y - m_s) -> sum (y - M)
      SY += __builtin_fmaf((float)n, ms - Ms, w[2]);
    }
    stats[row] = f32x2{Ms, 1.f / Lsum};
    const int64_t t = label_at(labels, label64, row);
    float loss = 0.f;
    if (t != ignore) {
      ++cnt;
      if (t < 0 || t >= C) {
        loss = __builtin_nanf("");
      } else {
        const f32x4 wt = rec[(int)(t / L)];
        const float yt = wt[3] + (finite_max(wt[0]) - Ms);  // y_t - M
        const float logl = __builtin_logf(Lsum);
        const float nll = logl - yt;
        loss = eps > 0.f ? (1.f - eps) * nll + eps * (logl - SY * inv_c) : nll;
      }
      sum += loss;
    }
    if (reduction == kNone) out[row] = loss;
  }
  // threads -> wave -> workgroup, in a fixed order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += xor_lane(sum, lane, off);
    cnt += __builtin_amdgcn_ds_bpermute((lane ^ off) << 2, cnt);
  }
  if (lane == 0) wsum[wave] = sum, wcnt[wave] = cnt;
  block_sync();
  if (tid == 0) {
    const float total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const float count = (float)(((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3]);
    if (reduction == kMean) out[0] = total / count;  // 0 / 0: NaN, as torch
    if (reduction == kSum) out[0] = total;
    inv_count[0] = reduction == kMean ? 1.f / count : 1.f;
  }
}

// What the backward knows of one row.
struct RowGrad {
  float M, rl, g;  // row maximum, 1/L, incoming gradient * inv_count
  int64_t t;       // the label's column, or -1
  bool ignored;
};
__device__ __forceinline__ RowGrad row_grad(
    const f32x2* stats, const void* labels, int label64, const float* gin,
    int per_row, const float* inv_count, int64_t row, int C, int64_t ignore) {
  RowGrad rg;
  const int64_t t = label_at(labels, label64, row);
  rg.ignored = t == ignore;
  rg.t = -1;
  if (rg.ignored) {
    rg.M = rg.rl = rg.g = 0.f;
    return rg;
  }
  const f32x2 st = stats[row];
  rg.M = st[0], rg.rl = st[1];
  rg.g = inv_count[0];
  if (gin) rg.g *= gin[per_row ? row : 0];
  if (t < 0 || t >= C) rg.g = __builtin_nanf("");  // invalid: a NaN row
  else rg.t = t;
  return rg;
}

// dlogits over one span by the `nthreads` threads of a wave or a workgroup;
// tl is the label's column relative to the span (any value outside it: none).
template <typename T>
__device__ __forceinline__ void cei_bwd_span(
    const T* __restrict__ p, T* __restrict__ dp, const Span& sp,
    const RowGrad& rg, int64_t tl, float a, float b, int tid, int nthreads) {
  const T* body = p + sp.h;
  T* dbody = dp + sp.h;
  const int ec = edge_col(sp, tid);
  if (rg.ignored) {
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = tid; v < sp.nvec; v += nthreads) st4(dbody + 4 * v, z);
    if (ec >= 0) st1(dp + ec, 0.f);
    return;
  }
  const int tb = (int)(tl - sp.h);  // relative to the body
  for (int v = tid; v < sp.nvec; v += nthreads) {
    float d[4], o[4];
    ld4(body + 4 * v, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float pr = ex2((d[i] - rg.M) * kLog2e) * rg.rl;
      o[i] = ((pr - a) - (4 * v + i == tb ? b : 0.f)) * rg.g;
    }
    st4(dbody + 4 * v, o);
  }
  if (ec >= 0) {
    const float pr = ex2((ld1(p + ec) - rg.M) * kLog2e) * rg.rl;
    st1(dp + ec, ((pr - a) - (ec == tl ? b : 0.f)) * rg.g);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_cei_bwd_row(
    const T* __restrict__ y, const void* __restrict__ labels, int label64,
    const f32x2* __restrict__ stats, const float* __restrict__ gin,
    int per_row, const float* __restrict__ inv_count, T* __restrict__ dy,
    int64_t B, int C, int64_t ignore, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float a = eps / (float)C, b = 1.f - eps;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < B;
       row += (int64_t)gridDim.x * 4) {
    const RowGrad rg = row_grad(stats, labels, label64, gin, per_row,
                                inv_count, row, C, ignore);
    cei_bwd_span(y + row * C, dy + row * C, span_of(row * C, C), rg, rg.t, a,
                 b, lane, 64);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_cei_bwd_seg(
    const T* __restrict__ y, const void* __restrict__ labels, int label64,
    const f32x2* __restrict__ stats, const float* __restrict__ gin,
    int per_row, const float* __restrict__ inv_count, T* __restrict__ dy,
    int C, int S, int L, int64_t ignore, float eps) {
  const int64_t row = blockIdx.x / S;
  const int seg = (int)(blockIdx.x - row * S);
  const int c0 = seg * L, len = imin(L, C - c0);
  const float a = eps / (float)C, b = 1.f - eps;
  const RowGrad rg = row_grad(stats, labels, label64, gin, per_row, inv_count,
                              row, C, ignore);
  const int64_t first = row * C + c0;
  cei_bwd_span(y + first, dy + first, span_of(first, len), rg,
               rg.t < 0 ? (int64_t)-1 : rg.t - c0, a, b, (int)threadIdx.x, 256);
}

struct CeiPlan {
  int S, L;  // segments per row, columns per segment (the last may be shorter)
};
CeiPlan cei_plan_of(int64_t B, int64_t C) {
  if (C <= kCeiRowMaxC) return {1, (int)C};
  int64_t S = std::min<int64_t>((kCeiTargetGrid + std::max<int64_t>(B, 1) - 1) /
                                    std::max<int64_t>(B, 1),
                                std::max<int64_t>(1, C / kCeiMinSeg));
  const int64_t L = ((C + S - 1) / S + 3) / 4 * 4;
  return {(int)((C + L - 1) / L), (int)L};
}

struct CeiDims {
  int64_t B, C;
  int reduction;
  bool label64;
  CeiPlan plan;
};

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// The argument check shared by cei_fwd and cei_bwd, complete before any launch.
CeiDims cei_check_args(const char* who, const torch::Tensor& logits,
                       const torch::Tensor& labels, double label_smoothing,
                       const std::string& reduction) {
  TORCH_CHECK(logits.defined() && logits.is_cuda(), who,
              ": logits must be on a GPU");
  const auto dt = logits.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": logits must be f32 or bf16, got ", dt);
  TORCH_CHECK(logits.dim() >= 1 && logits.is_contiguous() && aligned16(logits),
              who, ": logits must be [..., C], contiguous and 16-byte aligned");
  const int64_t C = logits.size(-1);
  TORCH_CHECK(C >= 1 && C <= kCeiMaxC, who, ": C must be in [1, 2^30], got ",
              C);
  TORCH_CHECK(labels.defined() && labels.device() == logits.device(), who,
              ": labels must be on the logits' device");
  const auto lt = labels.scalar_type();
  TORCH_CHECK(lt == at::kLong || lt == at::kInt, who,
              ": labels must be int64 or int32, got ", lt);
  TORCH_CHECK(labels.sizes() == logits.sizes().slice(0, logits.dim() - 1) &&
                  labels.is_contiguous(),
              who, ": labels must be contiguous with the logits' leading "
              "shape, got ", labels.sizes(), " for logits ", logits.sizes());
  TORCH_CHECK(label_smoothing >= 0.0 && label_smoothing <= 1.0, who,
              ": label_smoothing must be in [0, 1], got ", label_smoothing);
  int red;
  if (reduction == "mean") red = kMean;
  else if (reduction == "sum") red = kSum;
  else if (reduction == "none") red = kNone;
  else TORCH_CHECK(false, who, ": reduction must be 'mean', 'sum' or 'none', "
                   "got '", reduction, "'");
  const int64_t B = logits.numel() / C;
  const CeiPlan plan = cei_plan_of(B, C);
  TORCH_CHECK(B * plan.S < (int64_t(1) << 31), who, ": too many rows");
  return {B, C, red, lt == at::kLong, plan};
}

// A caller's preallocated f32 or logits-typed buffer, checked, or a fresh one.
torch::Tensor cei_result(const char* who, const char* name,
                         const c10::optional<torch::Tensor>& given,
                         at::IntArrayRef shape, at::TensorOptions opts) {
  if (!given.has_value()) return torch::empty(shape, opts);
  TORCH_CHECK(given->device() == opts.device() &&
                  given->scalar_type() ==
                      c10::typeMetaToScalarType(opts.dtype()) &&
                  given->is_contiguous() && given->sizes() == shape &&
                  aligned16(*given),
              who, ": ", name, " must be contiguous, 16-byte aligned, ",
              opts.dtype(), " ", shape, " on the logits' device");
  return *given;
}

int cei_row_grid(int64_t B) {
  return (int)std::min<int64_t>(kCeiGridCap, (B + 3) / 4);
}

// f(NV) as an integral constant, NV the smallest of 1, 2, 4, 8 with
// 256 * NV >= C.
template <typename F>
void with_cei_nv(int64_t C, F&& f) {
  if (C <= 256) f(std::integral_constant<int, 1>{});
  else if (C <= 512) f(std::integral_constant<int, 2>{});
  else if (C <= 1024) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}

}  // namespace

std::vector<int64_t> cei_plan(int64_t B, int64_t C) {
  TORCH_CHECK(B >= 0 && C >= 1 && C <= kCeiMaxC, "cei_plan: bad shape");
  const CeiPlan p = cei_plan_of(B, C);
  return {p.S, p.L};
}

int64_t cei_grid_cap() { return kCeiGridCap; }

std::vector<torch::Tensor> cei_fwd(torch::Tensor logits, torch::Tensor labels,
                                   double label_smoothing,
                                   int64_t ignore_index,
                                   const std::string& reduction,
                                   c10::optional<torch::Tensor> row_stats_,
                                   c10::optional<torch::Tensor> workspace_) {
  const char* who = "cei_fwd";
  const CeiDims d =
      cei_check_args(who, logits, labels, label_smoothing, reduction);
  const auto f32 = logits.options().dtype(at::kFloat);
  const int S = d.plan.S, L = d.plan.L;
  auto stats = cei_result(who, "row_stats", row_stats_, {d.B, 2}, f32);
  auto ws = cei_result(who, "workspace", workspace_, {d.B, S, 4}, f32);
  if (d.B == 0) {  // torch: the mean over nothing is NaN, the sum 0
    auto loss = d.reduction == kNone ? torch::empty(labels.sizes(), f32)
                : d.reduction == kSum
                    ? torch::zeros({}, f32)
                    : torch::full({}, std::numeric_limits<float>::quiet_NaN(),
                                  f32);
    return {loss, stats, torch::ones({1}, f32)};
  }
  auto loss = torch::empty(
      d.reduction == kNone ? labels.sizes() : at::IntArrayRef{}, f32);
  auto inv_count = torch::empty({1}, f32);
  const void* lab = labels.data_ptr();
  DISPATCH_F32_BF16(logits.scalar_type(), who, {
    if (d.C <= kCeiRowMaxC) {
      with_cei_nv(d.C, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL((k_cei_fwd_row<scalar_t, NV>),
                           dim3(cei_row_grid(d.B)), dim3(256), 0, cur_stream(),
                           cdptr<scalar_t>(logits), lab, (int)d.label64,
                           dptr<f32x4>(ws), d.B, (int)d.C, ignore_index);
      });
    } else {
      hipLaunchKernelGGL((k_cei_fwd_seg<scalar_t>), dim3((unsigned)(d.B * S)),
                         dim3(256), 0, cur_stream(), cdptr<scalar_t>(logits),
                         lab, (int)d.label64, dptr<f32x4>(ws), (int)d.C, S, L,
                         ignore_index);
    }
  });
  hipLaunchKernelGGL(k_cei_finish, dim3(1), dim3(256), 0, cur_stream(),
                     cdptr<f32x4>(ws), lab, (int)d.label64, dptr<f32x2>(stats),
                     dptr<float>(loss), dptr<float>(inv_count), d.B, (int)d.C,
                     S, L, ignore_index, (float)label_smoothing, d.reduction);
  HIP_OK(hipGetLastError());
  return {loss, stats, inv_count};
}

torch::Tensor cei_bwd(c10::optional<torch::Tensor> grad, torch::Tensor logits,
                      torch::Tensor labels, torch::Tensor row_stats,
                      torch::Tensor inv_count, double label_smoothing,
                      int64_t ignore_index, const std::string& reduction,
                      c10::optional<torch::Tensor> dlogits_) {
  const char* who = "cei_bwd";
  const CeiDims d =
      cei_check_args(who, logits, labels, label_smoothing, reduction);
  const auto f32 = logits.options().dtype(at::kFloat);
  auto f32_on_device = [&](const torch::Tensor& t, int64_t numel) {
    return t.defined() && t.device() == logits.device() &&
           t.scalar_type() == at::kFloat && t.is_contiguous() &&
           t.numel() == numel;
  };
  TORCH_CHECK(f32_on_device(row_stats, 2 * d.B) && row_stats.dim() == 2 &&
                  row_stats.size(1) == 2,
              who, ": row_stats must be cei_fwd's f32 [B, 2] = [", d.B,
              ", 2] on the logits' device");
  TORCH_CHECK(f32_on_device(inv_count, 1), who,
              ": inv_count must be cei_fwd's f32 [1] on the logits' device");
  const bool per_row = d.reduction == kNone;
  if (grad.has_value())
    TORCH_CHECK(f32_on_device(*grad, per_row ? d.B : 1), who,
                ": grad must be a contiguous f32 device tensor with ",
                per_row ? "one value per row" : "one value");
  auto dy = cei_result(who, "dlogits", dlogits_, logits.sizes(),
                       logits.options());
  if (d.B == 0) return dy;
  const float* gin = grad.has_value() ? cdptr<float>(*grad) : nullptr;
  const void* lab = labels.data_ptr();
  DISPATCH_F32_BF16(logits.scalar_type(), who, {
    if (d.C <= kCeiRowMaxC) {
      hipLaunchKernelGGL((k_cei_bwd_row<scalar_t>), dim3(cei_row_grid(d.B)),
                         dim3(256), 0, cur_stream(), cdptr<scalar_t>(logits),
                         lab, (int)d.label64, cdptr<f32x2>(row_stats), gin,
                         (int)per_row, cdptr<float>(inv_count),
                         dptr<scalar_t>(dy), d.B, (int)d.C, ignore_index,
                         (float)label_smoothing);
    } else {
      hipLaunchKernelGGL((k_cei_bwd_seg<scalar_t>),
                         dim3((unsigned)(d.B * d.plan.S)), dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(logits), lab,
                         (int)d.label64, cdptr<f32x2>(row_stats), gin,
                         (int)per_row, cdptr<float>(inv_count),
                         dptr<scalar_t>(dy), (int)d.C, d.plan.S, d.plan.L,
                         ignore_index, (float)label_smoothing);
    }
  });
  HIP_OK(hipGetLastError());
  return dy;
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
