// Fused BatchNorm (+ residual add) (+ ReLU) for gfx950 (MI355X), forward and
// backward, over the rows of a channels-last activation.
//
//   x, residual, z, dz, dx, dresidual  [R, C]  R = N*H*W pixels, C channels
//                                              contiguous, storage T (f32|bf16)
//   weight, bias, running_mean/var,
//   dgamma, dbeta                      [C]     f32
//   col_stats                          [2, C]  f32 (mean row, rstd row)
//   workspace                          [GR, 3, C] f32 forward, [GR, 2, C]
//                                              backward
//
// C % 4 == 0, 4 <= C <= 4096. All arithmetic is f32, all indices int64.
//
// Work split. The reduction runs over the ROWS, for every column: LayerNorm's
// split turned by 90 degrees. A lane holds one vector of four adjacent
// channels (16 bytes f32, 8 bytes bf16). A 256-thread workgroup is LC lanes
// along the channels by LR = 256 / LC lanes along the rows, LC the smallest
// power of two >= min(C/4, 64); vector lanes at or past C/4 are masked (not
// loaded, not stored, zero in every sum). At C = 64 a wave reads four whole
// rows, 1 KB contiguous; at C >= 256 it reads 256 adjacent channels of one
// row. The workgroup owns a slab of 4*LC columns and walks chunks of
// kBnBlocks = 4 blocks of LR rows, all four loads issued before the first is
// used; loads are branch-free (row clamped to R - 1, the use masked).
//
// Plan. bn_plan(R, C) = (LC, slabs, GR): slabs = ceil(C / (4 LC)) column
// slabs, GR = min(ceil(R / (4 LR)), max(1, kBnTargetGrid / slabs)) workgroups
// along the rows, the grid slabs * GR; workgroup (slab, g) takes chunks g,
// g + GR, ... It is a function of the shape alone, never of a device query, so
// the captured launch is the eager launch and the workspace size is known
// from the shape.
//
// Forward, training: three launches.
//   k_bn_stats   reads x once. A thread keeps (n, mean[4], M2[4]) and updates
//     it row by row (Welford; 1/n once per row for the four columns), never
//     E[x^2] - mean^2. The values it sees are x - K with K = x[0, column], one
//     shift for the whole column: Welford's M2 carries the rounding of its
//     running mean to first order, so that mean has to be of the size of the
//     spread, not of the offset (a column of 1000 + noise keeps its digits).
//     M2 does not depend on the shift. The column's mean itself comes from a
//     plain sum of the unshifted x kept beside the record: adding K back to
//     the shifted mean would cost digits where the mean is small against the
//     spread. The LR row lanes are merged with the pairwise (Chan)
//     formula in a fixed order: a shift-down tree over the lanes of a wave
//     that share a column vector, then waves 1..3 through LDS into wave 0 in
//     wave order. A record with n = 0 merges as the identity. The workgroup
//     stores (sum, shifted mean, M2) into its slice of the workspace; the
//     counts follow
//     from the shape. Every slice is stored whole: nothing pre-zeroed, no
//     atomics.
//   k_bn_finish  16 waves own 64 adjacent columns; wave w merges slices w,
//     w + 16, ... in order, the waves meet in LDS in wave order. It stores
//     col_stats = (sum/R, 1/sqrt(M2/R + eps)), updates the running statistics
//     in place (unbiased M2/(R-1)) and increments num_batches_tracked.
//   k_bn_apply   reads x again (and the residual), forms (x - mean) * rstd *
//     gamma + beta (+ residual) in f32, applies ReLU, rounds once.
// Forward, evaluation: k_bn_apply alone, from the running statistics.
//
// Backward: three launches. g = dz * (z > 0), the mask read from the saved
// OUTPUT; xhat = (x - mean) * rstd.
//   k_bn_bwd_reduce  the statistics kernel's walk; sum g and sum g * xhat per
//     column, merged in the same fixed order into the workspace.
//   k_bn_finish<false>  sums the slices in order into dbeta and dgamma.
//   k_bn_bwd_apply   dx = gamma * rstd * (g - dbeta/R - xhat * dgamma/R) and,
//     with ADD, dresidual = g.
// col_stats, the running statistics, dgamma and dbeta are the same bits run
// to run.
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

constexpr int kBnTargetGrid = 1024;  // workgroups, before rounding by slabs
constexpr int kBnMaxC = 4096;
constexpr int kBnBlocks = 4;         // row blocks in flight per thread
constexpr int kFinishWaves = 16;     // k_bn_finish: waves per workgroup

// clang vector types and builtins only: a function of the HIP headers does
// not carry this file's target attribute and would stay a CALL.
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
// v of lane (lane + off) mod 64: one ds_bpermute_b32.
__device__ __forceinline__ float down_lane(float v, int lane, int off) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(((lane + off) & 63) << 2,
                                          __builtin_bit_cast(int, v)));
}
// __syncthreads, spelled out.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Where a thread stands in the plan.
struct BnLane {
  int LR, lr, g, vec;  // row lanes, this row lane, row group, column vector
  bool live;           // vec < C / 4
};
__device__ __forceinline__ BnLane bn_lane(int C, int lcs, int slabs) {
  BnLane l;
  const int LC = 1 << lcs;
  l.LR = 256 >> lcs;
  l.lr = threadIdx.x >> lcs;
  l.g = blockIdx.x / slabs;
  l.vec = (blockIdx.x % slabs) * LC + (threadIdx.x & (LC - 1));
  l.live = l.vec < (C >> 2);
  return l;
}

// (ma, qa) <- mean and M2 of both sets (Chan et al.), from the count na of the
// first set and w = chan_weight(na, nb); the caller adds the counts. An empty
// side (n = 0, mean = 0, M2 = 0) is the identity, two empty sides give the
// empty record, and equal means stay that mean exactly.
__device__ __forceinline__ void chan_merge(float na, float& ma, float& qa,
                                           float mb, float qb, float w) {
  const float d = mb - ma;
  ma = fmaf(d, w, ma);
  qa = (qa + qb) + (d * d) * (na * w);
}
__device__ __forceinline__ float chan_weight(float na, float nb) {
  const float n = na + nb;
  return n > 0.f ? nb / n : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bn_stats(
    const T* __restrict__ x, float* __restrict__ ws, int64_t R, int C, int lcs,
    int slabs, int GR) {
  __shared__ float hand[3][13][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const BnLane l = bn_lane(C, lcs, slabs);
  const T* xc = x + 4 * (l.live ? l.vec : 0);
  const int64_t Rl = l.live ? R : 0;
  float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
  float shift[4], sum[4] = {0.f, 0.f, 0.f, 0.f};
  ld4(xc, shift);  // row 0 of the thread's columns
  for (int64_t r0 = (int64_t)l.g * kBnBlocks * l.LR + l.lr; r0 < Rl;
       r0 += (int64_t)GR * kBnBlocks * l.LR) {
    float v[kBnBlocks][4];
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      ld4(xc + (row < R ? row : R - 1) * C, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const bool ok = r0 + (int64_t)u * l.LR < R;
      n += ok ? 1.f : 0.f;
      const float inv = ok ? 1.f / n : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = v[u][i] - shift[i];
        const float d = ok ? s - mean[i] : 0.f;
        sum[i] += ok ? v[u][i] : 0.f;
        mean[i] = fmaf(d, inv, mean[i]);
        m2[i] = fmaf(d, s - mean[i], m2[i]);
      }
    }
  }
  // row lanes of this wave that share the column vector: shift-down tree
  for (int off = 32; off >> lcs; off >>= 1) {
    const float nb = down_lane(n, lane, off), w = chan_weight(n, nb);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      chan_merge(n, mean[i], m2[i], down_lane(mean[i], lane, off),
                 down_lane(m2[i], lane, off), w);
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += down_lane(sum[i], lane, off);
    n += nb;
  }
  // waves 1..3 -> LDS -> wave 0, merged in wave order
  const bool head = (lane >> lcs) == 0 || lcs == 6;
  if (wave > 0 && head) {
    hand[wave - 1][0][lane] = n;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hand[wave - 1][1 + i][lane] = mean[i], hand[wave - 1][5 + i][lane] = m2[i],
                                 hand[wave - 1][9 + i][lane] = sum[i];
  }
  block_sync();
  if (wave == 0 && head && l.live) {
#pragma unroll
    for (int w3 = 0; w3 < 3; ++w3) {
      const float nb = hand[w3][0][lane], w = chan_weight(n, nb);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        chan_merge(n, mean[i], m2[i], hand[w3][1 + i][lane],
                   hand[w3][5 + i][lane], w);
#pragma unroll
      for (int i = 0; i < 4; ++i) sum[i] += hand[w3][9 + i][lane];
      n += nb;
    }
    float* slice = ws + (int64_t)l.g * 3 * C + 4 * l.vec;
    st4(slice, sum);
    st4(slice + C, mean);
    st4(slice + 2 * C, m2);
  }
}

// Rows that workgroup row-group k of GR walks: its chunks k, k + GR, ... of
// `chunk` rows, the last chunk of all ragged.
__device__ __forceinline__ float bn_rows_of(int64_t k, int64_t R, int64_t chunk,
                                            int64_t GR) {
  const int64_t chunks = (R + chunk - 1) / chunk;
  int64_t rows = (chunks - k + GR - 1) / GR * chunk;
  if ((chunks - 1) % GR == k) rows -= chunks * chunk - R;
  return (float)rows;
}

// workspace [GR, 3 or 2, C] -> per-column results. 16 waves x 64 columns per
// workgroup; wave w takes slices w, w + 16, ... in order, wave 0 then takes
// the 16 partial results in wave order.
// FWD:  rows are (sum x, mean of x - x[0, column], M2): the sums are added,
//       the records merged by Chan's formula with the counts of the plan;
//       out0/out1 = col_stats' mean and rstd rows, the running statistics and
//       the batch counter are updated in place.
// !FWD: rows are (sum g, sum g * xhat), added; out0/out1 = dbeta, dgamma.
template <bool FWD>
__global__ __launch_bounds__(kFinishWaves * 64) void k_bn_finish(
    const float* __restrict__ ws, int GR, int C, int64_t R, int chunk,
    float* __restrict__ out0, float* __restrict__ out1,
    float* __restrict__ run_mean, float* __restrict__ run_var,
    int64_t* __restrict__ batches, float momentum, float eps) {
  __shared__ float part[kFinishWaves][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  float n = 0.f, a = 0.f, b = 0.f, sum = 0.f;
  if (col < C) {
#pragma unroll 4
    for (int k = wave; k < GR; k += kFinishWaves) {
      const float* p = ws + (int64_t)k * (FWD ? 3 : 2) * C + col;
      if (FWD) {
        const float nb = bn_rows_of(k, R, chunk, GR), w = chan_weight(n, nb);
        chan_merge(n, a, b, p[C], p[2 * C], w);
        n += nb, sum += p[0];
      } else {
        a += p[0], b += p[C];
      }
    }
  }
  part[wave][0][lane] = n, part[wave][1][lane] = a, part[wave][2][lane] = b;
  part[wave][3][lane] = sum;
  block_sync();
  if (wave != 0 || col >= C) return;
#pragma unroll
  for (int w16 = 1; w16 < kFinishWaves; ++w16) {
    if (FWD) {
      const float nb = part[w16][0][lane], w = chan_weight(n, nb);
      chan_merge(n, a, b, part[w16][1][lane], part[w16][2][lane], w);
      n += nb, sum += part[w16][3][lane];
    } else {
      a += part[w16][1][lane], b += part[w16][2][lane];
    }
  }
  if (FWD) {
    const float rows = (float)R;
    a = sum / rows;
    out0[col] = a;
    out1[col] = 1.f / sqrtf(b / rows + eps);
    run_mean[col] = fmaf(momentum, a, (1.f - momentum) * run_mean[col]);
    run_var[col] =
        fmaf(momentum, b / (rows - 1.f), (1.f - momentum) * run_var[col]);
    if (batches != nullptr && col == 0) *batches += 1;
  } else {
    out0[col] = a;
    out1[col] = b;
  }
}

// z = act((x - mean) * rstd * gamma + beta (+ residual)). `second` is the
// rstd row of col_stats, or (second_is_var) the running variance.
template <typename T, bool ACT, bool ADD>
__global__ __launch_bounds__(256) void k_bn_apply(
    const T* __restrict__ x, const T* __restrict__ res,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ mean, const float* __restrict__ second,
    bool second_is_var, float eps, T* __restrict__ z, int64_t R, int C,
    int lcs, int slabs, int GR) {
  const BnLane l = bn_lane(C, lcs, slabs);
  if (!l.live) return;
  float mu[4], rs[4], gm[4], bt[4];
  ld4(mean + 4 * l.vec, mu), ld4(second + 4 * l.vec, rs);
  ld4(gamma + 4 * l.vec, gm), ld4(beta + 4 * l.vec, bt);
  if (second_is_var) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rs[i] = 1.f / sqrtf(rs[i] + eps);
  }
  const int64_t c0 = 4 * l.vec;
  for (int64_t r0 = (int64_t)l.g * kBnBlocks * l.LR + l.lr; r0 < R;
       r0 += (int64_t)GR * kBnBlocks * l.LR) {
    float v[kBnBlocks][4], a[kBnBlocks][4];
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      const int64_t at = (row < R ? row : R - 1) * C + c0;
      ld4(x + at, v[u]);
      if (ADD) ld4(res + at, a[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      if (row < R) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = fmaf((v[u][i] - mu[i]) * rs[i], gm[i], bt[i]);
          if (ADD) o[i] += a[u][i];
          if (ACT) o[i] = o[i] > 0.f ? o[i] : 0.f;
        }
        st4(z + row * C + c0, o);
      }
    }
  }
}

// Per column sum g and sum g * xhat over the rows, g = dz * (z > 0).
template <typename T, bool ACT>
__global__ __launch_bounds__(256) void k_bn_bwd_reduce(
    const T* __restrict__ dz, const T* __restrict__ z, const T* __restrict__ x,
    const float* __restrict__ stats, float* __restrict__ ws, int64_t R, int C,
    int lcs, int slabs, int GR) {
  __shared__ float hand[3][8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const BnLane l = bn_lane(C, lcs, slabs);
  const int64_t c0 = 4 * (l.live ? l.vec : 0);
  const int64_t Rl = l.live ? R : 0;
  float mu[4], rs[4];
  ld4(stats + c0, mu), ld4(stats + C + c0, rs);
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = (int64_t)l.g * kBnBlocks * l.LR + l.lr; r0 < Rl;
       r0 += (int64_t)GR * kBnBlocks * l.LR) {
    float v[kBnBlocks][4], d[kBnBlocks][4], o[kBnBlocks][4];
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      const int64_t at = (row < R ? row : R - 1) * C + c0;
      ld4(x + at, v[u]), ld4(dz + at, d[u]);
      if (ACT) ld4(z + at, o[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const bool ok = r0 + (int64_t)u * l.LR < R;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float g = ok && (!ACT || o[u][i] > 0.f) ? d[u][i] : 0.f;
        sg[i] += g;
        sx[i] = fmaf(g, (v[u][i] - mu[i]) * rs[i], sx[i]);
      }
    }
  }
  for (int off = 32; off >> lcs; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sg[i] += down_lane(sg[i], lane, off);
      sx[i] += down_lane(sx[i], lane, off);
    }
  }
  const bool head = (lane >> lcs) == 0 || lcs == 6;
  if (wave > 0 && head) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hand[wave - 1][i][lane] = sg[i], hand[wave - 1][4 + i][lane] = sx[i];
  }
  block_sync();
  if (wave == 0 && head && l.live) {
#pragma unroll
    for (int w3 = 0; w3 < 3; ++w3) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sg[i] += hand[w3][i][lane], sx[i] += hand[w3][4 + i][lane];
    }
    float* slice = ws + (int64_t)l.g * 2 * C + c0;
    st4(slice, sg);
    st4(slice + C, sx);
  }
}

// dx = gamma * rstd * (g - dbeta/R - xhat * dgamma/R); with ADD dres = g.
template <typename T, bool ACT, bool ADD>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(
    const T* __restrict__ dz, const T* __restrict__ z, const T* __restrict__ x,
    const float* __restrict__ stats, const float* __restrict__ gamma,
    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
    T* __restrict__ dx, T* __restrict__ dres, float inv_rows, int64_t R, int C,
    int lcs, int slabs, int GR) {
  const BnLane l = bn_lane(C, lcs, slabs);
  if (!l.live) return;
  const int64_t c0 = 4 * l.vec;
  float mu[4], rs[4], k[4], mg[4], mb[4];
  ld4(stats + c0, mu), ld4(stats + C + c0, rs);
  ld4(gamma + c0, k), ld4(dgamma + c0, mg), ld4(dbeta + c0, mb);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    k[i] *= rs[i], mg[i] *= inv_rows, mb[i] *= inv_rows;
  for (int64_t r0 = (int64_t)l.g * kBnBlocks * l.LR + l.lr; r0 < R;
       r0 += (int64_t)GR * kBnBlocks * l.LR) {
    float v[kBnBlocks][4], d[kBnBlocks][4], o[kBnBlocks][4];
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      const int64_t at = (row < R ? row : R - 1) * C + c0;
      ld4(x + at, v[u]), ld4(dz + at, d[u]);
      if (ACT) ld4(z + at, o[u]);
    }
#pragma unroll
    for (int u = 0; u < kBnBlocks; ++u) {
      const int64_t row = r0 + (int64_t)u * l.LR;
      if (row < R) {
        float g[4], r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          g[i] = !ACT || o[u][i] > 0.f ? d[u][i] : 0.f;
          const float xh = (v[u][i] - mu[i]) * rs[i];
          r[i] = k[i] * ((g[i] - mb[i]) - xh * mg[i]);
        }
        st4(dx + row * C + c0, r);
        if (ADD) st4(dres + row * C + c0, g);
      }
    }
  }
}

struct BnPlan {
  int lcs, LR, slabs, GR;  // LC = 1 << lcs
};

BnPlan bn_plan_of(int64_t R, int64_t C) {
  const int nvec = (int)(C / 4);
  BnPlan p;
  p.lcs = 0;
  while ((1 << p.lcs) < std::min(nvec, 64)) ++p.lcs;
  const int LC = 1 << p.lcs;
  p.LR = 256 / LC;
  p.slabs = (nvec + LC - 1) / LC;
  const int64_t chunks = (R + kBnBlocks * p.LR - 1) / (kBnBlocks * p.LR);
  p.GR = (int)std::max<int64_t>(
      1, std::min<int64_t>(chunks, std::max(1, kBnTargetGrid / p.slabs)));
  return p;
}

struct BnDims {
  int64_t R, C;
};

using NamedTensors =
    std::initializer_list<std::pair<const char*, const torch::Tensor*>>;

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// The argument check shared by bn_fwd and bn_bwd, complete before any launch.
// `same` are the optional operands of x's shape and dtype (residual, z, dz),
// `per_channel` the f32 [C] tensors, `col_stats` the backward's statistics,
// `batches` the optional int64 counter.
BnDims bn_check_args(const char* who, const torch::Tensor& x, NamedTensors same,
                     NamedTensors per_channel, const torch::Tensor* col_stats,
                     const torch::Tensor* batches, bool training, bool relu,
                     bool has_residual, double momentum, double eps) {
  TORCH_CHECK(x.defined() && x.is_cuda(), who, ": x must be on a GPU");
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && aligned16(x), who,
              ": x must be 2-D [rows, channels], contiguous and 16-byte "
              "aligned");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK(C % 4 == 0 && C >= 4 && C <= kBnMaxC, who,
              " supports a channel count that is a multiple of 4 in [4, ",
              kBnMaxC, "], got C = ", C);
  TORCH_CHECK(R >= (training ? 2 : 1), who, ": needs at least ",
              training ? 2 : 1, " rows per channel, got ", R);
  TORCH_CHECK(relu || !has_residual, who,
              ": a residual is only taken together with ReLU");
  for (const auto& [name, t] : same) {
    if (!t) continue;
    TORCH_CHECK(t->defined() && t->device() == x.device() &&
                    t->scalar_type() == dt,
                who, ": ", name, " must have x's dtype and device");
    TORCH_CHECK(t->sizes() == x.sizes() && t->is_contiguous() && aligned16(*t),
                who, ": ", name,
                " must be contiguous, 16-byte aligned and of x's shape ",
                x.sizes(), ", got ", t->sizes());
  }
  for (const auto& [name, t] : per_channel) {
    if (!t) continue;
    TORCH_CHECK(t->defined() && t->device() == x.device() &&
                    t->scalar_type() == at::kFloat && t->dim() == 1 &&
                    t->size(0) == C && t->is_contiguous() && aligned16(*t),
                who, ": ", name, " must be f32 [", C,
                "], contiguous and 16-byte aligned, on x's device");
  }
  if (col_stats)
    TORCH_CHECK(col_stats->defined() && col_stats->device() == x.device() &&
                    col_stats->scalar_type() == at::kFloat &&
                    col_stats->dim() == 2 && col_stats->size(0) == 2 &&
                    col_stats->size(1) == C && col_stats->is_contiguous() &&
                    aligned16(*col_stats),
                who, ": col_stats must be bn_fwd's f32 [2, C] = [2, ", C,
                "] on x's device");
  if (batches)
    TORCH_CHECK(batches->defined() && batches->device() == x.device() &&
                    batches->scalar_type() == at::kLong &&
                    batches->numel() == 1,
                who, ": num_batches_tracked must be one int64 on x's device");
  TORCH_CHECK(momentum >= 0 && momentum <= 1, who,
              ": momentum must be in [0, 1], got ", momentum);
  TORCH_CHECK(eps >= 0, who, ": eps must be >= 0, got ", eps);
  return {R, C};
}

// A caller's preallocated result, checked, or a fresh one.
torch::Tensor bn_result(const char* who, const char* name,
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

// f(ACT, ADD) as integral constants for the three forms.
template <typename F>
void with_bn_form(bool relu, bool add, F&& f) {
  if (!relu) f(std::false_type{}, std::false_type{});
  else if (!add) f(std::true_type{}, std::false_type{});
  else f(std::true_type{}, std::true_type{});
}

}  // namespace

std::vector<int64_t> bn_plan(int64_t R, int64_t C) {
  TORCH_CHECK(R >= 1 && C % 4 == 0 && C >= 4 && C <= kBnMaxC,
              "bn_plan: bad shape");
  const BnPlan p = bn_plan_of(R, C);
  return {int64_t(1) << p.lcs, p.slabs, p.GR};
}

std::vector<torch::Tensor> bn_fwd(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, bool training,
    double momentum, double eps, bool relu,
    c10::optional<torch::Tensor> residual,
    c10::optional<torch::Tensor> num_batches_tracked,
    c10::optional<torch::Tensor> z_, c10::optional<torch::Tensor> col_stats_) {
  const char* who = "bn_fwd";
  const BnDims d = bn_check_args(
      who, x, {{"residual", opt_ptr(residual)}},
      {{"weight", &weight},
       {"bias", &bias},
       {"running_mean", &running_mean},
       {"running_var", &running_var}},
      nullptr, opt_ptr(num_batches_tracked), training, relu,
      residual.has_value(), momentum, eps);
  TORCH_CHECK(training || !col_stats_.has_value(), who,
              ": col_stats is a result of the training forward only");
  const auto f32 = x.options().dtype(at::kFloat);
  auto z = bn_result(who, "z", z_, x.sizes(), x.options());
  torch::Tensor stats;
  if (training) stats = bn_result(who, "col_stats", col_stats_, {2, d.C}, f32);
  const BnPlan p = bn_plan_of(d.R, d.C);
  const dim3 grid(p.slabs * p.GR);
  const int C = (int)d.C;
  const bool add = residual.has_value();
  if (training) {
    auto ws = torch::empty({p.GR, 3, d.C}, f32);
    DISPATCH_F32_BF16(x.scalar_type(), who, {
      hipLaunchKernelGGL((k_bn_stats<scalar_t>), grid, dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(x), dptr<float>(ws),
                         d.R, C, p.lcs, p.slabs, p.GR);
    });
    hipLaunchKernelGGL(
        (k_bn_finish<true>), dim3(cdiv(d.C, 64)), dim3(kFinishWaves * 64), 0,
        cur_stream(), cdptr<float>(ws), p.GR, C, d.R, kBnBlocks * p.LR,
        dptr<float>(stats), dptr<float>(stats) + d.C,
        dptr<float>(running_mean), dptr<float>(running_var),
        num_batches_tracked.has_value() ? dptr<int64_t>(*num_batches_tracked)
                                        : nullptr,
        (float)momentum, (float)eps);
  }
  const float* mean = training ? cdptr<float>(stats) : cdptr<float>(running_mean);
  const float* second =
      training ? cdptr<float>(stats) + d.C : cdptr<float>(running_var);
  DISPATCH_F32_BF16(x.scalar_type(), who, {
    with_bn_form(relu, add, [&](auto act, auto ad) {
      constexpr bool ACT = decltype(act)::value, ADD = decltype(ad)::value;
      hipLaunchKernelGGL(
          (k_bn_apply<scalar_t, ACT, ADD>), grid, dim3(256), 0, cur_stream(),
          cdptr<scalar_t>(x), ADD ? cdptr<scalar_t>(*residual) : nullptr,
          cdptr<float>(weight), cdptr<float>(bias), mean, second, !training,
          (float)eps, dptr<scalar_t>(z), d.R, C, p.lcs, p.slabs, p.GR);
    });
  });
  HIP_OK(hipGetLastError());
  if (training) return {z, stats};
  return {z};
}

std::vector<torch::Tensor> bn_bwd(
    torch::Tensor dz, torch::Tensor x, torch::Tensor col_stats,
    torch::Tensor weight, c10::optional<torch::Tensor> z, bool add,
    c10::optional<torch::Tensor> dx_, c10::optional<torch::Tensor> dresidual_,
    c10::optional<torch::Tensor> dgamma_, c10::optional<torch::Tensor> dbeta_) {
  const char* who = "bn_bwd";
  const bool relu = z.has_value();
  const BnDims d =
      bn_check_args(who, x, {{"dz", &dz}, {"z", opt_ptr(z)}},
                    {{"weight", &weight}}, &col_stats, nullptr,
                    /*training=*/true, relu, add, 0.0, 0.0);
  TORCH_CHECK(add || !dresidual_.has_value(), who,
              ": dresidual needs the residual form");
  const auto f32 = x.options().dtype(at::kFloat);
  auto dx = bn_result(who, "dx", dx_, x.sizes(), x.options());
  torch::Tensor dres;
  if (add) dres = bn_result(who, "dresidual", dresidual_, x.sizes(), x.options());
  auto dgamma = bn_result(who, "dgamma", dgamma_, {d.C}, f32);
  auto dbeta = bn_result(who, "dbeta", dbeta_, {d.C}, f32);
  const BnPlan p = bn_plan_of(d.R, d.C);
  const dim3 grid(p.slabs * p.GR);
  const int C = (int)d.C;
  auto ws = torch::empty({p.GR, 2, d.C}, f32);
  DISPATCH_F32_BF16(x.scalar_type(), who, {
    with_bn_form(relu, add, [&](auto act, auto ad) {
      constexpr bool ACT = decltype(act)::value, ADD = decltype(ad)::value;
      const scalar_t* zp = ACT ? cdptr<scalar_t>(*z) : nullptr;
      hipLaunchKernelGGL((k_bn_bwd_reduce<scalar_t, ACT>), grid, dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(dz), zp,
                         cdptr<scalar_t>(x), cdptr<float>(col_stats),
                         dptr<float>(ws), d.R, C, p.lcs, p.slabs, p.GR);
      hipLaunchKernelGGL((k_bn_finish<false>), dim3(cdiv(d.C, 64)),
                         dim3(kFinishWaves * 64), 0, cur_stream(),
                         cdptr<float>(ws), p.GR, C, d.R, kBnBlocks * p.LR,
                         dptr<float>(dbeta), dptr<float>(dgamma),
                         (float*)nullptr, (float*)nullptr, (int64_t*)nullptr,
                         0.f, 0.f);
      hipLaunchKernelGGL(
          (k_bn_bwd_apply<scalar_t, ACT, ADD>), grid, dim3(256), 0,
          cur_stream(), cdptr<scalar_t>(dz), zp, cdptr<scalar_t>(x),
          cdptr<float>(col_stats), cdptr<float>(weight), cdptr<float>(dgamma),
          cdptr<float>(dbeta), dptr<scalar_t>(dx),
          ADD ? dptr<scalar_t>(dres) : nullptr, 1.f / (float)d.R, d.R, C,
          p.lcs, p.slabs, p.GR);
    });
  });
  HIP_OK(hipGetLastError());
  if (add) return {dx, dgamma, dbeta, dres};
  return {dx, dgamma, dbeta};
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
