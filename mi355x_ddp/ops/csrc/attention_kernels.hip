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
// Three kernel families: the short one described here, below it the tiled
// one for up to 4096 tokens (k_attn_tiled_*), which shares its helpers, and
// last the bf16-only one on the wide bf16 MFMA (k_attn_bf16_*).
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

// Clang vector types and builtins, not the HIP headers' float4, __shfl_xor
// and the like: under this file's target attribute those stay as CALLS
// (docs/KERNELS.md, "No header calls").
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

__device__ __forceinline__ float as_f32(uint32_t u) {
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ void load4(const float* p, float v[4]) {
  const f32x4 x = *reinterpret_cast<const f32x4*>(p);
  v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
}
__device__ __forceinline__ void load4(const __hip_bfloat16* p, float v[4]) {
  const u32x2 x = *reinterpret_cast<const u32x2*>(p);
  v[0] = as_f32(x[0] << 16), v[1] = as_f32(x[0] & 0xffff0000u);
  v[2] = as_f32(x[1] << 16), v[3] = as_f32(x[1] & 0xffff0000u);
}
// The value of lane `src` (ds_bpermute).
__device__ __forceinline__ float from_lane(float v, int src) {
  return __builtin_bit_cast(
      float,
      __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
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
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1)
    v = fmaxf(v, from_lane(v, lane ^ off));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += from_lane(v, lane ^ off);
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

// ===========================================================================
// The tiled family: 64 < N <= 4096 (and any N >= 1), same operands and
// arithmetic. A workgroup owns 64 rows (16 per wave) whose operands stay in
// A-operand registers (D/4 words per lane, read from global memory once)
// and walks the other side in blocks of 64 rows that every wave stages
// together. The next block's global loads are issued right after the current
// block's LDS stores, ahead of its MFMAs. A 16 x 64 strip goes from
// D-fragment to A-operand layout through the wave's own piece of LDS: no
// other wave touches it, so it takes wave-scope ordering and no barrier.
//
//   fwd     rows: queries  walks keys     online softmax, O rescaled in place
//   bwd_q   rows: queries  walks keys     delta = rowsum(dO * O), dQ
//   bwd_kv  rows: KEYS     walks queries  dK, dV from the TRANSPOSED strips
//
// Every result row is written once by the one wave that owns it: no atomics,
// nothing pre-zeroed. Rows >= N are zero in every operand, never read from
// global memory and never stored; keys >= N get -inf (forward) or P = 0
// (backward), so the last block may hold a single row.
// ===========================================================================
constexpr int kAttnTiledMaxN = 4096;
constexpr int kBlk = 64;   // rows per workgroup and per staged block
constexpr int kStripP = 68;  // pitch of a wave's strip, read rk only

// One block of 64 rows x D, fetched into registers (rows >= N zero) ...
template <typename T, int D>
__device__ __forceinline__ void fetch_block(float regs[D / 16][4],
                                            const T* src, size_t ld, int row0,
                                            int N) {
  constexpr int CH = D / 4;
#pragma unroll
  for (int u = 0; u < D / 16; ++u) {
    const int idx = threadIdx.x + u * 256;
    const int row = row0 + idx / CH, c = (idx % CH) * 4;
    regs[u][0] = regs[u][1] = regs[u][2] = regs[u][3] = 0.f;
    if (row < N) load4(src + (size_t)row * ld + c, regs[u]);
  }
}
// ... and put into its LDS image.
template <int D>
__device__ __forceinline__ void put_block(float* img, int pitch,
                                          const float regs[D / 16][4]) {
  constexpr int CH = D / 4;
#pragma unroll
  for (int u = 0; u < D / 16; ++u) {
    const int idx = threadIdx.x + u * 256;
    *reinterpret_cast<f32x4*>(&img[(idx / CH) * pitch + (idx % CH) * 4]) =
        f32x4{regs[u][0], regs[u][1], regs[u][2], regs[u][3]};
  }
}

// The lane's A operand of one row for a contraction over D, from global.
template <typename T, int D>
__device__ __forceinline__ void load_a(float a[D / 4], const T* src, size_t ld,
                                       int row, int N, int q) {
#pragma unroll
  for (int s = 0; s < D / 4; ++s)
    a[s] = row < N ? ldf(&src[(size_t)row * ld + s * 4 + q]) : 0.f;
}

// Fragment-layout strip -> the wave's own LDS piece. LDS serves one wave's
// accesses in program order; the fences keep the compiler from reordering
// the stores and the loads around them.
__device__ __forceinline__ void strip_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void put_strip(float* strip, const f32x4 f[4],
                                          int nt, int r, int q) {
  strip_sync();  // the previous use's loads come first
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        strip[(q * 4 + i) * kStripP + j * 16 + r] = f[j][i];
    }
  strip_sync();
}

struct TiledBlock {
  int b, h, blk;  // batch, head, 64-row block of this workgroup
};
__device__ __forceinline__ TiledBlock tiled_block(int H, int nblk) {
  const int bh = blockIdx.x / nblk;
  return {bh / H, bh % H, (int)(blockIdx.x % nblk)};
}

// Forward. Images: K (rk, 68), V (kr, 80), four strips (P).
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void k_attn_tiled_fwd(
    const T* __restrict__ qkv, T* __restrict__ out, f32x2* __restrict__ stats,
    int N, int H, int nblk, float scale) {
  constexpr int PK = 68, PV = 80;
  __shared__ float sK[kBlk * PK];
  __shared__ float sV[kBlk * PV];
  __shared__ float sP[kBlk * kStripP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const T* src = qkv + (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const int row0 = w.blk * kBlk + wave * 16;
  const bool active = row0 < N;  // the others only stage
  float* strip = sP + wave * 16 * kStripP;
  const float c = scale * kLog2e;

  float a[D / 4];
  load_a<T, D>(a, src, 3 * E, row0 + r, N, q);
  float m[4], l[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = -INFINITY;
  f32x4 o[D / 16] = {};

  float kreg[D / 16][4], vreg[D / 16][4];
  fetch_block<T, D>(kreg, src + E, 3 * E, 0, N);
  fetch_block<T, D>(vreg, src + 2 * E, 3 * E, 0, N);
  for (int k0 = 0; k0 < N; k0 += kBlk) {
    block_sync();  // the previous block's reads are done
    put_block<D>(sK, PK, kreg);
    put_block<D>(sV, PV, vreg);
    block_sync();
    if (k0 + kBlk < N) {
      fetch_block<T, D>(kreg, src + E, 3 * E, k0 + kBlk, N);
      fetch_block<T, D>(vreg, src + 2 * E, 3 * E, k0 + kBlk, N);
    }
    if (!active) continue;
    const int nt = min(4, (N - k0 + 15) >> 4);
    f32x4 s4[4] = {};
    strip_rk<D>(s4, a, sK, PK, nt, r, q);
    // online softmax on the fragments: row = row0 + 4q + i, key k0 + 16j + r
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float mb = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= nt || k0 + j * 16 + r >= N) s4[j][i] = -INFINITY;
        mb = fmaxf(mb, s4[j][i]);
      }
      // finite: key k0 exists. From m = -inf the factor is exp2(-inf) = 0.
      const float mn = fmaxf(m[i], row16_max(mb));
      const float f = __builtin_amdgcn_exp2f((m[i] - mn) * c);
      m[i] = mn;
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __builtin_amdgcn_exp2f((s4[j][i] - mn) * c);
        s4[j][i] = p;
        sum += p;
      }
      l[i] = l[i] * f + row16_sum(sum);
#pragma unroll
      for (int t = 0; t < D / 16; ++t) o[t][i] *= f;
    }
    put_strip(strip, s4, nt, r, q);
    strip_out<D, false>(o, strip, kStripP, 0, sV, PV, nt * 16, r, q);
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      l[i] = 1.f / l[i];
      const int row = row0 + q * 4 + i;
      if (r == 0 && row < N)
        stats[((size_t)w.b * H + w.h) * N + row] = f32x2{m[i], l[i]};
    }
    store_strip<T, D>(out + (size_t)w.b * N * E + (size_t)w.h * D, E, o, row0,
                      N, l, r, q);
  }
}

// P of one fragment element from the saved statistics, as the forward's.
__device__ __forceinline__ float p_from_stats(float s, f32x2 st, float c,
                                              bool live) {
  return live ? __builtin_amdgcn_exp2f((s - st[0]) * c) * st[1] : 0.f;
}

// Backward, query side. Images: K (S: rk, dQ: kr; 72), V (dP: rk; 68), four
// strips (dS). Also leaves delta[b, h, row] for k_attn_tiled_bwd_kv.
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void k_attn_tiled_bwd_q(
    const T* __restrict__ qkv, const T* __restrict__ dout,
    const T* __restrict__ out, const f32x2* __restrict__ stats,
    float* __restrict__ delta, T* __restrict__ dqkv, int N, int H, int nblk,
    float scale) {
  constexpr int PK = 72, PV = 68;
  __shared__ float sK[kBlk * PK];
  __shared__ float sV[kBlk * PV];
  __shared__ float sS[kBlk * kStripP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const size_t hq = (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const size_t ho = (size_t)w.b * N * E + (size_t)w.h * D;
  const size_t hs = ((size_t)w.b * H + w.h) * N;
  const int row0 = w.blk * kBlk + wave * 16;
  const bool active = row0 < N;
  float* strip = sS + wave * 16 * kStripP;
  const float c = scale * kLog2e;

  float a_q[D / 4], a_do[D / 4];
  load_a<T, D>(a_q, qkv + hq, 3 * E, row0 + r, N, q);
  load_a<T, D>(a_do, dout + ho, E, row0 + r, N, q);
  // delta = the diagonal of dO O^T, by the MFMA steps that form dP = dO V^T:
  // O's rows in A-operand registers are also its B operand here. Where a row
  // has one key (O = V) delta then equals dP bit for bit and dS is exactly 0.
  f32x2 st[4];
  float dl[4];
  {
    float a_o[D / 4];
    load_a<T, D>(a_o, out + ho, E, row0 + r, N, q);
    f32x4 t = {};
#pragma unroll
    for (int s = 0; s < D / 4; ++s) t = mfma4(a_do[s], a_o[s], t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // fragment row 4q + i, column r
      const int row = row0 + q * 4 + i;
      dl[i] = from_lane(t[i], q * 16 + q * 4 + i);
      if (r == q * 4 + i && row < N) delta[hs + row] = t[i];
      st[i] = active && row < N ? stats[hs + row] : f32x2{0.f, 0.f};
    }
  }
  f32x4 dq[D / 16] = {};

  float kreg[D / 16][4], vreg[D / 16][4];
  fetch_block<T, D>(kreg, qkv + hq + E, 3 * E, 0, N);
  fetch_block<T, D>(vreg, qkv + hq + 2 * E, 3 * E, 0, N);
  for (int k0 = 0; k0 < N; k0 += kBlk) {
    block_sync();
    put_block<D>(sK, PK, kreg);
    put_block<D>(sV, PV, vreg);
    block_sync();
    if (k0 + kBlk < N) {
      fetch_block<T, D>(kreg, qkv + hq + E, 3 * E, k0 + kBlk, N);
      fetch_block<T, D>(vreg, qkv + hq + 2 * E, 3 * E, k0 + kBlk, N);
    }
    if (!active) continue;
    const int nt = min(4, (N - k0 + 15) >> 4);
    f32x4 s4[4] = {}, ds4[4] = {};
    strip_rk<D>(s4, a_q, sK, PK, nt, r, q);    // S
    strip_rk<D>(ds4, a_do, sV, PV, nt, r, q);  // dP
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool row_live = row0 + q * 4 + i < N;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = row_live && j < nt && k0 + j * 16 + r < N;
        const float p = p_from_stats(s4[j][i], st[i], c, live);
        ds4[j][i] = p * (ds4[j][i] - dl[i]) * scale;
      }
    }
    put_strip(strip, ds4, nt, r, q);
    strip_out<D, false>(dq, strip, kStripP, 0, sK, PK, nt * 16, r, q);
  }
  if (active) {
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    store_strip<T, D>(dqkv + hq, 3 * E, dq, row0, N, one, r, q);
  }
}

// Backward, key side. The wave's rows are KEYS, so its strips are S^T, dP^T:
// row = key row0 + 4q + i, column = query q0 + 16j + r, and the statistics
// and delta are one value per lane and query tile j. Images: Q (S^T: rk,
// dK: kr; 72), dO (dP^T: rk, dV: kr; 72), four strips (P^T, then dS^T).
template <typename T, int D>
__global__ __launch_bounds__(256, 2) void k_attn_tiled_bwd_kv(
    const T* __restrict__ qkv, const T* __restrict__ dout,
    const f32x2* __restrict__ stats, const float* __restrict__ delta,
    T* __restrict__ dqkv, int N, int H, int nblk, float scale) {
  constexpr int PQ = 72;
  __shared__ float sQ[kBlk * PQ];
  __shared__ float sO[kBlk * PQ];
  __shared__ float sS[kBlk * kStripP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const size_t hq = (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const size_t ho = (size_t)w.b * N * E + (size_t)w.h * D;
  const size_t hs = ((size_t)w.b * H + w.h) * N;
  const int row0 = w.blk * kBlk + wave * 16;
  const bool active = row0 < N;
  float* strip = sS + wave * 16 * kStripP;
  const float c = scale * kLog2e;

  float a_k[D / 4], a_v[D / 4];
  load_a<T, D>(a_k, qkv + hq + E, 3 * E, row0 + r, N, q);
  load_a<T, D>(a_v, qkv + hq + 2 * E, 3 * E, row0 + r, N, q);
  f32x4 dk[D / 16] = {}, dv[D / 16] = {};

  float qreg[D / 16][4], oreg[D / 16][4];
  fetch_block<T, D>(qreg, qkv + hq, 3 * E, 0, N);
  fetch_block<T, D>(oreg, dout + ho, E, 0, N);
  for (int q0 = 0; q0 < N; q0 += kBlk) {
    block_sync();
    put_block<D>(sQ, PQ, qreg);
    put_block<D>(sO, PQ, oreg);
    block_sync();
    if (q0 + kBlk < N) {
      fetch_block<T, D>(qreg, qkv + hq, 3 * E, q0 + kBlk, N);
      fetch_block<T, D>(oreg, dout + ho, E, q0 + kBlk, N);
    }
    if (!active) continue;
    const int nt = min(4, (N - q0 + 15) >> 4);
    f32x2 st[4];
    float dl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = q0 + j * 16 + r;
      const bool in = j < nt && col < N;
      st[j] = in ? stats[hs + col] : f32x2{0.f, 0.f};
      dl[j] = in ? delta[hs + col] : 0.f;
    }
    f32x4 p4[4] = {}, ds4[4] = {};
    strip_rk<D>(p4, a_k, sQ, PQ, nt, r, q);   // S^T
    strip_rk<D>(ds4, a_v, sO, PQ, nt, r, q);  // dP^T
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool row_live = row0 + q * 4 + i < N;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = row_live && j < nt && q0 + j * 16 + r < N;
        const float p = p_from_stats(p4[j][i], st[j], c, live);
        p4[j][i] = p;
        ds4[j][i] = p * (ds4[j][i] - dl[j]) * scale;
      }
    }
    put_strip(strip, p4, nt, r, q);
    strip_out<D, false>(dv, strip, kStripP, 0, sO, PQ, nt * 16, r, q);
    put_strip(strip, ds4, nt, r, q);
    strip_out<D, false>(dk, strip, kStripP, 0, sQ, PQ, nt * 16, r, q);
  }
  if (active) {
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    store_strip<T, D>(dqkv + hq + E, 3 * E, dk, row0, N, one, r, q);
    store_strip<T, D>(dqkv + hq + 2 * E, 3 * E, dv, row0, N, one, r, q);
  }
}

// ===========================================================================
// The bf16 family: bf16 storage only, D in {32, 64}, 1 <= N <= 4096, all five
// products on v_mfma_f32_16x16x32_bf16. The work split, grid, two backward
// launches, layouts and masking are the tiled family's; the operands are not.
//
// Lane maps of the wide MFMA (r = lane & 15, q = lane >> 4): A[m = r][k =
// 8q + e], B[k = 8q + e][n = r], e < 8; C/D col = r, row = 4q + reg. The
// contraction only needs A and B to agree on which index a slot (q, e) means.
//
// The wave's own 16 rows are always the B operand (n = r), 16 bytes per lane
// and step from global memory. Every product has the walked side as A (m):
//   first   S^T = K_blk Q_own^T (fwd, bwd_q), dP^T = V_blk dO_own^T (bwd_q),
//           S = Q_blk K_own^T, dP = dO_blk V_own^T (bwd_kv): A is one
//           ds_read_b128 from a straight [64][D] image. Lane (r, q) of
//           fragment j then holds walked rows 16j + 4q .. + 3 of own row r.
//   second  O^T = V^T P^T, dQ^T = K^T dS^T, dV^T = dO^T P, dK^T = Q^T dS:
//           the contraction runs over the walked rows. Fragments 2t, 2t + 1,
//           rounded and packed, ARE the lane's B operand of wide step t with
//           slot e < 4 = walked row 32t + 4q + e, e >= 4 = 32t + 16 + 4q +
//           e - 4; A comes from a transposed [D][64] image with two
//           ds_read_b64 at those offsets. P and dS never touch LDS.
// Every result lands as own row r, columns 16u + 4q .. + 3 of lane (r, q):
// the softmax statistics of a query are per lane column in fwd and bwd_q
// (two cross-lane steps), and a result row is stored 8 bytes per lane.
//
// Images. Straight: pitch D/2 + 4 words (4 * odd: the 16 lanes of one
// quarter of a ds_read_b128 cover all 64 banks). Transposed: two adjacent
// walked rows interleaved into words while storing, pitch 36 words: the 32
// lanes of half a ds_read_b64 (r, q & 1) hit words 36 r + 2 (q & 1) + const,
// all 64 banks once.
// ===========================================================================
using bf16_t = __hip_bfloat16;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
constexpr int kPT = 36;  // words per row of a transposed image

// Two floats to two bf16, round to nearest even (v_cvt_pk_bf16_f32).
__device__ __forceinline__ uint32_t bf16_pack(float lo, float hi) {
  const bf16x2 p = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, p);
}
// Fragments 2t and 2t + 1 as the B operand of wide step t.
__device__ __forceinline__ u32x4 pack_pair(f32x4 x, f32x4 y) {
  return u32x4{bf16_pack(x[0], x[1]), bf16_pack(x[2], x[3]),
               bf16_pack(y[0], y[1]), bf16_pack(y[2], y[3])};
}
__device__ __forceinline__ f32x4 mfma32(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
      0);
}
// Over the four lanes that share r (one own row).
__device__ __forceinline__ float col4_max(float v, int lane) {
  v = fmaxf(v, from_lane(v, lane ^ 16));
  return fmaxf(v, from_lane(v, lane ^ 32));
}
__device__ __forceinline__ float col4_sum(float v, int lane) {
  v += from_lane(v, lane ^ 16);
  return v + from_lane(v, lane ^ 32);
}

// The lane's B operand of its own row for a contraction over D.
template <int D>
__device__ __forceinline__ void load_own(u32x4 b[D / 32], const bf16_t* src,
                                         size_t ld, int row, int N, int q) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    b[s] = u32x4{0u, 0u, 0u, 0u};
    if (row < N)
      b[s] = *reinterpret_cast<const u32x4*>(src + (size_t)row * ld + 32 * s +
                                             8 * q);
  }
}

// A walked block of 64 rows x D: a thread moves the same 8 columns (chunk c)
// of the adjacent rows 2p, 2p + 1, first into registers (rows >= N zero),
// then into the straight image as loaded and/or the transposed one with the
// two rows interleaved. Four chunks per row and wave, 16 row pairs per wave:
// 64-byte global segments, and the interleaved stores of a wave meet 32
// banks (two-way, as k_gemm_tile's). At D = 32 waves 2 and 3 have no chunk.
template <int D>
struct Walked {
  static constexpr int PS = D / 2 + 4;  // words per row of a straight image
  int c, p;
  __device__ __forceinline__ Walked() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c = 4 * (wave % (D / 32)) + (lane & 3);
    p = 16 * (wave / (D / 32)) + (lane >> 2);
  }
  __device__ __forceinline__ void fetch(u32x4 v[2], const bf16_t* src,
                                        size_t ld, int row0, int N) const {
    v[0] = v[1] = u32x4{0u, 0u, 0u, 0u};
    const int row = row0 + 2 * p;
    if (p < 32 && row < N)
      v[0] = *reinterpret_cast<const u32x4*>(src + (size_t)row * ld + 8 * c);
    if (p < 32 && row + 1 < N)
      v[1] =
          *reinterpret_cast<const u32x4*>(src + (size_t)(row + 1) * ld + 8 * c);
  }
  template <bool STRAIGHT, bool TRANSPOSED>
  __device__ __forceinline__ void put(uint32_t* simg, uint32_t* timg,
                                      const u32x4 v[2]) const {
    if (p >= 32) return;
    if constexpr (STRAIGHT) {
      *reinterpret_cast<u32x4*>(&simg[(2 * p) * PS + 4 * c]) = v[0];
      *reinterpret_cast<u32x4*>(&simg[(2 * p + 1) * PS + 4 * c]) = v[1];
    }
    if constexpr (TRANSPOSED) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint32_t lo = v[0][w], hi = v[1][w];
        timg[(8 * c + 2 * w) * kPT + p] = (lo & 0xffffu) | (hi << 16);
        timg[(8 * c + 2 * w + 1) * kPT + p] = (lo >> 16) | (hi & 0xffff0000u);
      }
    }
  }
};

// acc[j] += simg rows 16j .. 16j + 15 (A) . the own rows (B), j < nt.
template <int D>
__device__ __forceinline__ void first_product(f32x4 acc[4],
                                              const uint32_t* simg,
                                              const u32x4 b[D / 32], int nt,
                                              int r, int q) {
  constexpr int PS = Walked<D>::PS;
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nt)
        acc[j] = mfma32(*reinterpret_cast<const u32x4*>(
                            &simg[(16 * j + r) * PS + 16 * s + 4 * q]),
                        b[s], acc[j]);
  }
}
// acc[u] += timg columns 16u .. 16u + 15 (A) . the packed fragments (B) over
// the wide steps t < nw, the image read in the fragments' row order.
template <int D>
__device__ __forceinline__ void second_product(f32x4 acc[D / 16],
                                               const uint32_t* timg,
                                               const u32x4 b[2], int nw, int r,
                                               int q) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (t < nw) {
#pragma unroll
      for (int u = 0; u < D / 16; ++u) {
        const uint32_t* at = &timg[(16 * u + r) * kPT + 16 * t + 2 * q];
        const u32x2 lo = *reinterpret_cast<const u32x2*>(at);
        const u32x2 hi = *reinterpret_cast<const u32x2*>(at + 8);
        acc[u] = mfma32(u32x4{lo[0], lo[1], hi[0], hi[1]}, b[t], acc[u]);
      }
    }
}
// Own row `row`, columns 16u + 4q .. + 3, times mul, rounded once.
template <int D>
__device__ __forceinline__ void store_own(bf16_t* dst, size_t ld,
                                          const f32x4 acc[D / 16], int row,
                                          int N, float mul, int q) {
  if (row >= N) return;
#pragma unroll
  for (int u = 0; u < D / 16; ++u)
    *reinterpret_cast<u32x2*>(dst + (size_t)row * ld + 16 * u + 4 * q) =
        u32x2{bf16_pack(acc[u][0] * mul, acc[u][1] * mul),
              bf16_pack(acc[u][2] * mul, acc[u][3] * mul)};
}

// Forward. Images: K straight, V transposed. P is rounded to bf16 once, on
// its way into O^T += V^T P^T, and l sums the ROUNDED P: a row of out is an
// exact convex combination of V rows.
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 3 : 4) void k_attn_bf16_fwd(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
    f32x2* __restrict__ stats, int N, int H, int nblk, float scale) {
  __shared__ __attribute__((aligned(16))) uint32_t sK[kBlk * Walked<D>::PS];
  __shared__ __attribute__((aligned(16))) uint32_t sVt[D * kPT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const bf16_t* src = qkv + (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const int row0 = w.blk * kBlk + wave * 16;
  const bool active = row0 < N;  // the others only stage
  const float c = scale * kLog2e;

  u32x4 b_q[D / 32];
  load_own<D>(b_q, src, 3 * E, row0 + r, N, q);
  float m = -INFINITY, l = 0.f;  // of query row0 + r, alike in its four lanes
  f32x4 o[D / 16] = {};

  const Walked<D> wk;
  u32x4 kreg[2], vreg[2];
  wk.fetch(kreg, src + E, 3 * E, 0, N);
  wk.fetch(vreg, src + 2 * E, 3 * E, 0, N);
  for (int k0 = 0; k0 < N; k0 += kBlk) {
    block_sync();  // the previous block's reads are done
    wk.template put<true, false>(sK, nullptr, kreg);
    wk.template put<false, true>(nullptr, sVt, vreg);
    block_sync();
    if (k0 + kBlk < N) {
      wk.fetch(kreg, src + E, 3 * E, k0 + kBlk, N);
      wk.fetch(vreg, src + 2 * E, 3 * E, k0 + kBlk, N);
    }
    if (!active) continue;
    const int rows = min(kBlk, N - k0);
    const int nt = (rows + 15) >> 4, nw = (rows + 31) >> 5;
    f32x4 s4[4] = {};
    first_product<D>(s4, sK, b_q, nt, r, q);
    // lane (r, q), fragment j, word i: query row0 + r, key k0 + 16j + 4q + i
    float mb = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (j >= nt || k0 + 16 * j + 4 * q + i >= N) s4[j][i] = -INFINITY;
        mb = fmaxf(mb, s4[j][i]);
      }
    }
    // finite: key k0 exists. From m = -inf the factor is exp2(-inf) = 0.
    const float mn = fmaxf(m, col4_max(mb, lane));
    const float f = __builtin_amdgcn_exp2f((m - mn) * c);
    m = mn;
    u32x4 pk[2];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        const uint32_t two =
            bf16_pack(__builtin_amdgcn_exp2f((s4[j][i] - mn) * c),
                      __builtin_amdgcn_exp2f((s4[j][i + 1] - mn) * c));
        pk[j >> 1][(j & 1) * 2 + (i >> 1)] = two;
        sum += as_f32(two << 16) + as_f32(two & 0xffff0000u);
      }
    }
    l = l * f + col4_sum(sum, lane);
#pragma unroll
    for (int u = 0; u < D / 16; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[u][i] *= f;
    }
    second_product<D>(o, sVt, pk, nw, r, q);
  }
  if (active) {
    const int row = row0 + r;
    const float il = 1.f / l;
    if (q == 0 && row < N)
      stats[((size_t)w.b * H + w.h) * N + row] = f32x2{m, il};
    store_own<D>(out + (size_t)w.b * N * E + (size_t)w.h * D, E, o, row, N, il,
                 q);
  }
}

// Backward, query side. Images: K straight (S^T) and transposed (dQ^T), V
// straight (dP^T). P comes back from the statistics in f32 and dS is rounded
// once, on its way into dQ^T += K^T dS^T. Leaves delta[b, h, row] for bwd_kv.
template <int D>
__global__ __launch_bounds__(256, 3) void k_attn_bf16_bwd_q(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    const bf16_t* __restrict__ out, const f32x2* __restrict__ stats,
    float* __restrict__ delta, bf16_t* __restrict__ dqkv, int N, int H,
    int nblk, float scale) {
  __shared__ __attribute__((aligned(16))) uint32_t sK[kBlk * Walked<D>::PS];
  __shared__ __attribute__((aligned(16))) uint32_t sKt[D * kPT];
  __shared__ __attribute__((aligned(16))) uint32_t sV[kBlk * Walked<D>::PS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const size_t hq = (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const size_t ho = (size_t)w.b * N * E + (size_t)w.h * D;
  const size_t hs = ((size_t)w.b * H + w.h) * N;
  const int row0 = w.blk * kBlk + wave * 16, row = row0 + r;
  const bool active = row0 < N;
  const float c = scale * kLog2e;

  u32x4 b_q[D / 32], b_do[D / 32];
  load_own<D>(b_q, qkv + hq, 3 * E, row, N, q);
  load_own<D>(b_do, dout + ho, E, row, N, q);
  // delta = the diagonal of O dO^T, by the MFMA steps that form dP^T = V dO^T
  // with O's rows in V's place: where a row has one key (O = V) delta equals
  // dP bit for bit and dS is exactly 0. Element (r, r) sits in lane (r, r / 4),
  // word r % 4; the row's other three lanes fetch it from there.
  float dl;
  {
    u32x4 a_o[D / 32];
    load_own<D>(a_o, out + ho, E, row, N, q);
    f32x4 t = {};
#pragma unroll
    for (int s = 0; s < D / 32; ++s) t = mfma32(a_o[s], b_do[s], t);
    const int i = r & 3;
    const float d = i == 0 ? t[0] : i == 1 ? t[1] : i == 2 ? t[2] : t[3];
    dl = from_lane(d, (r >> 2) * 16 + r);
    if (q == (r >> 2) && row < N) delta[hs + row] = d;
  }
  const f32x2 st = active && row < N ? stats[hs + row] : f32x2{0.f, 0.f};
  f32x4 dq[D / 16] = {};

  const Walked<D> wk;
  u32x4 kreg[2], vreg[2];
  wk.fetch(kreg, qkv + hq + E, 3 * E, 0, N);
  wk.fetch(vreg, qkv + hq + 2 * E, 3 * E, 0, N);
  for (int k0 = 0; k0 < N; k0 += kBlk) {
    block_sync();
    wk.template put<true, true>(sK, sKt, kreg);
    wk.template put<true, false>(sV, nullptr, vreg);
    block_sync();
    if (k0 + kBlk < N) {
      wk.fetch(kreg, qkv + hq + E, 3 * E, k0 + kBlk, N);
      wk.fetch(vreg, qkv + hq + 2 * E, 3 * E, k0 + kBlk, N);
    }
    if (!active) continue;
    const int rows = min(kBlk, N - k0);
    const int nt = (rows + 15) >> 4, nw = (rows + 31) >> 5;
    f32x4 s4[4] = {}, ds4[4] = {};
    first_product<D>(s4, sK, b_q, nt, r, q);    // S^T
    first_product<D>(ds4, sV, b_do, nt, r, q);  // dP^T
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool live = row < N && j < nt && k0 + 16 * j + 4 * q + i < N;
        const float p = p_from_stats(s4[j][i], st, c, live);
        ds4[j][i] = p * (ds4[j][i] - dl) * scale;
      }
    }
    const u32x4 pk[2] = {pack_pair(ds4[0], ds4[1]), pack_pair(ds4[2], ds4[3])};
    second_product<D>(dq, sKt, pk, nw, r, q);
  }
  if (active) store_own<D>(dqkv + hq, 3 * E, dq, row, N, 1.f, q);
}

// Backward, key side. The wave's rows are KEYS: lane (r, q) of fragment j
// holds queries q0 + 16j + 4q .. + 3 of key row0 + r, so the statistics and
// delta are four words per fragment, staged per block beside the images
// (Q and dO, each straight and transposed). P is used in f32 for dS and a
// rounded copy feeds dV^T += dO^T P; dS is rounded into dK^T += Q^T dS.
template <int D>
__global__ __launch_bounds__(256, D == 64 ? 2 : 3) void k_attn_bf16_bwd_kv(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    const f32x2* __restrict__ stats, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int N, int H, int nblk, float scale) {
  __shared__ __attribute__((aligned(16))) uint32_t sQ[kBlk * Walked<D>::PS];
  __shared__ __attribute__((aligned(16))) uint32_t sQt[D * kPT];
  __shared__ __attribute__((aligned(16))) uint32_t sO[kBlk * Walked<D>::PS];
  __shared__ __attribute__((aligned(16))) uint32_t sOt[D * kPT];
  __shared__ __attribute__((aligned(16))) float sSt[3][kBlk];  // m, 1/l, delta
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TiledBlock w = tiled_block(H, nblk);
  const size_t E = (size_t)H * D;
  const size_t hq = (size_t)w.b * N * 3 * E + (size_t)w.h * D;
  const size_t ho = (size_t)w.b * N * E + (size_t)w.h * D;
  const size_t hs = ((size_t)w.b * H + w.h) * N;
  const int row0 = w.blk * kBlk + wave * 16, row = row0 + r;
  const bool active = row0 < N;
  const float c = scale * kLog2e;

  u32x4 b_k[D / 32], b_v[D / 32];
  load_own<D>(b_k, qkv + hq + E, 3 * E, row, N, q);
  load_own<D>(b_v, qkv + hq + 2 * E, 3 * E, row, N, q);
  f32x4 dk[D / 16] = {}, dv[D / 16] = {};

  const Walked<D> wk;
  u32x4 qreg[2], oreg[2];
  f32x2 streg = {0.f, 0.f};  // wave 0: the statistics of query q0 + lane
  float dlreg = 0.f;
  auto fetch_stats = [&](int q0) {
    const bool in = wave == 0 && q0 + lane < N;
    streg = in ? stats[hs + q0 + lane] : f32x2{0.f, 0.f};
    dlreg = in ? delta[hs + q0 + lane] : 0.f;
  };
  wk.fetch(qreg, qkv + hq, 3 * E, 0, N);
  wk.fetch(oreg, dout + ho, E, 0, N);
  fetch_stats(0);
  for (int q0 = 0; q0 < N; q0 += kBlk) {
    block_sync();
    wk.template put<true, true>(sQ, sQt, qreg);
    wk.template put<true, true>(sO, sOt, oreg);
    if (wave == 0)
      sSt[0][lane] = streg[0], sSt[1][lane] = streg[1], sSt[2][lane] = dlreg;
    block_sync();
    if (q0 + kBlk < N) {
      wk.fetch(qreg, qkv + hq, 3 * E, q0 + kBlk, N);
      wk.fetch(oreg, dout + ho, E, q0 + kBlk, N);
      fetch_stats(q0 + kBlk);
    }
    if (!active) continue;
    const int rows = min(kBlk, N - q0);
    const int nt = (rows + 15) >> 4, nw = (rows + 31) >> 5;
    f32x4 p4[4] = {}, ds4[4] = {};
    first_product<D>(p4, sQ, b_k, nt, r, q);   // S
    first_product<D>(ds4, sO, b_v, nt, r, q);  // dP
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(&sSt[0][16 * j + 4 * q]);
      const f32x4 il4 =
          *reinterpret_cast<const f32x4*>(&sSt[1][16 * j + 4 * q]);
      const f32x4 dl4 =
          *reinterpret_cast<const f32x4*>(&sSt[2][16 * j + 4 * q]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool live = row < N && j < nt && q0 + 16 * j + 4 * q + i < N;
        const float p =
            p_from_stats(p4[j][i], f32x2{m4[i], il4[i]}, c, live);
        p4[j][i] = p;
        ds4[j][i] = p * (ds4[j][i] - dl4[i]) * scale;
      }
    }
    const u32x4 pp[2] = {pack_pair(p4[0], p4[1]), pack_pair(p4[2], p4[3])};
    second_product<D>(dv, sOt, pp, nw, r, q);
    const u32x4 pd[2] = {pack_pair(ds4[0], ds4[1]), pack_pair(ds4[2], ds4[3])};
    second_product<D>(dk, sQt, pd, nw, r, q);
  }
  if (active) {
    store_own<D>(dqkv + hq + E, 3 * E, dk, row, N, 1.f, q);
    store_own<D>(dqkv + hq + 2 * E, 3 * E, dv, row, N, 1.f, q);
  }
}

struct AttnDims {
  int64_t B, N, H, D;
};

// The argument check shared by the forward and backward launchers of both
// families, complete before any launch.
AttnDims attn_check_args(const char* who, const torch::Tensor& qkv,
                         int64_t heads, int64_t max_n = kAttnMaxN) {
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
  TORCH_CHECK(N >= 1 && N <= max_n, who, " supports 1 <= N <= ", max_n,
              " tokens, got N = ", N);
  TORCH_CHECK(B * heads * ((N + kBlk - 1) / kBlk) <= INT32_MAX, who,
              ": B * heads exceeds the grid");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, who,
              ": qkv must be 16-byte aligned");
  return {B, N, heads, D};
}

// A [B, N, E] operand beside qkv (dout, out) and the forward's statistics.
void attn_check_slab(const char* who, const char* name, const torch::Tensor& t,
                     const torch::Tensor& qkv, const AttnDims& d) {
  TORCH_CHECK(t.defined() && t.device() == qkv.device() &&
                  t.scalar_type() == qkv.scalar_type(),
              who, ": ", name, " must have qkv's dtype and device");
  TORCH_CHECK(t.dim() == 3 && t.is_contiguous() && t.size(0) == d.B &&
                  t.size(1) == d.N && t.size(2) == d.H * d.D,
              who, ": ", name, " must be [B, N, E] = [", d.B, ", ", d.N, ", ",
              d.H * d.D, "] and contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, who, ": ",
              name, " must be 16-byte aligned");
}
void attn_check_stats(const char* who, const torch::Tensor& row_stats,
                      const torch::Tensor& qkv, const AttnDims& d) {
  TORCH_CHECK(row_stats.defined() && row_stats.device() == qkv.device() &&
                  row_stats.scalar_type() == at::kFloat &&
                  row_stats.is_contiguous() && row_stats.dim() == 4 &&
                  row_stats.size(0) == d.B && row_stats.size(1) == d.H &&
                  row_stats.size(2) == d.N && row_stats.size(3) == 2,
              who, ": row_stats must be the forward's f32 [B, H, N, 2] = [",
              d.B, ", ", d.H, ", ", d.N, ", 2] on qkv's device");
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
  attn_check_slab(who, "dout", dout, qkv, d);
  attn_check_stats(who, row_stats, qkv, d);
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

std::vector<torch::Tensor> attn_tiled_fwd(
    torch::Tensor qkv, int64_t heads, c10::optional<torch::Tensor> out_,
    c10::optional<torch::Tensor> row_stats_) {
  const char* who = "attn_tiled_fwd";
  const AttnDims d = attn_check_args(who, qkv, heads, kAttnTiledMaxN);
  auto out = attn_result(who, "out", out_, {d.B, d.N, d.H * d.D},
                         qkv.options());
  auto stats = attn_result(who, "row_stats", row_stats_, {d.B, d.H, d.N, 2},
                           qkv.options().dtype(at::kFloat));
  if (d.B == 0) return {out, stats};
  const float scale = 1.f / std::sqrt((float)d.D);
  const int nblk = cdiv(d.N, kBlk);
  DISPATCH_F32_BF16(qkv.scalar_type(), who, {
    with_head_dim(d.D, [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      hipLaunchKernelGGL((k_attn_tiled_fwd<scalar_t, D>),
                         dim3(d.B * d.H * nblk), dim3(256), 0, cur_stream(),
                         cdptr<scalar_t>(qkv), dptr<scalar_t>(out),
                         dptr<f32x2>(stats), (int)d.N, (int)d.H, nblk, scale);
    });
  });
  HIP_OK(hipGetLastError());
  return {out, stats};
}

torch::Tensor attn_tiled_bwd(torch::Tensor dout, torch::Tensor qkv,
                             torch::Tensor out, torch::Tensor row_stats,
                             int64_t heads,
                             c10::optional<torch::Tensor> dqkv_) {
  const char* who = "attn_tiled_bwd";
  const AttnDims d = attn_check_args(who, qkv, heads, kAttnTiledMaxN);
  attn_check_slab(who, "dout", dout, qkv, d);
  attn_check_slab(who, "out", out, qkv, d);
  attn_check_stats(who, row_stats, qkv, d);
  auto dqkv = attn_result(who, "dqkv", dqkv_, qkv.sizes(), qkv.options());
  if (d.B == 0) return dqkv;
  // rowsum(dO * O): written by the query-side kernel, read by the key-side one
  auto delta = torch::empty({d.B, d.H, d.N}, qkv.options().dtype(at::kFloat));
  const float scale = 1.f / std::sqrt((float)d.D);
  const int nblk = cdiv(d.N, kBlk);
  DISPATCH_F32_BF16(qkv.scalar_type(), who, {
    with_head_dim(d.D, [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      const dim3 grid(d.B * d.H * nblk);
      hipLaunchKernelGGL((k_attn_tiled_bwd_q<scalar_t, D>), grid, dim3(256), 0,
                         cur_stream(), cdptr<scalar_t>(qkv),
                         cdptr<scalar_t>(dout), cdptr<scalar_t>(out),
                         cdptr<f32x2>(row_stats), dptr<float>(delta),
                         dptr<scalar_t>(dqkv), (int)d.N, (int)d.H, nblk, scale);
      hipLaunchKernelGGL((k_attn_tiled_bwd_kv<scalar_t, D>), grid, dim3(256),
                         0, cur_stream(), cdptr<scalar_t>(qkv),
                         cdptr<scalar_t>(dout), cdptr<f32x2>(row_stats),
                         cdptr<float>(delta), dptr<scalar_t>(dqkv), (int)d.N,
                         (int)d.H, nblk, scale);
    });
  });
  HIP_OK(hipGetLastError());
  return dqkv;
}

namespace {

// The bf16 family's own limits, complete before any launch.
AttnDims attn_bf16_check_args(const char* who, const torch::Tensor& qkv,
                              int64_t heads) {
  TORCH_CHECK(qkv.defined() && qkv.is_cuda(), who, ": qkv must be on a GPU");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16, who,
              ": storage must be bf16 (the wide MFMA has no f32 form), got ",
              qkv.scalar_type());
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(), who,
              ": qkv must be [B, N, 3*E] and contiguous");
  TORCH_CHECK(heads >= 1 && qkv.size(2) % (3 * heads) == 0, who,
              ": the last dimension (", qkv.size(2),
              ") must be 3 * heads * D with heads = ", heads);
  const int64_t B = qkv.size(0), N = qkv.size(1);
  const int64_t D = qkv.size(2) / (3 * heads);
  TORCH_CHECK(D == 32 || D == 64, who,
              " supports head sizes 32 and 64, got D = ", D);
  TORCH_CHECK(N >= 1 && N <= kAttnTiledMaxN, who, " supports 1 <= N <= ",
              kAttnTiledMaxN, " tokens, got N = ", N);
  TORCH_CHECK(B * heads * ((N + kBlk - 1) / kBlk) <= INT32_MAX, who,
              ": B * heads exceeds the grid");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0, who,
              ": qkv must be 16-byte aligned");
  return {B, N, heads, D};
}

template <typename F>
void with_wide_head_dim(int64_t D, F&& f) {
  if (D == 32) f(std::integral_constant<int, 32>{});
  else f(std::integral_constant<int, 64>{});
}

}  // namespace

std::vector<torch::Tensor> attn_bf16_fwd(
    torch::Tensor qkv, int64_t heads, c10::optional<torch::Tensor> out_,
    c10::optional<torch::Tensor> row_stats_) {
  const char* who = "attn_bf16_fwd";
  const AttnDims d = attn_bf16_check_args(who, qkv, heads);
  auto out = attn_result(who, "out", out_, {d.B, d.N, d.H * d.D},
                         qkv.options());
  auto stats = attn_result(who, "row_stats", row_stats_, {d.B, d.H, d.N, 2},
                           qkv.options().dtype(at::kFloat));
  if (d.B == 0) return {out, stats};
  const float scale = 1.f / std::sqrt((float)d.D);
  const int nblk = cdiv(d.N, kBlk);
  with_wide_head_dim(d.D, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    hipLaunchKernelGGL((k_attn_bf16_fwd<D>), dim3(d.B * d.H * nblk), dim3(256),
                       0, cur_stream(), cdptr<bf16_t>(qkv), dptr<bf16_t>(out),
                       dptr<f32x2>(stats), (int)d.N, (int)d.H, nblk, scale);
  });
  HIP_OK(hipGetLastError());
  return {out, stats};
}

torch::Tensor attn_bf16_bwd(torch::Tensor dout, torch::Tensor qkv,
                            torch::Tensor out, torch::Tensor row_stats,
                            int64_t heads,
                            c10::optional<torch::Tensor> dqkv_) {
  const char* who = "attn_bf16_bwd";
  const AttnDims d = attn_bf16_check_args(who, qkv, heads);
  attn_check_slab(who, "dout", dout, qkv, d);
  attn_check_slab(who, "out", out, qkv, d);
  attn_check_stats(who, row_stats, qkv, d);
  auto dqkv = attn_result(who, "dqkv", dqkv_, qkv.sizes(), qkv.options());
  if (d.B == 0) return dqkv;
  // diag(O dO^T): written by the query-side kernel, read by the key-side one
  auto delta = torch::empty({d.B, d.H, d.N}, qkv.options().dtype(at::kFloat));
  const float scale = 1.f / std::sqrt((float)d.D);
  const int nblk = cdiv(d.N, kBlk);
  with_wide_head_dim(d.D, [&](auto dd) {
    constexpr int D = decltype(dd)::value;
    const dim3 grid(d.B * d.H * nblk);
    hipLaunchKernelGGL((k_attn_bf16_bwd_q<D>), grid, dim3(256), 0,
                       cur_stream(), cdptr<bf16_t>(qkv), cdptr<bf16_t>(dout),
                       cdptr<bf16_t>(out), cdptr<f32x2>(row_stats),
                       dptr<float>(delta), dptr<bf16_t>(dqkv), (int)d.N,
                       (int)d.H, nblk, scale);
    hipLaunchKernelGGL((k_attn_bf16_bwd_kv<D>), grid, dim3(256), 0,
                       cur_stream(), cdptr<bf16_t>(qkv), cdptr<bf16_t>(dout),
                       cdptr<f32x2>(row_stats), cdptr<float>(delta),
                       dptr<bf16_t>(dqkv), (int)d.N, (int)d.H, nblk, scale);
  });
  HIP_OK(hipGetLastError());
  return dqkv;
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
