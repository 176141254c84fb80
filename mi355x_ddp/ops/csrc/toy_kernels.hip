// Fused toy training-step kernels of the MI355X (gfx950, CDNA4) kernel pack:
// the reference hot loop (single_gpu.py:21-26) for model = Linear(K,1) as
// one single-wave launch per step (`k_toy_fused`) or per S steps (the
// multi-step trainers), with their selector and host launchers. Shared
// scaffolding is in kernel_common.h; the general kernels are in kernels.hip.
//
// Matmul compute is the exact-f32 MFMA `v_mfma_f32_16x16x4_f32` for f32
// storage and `v_mfma_f32_16x16x32_bf16` for bf16. The one exception is the
// fp32 world-1 multi-step fast path (batch 32/64, K 20):
// `k_toy_multistep_chain` runs the same k-ordered fmaf chains the f32 MFMA
// evaluates, bit for bit, on the vector ALU — one row (forward) / one
// column (backward) per lane, cross-lane hand-offs folded into the
// multiply-add as DPP row broadcasts (v_fmac_f32_dpp row_newbcast) —
// because those MFMA tiles discard 15/16 of their work on the serial
// critical path (profiles r03a, r03c). One wave computes; loader waves on
// the other SIMDs feed it through an LDS ring, one workgroup barrier per
// chunk of steps (profiles r03d).
// The MFMA spec kernel stays selectable (set_toy_multistep_impl /
// MI355X_TOY_MULTISTEP).
//
// Beyond parity (design notes in docs/KERNELS.md): the multi-step
// trainers (`k_toy_multistep_spec` for f32, `k_toy_multistep_bf16w` for
// bf16) run S sequential SGD steps per launch with LDS-resident weights;
// their MESH variants embed a per-step device-side xGMI all-reduce
// (p2p_mesh.h).
//
// Order: the generic tile step, k_toy_fused, k_toy_multistep; mesh_exchange,
// k_toy_multistep_spec, k_toy_multistep_bf16w; the chain kernel; the host.

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "kernel_common.h"
#include "ops.h"
#include "p2p_mesh.h"

namespace mi355x {

// ---------------------------------------------------------------------------
// The generic tile step (fwd + loss-grad + bwd) for any B <= 128, K <= 32,
// shared by k_toy_fused and k_toy_multistep so that S multi-steps equal S
// single-step launches bitwise by construction.
// MT = M-tiles (ceil(B/16), compile-time), KT = K-tiles (ceil(K/16)).
// Both MFMA phases run off LDS (xs [B][K], ts [B], ws = w (K) + bias at
// ws[32]) with the tile accumulators interleaved so the 40-cycle
// dependent-accumulator latency of v_mfma_f32_16x16x4_f32 hides behind the
// other tile's issue (cdna_hip_programming.md §3: >=2 independent
// accumulators reach the issue rate).
// Leaves dY in dy_s and the gradient tiles in gacc: D row j=0 lives in
// reg 0 of lanes with q==0, col k = tk*16 + r holds dw_k. Returns this
// lane's partial sum of squared residuals. bterm (= ws[32]) and mfma_db
// (= toy_mfma_db(K)) come from the caller, which needs both again for its
// update.
// ---------------------------------------------------------------------------

// db rides a FREE output column: when K is not a multiple of 16,
// column K of the bwd tile multiplies dY against a constant-1 operand,
// so the bias gradient falls out of the same MFMA chain — no LDS
// re-read, no wave_sum of 6 dependent cross-lane shuffles per step.
__device__ __forceinline__ bool toy_mfma_db(int K) { return (K & 15) != 0; }

// db when no free column exists (K a multiple of 16): wave sum of dY
__device__ __forceinline__ float toy_db_wave_sum(const float* dy_s, int B,
                                                 int lane) {
  float dbp = 0.f;
  for (int i = lane; i < B; i += 64) dbp += dy_s[i];
  return wave_sum(dbp);
}

template <int MT, int KT>
__device__ __forceinline__ float toy_tile_step(
    const float* xs, const float* ts, const float* ws, float* dy_s,
    float bterm, bool mfma_db, int B, int K, int use_mse, int r, int q,
    f32x4 (&gacc)[KT]) {
  // forward: y = X @ w + b; MT interleaved 16-row tiles, j=0 column only
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
  __syncthreads();  // dy_s visible to all lanes before the bwd MFMAs

  // backward: dw_k = sum_i dY_i X[i,k]; KT interleaved K-tiles; db = sum dY
#pragma unroll
  for (int tk = 0; tk < KT; ++tk) gacc[tk] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < B; i0 += 4) {
    const int i = i0 + q;
    const float a = (r == 0 && i < B) ? dy_s[i] : 0.f;  // A[j=0][i]
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      const float b = (i < B && k < K) ? xs[i * K + k]
                     : (i < B && k == K && mfma_db) ? 1.f : 0.f;
      gacc[tk] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, gacc[tk], 0, 0, 0);
    }
  }
  return loss_acc;
}

// ---------------------------------------------------------------------------
// Fused toy training step (fwd + loss-grad + bwd [+ SGD] in ONE kernel):
// the reference hot loop single_gpu.py:21-26 for model = Linear(K,1).
// Single workgroup, 64 threads (one wave): at 84 B of gradients the step is
// launch-latency bound, so one launch replaces five (SURVEY §7 hard-part 2).
// lr > 0: apply SGD in-kernel (world-1 path — no all-reduce exists);
// lr <= 0: write grads into the bucket for the all-reduce + sgd_flat path.
// Supports B <= 128, K <= 32.
// One coalesced LDS burst loads X, t, w, bias up front (one global round
// trip instead of per-MFMA dependent loads), then the tile step runs.
// ---------------------------------------------------------------------------
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

  const float bterm = ws[32];
  const bool mfma_db = toy_mfma_db(K);
  f32x4 acc[KT];
  float loss_acc = toy_tile_step<MT, KT>(xs, ts, ws, dy_s, bterm, mfma_db, B,
                                         K, use_mse, r, q, acc);
#pragma unroll
  for (int tk = 0; tk < KT; ++tk) {
    const int k = tk * 16 + r;
    if (q == 0 && k < K) {
      if (lr > 0.f) stf(&param[w_off + k], ws[k] - lr * acc[tk][0]);
      else stf(&grad[w_off + k], acc[tk][0]);
    } else if (q == 0 && k == K && mfma_db) {
      if (lr > 0.f) stf(&param[b_off], bterm - lr * acc[tk][0]);
      else stf(&grad[b_off], acc[tk][0]);
    }
  }
  if (!mfma_db) {
    const float dbp = toy_db_wave_sum(dy_s, B, lane);
    if (lane == 0) {
      if (lr > 0.f) stf(&param[b_off], bterm - lr * dbp);
      else stf(&grad[b_off], dbp);
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
// arithmetic is the SAME toy_tile_step as k_toy_fused, with the same update
// order and bf16 rounding of the stored params, so S multi-steps == S
// single-step launches bitwise; tests/test_engine_gpu.py holds it to that.
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

    const float bterm = ws[32];
    const bool mfma_db = toy_mfma_db(K);
    f32x4 acc[KT];
    const float loss_acc = toy_tile_step<MT, KT>(
        xs, ts, ws, dy_s, bterm, mfma_db, B, K, use_mse, r, q, acc);
    __syncthreads();  // all ws reads of this step done before the update
    // in-LDS SGD update
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (q == 0 && k < K)
        ws[k] = round_store<T>(ws[k] - lr * acc[tk][0]);
      else if (q == 0 && k == K && mfma_db)
        ws[32] = round_store<T>(bterm - lr * acc[tk][0]);
    }
    if (!mfma_db) {
      const float dbp = toy_db_wave_sum(dy_s, B, lane);
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

// Mesh arguments of the fast MFMA kernels; the defaults are the no-mesh
// call. The kernels take them loose (in a by-value struct the pointers lose
// __restrict__ and the MESH step loops gain loads) and bundle for
// mesh_exchange.
struct MeshArgs {
  MeshSlot* const* peer_slots = nullptr;
  MeshSlot* my_mb = nullptr;
  int world = 1;
  float inv_world = 1.f;
  unsigned long long seq0 = 0;
  unsigned int* err = nullptr;
};

// In-kernel mesh exchange for the multi-step trainers: scatter this
// rank's 21-float gradient vector (held one value per q==0 lane per
// K-tile, db on the free column) into every rank's mailbox, publish the
// sequence number of step s, bounded-wait for all peers, and return the
// averaged value for this lane's tile. Returns false on timeout (caller
// must set the error flag and exit).
template <int KT>
__device__ __forceinline__ bool mesh_exchange(float (&gval)[KT], int K_,
                                              int lane, int r, int q,
                                              const MeshArgs& m, int s) {
  const unsigned long long sq = m.seq0 + (unsigned long long)s;
  if (q == 0) {
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      if (k <= K_) {
        for (int p = 0; p < m.world; ++p) m.peer_slots[p]->data[k] = gval[tk];
      }
    }
  }
  __threadfence_system();
  __syncthreads();
  if (lane == 0) {
    for (int p = 0; p < m.world; ++p)
      __hip_atomic_store(&m.peer_slots[p]->seq, sq, __ATOMIC_RELEASE,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
  bool timed_out = false;
  if (lane < m.world) {
    const unsigned long long t0c = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(&m.my_mb[lane].seq, __ATOMIC_ACQUIRE,
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
        for (int p = 0; p < m.world; ++p) sum += m.my_mb[p].data[k];
        gval[tk] = sum * m.inv_world;
      }
    }
  }
  return true;
}

// ---------------------------------------------------------------------------
// Compile-time-shape f32 multi-step trainer for the canonical toy shape.
// All loop bounds are template constants so every MFMA operand lives in a
// REGISTER, prefetched from global memory in operand layout during the
// previous step's compute (the epoch shard is L2-resident after its
// gather, so the depth-1 prefetch covers the latency). LDS is used only
// where data must cross lanes: the w vector (updated by q==0 lanes, read
// by r==0 lanes) and the per-row dY exchange between the forward readout
// and the backward MFMA.
// ---------------------------------------------------------------------------
template <int B_, int K_, bool MESH = false>
__global__ void __launch_bounds__(64, 1)
k_toy_multistep_spec(const float* __restrict__ X, const float* __restrict__ Tg,
                     float* __restrict__ param, float* __restrict__ loss_out,
                     int S, int use_mse, int w_off, int b_off, float lr,
                     MeshSlot* const* __restrict__ peer_slots,
                     MeshSlot* __restrict__ my_mb, int mworld,
                     float minv_world, unsigned long long seq0,
                     unsigned int* __restrict__ mesh_err) {
  static_assert(B_ % 16 == 0, "whole 16-row tiles: rows carry no guards");
  constexpr int MT = B_ / 16;          // fwd 16-row tiles
  constexpr int KT = (K_ + 15) / 16;   // bwd 16-col tiles
  constexpr int KS = (K_ + 3) / 4;     // fwd k-steps
  constexpr int BS = B_ / 4;           // bwd i-steps
  const int lane = threadIdx.x;
  const int r = lane & 15, q = lane >> 4;
  __shared__ float ws[33];             // w (K_) + bias at ws[32]
  __shared__ float dy_s[B_];

  if (lane < K_) ws[lane] = param[w_off + lane];
  if (lane == K_) ws[32] = param[b_off];
  const float inv2B = 2.f / (float)B_;
  // updater lanes (q==0) also keep their w values in registers so the
  // end-of-iteration update is WRITE-only to LDS (no dependent LDS read
  // on the critical path); readers still take w from LDS
  float wreg[KT];
#pragma unroll
  for (int tk = 0; tk < KT; ++tk) {
    const int k = tk * 16 + r;
    wreg[tk] = (k < K_) ? param[w_off + ((k < K_) ? k : 0)] : 0.f;
  }

  // Per-lane operand registers, software-pipelined: `c*` hold the step
  // being computed and receive the next step's loads as soon as they are
  // dead (see below). Loads are raw (address-clamped, no value select):
  // lanes with k >= K_ load in-bounds garbage whose products are either
  // multiplied by a zeroed LDS-side operand (wv) or discarded by the
  // guarded ws writes — so no per-load mask, and therefore no vmcnt wait
  // until the next iteration's first MFMA use. (Ternary-guarded loads
  // compile to exec-masked branch-per-element code that serializes the
  // burst, seen in the r01b ISA.)
  float cfA[MT][KS];  // fwd A: X[tm*16+r][4*kk+q]
  float cbB[KT][BS];  // bwd B: X[4*ii+q][tk*16+r]
  float ctR[MT][4];   // targets for rows tm*16+q*4+i

  auto prefetch = [&](int s) {
    const float* Xs = X + (size_t)s * (B_ * K_);
    const float* Ts = Tg + (size_t)s * B_;
#pragma unroll
    for (int tm = 0; tm < MT; ++tm) {
      const int m = tm * 16 + r;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        const int k = 4 * kk + q;
        const int kc = (k < K_) ? k : K_ - 1;
        cfA[tm][kk] = Xs[m * K_ + kc];
      }
    }
#pragma unroll
    for (int tk = 0; tk < KT; ++tk) {
      const int k = tk * 16 + r;
      const int kc = (k < K_) ? k : K_ - 1;
#pragma unroll
      for (int ii = 0; ii < BS; ++ii) cbB[tk][ii] = Xs[(4 * ii + q) * K_ + kc];
    }
#pragma unroll
    for (int tm = 0; tm < MT; ++tm)
#pragma unroll
      for (int i = 0; i < 4; ++i) ctR[tm][i] = Ts[tm * 16 + q * 4 + i];
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
    // The squares are summed by one explicit fma per row: that is part of
    // the loss word's bits (k_toy_multistep_chain reproduces it), and left
    // to the compiler these unguarded rows become v_pk_mul + unfused adds
    // (as in k_toy_multistep_bf16w, whose loss word is thus the compiler's
    // choice and not bit-stable across compilers).
    float loss_acc = 0.f;
    if (r == 0) {
#pragma unroll
      for (int tm = 0; tm < MT; ++tm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float dy = 0.f;
          if (use_mse) {
            const float d = acc[tm][i] + bterm - ctR[tm][i];
            loss_acc = __builtin_fmaf(d, d, loss_acc);
            dy = d * inv2B;
          }
          dy_s[tm * 16 + q * 4 + i] = dy;
        }
    }
    __syncthreads();  // dy_s visible to all lanes

    // ---- backward: dw_k = sum_i dY_i X[i,k] ----
    float av[BS];
#pragma unroll
    for (int ii = 0; ii < BS; ++ii) {
      const float v = dy_s[4 * ii + q];  // unconditional read + select, as wv
      av[ii] = (r == 0) ? v : 0.f;
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
      const MeshArgs m{peer_slots, my_mb, mworld, minv_world, seq0, mesh_err};
      if (!mesh_exchange<KT>(gval, K_, lane, r, q, m, s)) {
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
        wreg[tk] = wreg[tk] - lr * gacc[tk][0];
        ws[k] = wreg[tk];
      } else if (q == 0 && k == K_) {
        ws[32] = bterm - lr * gacc[tk][0];
      }
    }
    __syncthreads();  // ws update visible before next iteration's forward
  }

  if (lane < K_) param[w_off + lane] = ws[lane];
  if (lane == K_) param[b_off] = ws[32];
  if (lane == 0 && loss_out) *loss_out = use_mse ? loss_last / (float)B_ : 0.f;
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
                      MeshSlot* const* __restrict__ peer_slots,
                      MeshSlot* __restrict__ my_mb, int mworld,
                      float minv_world, unsigned long long seq0,
                      unsigned int* __restrict__ mesh_err) {
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
      const MeshArgs m{peer_slots, my_mb, mworld, minv_world, seq0, mesh_err};
      if (!mesh_exchange<KT>(gval, K_, lane, r, q, m, s)) {
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
// row lanes, dy[i] to the column lanes), and they cost no instruction per
// term: the multiply-add itself reads the broadcast lane, as
// `v_fmac_f32_dpp acc, src, x row_newbcast:n` (first factor = lane n of
// the reading lane's own 16-lane row). Chain k lives in lane k — row 0
// holds k = 0..15, row 1 holds k = 16..19 and the bias/db lane 20 — so one
// v_permlane16_swap per hand-off (bcast_rows01) first copies the value's
// rows 0 and 1 into every row that reads them; at batch 64 a
// v_permlane32_swap in front also carries rows 2 and 3 down. The DPP reads
// need EXEC full, which holds through the whole step loop (no divergent
// branch; lanes 21..63 compute unused copies).
// That wave is bound by its own instruction issue, so it issues nothing
// but the chain and 14 (22 at batch 64) LDS reads per step: loader waves on
// the CU's other SIMDs fetch the tiles and stage them in an LDS ring, once
// row-major and once transposed (ChainSlot and the kernel's comment below).
// The compute wave keeps two operand register sets and fetches step s + 1
// from LDS while step s computes.
// ---------------------------------------------------------------------------

// Rows 0 and 1 (lanes 0..15, 16..31) of a per-lane value, each copied into
// BOTH rows of its half-wave: lo = {r0, r0, r2, r2}, hi = {r1, r1, r3, r3}.
// The builtin, not asm, so the compiler pads the swap's own hazards.
struct RowPair {
  float lo, hi;
};
// (v and v2 hold the same value: the swap works in place on two registers,
// and a caller that makes the two copies itself decides where they stand.)
__device__ __forceinline__ RowPair bcast_rows01(float v, float v2) {
  const auto r = __builtin_amdgcn_permlane16_swap(
      __float_as_uint(v), __float_as_uint(v2), false, false);
  return {__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ RowPair bcast_rows01(float v) {
  return bcast_rows01(v, v);
}
// Both half-waves of a per-lane value copied into both: lo = {r0, r1, r0,
// r1}, hi = {r2, r3, r2, r3}.
__device__ __forceinline__ RowPair bcast_halves(float v, float v2) {
  const auto r = __builtin_amdgcn_permlane32_swap(
      __float_as_uint(v), __float_as_uint(v2), false, false);
  return {__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ RowPair bcast_halves(float v) {
  return bcast_halves(v, v);
}

// acc = fmaf(src[lane n of the reader's row], x, acc): the same fused
// operation, operand order and rounding as the v_fmac_f32 the compiler
// selects for __builtin_fmaf; only where the first factor is read differs.
// The compiler does not fold a DPP broadcast into the fma by itself
// (update_dpp becomes v_mov_b32_dpp + v_fmac), hence asm; and one asm
// statement per term gets an s_nop between every two, hence whole runs of
// terms per statement (clang allows 30 operands). "+v" on the accumulator
// keeps the statements in chain order, and `volatile` keeps them where
// they stand among the step's other volatile statements and barriers: in
// straight-line code the scheduler otherwise pulls the next step's settle,
// barrier and fetch up between a step's forward and backward chains, into
// fresh registers and with a wait right behind the reads. The forward
// statement's memory clobber keeps the LDS reads issued ahead of it there.
#define BC_DPP(n) " row_newbcast:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define BC_FMAC(src, x, n) \
  "v_fmac_f32_dpp %[acc], %[" #src "], %[" #x "]" BC_DPP(n)
#define BC_FMAC4(src, p, n0, n1, n2, n3)                  \
  BC_FMAC(src, p##0, n0) BC_FMAC(src, p##1, n1)           \
  BC_FMAC(src, p##2, n2) BC_FMAC(src, p##3, n3)
#define BC_FMAC16(src, p)                                             \
  BC_FMAC4(src, p##0, 0, 1, 2, 3) BC_FMAC4(src, p##1, 4, 5, 6, 7)     \
  BC_FMAC4(src, p##2, 8, 9, 10, 11) BC_FMAC4(src, p##3, 12, 13, 14, 15)
#define BC_IN4(p, x)                                            \
  [p##0] "v"((x)[0]), [p##1] "v"((x)[1]), [p##2] "v"((x)[2]),   \
  [p##3] "v"((x)[3])
#define BC_IN16(p, x)                                     \
  BC_IN4(p##0, (x)) , BC_IN4(p##1, (x) + 4),              \
  BC_IN4(p##2, (x) + 8), BC_IN4(p##3, (x) + 12)
// gfx9 wants 2 wait states between a VALU write of a VGPR and a DPP read
// of it, and the hazard recogniser does not look inside asm: a statement
// that may directly follow the swap that wrote its DPP source pads itself.
// Every instruction of a lone wave costs an issue slot, an s_nop included
// (profiles r07a), so a statement that starts a chain spends the first
// wait state on zeroing its accumulator (BC_ZERO) instead of idling.
#define BC_PAD "s_nop 1\n\t"
#define BC_ZERO "v_mov_b32 %[acc], 0\n\ts_nop 0\n\t"

// The recogniser also takes every VGPR an asm statement writes for a
// dst_sel write, and puts a wait state in front of a VALU instruction that
// reads one right behind the statement. So the plain instructions that
// consume a chain's result stand inside its statement: the residual and
// the loss gradient behind the forward chain, the parameter update behind
// the last backward statement. They are the instructions the compiler
// selects for the same expressions (v_sub_f32, v_mul_f32 by the constant,
// and the one contracted v_fma_f32 of `w - lr * g`).

// forward: y = sum_k w[k] * x[k] from +0 in k order (w[0..15] in row 0 =
// w.lo, w[16..19] in row 1 = w.hi), then + bias (lane 20 = lane 4 of row 1);
// d = y - t, and with MSE dy = d * scale
template <bool MSE>
__device__ __forceinline__ void chain_fwd20(const RowPair& w,
                                            const float (&x)[20], float t,
                                            float scale, float& d,
                                            float& dy) {
  float acc;
  if constexpr (MSE) {
    asm volatile(BC_ZERO BC_FMAC16(lo, a) BC_FMAC4(hi, b, 0, 1, 2, 3)
                 "v_add_f32_dpp %[acc], %[hi], %[acc]" BC_DPP(4)
                 "v_sub_f32 %[d], %[acc], %[t]\n\t"
                 "v_mul_f32 %[dy], %[c], %[d]"
                 : [acc] "=&v"(acc), [d] "=&v"(d), [dy] "=&v"(dy)
                 : [lo] "v"(w.lo), [hi] "v"(w.hi), BC_IN16(a, x),
                   BC_IN4(b, x + 16), [t] "v"(t), [c] "s"(scale)
                 : "memory");
  } else {
    asm volatile(BC_ZERO BC_FMAC16(lo, a) BC_FMAC4(hi, b, 0, 1, 2, 3)
                 "v_add_f32_dpp %[acc], %[hi], %[acc]" BC_DPP(4)
                 "v_sub_f32 %[d], %[acc], %[t]"
                 : [acc] "=&v"(acc), [d] "=&v"(d)
                 : [lo] "v"(w.lo), [hi] "v"(w.hi), BC_IN16(a, x),
                   BC_IN4(b, x + 16), [t] "v"(t)
                 : "memory");
    dy = 0.f;
  }
}
// backward: 16 terms acc += src[n] * x[n], n = 0..15 in order. kStart
// begins the chain from +0 behind the swap that wrote src; kPad continues
// a chain behind such a swap; kPlain continues it 16 terms later, and
// chain_bwd16_update is kPlain followed by the update w = fma(-lr, acc, w).
enum ChainLink { kStart, kPad, kPlain };
template <ChainLink LINK>
__device__ __forceinline__ void chain_bwd16(float& acc, float src,
                                            const float* x) {
  if constexpr (LINK == kStart)
    asm volatile(BC_ZERO BC_FMAC16(s, a)
                 : [acc] "=&v"(acc)
                 : [s] "v"(src), BC_IN16(a, x));
  else if constexpr (LINK == kPad)
    asm volatile(BC_PAD BC_FMAC16(s, a)
                 : [acc] "+v"(acc)
                 : [s] "v"(src), BC_IN16(a, x));
  else
    asm volatile(BC_FMAC16(s, a)
                 : [acc] "+v"(acc)
                 : [s] "v"(src), BC_IN16(a, x));
}
__device__ __forceinline__ void chain_bwd16_update(float& acc, float src,
                                                   const float* x, float& w,
                                                   float lr) {
  asm volatile(BC_FMAC16(s, a) "v_fma_f32 %[w], -%[lr], %[acc], %[w]"
               : [acc] "+v"(acc), [w] "+v"(w)
               : [s] "v"(src), BC_IN16(a, x), [lr] "s"(lr));
}
#undef BC_ZERO
#undef BC_PAD
#undef BC_IN16
#undef BC_IN4
#undef BC_FMAC16
#undef BC_FMAC4
#undef BC_FMAC
#undef BC_DPP

// LDS slot of one training step, filled by the loader waves: the X tile
// twice (row-major for the forward, transposed for the backward) plus its
// targets. All in dwords.
//   row image   [B][K]        lane m reads row m as K/4 ds_read_b128; the
//                             80-byte pitch puts any 16 rows with distinct
//                             m mod 16 on 16 disjoint 4-bank groups
//   transposed  [K + 1][B + 4] lane k reads row k (= column k of X) as B/4
//                             ds_read_b128; the pitch (36 / 68 dwords)
//                             likewise spreads 16 rows with distinct
//                             k mod 16 over all 64 banks. Row K is the
//                             constant-ones column of db: written once per
//                             slot, never rewritten. Columns B..B+3 are
//                             padding, never read.
//   targets     [B]
// A ds_read_b128 is served in four groups of 16 lanes whose lane numbers
// are distinct mod 16, so both images read conflict-free as long as lane l
// reads row l or row l mod 16.
template <int B_, int K_>
struct ChainSlot {
  static constexpr int kPitch = B_ + 4;
  static constexpr int kRow = 0;
  static constexpr int kTr = B_ * K_;
  static constexpr int kOnes = kTr + K_ * kPitch;
  static constexpr int kTgt = kTr + (K_ + 1) * kPitch;
  static constexpr int kSize = kTgt + B_;  // 1428 (5712 B) / 2772 (11088 B)
  // two ring halves of H slots in 64 KB of static LDS: H <= 5 / H <= 2
  static constexpr int kMaxH = (64 * 1024 / 4) / kSize / 2;
  static_assert(kSize % 4 == 0 && kTr % 4 == 0 && kPitch % 4 == 0 &&
                    K_ % 4 == 0 && B_ % 4 == 0,
                "every ds_read_b128 must be 16-byte aligned");
};

// Tiles the loaders keep in registers ahead of the one they are writing to
// LDS. Their global loads stay in flight across the barriers, so the HBM
// latency (~900 cycles) hides behind kChainTilesAhead tiles of loader work.
static constexpr int kChainTilesAhead = 4;

// One workgroup of four waves, one per SIMD. Wave 0 computes; the waves
// whose bit is set in LMASK load; any other wave is parked (it executes the
// barriers and nothing else). The loaders stage each [B][K] tile (dword
// loads, so no alignment requirement on the base) into an LDS ring of two
// halves of H slots; the compute wave works through half c & 1 (chunk c =
// steps cH .. cH + H - 1) while the loaders fill the other half with chunk
// c + 1.
//
// Roles follow the wave index because SIMD placement does: a workgroup's
// waves go to SIMDs in the cyclic order 0 -> 2 -> 1 -> 3 from a start that
// varies per launch, so waves 0 and 2 always share one half of the CU's LDS
// store path (SIMDs {0,1} or {2,3}) and waves 1 and 3 the other (read back
// from HW_ID over 24 launches, profiles r09a). A loader on the compute
// wave's half puts its store traffic in the way of the compute wave's read
// addresses, so the loaders are waves 1 and 3 and wave 2 is the parked one.
//
// Loader lane-to-element map. A 32-lane group of a ds_write_b32 is served
// in one pass when it touches each of the 32 banks at most twice. In the
// transposed image (pitch = 4 mod 32 dwords) element (row, k) lies in bank
// (4 k + row) mod 32, so a group covers a block of 4 rows x 8 k (lane l:
// row l / 8, k l % 8: 32 distinct banks) for k < 16, and a block of 8 rows
// x 4 k (row l / 4, k 16 + l % 4: banks c .. c + 19, twelve of them twice)
// for k = 16..19. In the row image (bank (20 row + k) mod 32) the 4 x 8
// blocks hit four banks twice and the 8 x 4 blocks every bank once. The
// 2-way passes still count as LDS-array cycles (SQ_LDS_BANK_CONFLICT: 20
// per tile at batch 32, 36 with the flat-index walk, profiles r09a). The G = 2 NL groups of the loaders take G such blocks
// per element index i, stacked along the rows, so a lane's elements differ
// by compile-time constants in global memory and in both images. The price
// is global loads in 32-byte (16-byte) runs in place of 256-byte ones, on a
// tile of 2.5 KB that the loaders fetch four steps ahead.
//
// Barrier protocol. Barrier c (c = 0 .. NC - 1, NC = ceil(S / H)) is the
// only synchronisation, and every wave executes exactly NC of them, a
// function of S and H alone; no wave returns before its last one.
//   loaders   write chunk c, then arrive at barrier c
//   compute   arrives at barrier c just before its first LDS read of
//             chunk c, i.e. while step cH - 1 is still to be computed but
//             already sits in registers (the barrier's lgkmcnt(0))
// So passing barrier c tells the compute wave that chunk c is complete,
// and tells the loaders that every read of chunk c - 1 has returned: its
// half is free for chunk c + 1.
// Invariant: the loaders never address a tile index >= S, in global memory
// or in LDS. LDS writes are guarded on the step index; the slots the tail
// of the last chunk skips keep stale data that the compute wave, which
// reads steps < S only, never consumes. The run-ahead loads past the end
// re-read tile S - 1 into registers that are never written out.
static constexpr int kChainWaves = 4;
template <int B_, int K_, unsigned LMASK>
__global__ void __launch_bounds__(64 * kChainWaves)
k_toy_multistep_chain(const float* __restrict__ X,
                      const float* __restrict__ Tg,
                      float* __restrict__ param, float* __restrict__ loss_out,
                      int S, int H, int use_mse, int w_off, int b_off,
                      float lr) {
  constexpr int NL = __builtin_popcount(LMASK);  // loader waves
  constexpr int G = 2 * NL;                      // their 32-lane groups
  static_assert((B_ == 32 || B_ == 64) && K_ == 20 && (LMASK & 1u) == 0 &&
                    LMASK < (1u << kChainWaves) && (NL == 1 || NL == 2),
                "chain path: B in {32, 64}, K = 20, wave 0 computes, one or "
                "two of waves 1..3 load");
  static_assert((B_ / 4) % G == 0 && (B_ / 8) % G == 0,
                "the loader groups tile the rows exactly");
  using L = ChainSlot<B_, K_>;
  __shared__ __attribute__((aligned(16))) float ring[2 * L::kMaxH * L::kSize];
  // scalar wave index: the role branch is uniform, EXEC stays full
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));

  if (wave != 0 && !((LMASK >> wave) & 1u)) {
    // ---------------- parked wave ----------------
    const int NC = (S + H - 1) / H;
    for (int c = 0; c < NC; ++c) __syncthreads();
    return;
  }
  if (wave != 0) {
    // ---------------- loader waves ----------------
    // X dwords per lane and tile: NXA from the 4-row x 8-k blocks (k < 16),
    // NXB from the 8-row x 4-k blocks (k = 16..19)
    constexpr int RPI = B_ / 4 / G;  // 4-row blocks a lane has per 8 k
    constexpr int NXA = 2 * RPI, NXB = B_ / 8 / G, NX = NXA + NXB;
    static_assert(NX * 64 * NL == B_ * K_, "every element exactly once");
    constexpr int R = kChainTilesAhead;
    // thread index among the loaders: 64 x (rank of the wave in LMASK) + lane
    const int lt = 64 * __builtin_popcount(LMASK & ((1u << wave) - 1u)) +
                   (int)(threadIdx.x & 63);
    const int g = lt >> 5, l = lt & 31;
    const int rowA = 4 * g + (l >> 3), kA = l & 7;
    const int rowB = 8 * g + (l >> 2), kB = 16 + (l & 3);
    // element i of this lane as a dword offset in the [B][K] tile (the row
    // image is the tile itself) and in the transposed image; rows < B_ and
    // k < K_ by construction
    auto row_off = [&](int i) {
      return i < NXA ? (rowA + 4 * G * (i % RPI)) * K_ + kA + 8 * (i / RPI)
                     : (rowB + 8 * G * (i - NXA)) * K_ + kB;
    };
    auto tr_off = [&](int i) {
      return i < NXA
                 ? (kA + 8 * (i / RPI)) * L::kPitch + rowA + 4 * G * (i % RPI)
                 : kB * L::kPitch + rowB + 8 * G * (i - NXA);
    };
    const int total = (S + H - 1) / H * H;  // NC whole chunks
    float xv[R][NX], tv[R];

    // Loads are unconditional, so that the compiler can count them and
    // wait for exactly the oldest tile (a load inside a branch makes every
    // wait behind it a full drain). Past the end the tile index is clamped
    // to S - 1: those registers are never written to LDS.
    auto load_tile = [&](float (&x)[NX], float& t, int tile) {
      const int tc = tile < S ? tile : S - 1;
      const float* xt = X + (size_t)tc * (B_ * K_);
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = xt[row_off(i)];
      t = Tg[(size_t)tc * B_ + (lt & (B_ - 1))];
    };
    auto write_tile = [&](const float (&x)[NX], float t, int slot) {
      float* sl = ring + slot * L::kSize;
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        sl[L::kRow + row_off(i)] = x[i];
        sl[L::kTr + tr_off(i)] = x[i];
      }
      if (lt < B_) sl[L::kTgt + lt] = t;
    };

    // The first R tiles, issued tile by tile as the loop below issues them:
    // vmcnt counts in issue order, and left to itself the scheduler groups
    // these loads by address register across the tiles, after which the
    // loop's waits for "the oldest tile" drain most of the run-ahead
    // (vmcnt(16), (7), (3) where (23) .. (18) are meant; 186 ns/step
    // against 171 at batch 32). Nothing but the listing shows a relapse:
    // after a compiler change, look at the s_waitcnt vmcnt in front of the
    // ds_write_b32 of the loaders' tile loop (device-only -S -O3). Each of
    // the R unrolled tiles must wait with vmcnt(R (NX + 1) - 1) falling to
    // vmcnt((R - 1)(NX + 1)): 23 .. 18 at batch 32, 43 .. 33 at batch 64.
#pragma unroll
    for (int r = 0; r < R; ++r) {
      load_tile(xv[r], tv[r], r);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (lt < B_)
      for (int sl = 0; sl < 2 * H; ++sl) ring[sl * L::kSize + L::kOnes + lt] = 1.f;
    int slot = 0, togo = H;
    for (int t0 = 0; t0 < total; t0 += R) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int tile = t0 + r;
        if (tile < S) write_tile(xv[r], tv[r], slot);
        load_tile(xv[r], tv[r], tile + R);  // in flight across barriers
        slot = (slot + 1 == 2 * H) ? 0 : slot + 1;
        if (--togo == 0) {
          togo = H;
          if (tile < total) __syncthreads();  // barrier tile / H
        }
      }
    }
    return;
  }

  // ---------------- compute wave ----------------
  const int lane = threadIdx.x;
  const int mr = lane & (B_ - 1);  // row owned in the forward
  // transposed-image row read in the backward: column `lane` of X for
  // lanes < K_, the ones row for the db lane K_; the idle lanes above read
  // row lane mod 16 to stay off the live lanes' banks
  const int cr = (lane <= K_) ? lane : (lane & 15);
  const float inv2B = 2.f / (float)B_;
  // w[k] in lane k, bias in lane K_ (lanes above hold an unused copy)
  float wv = param[(lane < K_) ? w_off + lane : b_off];
  const float* rowp = ring + L::kRow + mr * K_;
  const float* colp = ring + L::kTr + cr * L::kPitch;
  const float* tgtp = ring + L::kTgt + mr;

  // One step's operands as they come out of LDS, 16 bytes per read
  struct LSet {
    f32x4 xr[K_ / 4];  // fwd: X[mr][0..K_)
    f32x4 xc[B_ / 4];  // bwd: X[0..B_)[lane] (ones on the db lane)
    float t;           // target of row mr
  };
  LSet setA, setB;

  // o = the slot's dword offset in the ring; a constant one folds into the
  // reads' immediate offsets
  auto fetch = [&](LSet& R, int o) {
#pragma unroll
    for (int j = 0; j < K_ / 4; ++j)
      R.xr[j] = *reinterpret_cast<const f32x4*>(rowp + o + 4 * j);
#pragma unroll
    for (int j = 0; j < B_ / 4; ++j)
      R.xc[j] = *reinterpret_cast<const f32x4*>(colp + o + 4 * j);
    R.t = tgtp[o];
  };
  // Pass a set's registers through empty asm statements before its step
  // starts and before the next set's reads are issued. Two things hang on
  // it. The compiler can no longer see the chains take the reads apart
  // dword by dword, so they stay ds_read_b128 (it otherwise splits some
  // into ds_read2_b32 pairs with an address add each). And the one
  // s_waitcnt of the step lands here, where everything outstanding was
  // issued a whole step ago, instead of behind the freshly issued reads.
  // (As few statements as clang's 30 asm operands allow: each one gets a
  // wait of its own.)
  auto settle = [&](LSet& R) {
    static_assert(K_ == 20, "five row reads");
    if constexpr (B_ == 64)
      asm volatile(""
                   : "+v"(R.xc[8]), "+v"(R.xc[9]), "+v"(R.xc[10]),
                     "+v"(R.xc[11]), "+v"(R.xc[12]), "+v"(R.xc[13]),
                     "+v"(R.xc[14]), "+v"(R.xc[15]));
    asm volatile(""
                 : "+v"(R.xr[0]), "+v"(R.xr[1]), "+v"(R.xr[2]), "+v"(R.xr[3]),
                   "+v"(R.xr[4]), "+v"(R.xc[0]), "+v"(R.xc[1]), "+v"(R.xc[2]),
                   "+v"(R.xc[3]), "+v"(R.xc[4]), "+v"(R.xc[5]), "+v"(R.xc[6]),
                   "+v"(R.xc[7]), "+v"(R.t)
                 :
                 : "memory");
  };

  struct CSet {
    float xr[K_];
    float xc[B_];
    float t;
  };
  // The forward swap's two copies of wv, made ahead of the step's fetch:
  // the reads then stand in the wait states between the copies and the
  // swap, where the compiler otherwise pads with an s_nop.
  float wa, wb;
  auto dup = [&] {
    wa = wv, wb = wv;
    asm volatile("" : "+v"(wa), "+v"(wb)::"memory");
  };
  float d_last = 0.f;
  // mse = std::bool_constant of the launch's use_mse: the choice is made
  // once around the step loops, not by a v_cndmask in every step
  auto compute = [&](const LSet& V, auto mse) {
    CSet R;
#pragma unroll
    for (int k = 0; k < K_; ++k) R.xr[k] = V.xr[k / 4][k % 4];
#pragma unroll
    for (int i = 0; i < B_; ++i) R.xc[i] = V.xc[i / 4][i % 4];
    R.t = V.t;
    // ---- forward: y = X @ w + b, k-ordered chain from +0 ----
    // rows 0/1 of wv reach every row that owns a batch row: rows 0..1 at
    // B_ = 32 (rows 2..3 run on copies of the bias, unused), all at 64
    RowPair w;
    if constexpr (B_ == 64) w = bcast_rows01(bcast_halves(wa, wb).lo);
    else w = bcast_rows01(wa, wb);
    // ---- loss grad, one row per lane: d = y - t, dy = d * 2/B (or 0) ----
    float d, dy;
    chain_fwd20<decltype(mse)::value>(w, R.xr, R.t, inv2B, d, dy);
    d_last = d;

    // ---- backward: dw_k = sum_i dY_i X[i,k]; db on the ones lane ----
    // dy[i] lives in lane i; the chains live in rows 0..1. Only the first
    // reader of each swap's pair pads: the second runs 16 terms later.
    float g;
    if constexpr (B_ == 64) {
      const RowPair h = bcast_halves(dy);
      const RowPair p01 = bcast_rows01(h.lo), p23 = bcast_rows01(h.hi);
      chain_bwd16<kStart>(g, p01.lo, R.xc);
      chain_bwd16<kPlain>(g, p01.hi, R.xc + 16);
      chain_bwd16<kPad>(g, p23.lo, R.xc + 32);
      chain_bwd16_update(g, p23.hi, R.xc + 48, wv, lr);
    } else {
      const RowPair p = bcast_rows01(dy);
      chain_bwd16<kStart>(g, p.lo, R.xc);
      chain_bwd16_update(g, p.hi, R.xc + 16, wv, lr);
    }
    // compiler-only ordering point between steps
    __builtin_amdgcn_wave_barrier();
  };

  // Step s lives in slot s mod 2H. `slot` is the slot of the next step to
  // fetch; entering a ring half (slot 0 or H) means entering a new chunk,
  // which is where the chunk's barrier goes.
  int slot = 0;
  int togo = 0;  // steps left to fetch in the current ring half
  const int slots = 2 * H;
  auto fetch_step = [&](LSet& R, int s) {
    if (s < S) {
      if (togo == 0) {
        __syncthreads();
        togo = H;
      }
      --togo;
      fetch(R, slot * L::kSize);
      slot = (slot + 1 == slots) ? 0 : slot + 1;
    }
  };
  // Step s + 1 is fetched while step s computes: even steps through setA,
  // odd steps through setB.
  asm volatile("" : "+v"(wv));  // the param load's wait, out of the loop
  fetch_step(setA, 0);
  int s = 0;

  // Whole turns of the ring, 2 HC steps with the depth a constant: the slot
  // offsets are immediates of the reads and the two barriers stand at fixed
  // places, so a step executes no bookkeeping and no branch at all. A turn
  // starts and ends in the state fetch_step(setA, 0) leaves (step s in
  // flight in setA from slot 0, slot = 1, togo = H - 1), runs only while
  // each of its steps has a successor to fetch (s + 2 HC < S), and executes
  // the barriers of the chunks it enters, exactly as the general loop
  // below does; that loop takes over for the last 1 .. 2 HC steps.
  auto turns = [&](auto hc) {
    constexpr int HC = decltype(hc)::value;
    for (; s + 2 * HC < S; s += 2 * HC) {
#pragma unroll
      for (int p = 0; p < HC; ++p) {
        constexpr int kTurn = 2 * HC;
        settle(setA);
        if ((2 * p + 1) % HC == 0) __syncthreads();
        dup();
        fetch(setB, (2 * p + 1) * L::kSize);
        compute(setA, std::true_type{});  // step s + 2 p
        settle(setB);
        if ((2 * p + 2) % HC == 0) __syncthreads();
        dup();
        fetch(setA, (2 * p + 2) % kTurn * L::kSize);
        compute(setB, std::true_type{});  // step s + 2 p + 1
      }
    }
  };
  auto steps = [&](auto mse) {
    for (; s < S; s += 2) {
      settle(setA);
      dup();
      fetch_step(setB, s + 1);
      compute(setA, mse);  // step s
      if (s + 1 < S) {
        settle(setB);
        dup();
        fetch_step(setA, s + 2);
        compute(setB, mse);  // step s + 1
      }
    }
  };
  if (use_mse) {
    if (H == 2) turns(std::integral_constant<int, 2>{});
    if constexpr (L::kMaxH >= 4) {
      if (H == 3) turns(std::integral_constant<int, 3>{});
      if (H == 4) turns(std::integral_constant<int, 4>{});
    }
    steps(std::true_type{});
  } else {
    // the degenerate cross-entropy path (dy = 0 whatever d is): general
    // loop only
    steps(std::false_type{});
  }

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
              "chain ring depth (steps per ring half) must be 0 (default), "
              "2, 3 or 4");
  g_chain_depth.store((int)depth);
}

// The chain depth is H, the steps per ring half (one barrier per H steps),
// a runtime kernel argument clamped to what 64 KB of LDS holds (5 at batch
// 32, 2 at batch 64). Measured at batch 32 with the loaders below (profiles
// r09a), H = 2 / 3 / 4: S = 1024 -> 172 / 167 / 166 ns/step, S = 64 -> 206 /
// 204 / 208 (a launch cannot start before its first H tiles are staged),
// S <= 32 equal within the spread of a launch. Up to r07a the depth bought
// 1 to 3 ns and the default was 2; with the loaders' stores out of the
// compute wave's way what is left at H = 2 is a loader arriving late at a
// barrier now and then, which a third slot per half absorbs. Batch 64 holds
// two.
static constexpr int kChainDefaultH = 3;
// The loader set, as a mask of wave indices: waves 1 and 3, the two that
// never share the compute wave's half of the LDS store path (the kernel's
// comment). Measured (r09a), S = 1024 / 64, ns/step at H = 2:
//   batch 32   waves {1,3} 172 / 206   {1,2} 174 / 207   {1} 189 / 224
//   batch 64   waves {1,3} 286 / 322   {1,2} 292 / 328   {1} 283 / 325
// One loader wave keeps up at batch 64 (a step is 670 cycles there) and not
// at batch 32; two are kept at both, for batch 64's short launches. A third
// loader would have to be wave 2: with the old store map that gave 180 / 215
// and 297 / 336.
static constexpr unsigned kChainLoaders32 = 0b1010;
static constexpr unsigned kChainLoaders64 = 0b1010;

template <int B_>
static void launch_toy_multistep_chain(const float* xp, const float* tp,
                                       float* pp, float* lossp, bool use_mse,
                                       int w_off, int b_off, float lr, int S) {
  constexpr int kMaxH = ChainSlot<B_, 20>::kMaxH;
  static_assert(kMaxH >= 2, "the ring needs two steps per half");
  int H = g_chain_depth.load();
  if (H == 0) H = kChainDefaultH;
  if (H > kMaxH) H = kMaxH;
  constexpr unsigned LM = B_ == 64 ? kChainLoaders64 : kChainLoaders32;
  hipLaunchKernelGGL((k_toy_multistep_chain<B_, 20, LM>), dim3(1),
                     dim3(64 * kChainWaves), 0, cur_stream(), xp, tp, pp,
                     lossp, S, H, use_mse ? 1 : 0, w_off, b_off, lr);
}

// fn(integral_constant<int, B>) for the two fast-path batch sizes
template <typename F>
static void with_fast_batch(int B, F&& fn) {
  if (B == 32) fn(std::integral_constant<int, 32>{});
  else fn(std::integral_constant<int, 64>{});
}

// The fast MFMA multi-step kernels (batch 32/64, K 20): native bf16 MFMA
// (16x16x32, whole contraction in one MFMA per tile; the batch-64 backward
// as two chained chunks) for bf16 storage, the f32 spec kernel otherwise.
template <typename T, int B_, bool MESH>
static void launch_toy_multistep_mfma(const T* xp, const T* tp, T* pp,
                                      float* lossp, bool use_mse, int w_off,
                                      int b_off, float lr, int S,
                                      const MeshArgs& m = {}) {
  auto kptr = [] {
    if constexpr (std::is_same<T, __hip_bfloat16>::value)
      return &k_toy_multistep_bf16w<B_, 20, MESH>;
    else
      return &k_toy_multistep_spec<B_, 20, MESH>;
  }();
  hipLaunchKernelGGL(kptr, dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp,
                     lossp, S, use_mse ? 1 : 0, w_off, b_off, lr, m.peer_slots,
                     m.my_mb, m.world, m.inv_world, m.seq0, m.err);
}

// (B, K) -> the (MT, KT) instantiation of the generic kernels: calls
// fn(integral_constant MT, integral_constant KT), MT in {1, 2, 4, 8} and
// KT in {1, 2} the smallest that cover ceil(B/16) and ceil(K/16).
template <typename F>
static void with_toy_tiles(int B, int K, F&& fn) {
  using c1 = std::integral_constant<int, 1>;
  using c2 = std::integral_constant<int, 2>;
  using c4 = std::integral_constant<int, 4>;
  using c8 = std::integral_constant<int, 8>;
  const int mt = (B + 15) / 16, kt = (K + 15) / 16;
  auto by_mt = [&](auto ktc) {
    if (mt <= 1) fn(c1{}, ktc);
    else if (mt <= 2) fn(c2{}, ktc);
    else if (mt <= 4) fn(c4{}, ktc);
    else fn(c8{}, ktc);
  };
  if (kt <= 1) by_mt(c1{});
  else by_mt(c2{});
}

// validated pointer for the optional f32 loss output (nullptr: not wanted)
static float* loss_ptr(const torch::Tensor& loss_out) {
  if (!loss_out.defined() || !loss_out.numel()) return nullptr;
  TORCH_CHECK(loss_out.scalar_type() == at::kFloat, "loss_out must be f32");
  return loss_out.data_ptr<float>();
}

// The one argument check of every toy entry point (toy_fused_fwd_bwd,
// toy_multistep, toy_multistep_mesh, ToyShardRun::bind_shard), run to the
// end BEFORE anything is launched or any other state is touched: the
// kernels take raw pointers and offsets on trust, so whatever passes here
// must keep every device access inside the tensors given.
//   batch < 0   the whole of x is one batch (the single step)
//   grad        nullptr: the entry point has no gradient bucket. Otherwise
//               checked like param when given (defined and not empty),
//               and required (need_grad) where the kernel writes it: the
//               single step with lr <= 0.
//   loss_out    undefined or empty: no loss wanted; else f32, >= 1 element
// Returns (B, K, S); S == 0 (no rows) means nothing to launch.
ToyDims toy_check_args(const char* who, const torch::Tensor& x,
                       const torch::Tensor& t, const torch::Tensor& param,
                       const torch::Tensor* grad, bool need_grad,
                       const torch::Tensor& loss_out, int64_t w_off,
                       int64_t b_off, int64_t batch) {
  TORCH_CHECK(x.defined() && t.defined() && param.defined(), who,
              ": x, t and param_flat must be tensors");
  TORCH_CHECK(x.is_cuda(), who, ": x must be on a GPU");
  const auto dev = x.device();
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), who,
              ": x must be [rows, K] and contiguous");
  const int64_t rows = x.size(0), K = x.size(1);
  TORCH_CHECK(t.device() == dev && t.scalar_type() == dt && t.is_contiguous() &&
                  t.numel() == rows,
              who, ": t must be contiguous, one target per row of x, with "
              "x's dtype and device");
  TORCH_CHECK(K >= 1 && K <= 32, who, " supports 1 <= K <= 32, got K = ", K);
  if (batch < 0) batch = rows > 0 ? rows : 1;
  TORCH_CHECK(batch >= 1 && batch <= 128, who,
              " supports 1 <= batch <= 128, got batch = ", batch);
  TORCH_CHECK(rows % batch == 0 && rows / batch <= INT32_MAX, who,
              ": x rows must be a multiple of batch");
  auto check_bucket = [&](const torch::Tensor& b, const char* name) {
    TORCH_CHECK(b.device() == dev && b.scalar_type() == dt &&
                    b.is_contiguous(),
                who, ": ", name, " must be contiguous with x's dtype and device");
    const int64_t n = b.numel();
    TORCH_CHECK(n <= INT32_MAX && w_off >= 0 && b_off >= 0 &&
                    w_off + K <= n && b_off < n,
                who, ": w_off/b_off with K = ", K, " fall outside ", name,
                " (", n, " elements)");
    TORCH_CHECK(b_off < w_off || b_off >= w_off + K, who,
                ": b_off lies inside the weights [w_off, w_off + K)");
  };
  check_bucket(param, "param_flat");
  if (grad != nullptr) {
    // "not given" is an undefined or an empty tensor, as for loss_out
    const bool given = grad->defined() && grad->numel() > 0;
    TORCH_CHECK(given || !need_grad, who,
                ": lr <= 0 writes the gradients: grad_flat is required");
    if (given) check_bucket(*grad, "grad_flat");
  }
  if (loss_out.defined() && loss_out.numel() > 0)
    TORCH_CHECK(loss_out.device() == dev &&
                    loss_out.scalar_type() == at::kFloat,
                who, ": loss_out must be f32 on x's device");
  return {(int)batch, (int)K, (int)(rows / batch)};
}

template <typename T>
static void launch_toy_multistep(const T* xp, const T* tp, T* pp, float* lossp,
                                 bool use_mse, int w_off, int b_off, float lr,
                                 int B, int K, int S) {
  if ((B == 32 || B == 64) && K == 20) {  // compile-time fast paths
    with_fast_batch(B, [&](auto b) {
      constexpr int B_ = decltype(b)::value;
      if constexpr (std::is_same<T, float>::value) {
        if (multistep_impl().load() == kImplChain) {
          launch_toy_multistep_chain<B_>(xp, tp, pp, lossp, use_mse, w_off,
                                         b_off, lr, S);
          return;
        }
      }
      launch_toy_multistep_mfma<T, B_, false>(xp, tp, pp, lossp, use_mse,
                                              w_off, b_off, lr, S);
    });
    return;
  }
  with_toy_tiles(B, K, [&](auto mt, auto kt) {
    hipLaunchKernelGGL((k_toy_multistep<T, decltype(mt)::value, decltype(kt)::value>),
                       dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp, lossp,
                       B, K, S, use_mse ? 1 : 0, w_off, b_off, lr);
  });
}

void toy_multistep_launch(const void* x, const void* t, void* param,
                          float* loss, bool use_mse, int w_off, int b_off,
                          float lr, int B, int K, int S, bool bf16) {
  if (bf16) {
    using T = __hip_bfloat16;
    launch_toy_multistep<T>(static_cast<const T*>(x), static_cast<const T*>(t),
                            static_cast<T*>(param), loss, use_mse, w_off,
                            b_off, lr, B, K, S);
  } else {
    launch_toy_multistep<float>(static_cast<const float*>(x),
                                static_cast<const float*>(t),
                                static_cast<float*>(param), loss, use_mse,
                                w_off, b_off, lr, B, K, S);
  }
  HIP_OK(hipGetLastError());
}

float* toy_loss_ptr(const torch::Tensor& loss_out) { return loss_ptr(loss_out); }

void toy_multistep(torch::Tensor x, torch::Tensor t, torch::Tensor param_flat,
                   torch::Tensor loss_out, bool use_mse,
                   int64_t w_off, int64_t b_off, double lr, int64_t batch) {
  TORCH_CHECK(batch >= 1, "toy_multistep: batch must be >= 1");
  const ToyDims d = toy_check_args("toy_multistep", x, t, param_flat, nullptr,
                                   false, loss_out, w_off, b_off, batch);
  TORCH_CHECK((float)lr > 0.f,
              "toy_multistep is the world-1 in-kernel-SGD path: lr must be > 0");
  if (d.S == 0) return;
  toy_multistep_launch(x.data_ptr(), t.data_ptr(), param_flat.data_ptr(),
                       loss_ptr(loss_out), use_mse, (int)w_off, (int)b_off,
                       (float)lr, d.B, d.K, d.S,
                       x.scalar_type() == at::kBFloat16);
}

void toy_check_mesh_args(const char* who, const ToyDims& d,
                         const P2pMesh& mesh) {
  TORCH_CHECK((d.B == 32 || d.B == 64) && d.K == 20, who,
              ": mesh multistep supports the fast-path shapes "
              "(batch 32 or 64, K 20)");
  TORCH_CHECK(mesh.connected(), who, ": the mesh is not connected");
}

void toy_multistep_mesh_launch(const void* x, const void* t, void* param,
                               float* loss, bool use_mse, int w_off,
                               int b_off, float lr, int B, int S, bool bf16,
                               P2pMesh& mesh) {
  // the sequence range is taken here, where nothing can refuse the launch
  // any more: one taken for a launch that never happens would desynchronise
  // the ranks
  const MeshArgs m{mesh.peer_slots(), mesh.my_mb(), mesh.world(),
                   1.f / (float)mesh.world(),
                   mesh.alloc_seq((unsigned long long)S), mesh.err_flag()};
  auto go = [&](auto zero) {
    using T = decltype(zero);
    with_fast_batch(B, [&](auto b) {
      launch_toy_multistep_mfma<T, decltype(b)::value, true>(
          static_cast<const T*>(x), static_cast<const T*>(t),
          static_cast<T*>(param), loss, use_mse, w_off, b_off, lr, S, m);
    });
  };
  if (!bf16) go(float{});
  else go(__hip_bfloat16{});
  HIP_OK(hipGetLastError());
}

void toy_multistep_mesh(torch::Tensor x, torch::Tensor t,
                        torch::Tensor param_flat, torch::Tensor loss_out,
                        bool use_mse, int64_t w_off, int64_t b_off, double lr,
                        int64_t batch, P2pMesh& mesh) {
  // everything is checked before the mesh is touched
  TORCH_CHECK(batch >= 1, "toy_multistep_mesh: batch must be >= 1");
  const ToyDims d = toy_check_args("toy_multistep_mesh", x, t, param_flat,
                                   nullptr, false, loss_out, w_off, b_off,
                                   batch);
  TORCH_CHECK((float)lr > 0.f,
              "mesh multistep applies SGD in-kernel: lr must be > 0");
  toy_check_mesh_args("toy_multistep_mesh", d, mesh);
  if (d.S == 0) return;
  toy_multistep_mesh_launch(x.data_ptr(), t.data_ptr(), param_flat.data_ptr(),
                            loss_ptr(loss_out), use_mse, (int)w_off,
                            (int)b_off, (float)lr, d.B, d.S,
                            x.scalar_type() == at::kBFloat16, mesh);
}

template <typename T>
static void launch_toy_fused(const torch::Tensor& x, const torch::Tensor& t,
                             torch::Tensor& param_flat, torch::Tensor& grad_flat,
                             float* lossp, bool use_mse, int w_off, int b_off,
                             float lr, int B, int K) {
  const T* xp = cdptr<T>(x);
  const T* tp = cdptr<T>(t);
  T* pp = dptr<T>(param_flat);
  // not given (lr > 0 only, checked): the kernel never touches it
  T* gp = grad_flat.defined() && grad_flat.numel() ? dptr<T>(grad_flat)
                                                   : nullptr;
  with_toy_tiles(B, K, [&](auto mt, auto kt) {
    hipLaunchKernelGGL((k_toy_fused<T, decltype(mt)::value, decltype(kt)::value>),
                       dim3(1), dim3(64), 0, cur_stream(), xp, tp, pp, gp,
                       lossp, B, K, use_mse ? 1 : 0, w_off, b_off, lr);
  });
}

void toy_fused_fwd_bwd(torch::Tensor x, torch::Tensor t,
                       torch::Tensor param_flat, torch::Tensor grad_flat,
                       torch::Tensor loss_out, bool use_mse,
                       int64_t w_off, int64_t b_off, double lr) {
  // the kernel chooses its branch on the f32 lr: one that rounds to zero
  // writes gradients like any lr <= 0
  const ToyDims d = toy_check_args("toy_fused_fwd_bwd", x, t, param_flat,
                                   &grad_flat, !((float)lr > 0.f), loss_out,
                                   w_off, b_off, -1);
  if (d.S == 0) return;
  const int B = d.B, K = d.K;
  float* lossp = loss_ptr(loss_out);
  DISPATCH_F32_BF16(x.scalar_type(), "toy_fused_fwd_bwd", {
    launch_toy_fused<scalar_t>(x, t, param_flat, grad_flat, lossp, use_mse,
                               (int)w_off, (int)b_off, (float)lr, B, K);
  });
  HIP_OK(hipGetLastError());
}

}  // namespace mi355x
