// Implicit-GEMM convolutions on the MFMA tile step of gemm_tile.h, for the
// 1x1 and 3x3 convolutions of a channels-last ResNet on gfx950 (MI355X):
// stride 1 or 2, padding k/2, no bias, no groups, no dilation; forward, input
// gradient and weight gradient.
//
// Activations are the 2-D channels-last matrices HipBatchNorm2d produces and
// consumes: x [N*H*W, Cin], y and dy [M, Cout] with M = N*Ho*Wo and
// Ho = (H + 2p - k)/s + 1. The weight is read PACKED, Wp [Cout, k*k, Cin]
// (tap-major, channels contiguous), and its gradient is stored straight into
// the parameter's own [Cout, Cin, k, k] layout. Storage T is f32 or bf16,
// alike for all operands; accumulation is f32 with one rounding on the store
// (v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x32_bf16, as k_gemm_tile).
//
//   k_conv_fwd         Y[M, Cout]      = sum_{tap, ci} x[pix(m, tap), ci] Wp[co, tap, ci]
//   k_conv_bwd_input   dX[N*H*W, Cin]  = sum_{tap, co} dy[opix(row, tap), co] Wp[co, tap, ci]
//   k_conv_bwd_weight  ws[g, co, tap, ci] = sum_{m in slice g} dy[m, co] x[pix(m, tap), ci]
//   k_conv_wgrad_finish  dW[co, ci, tap] = round(sum_g ws[g, co, tap, ci])
//
// Work split. 256 threads own a 128 x 128 tile of the output matrix, the four
// waves 2 x 2 on it, and walk the contraction in blocks of 32: tap by tap and
// inside a tap by 32 channels (forward, input gradient), or by 32 output
// pixels of one tap (weight gradient). The weight gradient's output is small
// and its contraction long, so it is split along M into GS slices
// (conv_wgrad_plan, a function of the shape alone); every workgroup stores
// its whole f32 tile into the workspace and k_conv_wgrad_finish adds the
// slices in slice order. No atomics and nothing pre-zeroed anywhere: the same
// bits run to run.
//
// The gather. A thread owns Geo<T>::NP row slots of an operand. For a
// gathered operand it splits each slot's row into (n, ho, wo) ONCE, ahead of
// the contraction loop, and keeps the image's first pixel and the tap-free
// part of the source coordinates; per tap the source pixel is an add and two
// range tests. The weight gradient's rows are contraction indices that move
// by 32 every block: its (n, ho, wo) advance by the split of 32, which the
// host passes in, with one carry each. No division runs in any loop.
// Loads are branch-free. A pixel that is padding, past the last row or (input
// gradient) off the stride grid gets pixel 0 of the same tensor as its
// ADDRESS and zero as its VALUE, by a select on the way into LDS; a channel
// chunk past the operand's width gets the first chunk of the same tap. No
// address outside an operand is formed. The loads of block k+1 are issued
// ahead of the MFMAs of block k; one LDS stage, two barriers per block.
//
// LDS images and pitches are k_gemm_tile's (gemm_kernels.hip): the gathered
// forward/input-gradient operand and the forward's Wp are "straight", Wp in
// the input gradient (contraction index co is Wp's ROW, the chunk runs along
// ci at column tap*Cin + ci0, row pitch k*k*Cin) and both operands of the
// weight gradient are "transposed" (bf16: transposed while storing).
#include <algorithm>

#include "gemm_tile.h"
#include "ops.h"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace mi355x {

namespace {

// Workgroups the weight gradient aims at (two per CU of an MI355X), and the
// shortest slice of output pixels worth a workgroup of its own.
constexpr int64_t kConvWgradTargetGrid = 512;
constexpr int64_t kConvWgradMinSlice = 256;

// The problem as the kernels see it. d_n, d_h, d_w: 32 = d_n*Ho*Wo + d_h*Wo +
// d_w, the step of the weight gradient's contraction rows; L: its rows per
// slice (a multiple of 32). Row counts are below 2^31 but a tile may reach
// past them, so rows are compared as unsigned numbers.
struct ConvGeo {
  int N, H, W, Cin, Cout, Ho, Wo, k, stride, pad, taps, M;
  int d_n, d_h, d_w, L;
};

__device__ __forceinline__ u32x4 ld16(const void* p) {
  return *reinterpret_cast<const u32x4*>(p);
}
__device__ __forceinline__ u32x4 zero4() { return u32x4{0u, 0u, 0u, 0u}; }

// The rows of a straight operand that are pixels of an output-shaped index
// space, gathered tap by tap from a channels-last source of C channels.
// BWD false: rows are output pixels (n, ho, wo), the source is x and tap
// (r, q) reads pixel (ho*s - p + r, wo*s - p + q) where that is inside.
// BWD true: rows are input pixels (n, h, w), the source is dy and tap (r, q)
// reads pixel ((h + p - r)/s, (w + p - q)/s) where both quotients are exact
// and inside.
template <typename T, bool BWD>
struct GatherRows {
  using G = Geo<T>;
  const T* src;
  int C, SH, SW;  // the source's channels, height and width
  int sh;         // stride - 1
  int col;        // the thread's chunk column, in elements
  int base[G::NP], hh[G::NP], ww[G::NP];
  unsigned live;  // bit j: slot j is a row of the problem
  unsigned mask;  // bit j: the chunk in v[j] is data, not a clamped address
  u32x4 v[G::NP];

  // rows: the index space is [n][RH][RW]; row0 the tile's first row.
  __device__ __forceinline__ void init(const T* s, const ConvGeo& g,
                                       const TileMap<T, false>& m, int row0) {
    src = s, sh = g.stride - 1, col = m.c * G::E, live = 0, mask = 0;
    const int RH = BWD ? g.H : g.Ho, RW = BWD ? g.W : g.Wo;
    const int rows = g.N * RH * RW;
    C = BWD ? g.Cout : g.Cin, SH = BWD ? g.Ho : g.H, SW = BWD ? g.Wo : g.W;
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      const unsigned row = (unsigned)row0 + (unsigned)m.slot_row(j);
      const bool ok = row < (unsigned)rows;
      const int rr = ok ? (int)row : 0;
      const int n = rr / (RH * RW), rem = rr - n * (RH * RW);
      const int h = rem / RW, w = rem - h * RW;
      base[j] = n * SH * SW;
      hh[j] = BWD ? h + g.pad : h * g.stride - g.pad;
      ww[j] = BWD ? w + g.pad : w * g.stride - g.pad;
      live |= (unsigned)ok << j;
    }
  }
  __device__ __forceinline__ void load(int r, int q, int c0) {
    const bool colok = c0 + col < C;
    const int cc = colok ? c0 + col : 0;
    mask = 0;
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      int sy, sx;
      bool ok = (live >> j) & 1u;
      if constexpr (BWD) {
        const int ty = hh[j] - r, tx = ww[j] - q;
        ok = ok && ty >= 0 && tx >= 0 && ((ty | tx) & sh) == 0;
        sy = ty >> sh, sx = tx >> sh;
      } else {
        sy = hh[j] + r, sx = ww[j] + q;
        ok = ok && sy >= 0 && sx >= 0;
      }
      ok = ok && sy < SH && sx < SW;
      const int pix = ok ? base[j] + sy * SW + sx : 0;
      v[j] = ld16(src + (int64_t)pix * C + cc);
      mask |= (unsigned)(ok && colok) << j;
    }
  }
  __device__ __forceinline__ void store(uint32_t* img,
                                        const TileMap<T, false>& m) const {
    u32x4 x[G::NP];
#pragma unroll
    for (int j = 0; j < G::NP; ++j) x[j] = (mask >> j) & 1u ? v[j] : zero4();
    m.template store<false>(img, x, nullptr);
  }
};

// The packed weight as an operand of the forward (TR false: rows co, chunks
// along ci) or of the input gradient (TR true: contraction rows co, chunks
// along the outputs ci). out0: the tile's first output.
template <typename T, bool TR>
struct WeightOp {
  using G = Geo<T>;
  const T* src;
  int Cin, Cout, out0, col;
  int64_t ld;  // k*k*Cin
  unsigned mask;
  u32x4 v[G::NP];

  __device__ __forceinline__ void init(const T* s, const ConvGeo& g,
                                       const TileMap<T, TR>& m, int o0) {
    src = s, Cin = g.Cin, Cout = g.Cout, out0 = o0, col = m.c * G::E;
    ld = (int64_t)g.taps * g.Cin, mask = 0;
  }
  // tap: r*k + q; c0: first channel (TR false: ci, TR true: co) of the block
  __device__ __forceinline__ void load(const TileMap<T, TR>& m, int tap,
                                       int c0) {
    mask = 0;
    // the chunk's ci, and whether it exists
    const int ci = TR ? out0 + col : c0 + col;
    const bool ciok = ci < Cin;
    const int64_t coff = (int64_t)tap * Cin + (ciok ? ci : 0);
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      const int co = (TR ? c0 : out0) + m.slot_row(j);
      const bool ok = co < Cout;
      v[j] = ld16(src + (int64_t)(ok ? co : Cout - 1) * ld + coff);
      mask |= (unsigned)(ok && ciok) << j;
    }
  }
  __device__ __forceinline__ void store(uint32_t* img,
                                        const TileMap<T, TR>& m) const {
    u32x4 x[G::NP];
#pragma unroll
    for (int j = 0; j < G::NP; ++j) x[j] = (mask >> j) & 1u ? v[j] : zero4();
    m.template store<false>(img, x, nullptr);
  }
};

__device__ __forceinline__ void zero_acc(f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The accumulators of a wave to C[I, J] (row-major, pitch J), one rounding.
template <typename TO>
__device__ __forceinline__ void store_tile(TO* __restrict__ C,
                                           const f32x4 (&acc)[4][4], int i0,
                                           int j0, int I, int J, int wave,
                                           int r, int q) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = j0 + (wave & 1) * 64 + r + 16 * j;
    if (col >= J) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned row =
            (unsigned)i0 + (unsigned)((wave >> 1) * 64 + 16 * i + 4 * q + e);
        if (row >= (unsigned)I) continue;
        st1(&C[(int64_t)row * J + col], acc[i][j][e]);
      }
    }
  }
}

// Forward (BWD false): C = Y [M, Cout], A gathered from x, B = Wp straight.
// Input gradient (BWD true): C = dX [N*H*W, Cin], A gathered from dy, B = Wp
// transposed. The contraction walks the taps and, inside one, the KC
// channels (Cin forward, Cout backward) in blocks of 32.
template <typename T, bool BWD>
__device__ __forceinline__ void conv_rows(const T* __restrict__ a_src,
                                          const T* __restrict__ wp,
                                          T* __restrict__ out,
                                          const ConvGeo& g) {
  using G = Geo<T>;
  __shared__ __attribute__((aligned(16))) uint32_t smem[2 * G::WORDS];
  uint32_t* imgA = smem;
  uint32_t* imgB = smem + G::WORDS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.x * kBM, j0 = blockIdx.y * kBN;
  const int rowA = (wave >> 1) * 64 + r, rowB = (wave & 1) * 64 + r;
  const int I = BWD ? g.N * g.H * g.W : g.M, J = BWD ? g.Cin : g.Cout;
  const int KC = BWD ? g.Cout : g.Cin;

  TileMap<T, false> ma;
  TileMap<T, BWD> mb;
  ma.init(tid), mb.init(tid);
  GatherRows<T, BWD> opA;
  WeightOp<T, BWD> opB;
  opA.init(a_src, g, ma, i0);
  opB.init(wp, g, mb, j0);
  f32x4 acc[4][4];
  zero_acc(acc);

  const int nblk = g.taps * ((KC + kBK - 1) / kBK);
  int tr = 0, tq = 0, c0 = 0;  // the tap (row, column) and first channel
  opA.load(0, 0, 0), opB.load(mb, 0, 0);
  for (int it = 0; it < nblk; ++it) {
    opA.store(imgA, ma);
    opB.store(imgB, mb);
    block_sync();
    c0 += kBK;
    if (c0 >= KC) {
      c0 = 0;
      if (++tq == g.k) tq = 0, ++tr;
    }
    if (it + 1 < nblk) opA.load(tr, tq, c0), opB.load(mb, tr * g.k + tq, c0);
    multiply_block<T, false, BWD>(imgA, imgB, rowA, rowB, q, acc);
    block_sync();
  }
  store_tile(out, acc, i0, j0, I, J, wave, r, q);
}

template <typename T>
__global__ __launch_bounds__(kGemmThreads) void k_conv_fwd(
    const T* __restrict__ x, const T* __restrict__ wp, T* __restrict__ y,
    const ConvGeo g) {
  conv_rows<T, false>(x, wp, y, g);
}

template <typename T>
__global__ __launch_bounds__(kGemmThreads) void k_conv_bwd_input(
    const T* __restrict__ dy, const T* __restrict__ wp, T* __restrict__ dx,
    const ConvGeo g) {
  conv_rows<T, true>(dy, wp, dx, g);
}

// Both operands of the weight gradient for one tap (tr, tq) and one slice
// [m_begin, m_end) of the output pixels: dy's rows as they lie, x's rows
// gathered. Both are transposed operands (the contraction index m is the
// source's row) and share one thread map.
template <typename T>
struct WgradOps {
  using G = Geo<T>;
  const T* dy;
  const T* x;
  ConvGeo g;
  TileMap<T, true> mp;
  int tr, tq, ca, cb;
  bool aok, bok;
  unsigned m_end;
  int pn[G::NP], ph[G::NP], pw[G::NP];  // the slots' pixels (n, ho, wo)
  unsigned maska, maskb;
  u32x4 va[G::NP], vb[G::NP];

  __device__ __forceinline__ void init(const T* dy_, const T* x_,
                                       const ConvGeo& g_, int tid, int i0,
                                       int j0, int tr_, int tq_,
                                       unsigned m_begin, unsigned m_end_) {
    dy = dy_, x = x_, g = g_, tr = tr_, tq = tq_, m_end = m_end_;
    mp.init(tid);
    const int colA = i0 + mp.c * G::E, colB = j0 + mp.c * G::E;
    aok = colA < g.Cout, bok = colB < g.Cin;
    ca = aok ? colA : 0, cb = bok ? colB : 0;
    maska = maskb = 0;
    const unsigned hw = (unsigned)(g.Ho * g.Wo);
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {  // the only divisions: once per slot
      const unsigned m = m_begin + (unsigned)mp.slot_row(j);
      const unsigned n = m / hw, rem = m - n * hw;
      const unsigned h = rem / (unsigned)g.Wo;
      pn[j] = (int)n, ph[j] = (int)h, pw[j] = (int)(rem - h * g.Wo);
    }
  }
  // Issue the loads of the block at m0, then move the pixels 32 rows on.
  __device__ __forceinline__ void load(unsigned m0) {
    maska = maskb = 0;
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      const unsigned m = m0 + (unsigned)mp.slot_row(j);
      const bool in = m < m_end;
      va[j] = ld16(dy + (int64_t)(in ? m : 0u) * g.Cout + ca);
      maska |= (unsigned)(in && aok) << j;
      const int sy = ph[j] * g.stride - g.pad + tr;
      const int sx = pw[j] * g.stride - g.pad + tq;
      const bool ok = in && sy >= 0 && sx >= 0 && sy < g.H && sx < g.W;
      const int64_t pix =
          ok ? (int64_t)pn[j] * (g.H * g.W) + sy * g.W + sx : (int64_t)0;
      vb[j] = ld16(x + pix * g.Cin + cb);
      maskb |= (unsigned)(ok && bok) << j;
      pw[j] += g.d_w;  // one carry per digit
      const bool cw = pw[j] >= g.Wo;
      pw[j] -= cw ? g.Wo : 0;
      ph[j] += g.d_h + (int)cw;
      const bool ch = ph[j] >= g.Ho;
      ph[j] -= ch ? g.Ho : 0;
      pn[j] += g.d_n + (int)ch;
    }
  }
  __device__ __forceinline__ void store(uint32_t* imgA, uint32_t* imgB) const {
    u32x4 xa[G::NP], xb[G::NP];
#pragma unroll
    for (int j = 0; j < G::NP; ++j) {
      xa[j] = (maska >> j) & 1u ? va[j] : zero4();
      xb[j] = (maskb >> j) & 1u ? vb[j] : zero4();
    }
    mp.template store<false>(imgA, xa, nullptr);
    mp.template store<false>(imgB, xb, nullptr);
  }
};

// One (Cout tile, Cin tile, tap, slice) of the weight gradient: the f32 tile
// of sum_{m in slice} dy[m, co] x[pix(m, tap), ci] into ws[g, co, tap, ci].
// grid: (Cout tiles, Cin tiles, taps * GS), z = tap * GS + slice.
template <typename T>
__global__ __launch_bounds__(kGemmThreads) void k_conv_bwd_weight(
    const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ ws,
    const ConvGeo g, int GS) {
  using G = Geo<T>;
  __shared__ __attribute__((aligned(16))) uint32_t smem[2 * G::WORDS];
  uint32_t* imgA = smem;
  uint32_t* imgB = smem + G::WORDS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int i0 = blockIdx.x * kBM, j0 = blockIdx.y * kBN;
  const int tap = blockIdx.z / GS, slice = blockIdx.z - tap * GS;
  const int tr = tap / g.k, tq = tap - tr * g.k;
  const int rowA = (wave >> 1) * 64 + r, rowB = (wave & 1) * 64 + r;
  const unsigned m_begin = (unsigned)slice * g.L;
  const unsigned m_end =
      m_begin + g.L < (unsigned)g.M ? m_begin + g.L : (unsigned)g.M;

  WgradOps<T> op;
  op.init(dy, x, g, tid, i0, j0, tr, tq, m_begin, m_end);
  f32x4 acc[4][4];
  zero_acc(acc);

  op.load(m_begin);
  for (unsigned m0 = m_begin; m0 < m_end; m0 += kBK) {
    op.store(imgA, imgB);
    block_sync();
    if (m0 + kBK < m_end) op.load(m0 + kBK);
    multiply_block<T, true, true>(imgA, imgB, rowA, rowB, q, acc);
    block_sync();
  }

  // ws[slice][co][tap][ci]: row pitch taps*Cin, this tap's columns
  float* tile = ws + (int64_t)slice * g.Cout * g.taps * g.Cin;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = j0 + rowB + 16 * j;
    if (ci >= g.Cin) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = i0 + (wave >> 1) * 64 + 16 * i + 4 * q + e;
        if (co >= g.Cout) continue;
        tile[((int64_t)co * g.taps + tap) * g.Cin + ci] = acc[i][j][e];
      }
    }
  }
}

// dW[co, ci, tap] = round(ws[0] + ws[1] + ... + ws[GS-1]) at (co, tap, ci):
// the slices in slice order, one rounding, the parameter's layout and dtype.
template <typename TO>
__global__ __launch_bounds__(kGemmThreads) void k_conv_wgrad_finish(
    const float* __restrict__ ws, TO* __restrict__ dw, int GS, int Cout,
    int taps, int Cin) {
  const int64_t total = (int64_t)Cout * taps * Cin;
  for (int64_t idx = (int64_t)blockIdx.x * kGemmThreads + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * kGemmThreads) {
    const int64_t t = idx / Cin;
    const int ci = (int)(idx - t * Cin);
    const int64_t co = t / taps;
    const int tap = (int)(t - co * taps);
    float s = ws[idx];
    for (int gs = 1; gs < GS; ++gs) s += ws[gs * total + idx];
    st1(&dw[(co * Cin + ci) * taps + tap], s);
  }
}

struct ConvArg {
  const char* name;
  const torch::Tensor* t;
  std::vector<int64_t> shape;
};

// (tile rows, tile columns, GS, L) of the weight gradient.
std::vector<int64_t> wgrad_plan(int64_t M, int64_t Cout, int64_t Cin,
                                int64_t taps) {
  const int64_t tiles = ((Cout + kBM - 1) / kBM) * ((Cin + kBN - 1) / kBN) *
                        std::max<int64_t>(taps, 1);
  int64_t GS = std::max<int64_t>(1, kConvWgradTargetGrid / tiles);
  GS = std::min(GS, std::max<int64_t>(
                        1, (M + kConvWgradMinSlice - 1) / kConvWgradMinSlice));
  int64_t L = (M + GS - 1) / GS;
  L = std::max<int64_t>(kBK, (L + kBK - 1) / kBK * kBK);
  GS = std::max<int64_t>(1, (M + L - 1) / L);  // no empty slice
  return {kBM, kBN, GS, L};
}

// The argument check of the three entry points, complete before any launch.
// The first of `args` fixes dtype and device.
ConvGeo conv_check_args(const char* who, std::initializer_list<ConvArg> args,
                        int64_t N, int64_t H, int64_t W, int64_t Cin,
                        int64_t Cout, int64_t k, int64_t stride) {
  TORCH_CHECK(k == 1 || k == 3, who, ": kernel size must be 1 or 3, got ", k);
  TORCH_CHECK(stride == 1 || stride == 2, who,
              ": stride must be 1 or 2, got ", stride);
  TORCH_CHECK(N >= 0 && H >= 1 && W >= 1, who, ": N >= 0, H >= 1, W >= 1");
  TORCH_CHECK(N * H * W < (int64_t(1) << 31) && H < (1 << 30) && W < (1 << 30),
              who, ": N*H*W must be below 2^31");
  TORCH_CHECK(Cin >= 16 && Cin % 16 == 0 && Cout >= 16 && Cout % 16 == 0 &&
                  Cin <= (1 << 20) && Cout <= (1 << 20),
              who, ": Cin and Cout must be multiples of 16, got ", Cin, ", ",
              Cout);
  const torch::Tensor& ref = *args.begin()->t;
  TORCH_CHECK(ref.defined() && ref.is_cuda(), who, ": ", args.begin()->name,
              " must be on a GPU");
  const auto dt = ref.scalar_type();
  TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16, who,
              ": dtype must be f32 or bf16, got ", dt);
  for (const auto& a : args) {
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
  ConvGeo g;
  g.N = (int)N, g.H = (int)H, g.W = (int)W, g.Cin = (int)Cin;
  g.Cout = (int)Cout, g.k = (int)k, g.stride = (int)stride;
  g.pad = (int)(k / 2), g.taps = (int)(k * k);
  g.Ho = (int)((H + 2 * g.pad - k) / stride + 1);
  g.Wo = (int)((W + 2 * g.pad - k) / stride + 1);
  g.M = (int)(N * g.Ho * g.Wo);
  const int hw = g.Ho * g.Wo;
  g.d_n = kBK / hw;
  g.d_h = (kBK - g.d_n * hw) / g.Wo;
  g.d_w = kBK - g.d_n * hw - g.d_h * g.Wo;
  g.L = kBK;
  return g;
}

int64_t taps_of(const char* who, const torch::Tensor& wp) {
  TORCH_CHECK(wp.dim() == 3 && (wp.size(1) == 1 || wp.size(1) == 9), who,
              ": wp must be [Cout, k*k, Cin] with k 1 or 3, got ", wp.sizes());
  return wp.size(1) == 1 ? 1 : 3;
}

}  // namespace

std::vector<int64_t> conv_wgrad_plan(int64_t M, int64_t Cout, int64_t Cin,
                                     int64_t taps) {
  TORCH_CHECK(M >= 0 && Cout >= 1 && Cin >= 1 && (taps == 1 || taps == 9),
              "conv_wgrad_plan: M >= 0, Cout, Cin >= 1, taps 1 or 9");
  return wgrad_plan(M, Cout, Cin, taps);
}

torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor wp, int64_t N,
                         int64_t H, int64_t W, int64_t stride) {
  const char* who = "conv2d_fwd";
  const int64_t k = taps_of(who, wp);
  TORCH_CHECK(x.dim() == 2, who, ": x must be [N*H*W, Cin]");
  const int64_t Cin = x.size(1), Cout = wp.size(0);
  const ConvGeo g = conv_check_args(
      who, {{"x", &x, {N * H * W, Cin}}, {"wp", &wp, {Cout, k * k, Cin}}}, N,
      H, W, Cin, Cout, k, stride);
  auto y = torch::empty({(int64_t)g.M, Cout}, x.options());
  if (g.M > 0) {
    DISPATCH_F32_BF16(x.scalar_type(), who, {
      hipLaunchKernelGGL((k_conv_fwd<scalar_t>),
                         dim3(cdiv(g.M, kBM), cdiv(Cout, kBN)),
                         dim3(kGemmThreads), 0, cur_stream(),
                         cdptr<scalar_t>(x), cdptr<scalar_t>(wp),
                         dptr<scalar_t>(y), g);
    });
    HIP_OK(hipGetLastError());
  }
  return y;
}

torch::Tensor conv2d_bwd_input(torch::Tensor dy, torch::Tensor wp, int64_t N,
                               int64_t H, int64_t W, int64_t stride) {
  const char* who = "conv2d_bwd_input";
  const int64_t k = taps_of(who, wp);
  TORCH_CHECK(dy.dim() == 2, who, ": dy must be [N*Ho*Wo, Cout]");
  const int64_t Cin = wp.size(2), Cout = wp.size(0);
  const int64_t p = k / 2;
  const int64_t Ho = H >= 1 && (stride == 1 || stride == 2)
                         ? (H + 2 * p - k) / stride + 1 : 0;
  const int64_t Wo = W >= 1 && (stride == 1 || stride == 2)
                         ? (W + 2 * p - k) / stride + 1 : 0;
  const ConvGeo g = conv_check_args(
      who,
      {{"dy", &dy, {N * Ho * Wo, Cout}}, {"wp", &wp, {Cout, k * k, Cin}}}, N,
      H, W, Cin, Cout, k, stride);
  auto dx = torch::empty({N * H * W, Cin}, dy.options());
  if (N > 0) {
    DISPATCH_F32_BF16(dy.scalar_type(), who, {
      hipLaunchKernelGGL((k_conv_bwd_input<scalar_t>),
                         dim3(cdiv(N * H * W, kBM), cdiv(Cin, kBN)),
                         dim3(kGemmThreads), 0, cur_stream(),
                         cdptr<scalar_t>(dy), cdptr<scalar_t>(wp),
                         dptr<scalar_t>(dx), g);
    });
    HIP_OK(hipGetLastError());
  }
  return dx;
}

torch::Tensor conv2d_bwd_weight(torch::Tensor dy, torch::Tensor x, int64_t N,
                                int64_t H, int64_t W, int64_t k,
                                int64_t stride,
                                c10::optional<torch::Tensor> dw_) {
  const char* who = "conv2d_bwd_weight";
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2, who, ": dy and x must be 2-D");
  const int64_t Cin = x.size(1), Cout = dy.size(1);
  const int64_t p = k / 2;
  const bool sane = H >= 1 && W >= 1 && (stride == 1 || stride == 2);
  const int64_t Ho = sane ? (H + 2 * p - k) / stride + 1 : 0;
  const int64_t Wo = sane ? (W + 2 * p - k) / stride + 1 : 0;
  ConvGeo g = conv_check_args(
      who, {{"dy", &dy, {N * Ho * Wo, Cout}}, {"x", &x, {N * H * W, Cin}}}, N,
      H, W, Cin, Cout, k, stride);
  auto dw = dw_.has_value() ? *dw_
                            : torch::empty({Cout, Cin, k, k}, dy.options());
  TORCH_CHECK(dw.device() == dy.device() &&
                  (dw.scalar_type() == at::kFloat ||
                   dw.scalar_type() == at::kBFloat16) &&
                  dw.sizes() == at::IntArrayRef({Cout, Cin, k, k}) &&
                  dw.is_contiguous(),
              who, ": dw must be a contiguous f32 or bf16 [Cout, Cin, k, k] "
                   "on dy's device, got ", dw.sizes());
  if (g.M == 0) {
    dw.zero_();
    return dw;
  }
  const auto plan = wgrad_plan(g.M, Cout, Cin, g.taps);
  const int GS = (int)plan[2];
  g.L = (int)plan[3];
  auto ws = torch::empty({GS, Cout, (int64_t)g.taps, Cin},
                         dy.options().dtype(at::kFloat));
  DISPATCH_F32_BF16(dy.scalar_type(), who, {
    hipLaunchKernelGGL((k_conv_bwd_weight<scalar_t>),
                       dim3(cdiv(Cout, kBM), cdiv(Cin, kBN), g.taps * GS),
                       dim3(kGemmThreads), 0, cur_stream(),
                       cdptr<scalar_t>(dy), cdptr<scalar_t>(x),
                       dptr<float>(ws), g, GS);
  });
  HIP_OK(hipGetLastError());
  const int64_t total = Cout * g.taps * Cin;
  DISPATCH_F32_BF16(dw.scalar_type(), who, {
    hipLaunchKernelGGL((k_conv_wgrad_finish<scalar_t>),
                       dim3((int)std::min<int64_t>(
                           4096, (total + kGemmThreads - 1) / kGemmThreads)),
                       dim3(kGemmThreads), 0, cur_stream(), cdptr<float>(ws),
                       dptr<scalar_t>(dw), GS, (int)Cout, g.taps, (int)Cin);
  });
  HIP_OK(hipGetLastError());
  return dw;
}

}  // namespace mi355x

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
