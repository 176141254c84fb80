// What does the issue slot behind a dependent v_fmac_f32_dpp cost to fill?
//
// k_toy_multistep_chain (mi355x_ddp/ops/csrc/toy_kernels.hip) is one wave
// running 53 dependent `v_fmac_f32_dpp ... row_newbcast:n` terms per step,
// priced at about 7.2 cycles each against 4.9 for any other instruction of
// a lone wave (profiles/README.md r03c, r03d). This probe times, with
// s_memtime around the loop, 4096 such terms on one accumulator in one
// wave of one workgroup, with different instructions placed between the
// terms, and prints cycles per term for each variant:
//
//   a    nothing between the terms
//   b    one s_nop 0 after every term
//   c    one independent SALU instruction (s_add_u32) after every term
//   d    one independent VALU instruction (v_mov_b32) after every term
//   e    one conflict-free ds_read_b128 into unrelated registers after
//        every term; nothing waits for the reads inside the timed loop
//   ew   as e, with s_waitcnt lgkmcnt(0) once per 8 terms
//   f    SALU + ds_read_b128 after every term, no wait
//   g    the same chain with plain v_fmac_f32 (no DPP)
//   b2 c2 d2 e2   the filler after every second term only
//   dd   two independent VALU instructions after every term
//   h    two independent DPP chains interleaved term by term (does a DPP
//        term hold the issue port, or only wait for its accumulator?)
//
//   hipcc --offload-arch=gfx950 -O3 -o chain_slot_probe tools/chain_slot_probe.hip
//   ./chain_slot_probe
//
// No arguments; every variant runs a fixed 4096 terms, three times, and
// the fastest of the three is reported (the first also loads the code).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int kTermsPerStmt = 64;
static constexpr int kStmts = 64;
static constexpr int kTerms = kTermsPerStmt * kStmts;
static constexpr int kRepeats = 3;

enum Variant { A, B, C, D, E, EW, F, G, B2, C2, D2, E2, DD, H, kVariants };
static const char* const kNames[kVariants] = {
    "a   dpp chain, nothing between",
    "b   + s_nop 0 per term",
    "c   + SALU (s_add_u32) per term",
    "d   + VALU (v_mov_b32) per term",
    "e   + ds_read_b128 per term, no wait",
    "ew  + ds_read_b128 per term, wait per 8",
    "f   + SALU + ds_read_b128 per term",
    "g   plain v_fmac_f32 chain",
    "b2  s_nop 0 per 2 terms",
    "c2  SALU per 2 terms",
    "d2  VALU per 2 terms",
    "e2  ds_read_b128 per 2 terms",
    "dd  + 2 VALU per term",
    "h   two dpp chains interleaved (per pair)",
};

#define DPP(n) " row_newbcast:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define TERM(n, xi) "v_fmac_f32_dpp %[acc], %[src], %[x" #xi "]" DPP(n)
#define TERM2(n, xi) "v_fmac_f32_dpp %[acc2], %[src], %[x" #xi "]" DPP(n)
#define PLAIN(n, xi) "v_fmac_f32 %[acc], %[src], %[x" #xi "]\n\t"
// fillers, F(i) with i = 0..7 the position in a run of 8 terms
#define F_NONE(i)
#define F_NOP(i) "s_nop 0\n\t"
#define F_SALU(i) "s_add_u32 %[sc], %[sc], 1\n\t"
#define F_VALU(i) "v_mov_b32 %[va], %[vb]\n\t"
#define F_VALU2(i) "v_mov_b32 %[va], %[vb]\n\tv_mov_b32 %[vc], %[vb]\n\t"
#define F_LDS(i) "ds_read_b128 %[d" #i "], %[addr] offset:" #i "*1024\n\t"
#define F_SALU_LDS(i) F_SALU(i) F_LDS(i)
#define F_TERM2(i) TERM2(i, 1)
#define WAIT "s_waitcnt lgkmcnt(0)\n\t"
#define NOWAIT
// 16 terms, row_newbcast 0..15, one filler per term / per second term
#define RUN16(T, F, W)                                                     \
  T(0, 0) F(0) T(1, 1) F(1) T(2, 2) F(2) T(3, 3) F(3) T(4, 0) F(4)         \
  T(5, 1) F(5) T(6, 2) F(6) T(7, 3) F(7) W T(8, 0) F(0) T(9, 1) F(1)       \
  T(10, 2) F(2) T(11, 3) F(3) T(12, 0) F(4) T(13, 1) F(5) T(14, 2) F(6)    \
  T(15, 3) F(7) W
#define RUN16_2(T, F, W)                                                   \
  T(0, 0) T(1, 1) F(0) T(2, 2) T(3, 3) F(1) T(4, 0) T(5, 1) F(2) T(6, 2)   \
  T(7, 3) F(3) T(8, 0) T(9, 1) F(4) T(10, 2) T(11, 3) F(5) T(12, 0)        \
  T(13, 1) F(6) T(14, 2) T(15, 3) F(7) W
#define RUN64(R, T, F, W) R(T, F, W) R(T, F, W) R(T, F, W) R(T, F, W)

struct State {
  float acc, acc2, src, x0, x1, x2, x3;
  unsigned va, vb, vc, addr, sc;
  f32x4 d0, d1, d2, d3, d4, d5, d6, d7;
};
#define STMT(body)                                                         \
  asm volatile(body                                                        \
               : [acc] "+v"(s.acc), [acc2] "+v"(s.acc2), [va] "+v"(s.va),  \
                 [vc] "+v"(s.vc), [sc] "+s"(s.sc), [d0] "=&v"(s.d0),       \
                 [d1] "=&v"(s.d1), [d2] "=&v"(s.d2), [d3] "=&v"(s.d3),     \
                 [d4] "=&v"(s.d4), [d5] "=&v"(s.d5), [d6] "=&v"(s.d6),     \
                 [d7] "=&v"(s.d7)                                          \
               : [src] "v"(s.src), [x0] "v"(s.x0), [x1] "v"(s.x1),         \
                 [x2] "v"(s.x2), [x3] "v"(s.x3), [vb] "v"(s.vb),           \
                 [addr] "v"(s.addr)                                        \
               : "memory", "scc")

template <int V>
__device__ __forceinline__ void stmt64(State& s) {
  if constexpr (V == A) STMT(RUN64(RUN16, TERM, F_NONE, NOWAIT));
  if constexpr (V == B) STMT(RUN64(RUN16, TERM, F_NOP, NOWAIT));
  if constexpr (V == C) STMT(RUN64(RUN16, TERM, F_SALU, NOWAIT));
  if constexpr (V == D) STMT(RUN64(RUN16, TERM, F_VALU, NOWAIT));
  if constexpr (V == E) STMT(RUN64(RUN16, TERM, F_LDS, NOWAIT));
  if constexpr (V == EW) STMT(RUN64(RUN16, TERM, F_LDS, WAIT));
  if constexpr (V == F) STMT(RUN64(RUN16, TERM, F_SALU_LDS, NOWAIT));
  if constexpr (V == G) STMT(RUN64(RUN16, PLAIN, F_NONE, NOWAIT));
  if constexpr (V == B2) STMT(RUN64(RUN16_2, TERM, F_NOP, NOWAIT));
  if constexpr (V == C2) STMT(RUN64(RUN16_2, TERM, F_SALU, NOWAIT));
  if constexpr (V == D2) STMT(RUN64(RUN16_2, TERM, F_VALU, NOWAIT));
  if constexpr (V == E2) STMT(RUN64(RUN16_2, TERM, F_LDS, NOWAIT));
  if constexpr (V == DD) STMT(RUN64(RUN16, TERM, F_VALU2, NOWAIT));
  if constexpr (V == H) STMT(RUN64(RUN16, TERM, F_TERM2, NOWAIT));
}

template <int V>
__global__ void __launch_bounds__(64) k_probe(unsigned long long* cycles,
                                              float* sink) {
  // 8 reads of 16 bytes per lane, 1 KiB apart: lane l reads bytes
  // 16 l .. 16 l + 15 of each KiB, conflict-free and inside the array
  __shared__ __attribute__((aligned(16))) float lds[8 * 256];
  const unsigned lane = threadIdx.x;
  for (int i = lane; i < 8 * 256; i += 64) lds[i] = 1.f;
  __syncthreads();
  State s;
  s.acc = 0.f, s.acc2 = 0.f, s.src = 1e-3f * (float)lane;
  s.x0 = 0.5f, s.x1 = 0.25f, s.x2 = -0.5f, s.x3 = -0.25f;
  s.va = lane, s.vb = lane + 1, s.vc = lane + 2, s.sc = 0;
  s.addr = (unsigned)(size_t)lds + lane * 16;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
  for (int it = 0; it < kStmts; ++it) stmt64<V>(s);
  // the reads of the no-wait variants land in d0..d7 (the same registers in
  // every trip) until here; nothing reads those registers before
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) *cycles = t1 - t0;
  const f32x4 d = s.d0 + s.d1 + s.d2 + s.d3 + s.d4 + s.d5 + s.d6 + s.d7;
  sink[lane] = s.acc + s.acc2 + d[0] + d[1] + d[2] + d[3] +
               (float)(s.va + s.vc + s.sc);
}

#define CHECK(e)                                                      \
  do {                                                                \
    hipError_t err_ = (e);                                            \
    if (err_ != hipSuccess) {                                         \
      std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_)); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

template <int V>
static double run(unsigned long long* d_cycles, float* d_sink) {
  unsigned long long best = ~0ull;
  for (int r = 0; r < kRepeats; ++r) {
    unsigned long long c = 0;
    hipLaunchKernelGGL(k_probe<V>, dim3(1), dim3(64), 0, 0, d_cycles, d_sink);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&c, d_cycles, sizeof(c), hipMemcpyDeviceToHost));
    if (c < best) best = c;
  }
  return (double)best / kTerms;
}

template <int V = 0>
static void run_all(unsigned long long* d_cycles, float* d_sink) {
  if constexpr (V < kVariants) {
    std::printf("| %-42s | %6.2f |\n", kNames[V], run<V>(d_cycles, d_sink));
    run_all<V + 1>(d_cycles, d_sink);
  }
}

int main() {
  unsigned long long* d_cycles;
  float* d_sink;
  CHECK(hipMalloc(&d_cycles, sizeof(*d_cycles)));
  CHECK(hipMalloc(&d_sink, 64 * sizeof(float)));
  std::printf("%d dependent terms, one wave, s_memtime cycles per term\n",
              kTerms);
  std::printf("| %-42s | cycles |\n|---|---|\n", "variant");
  run_all(d_cycles, d_sink);
  CHECK(hipFree(d_cycles));
  CHECK(hipFree(d_sink));
  return 0;
}
