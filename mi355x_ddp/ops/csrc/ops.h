// Host-side launcher declarations for the MI355X (gfx950) kernel pack.
// Implementations in kernels.hip, for the toy training-step family
// (toy_fused_fwd_bwd, toy_multistep*) toy_kernels.hip, and for the
// flat-bucket optimizers optim_kernels.hip, for the fused self-attention
// attention_kernels.hip, for the fused LayerNorm layernorm_kernels.hip, for
// the fused BatchNorm batchnorm_kernels.hip, for the tiled GEMMs
// gemm_kernels.hip, for the implicit-GEMM convolutions conv_kernels.hip, for
// the class-index cross-entropy loss_kernels.hip; bound to Python in
// bindings.hip.
#pragma once
#include <torch/extension.h>
#include <cstdint>
#include <string>

#include "p2p_mesh.h"

namespace mi355x {

// y = x @ w^T + b          (reference call site: model(source), single_gpu.py:23)
torch::Tensor linear_fwd(torch::Tensor x, torch::Tensor w,
                         c10::optional<torch::Tensor> bias);

// dw = dy^T @ x, db = sum_i dy  (reference: loss.backward(), single_gpu.py:25)
// dw/db may be preallocated views into a gradient bucket; accumulate=true
// adds into them instead of overwriting. An empty db skips the bias gradient.
// Like every launcher here it checks dtype, shape and device of all operands
// before the launch, and empty work (no rows, no elements, an empty plan)
// returns torch's empty result without one.
void linear_bwd_weight(torch::Tensor x, torch::Tensor dy,
                       torch::Tensor dw, torch::Tensor db, bool accumulate);

// dx = dy @ w
torch::Tensor linear_bwd_input(torch::Tensor dy, torch::Tensor w);

// Standalone bf16 MFMA GEMM (v_mfma_f32_16x16x32_bf16, f32 accumulate):
// y = x @ w^T + bias. No model path routes to it; it is tested and timed.
torch::Tensor gemm_bf16(torch::Tensor x, torch::Tensor w,
                        c10::optional<torch::Tensor> bias);

// Fused short-sequence self-attention over the packed in-projection output
// (attention_kernels.hip): qkv [B, N, 3*E] contiguous f32/bf16, columns
// [0,E) Q, [E,2E) K, [2E,3E) V, head h at columns h*D.. of each, E = heads*D.
// 1 <= N <= 64, D in {16, 32, 64}, scale 1/sqrt(D), no mask, no dropout;
// anything else is refused before a launch, and B == 0 launches nothing.
// attn_fwd returns (out [B, N, E], row_stats f32 [B, heads, N, 2]: the max of
// a row's raw scores and the reciprocal of its sum of exponentials).
// attn_bwd returns dqkv [B, N, 3*E] in qkv's layout from dout [B, N, E]. It
// takes delta = rowsum(dO * O) as rowsum(P * dP) from its own registers, so
// the forward's `out` is neither read nor kept for it. Results may be
// preallocated (contiguous, 16-byte aligned, of the shapes above).
std::vector<torch::Tensor> attn_fwd(
    torch::Tensor qkv, int64_t heads,
    c10::optional<torch::Tensor> out = c10::nullopt,
    c10::optional<torch::Tensor> row_stats = c10::nullopt);
torch::Tensor attn_bwd(torch::Tensor dout, torch::Tensor qkv,
                       torch::Tensor row_stats, int64_t heads,
                       c10::optional<torch::Tensor> dqkv = c10::nullopt);

// The tiled family of the same file: the same operands, layouts, checks and
// arithmetic for 1 <= N <= 4096. A workgroup owns 64 rows and walks the other
// side in blocks of 64 (online softmax in the forward). The backward is two
// launches, dQ by query block and dK/dV by key block, without atomics; it
// takes delta = rowsum(dO * O) from the forward's `out` [B, N, E], which the
// caller therefore keeps.
std::vector<torch::Tensor> attn_tiled_fwd(
    torch::Tensor qkv, int64_t heads,
    c10::optional<torch::Tensor> out = c10::nullopt,
    c10::optional<torch::Tensor> row_stats = c10::nullopt);
torch::Tensor attn_tiled_bwd(torch::Tensor dout, torch::Tensor qkv,
                             torch::Tensor out, torch::Tensor row_stats,
                             int64_t heads,
                             c10::optional<torch::Tensor> dqkv = c10::nullopt);

// The bf16 family of the same file: the tiled family's operands, layouts and
// work split for bf16 storage ONLY, D in {32, 64}, 1 <= N <= 4096, with all
// five products on v_mfma_f32_16x16x32_bf16 (f32 accumulators, softmax and
// statistics). P and dS are rounded to bf16 once, on their way into the
// second product; row_stats' 1/l is that of the rounded P. f32 storage, any
// other D or N, a non-contiguous or misplaced operand are refused before a
// launch; B == 0 launches nothing.
std::vector<torch::Tensor> attn_bf16_fwd(
    torch::Tensor qkv, int64_t heads,
    c10::optional<torch::Tensor> out = c10::nullopt,
    c10::optional<torch::Tensor> row_stats = c10::nullopt);
torch::Tensor attn_bf16_bwd(torch::Tensor dout, torch::Tensor qkv,
                            torch::Tensor out, torch::Tensor row_stats,
                            int64_t heads,
                            c10::optional<torch::Tensor> dqkv = c10::nullopt);

// Fused LayerNorm over the last dimension, optionally with the residual add
// in front of it (layernorm_kernels.hip). Rows are the flattened leading
// dimensions of a contiguous x; E = x.size(-1), E % 4 == 0, 4 <= E <= 2048;
// every operand f32 or bf16 alike, arithmetic and row_stats in f32. Anything
// else is refused before a launch, and no rows launches nothing.
// ln_fwd returns (y, row_stats f32 [R, 2] = (mean, rstd)) or, with a
// residual, (s, y, row_stats): s = x + residual rounded to the storage dtype,
// y = LN(s) of that rounded s.
// ln_bwd takes the LN input (x, or s) and returns (dx, dgamma, dbeta); `ds`,
// the gradient arriving at s, is added into dx. dgamma/dbeta are reduced
// without atomics in an order fixed by the shape, so they are reproducible.
// Results may be preallocated (contiguous, 16-byte aligned).
// ln_grid_cap: the compile-time cap on the row kernels' grid.
std::vector<torch::Tensor> ln_fwd(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias, double eps,
    c10::optional<torch::Tensor> residual = c10::nullopt,
    c10::optional<torch::Tensor> y = c10::nullopt,
    c10::optional<torch::Tensor> row_stats = c10::nullopt,
    c10::optional<torch::Tensor> s = c10::nullopt);
std::vector<torch::Tensor> ln_bwd(
    torch::Tensor dy, torch::Tensor ln_input, torch::Tensor row_stats,
    torch::Tensor weight, c10::optional<torch::Tensor> ds = c10::nullopt,
    c10::optional<torch::Tensor> dx = c10::nullopt,
    c10::optional<torch::Tensor> dgamma = c10::nullopt,
    c10::optional<torch::Tensor> dbeta = c10::nullopt);
int64_t ln_grid_cap();

// Fused BatchNorm, optionally with ReLU, optionally with a residual add in
// front of the ReLU (batchnorm_kernels.hip): z = act(bn(x) + residual) over
// the rows of a channels-last activation. x, residual, z, dz, dx, dresidual
// are 2-D [R, C] (R = N*H*W pixels, C channels contiguous), contiguous,
// 16-byte aligned, f32 or bf16 alike; weight, bias, the running statistics,
// col_stats [2, C] = (mean row, rstd row), dgamma and dbeta are f32 whatever
// the storage; arithmetic is f32. C % 4 == 0, 4 <= C <= 4096; R >= 2 in
// training, R >= 1 in evaluation; a residual only with relu; momentum in
// [0, 1], eps >= 0. Anything else is refused before a launch.
// bn_fwd, training: returns (z, col_stats), updates running_mean/running_var
//   in place (unbiased variance) and adds one to num_batches_tracked (int64,
//   one element) on the device. Evaluation: returns (z) from the running
//   statistics and changes nothing.
// bn_bwd returns (dx, dgamma, dbeta) or, with add, (dx, dgamma, dbeta,
//   dresidual). With z, the forward's OUTPUT, the gradient first passes the
//   ReLU: g = dz * (z > 0); dresidual = g. Statistics and parameter gradients
//   are reduced without atomics in an order fixed by the shape: reproducible.
// Results may be preallocated.
// bn_plan: (LC, slabs, GR), the lanes along the channels, the column slabs
//   and the workgroups along the rows, a function of (R, C) alone.
std::vector<torch::Tensor> bn_fwd(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, bool training,
    double momentum, double eps, bool relu,
    c10::optional<torch::Tensor> residual = c10::nullopt,
    c10::optional<torch::Tensor> num_batches_tracked = c10::nullopt,
    c10::optional<torch::Tensor> z = c10::nullopt,
    c10::optional<torch::Tensor> col_stats = c10::nullopt);
std::vector<torch::Tensor> bn_bwd(
    torch::Tensor dz, torch::Tensor x, torch::Tensor col_stats,
    torch::Tensor weight, c10::optional<torch::Tensor> z = c10::nullopt,
    bool add = false, c10::optional<torch::Tensor> dx = c10::nullopt,
    c10::optional<torch::Tensor> dresidual = c10::nullopt,
    c10::optional<torch::Tensor> dgamma = c10::nullopt,
    c10::optional<torch::Tensor> dbeta = c10::nullopt);
std::vector<int64_t> bn_plan(int64_t R, int64_t C);

// LDS-tiled MFMA GEMMs for transformer-sized linears with the MLP's
// elementwise work in their epilogues (gemm_kernels.hip). Operands are 2-D,
// contiguous, 16-byte aligned, f32 or bf16 alike; every feature dimension is
// a multiple of 16, the row count M is any number >= 0. Anything else is
// refused before a launch; empty problems launch nothing, and an empty
// contraction gives zeros (plus the bias). Results may be preallocated.
// gemm_nt: y[M,N] = x[M,K] w[N,K]^T + bias. With gelu it returns (h, a):
//   h the linear output rounded to the storage dtype, a = gelu(h) (exact erf
//   form) of that rounded h; `y` is then the buffer for a.
// gemm_nn: dx[M,K] = dy[M,N] w[N,K]; with gelu_grad_of = h [M,K] the result
//   is multiplied by gelu'(h) on its way out.
// gemm_tn: (dw[N,K] = dy[M,N]^T x[M,K], db[N] = sum_m dy), both overwritten,
//   summed in an order fixed by the shape: reproducible, no atomics.
// gemm_tile_shape: (BM, BN, BK) of the workgroup tile.
// gelu_grad_mul: da * gelu'(h) elementwise, for a GELU whose gradient has no
//   GEMM to ride in (da and h as the operands above, of one shape).
std::vector<torch::Tensor> gemm_nt(
    torch::Tensor x, torch::Tensor w,
    c10::optional<torch::Tensor> bias = c10::nullopt, bool gelu = false,
    c10::optional<torch::Tensor> y = c10::nullopt,
    c10::optional<torch::Tensor> h = c10::nullopt);
torch::Tensor gemm_nn(torch::Tensor dy, torch::Tensor w,
                      c10::optional<torch::Tensor> gelu_grad_of = c10::nullopt,
                      c10::optional<torch::Tensor> dx = c10::nullopt);
std::vector<torch::Tensor> gemm_tn(
    torch::Tensor dy, torch::Tensor x,
    c10::optional<torch::Tensor> dw = c10::nullopt,
    c10::optional<torch::Tensor> db = c10::nullopt);
std::vector<int64_t> gemm_tile_shape();
torch::Tensor gelu_grad_mul(torch::Tensor da, torch::Tensor h);

// Implicit-GEMM convolutions for a channels-last ResNet (conv_kernels.hip):
// kernel size k in {1, 3}, padding k/2, stride 1 or 2, no bias, groups or
// dilation. x is [N*H*W, Cin], y and dy are [M, Cout] with M = N*Ho*Wo and
// Ho = (H + 2*(k/2) - k)/stride + 1: the 2-D channels-last matrices. wp is
// the weight PACKED as [Cout, k*k, Cin]. All of them contiguous, 16-byte
// aligned, f32 or bf16 alike; Cin and Cout multiples of 16; N*H*W < 2^31,
// N >= 0, H, W >= 1. Anything else is refused before a launch; N == 0
// launches none of our kernels (y and dx are empty, and the one thing that
// runs is torch's fill of dw with zeros, the sum over no pixels).
// Accumulation is f32 with one rounding on the store.
// conv2d_fwd returns y; conv2d_bwd_input returns dx [N*H*W, Cin], every row
//   stored once (the untouched rows of a strided 1x1 as zeros).
// conv2d_bwd_weight returns dw in the PARAMETER's layout [Cout, Cin, k, k];
//   a preallocated dw may be f32 or bf16 whatever the operands' dtype. The
//   sum over the M output pixels is split into GS slices whose f32 tiles go
//   through a workspace [GS, Cout, k*k, Cin] and are added in slice order: no
//   atomics, the same bits run to run.
// conv_wgrad_plan: (tile rows, tile columns, GS, rows per slice), a function
//   of (M, Cout, Cin, taps = k*k) alone.
torch::Tensor conv2d_fwd(torch::Tensor x, torch::Tensor wp, int64_t N,
                         int64_t H, int64_t W, int64_t stride);
torch::Tensor conv2d_bwd_input(torch::Tensor dy, torch::Tensor wp, int64_t N,
                               int64_t H, int64_t W, int64_t stride);
torch::Tensor conv2d_bwd_weight(torch::Tensor dy, torch::Tensor x, int64_t N,
                                int64_t H, int64_t W, int64_t k,
                                int64_t stride,
                                c10::optional<torch::Tensor> dw = c10::nullopt);
std::vector<int64_t> conv_wgrad_plan(int64_t M, int64_t Cout, int64_t Cin,
                                     int64_t taps);

// Cross-entropy with class-probability targets (C may be 1: the reference's
// degenerate Linear(20,1) case, single_gpu.py:24 + utils.py:7).
// Returns (loss[scalar], probs[B,C], tsum[B]).
std::vector<torch::Tensor> ce_fwd(torch::Tensor y, torch::Tensor t);
// gout: optional device f32 scalar (autograd's incoming grad) folded
// into the kernel — saves the separate dy*gout launch per step.
torch::Tensor ce_bwd(torch::Tensor probs, torch::Tensor t,
                     torch::Tensor tsum, double grad_scale,
                     c10::optional<torch::Tensor> gout = c10::nullopt);

// Cross-entropy on integer class labels with label smoothing, ignore_index
// and reduction "mean" | "sum" | "none" (loss_kernels.hip): F.cross_entropy's
// semantics for class indices without class weights. logits [..., C]
// contiguous, 16-byte aligned, f32 or bf16, C >= 1; labels int64 or int32,
// contiguous, of the leading shape; label_smoothing in [0, 1]. Anything else
// is refused before a launch; no rows launches nothing. Nothing is read back
// to the host. A label that is neither ignore_index nor in [0, C) is never
// used as an address: that row's loss and dlogits row are NaN and it counts
// as non-ignored.
// cei_fwd returns (loss f32 [] or [...], row_stats f32 [B, 2] = (row max,
//   1 / sum exp(y - max)), inv_count f32 [1] = 1 or 1 / #non-ignored rows).
//   workspace is f32 [B, S, 4] with S = cei_plan(B, C)[0].
// cei_bwd returns dlogits, rounded once to the logits' dtype. grad is the
//   incoming gradient as a contiguous f32 device tensor, one value ("mean",
//   "sum") or one per row ("none"); without it the gradient of the loss
//   itself. Loss, count and dlogits are the same bits run to run.
// cei_plan: (S, L), the column segments per row and their length, a function
//   of (B, C) alone. cei_grid_cap: the cap on the row kernels' grid.
std::vector<torch::Tensor> cei_fwd(
    torch::Tensor logits, torch::Tensor labels, double label_smoothing,
    int64_t ignore_index, const std::string& reduction,
    c10::optional<torch::Tensor> row_stats = c10::nullopt,
    c10::optional<torch::Tensor> workspace = c10::nullopt);
torch::Tensor cei_bwd(c10::optional<torch::Tensor> grad, torch::Tensor logits,
                      torch::Tensor labels, torch::Tensor row_stats,
                      torch::Tensor inv_count, double label_smoothing,
                      int64_t ignore_index, const std::string& reduction,
                      c10::optional<torch::Tensor> dlogits = c10::nullopt);
std::vector<int64_t> cei_plan(int64_t B, int64_t C);
int64_t cei_grid_cap();

// MSE (reference multinode_torchrun.py:46). Returns loss[scalar].
torch::Tensor mse_fwd(torch::Tensor y, torch::Tensor t);
torch::Tensor mse_bwd(torch::Tensor y, torch::Tensor t, double grad_scale,
                      c10::optional<torch::Tensor> gout = c10::nullopt);

// Fused SGD over a flat bucket (optim_kernels.hip): p -= lr*g; optionally
// g = 0 in the same kernel (folds reference optimizer.step() + zero_grad,
// single_gpu.py:22,26). Like the stateful optimizers below it requires
// device tensors of one dtype and length, padded and aligned to 4 elements.
// grad_scale (all three update ops): optional f32[1] device tensor, the
// clip coefficient of clip_coef below. With it the update uses g * coef
// (for bf16 rounded to bf16, as grad.mul_(coef) would store it); g itself
// is not rewritten — zeroed with zero_grad, left UNSCALED without.
void sgd_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
              double lr, bool zero_grad,
              c10::optional<torch::Tensor> grad_scale = c10::nullopt);

// Momentum SGD over a flat bucket, torch.optim.SGD's
// formula without dampening:
//   d = g + wd*p; buf = mu*buf + d; d = nesterov ? d + mu*buf : buf;
//   p -= lr*d; g = 0 when zero_grad.
// buf is f32 of the bucket's length whatever the parameter dtype and starts
// at zero (which reproduces torch's first-step buf = d); without a buf the
// momentum must be 0 (weight decay only).
void sgd_momentum_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
                       c10::optional<torch::Tensor> buf, double lr,
                       double momentum, double weight_decay, bool nesterov,
                       bool zero_grad,
                       c10::optional<torch::Tensor> grad_scale = c10::nullopt);

// AdamW over a flat bucket with the step count on the device, so that a
// captured graph advances it on replay. step_state is int32[4]:
// [0] the step t, [1]/[2] the f32 bits of -(lr/(1-b1^t)) and 1/sqrt(1-b2^t).
// adamw_tick advances it ONCE per optimizer step, ahead of the per-bucket
// adamw_flat launches on the same stream, which only read it.
// decay_mask: optional uint8, one byte per 4-element group; 0 = no decay.
void adamw_tick(torch::Tensor step_state, double lr, double beta1,
                double beta2);
void adamw_flat(torch::Tensor param_flat, torch::Tensor grad_flat,
                torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                torch::Tensor step_state, double lr, double beta1,
                double beta2, double eps, double weight_decay,
                c10::optional<torch::Tensor> decay_mask, bool zero_grad,
                c10::optional<torch::Tensor> grad_scale = c10::nullopt);

// Global grad-norm clipping over the flat buckets. grad_sumsq_flat leaves
// one f64 partial sum of squares per block in `partials`, which must have
// exactly sumsq_slots(numel) elements, all rewritten on every call (no
// atomics, nothing to pre-zero). clip_coef, once per step after every
// bucket's grad_sumsq_flat, sums all of `partials` (the buckets' segments
// side by side) in a fixed order and writes clip_state (f32[2]):
//   [0] total_norm = sqrt(sum), [1] coef = min(1, max_norm/(norm + 1e-6))
// in torch.nn.utils.clip_grad_norm_'s own f32 operation sequence.
int64_t sumsq_slots(int64_t numel);
void grad_sumsq_flat(torch::Tensor grad_flat, torch::Tensor partials);
void clip_coef(torch::Tensor partials, torch::Tensor clip_state,
               double max_norm);

// Bucket gather/scatter ("flatten/unflatten"): one launch
// moves every listed tensor <-> its segment of the flat bucket.
// plan: int64 device tensor [blocks, 3], one row (tensor chunk address,
// bucket byte offset, nbytes) per workgroup; build_copy_plan makes it once
// on `device` and the reducer reuses it every step.
torch::Tensor build_copy_plan(const std::vector<torch::Tensor>& tensors,
                              const std::vector<int64_t>& offsets,
                              torch::Device device);
void flatten_into(torch::Tensor bucket, torch::Tensor plan,
                  int64_t total_blocks, bool zero_src);
void unflatten_from(torch::Tensor bucket, torch::Tensor plan, int64_t total_blocks);

// Fused toy training step: given X[B,K], T[B,1], flat params (w|b) and flat
// grads (dw|db) for Linear(K,1), computes fwd+MSE-or-CE loss grad+bwd and
// writes gradients into the bucket in ONE kernel launch (the latency-bound
// toy path, SURVEY §7 hard-part 2).
// lr > 0: apply the SGD update in-kernel (world-size-1 single-launch step);
// lr <= 0: write gradients into grad_flat for the all-reduce path.
// With lr > 0 grad_flat is never touched and may be left out, which means an
// undefined or an EMPTY tensor (torch.Tensor() from Python). Any non-empty
// grad_flat is checked like param_flat (toy_check_args below) whatever lr
// is: a placeholder of another dtype, device or size is refused.
void toy_fused_fwd_bwd(torch::Tensor x, torch::Tensor t,
                       torch::Tensor param_flat, torch::Tensor grad_flat,
                       torch::Tensor loss_out, bool use_mse,
                       int64_t w_off, int64_t b_off, double lr);

// Epoch shard gather with an in-kernel seeded permutation (see
// kernels.hip): returns (xs [n/world, K], ts [n/world, 1]) for this rank.
std::vector<torch::Tensor> epoch_shard(torch::Tensor X, torch::Tensor Tg,
                                       int64_t seed, int64_t rank,
                                       int64_t world);

// Multi-epoch form: gathers `epochs` consecutive shards (seeds seed0,
// seed0+1, …) in ONE launch; block e is bitwise epoch_shard(seed0+e),
// which is this call with epochs = 1.
std::vector<torch::Tensor> epoch_shard_multi(torch::Tensor X, torch::Tensor Tg,
                                             int64_t seed0, int64_t epochs,
                                             int64_t rank, int64_t world);

// Multi-step persistent toy trainer (world-1): x is [S*batch, K] of S
// consecutive batches; runs S full fwd+loss+bwd+SGD steps in ONE launch
// (bitwise-identical per-step arithmetic to toy_fused_fwd_bwd with
// in-kernel SGD for f32). Dispatch: batch 32/64 with K 20 takes a
// compile-time kernel — fp32 the chain or MFMA spec kernel (selector below),
// bf16 the wide-MFMA k_toy_multistep_bf16w, which matches to bf16 accuracy;
// every other B <= 128, K <= 32 takes the generic k_toy_multistep, which
// shares its tile step with the single-step kernel. loss_out, when
// non-empty, receives the LAST step's loss.
void toy_multistep(torch::Tensor x, torch::Tensor t, torch::Tensor param_flat,
                   torch::Tensor loss_out, bool use_mse,
                   int64_t w_off, int64_t b_off, double lr, int64_t batch);

// The launcher under toy_multistep, on raw device pointers: x/t point at the
// first of S consecutive [B, K] / [B] tiles of storage dtype f32 or bf16
// (param has the same dtype, loss is f32 or null). It does toy_multistep's
// kernel dispatch, reading the selector and the ring depth below at launch
// time, launches on the current stream and checks hipGetLastError. The
// caller has validated shapes, dtypes and devices: B <= 128, K <= 32,
// S >= 1, lr > 0. The native stepper (ToyShardRun, bindings.hip) validates
// once per bind and then launches through this.
void toy_multistep_launch(const void* x, const void* t, void* param,
                          float* loss, bool use_mse, int w_off, int b_off,
                          float lr, int B, int K, int S, bool bf16);
// Validated pointer of the optional f32 loss output (nullptr when empty).
float* toy_loss_ptr(const torch::Tensor& loss_out);

// The argument check shared by every toy entry point, complete before any
// launch: x [rows, K] contiguous f32/bf16 on a GPU; t contiguous with one
// target per row; param (and grad, where given) contiguous, of x's dtype, on
// x's device; 1 <= batch <= 128 dividing rows (batch < 0: the whole of x),
// 1 <= K <= 32; w_off, b_off >= 0 with [w_off, w_off + K) and b_off inside
// the bucket and b_off outside the weights; loss_out empty or f32 on x's
// device. grad == nullptr: no gradient bucket; need_grad: it must be given,
// i.e. defined and not empty (the single step with lr <= 0 writes it).
// S == 0: nothing to run.
struct ToyDims {
  int B, K, S;
};
ToyDims toy_check_args(const char* who, const torch::Tensor& x,
                       const torch::Tensor& t, const torch::Tensor& param,
                       const torch::Tensor* grad, bool need_grad,
                       const torch::Tensor& loss_out, int64_t w_off,
                       int64_t b_off, int64_t batch);

// Process-wide kernel selector for the fp32 batch-32/64, K-20 multi-step
// fast path: "chain" (lane-parallel fmaf chains on the vector ALU, the
// default) or "mfma" (k_toy_multistep_spec). Both produce the same bits.
// Initialised from MI355X_TOY_MULTISTEP. The chain kernel's prefetch ring
// depth (2, 3 or 4; 0 = the measured default) is a tuning aid for
// tools/bench_multistep_curve.py.
void set_toy_multistep_impl(const std::string& name);
std::string get_toy_multistep_impl();
void set_toy_multistep_chain_depth(int64_t depth);

// Multi-step trainer with an IN-KERNEL xGMI mesh all-reduce per step
// (world > 1): the deferred-launch engine at any world size, one
// collective exchange per step without leaving the kernel.
void toy_multistep_mesh(torch::Tensor x, torch::Tensor t,
                        torch::Tensor param_flat, torch::Tensor loss_out,
                        bool use_mse, int64_t w_off, int64_t b_off, double lr,
                        int64_t batch, P2pMesh& mesh);

// What the mesh kernels need beyond toy_check_args: a fast-path shape (batch
// 32 or 64, K 20) and a connected mesh.
void toy_check_mesh_args(const char* who, const ToyDims& d,
                         const P2pMesh& mesh);
// The launcher under toy_multistep_mesh, on raw device pointers, as
// toy_multistep_launch is under toy_multistep (K is 20). The caller has
// passed toy_check_args and toy_check_mesh_args, S >= 1, lr > 0: nothing
// here can refuse the launch, so the S sequence numbers it takes from the
// mesh are always used.
void toy_multistep_mesh_launch(const void* x, const void* t, void* param,
                               float* loss, bool use_mse, int w_off,
                               int b_off, float lr, int B, int S, bool bf16,
                               P2pMesh& mesh);

}  // namespace mi355x
