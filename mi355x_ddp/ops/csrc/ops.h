// Host-side launcher declarations for the MI355X (gfx950) kernel pack.
// Implementations in kernels.hip, for the toy training-step family
// (toy_fused_fwd_bwd, toy_multistep*) toy_kernels.hip, and for the
// flat-bucket optimizers optim_kernels.hip; bound to Python in bindings.hip.
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

// Cross-entropy with class-probability targets (C may be 1: the reference's
// degenerate Linear(20,1) case, single_gpu.py:24 + utils.py:7).
// Returns (loss[scalar], probs[B,C], tsum[B]).
std::vector<torch::Tensor> ce_fwd(torch::Tensor y, torch::Tensor t);
// gout: optional device f32 scalar (autograd's incoming grad) folded
// into the kernel — saves the separate dy*gout launch per step.
torch::Tensor ce_bwd(torch::Tensor probs, torch::Tensor t,
                     torch::Tensor tsum, double grad_scale,
                     c10::optional<torch::Tensor> gout = c10::nullopt);

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
