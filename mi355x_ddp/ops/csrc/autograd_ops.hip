// C++ autograd Functions over the MI355X kernel pack.
//
// The Python dispatch layer (ops/__init__.py) originally wrapped the HIP
// kernels in Python torch.autograd.Function subclasses; every forward AND
// every backward node then re-entered the interpreter (GIL acquire +
// Python frame) — measured as the dominant cost of the generic DDP path
// (profiles/README.md r01f: 147 us/step, VERDICT round-1 weak #1).
// These torch::autograd::Function equivalents keep the whole
// forward/backward chain in C++: with the ReducerCore hooks the generic
// path's backward never enters Python at all.
//
// Semantics are identical to the Python Functions they replace
// (ops/__init__.py _HipLinearFn/_HipMSEFn/_HipCEFn), including the
// library-GEMM routing split (hipBLASLt/rocBLAS via torch::mm for plain
// library-sized GEMMs; hand MFMA kernels otherwise).
#include <torch/extension.h>

#include "ops.h"

namespace mi355x {

namespace {

// Measured crossover on MI355X (profiles/kernel_bench_r01.md): rocBLAS
// wins from ~2^20 K*N contractions; the hand MFMA kernels win below.
// Keep in sync with ops/__init__.py::_library_gemm_shape.
inline bool library_gemm_shape(int64_t k, int64_t n) {
  return k * n >= (int64_t(1) << 20);
}

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

struct LinearFn : public torch::autograd::Function<LinearFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor w, torch::Tensor b) {
    ctx->save_for_backward({x, w});
    ctx->saved_data["has_bias"] = b.defined();
    auto xc = x.contiguous();
    if (library_gemm_shape(w.size(1), w.size(0))) {
      if (b.defined()) return torch::addmm(b, xc, w.t());
      return torch::mm(xc, w.t());
    }
    return linear_fwd(xc, w, b.defined() ? c10::optional<torch::Tensor>(b)
                                         : c10::nullopt);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    auto x = saved[0], w = saved[1];
    bool has_bias = ctx->saved_data["has_bias"].toBool();
    auto dy = grads[0].contiguous();
    torch::Tensor dx, dw, db;
    auto needs = ctx->needs_input_grad(0);
    if (needs) {
      if (library_gemm_shape(w.size(1), w.size(0))) {
        dx = torch::mm(dy, w);
      } else {
        dx = linear_bwd_input(dy, w);
      }
    }
    if (ctx->needs_input_grad(1) ||
        (has_bias && ctx->needs_input_grad(2))) {
      dw = torch::empty_like(w);
      db = torch::empty({w.size(0)}, w.options());
      linear_bwd_weight(x, dy, dw, db, /*accumulate=*/false);
    }
    if (!has_bias) db = torch::Tensor();
    return {dx, dw, db};
  }
};

struct MseFn : public torch::autograd::Function<MseFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor y,
                               torch::Tensor t) {
    ctx->save_for_backward({y, t});
    return mse_fwd(y, t);
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const auto& g0 = grads[0];
    // capture-safe: no D2H read of the incoming grad — when it is the
    // usual device f32 scalar (autograd's seed), fold it INTO the bwd
    // kernel; otherwise scale with a separate elementwise multiply
    if (g0.defined() && g0.is_cuda() && g0.numel() == 1 &&
        g0.scalar_type() == at::kFloat) {
      return {mse_bwd(saved[0], saved[1], 1.0, g0), torch::Tensor()};
    }
    auto dy = mse_bwd(saved[0], saved[1], 1.0, c10::nullopt);
    dy = dy * g0;
    return {dy, torch::Tensor()};
  }
};

struct CeFn : public torch::autograd::Function<CeFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor y,
                               torch::Tensor t) {
    auto outs = ce_fwd(y, t);  // (loss, probs, tsum)
    ctx->save_for_backward({outs[1], t, outs[2]});
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const auto& g0 = grads[0];
    if (g0.defined() && g0.is_cuda() && g0.numel() == 1 &&
        g0.scalar_type() == at::kFloat) {  // fold the seed into the kernel
      return {ce_bwd(saved[0], saved[1], saved[2], 1.0, g0),
              torch::Tensor()};
    }
    auto dy = ce_bwd(saved[0], saved[1], saved[2], 1.0, c10::nullopt);
    dy = dy * g0;
    return {dy, torch::Tensor()};
  }
};

// Cross-entropy on class indices. Saved for the backward: the logits, the
// labels, row_stats [B, 2] and the device scalar inv_count; there is no
// [B, C] f32 tensor. The incoming gradient is read by the kernel when it is
// f32 on the device (the scalar seed, or one value per row for "none");
// anything else is multiplied in afterwards. Nothing is read back.
struct CeiFn : public torch::autograd::Function<CeiFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor logits,
                               torch::Tensor labels, double label_smoothing,
                               int64_t ignore_index, std::string reduction) {
    auto outs = cei_fwd(logits, labels, label_smoothing, ignore_index,
                        reduction);  // (loss, row_stats, inv_count)
    ctx->save_for_backward({logits, labels, outs[1], outs[2]});
    ctx->saved_data["label_smoothing"] = label_smoothing;
    ctx->saved_data["ignore_index"] = ignore_index;
    ctx->saved_data["reduction"] = reduction;
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const double eps = ctx->saved_data["label_smoothing"].toDouble();
    const int64_t ignore = ctx->saved_data["ignore_index"].toInt();
    const std::string red = ctx->saved_data["reduction"].toStringRef();
    const auto& g0 = grads[0];
    const bool fold = g0.defined() && g0.is_cuda() &&
                      g0.scalar_type() == at::kFloat &&
                      (red == "none" || g0.numel() == 1);
    auto dy = cei_bwd(fold ? c10::optional<torch::Tensor>(g0.contiguous())
                           : c10::nullopt,
                      saved[0], saved[1], saved[2], saved[3], eps, ignore, red);
    if (!fold) dy = dy * (red == "none" ? g0.unsqueeze(-1) : g0);
    return {dy, torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor()};
  }
};

// Fused self-attention on the packed in-projection output. Saved for the
// backward: qkv and the forward's row statistics, and above 64 tokens, where
// the tiled kernels run, the output too (their delta comes from it).
struct AttnFn : public torch::autograd::Function<AttnFn> {
  static bool tiled(const torch::Tensor& qkv) {
    return qkv.dim() == 3 && qkv.size(1) > 64;
  }

  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor qkv,
                               int64_t heads) {
    ctx->saved_data["heads"] = heads;
    if (tiled(qkv)) {
      auto outs = attn_tiled_fwd(qkv, heads);  // (out, row_stats)
      ctx->save_for_backward({qkv, outs[1], outs[0]});
      return outs[0];
    }
    auto outs = attn_fwd(qkv, heads);
    ctx->save_for_backward({qkv, outs[1]});
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const int64_t heads = ctx->saved_data["heads"].toInt();
    auto dout = grads[0].contiguous();
    return {tiled(saved[0])
                ? attn_tiled_bwd(dout, saved[0], saved[2], saved[1], heads)
                : attn_bwd(dout, saved[0], saved[1], heads),
            torch::Tensor()};
  }
};

// The same on the bf16 wide-MFMA kernels, for every N they take. Saved for the
// backward: qkv, the row statistics and the output.
struct AttnBf16Fn : public torch::autograd::Function<AttnBf16Fn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor qkv,
                               int64_t heads) {
    ctx->saved_data["heads"] = heads;
    auto outs = attn_bf16_fwd(qkv, heads);  // (out, row_stats)
    ctx->save_for_backward({qkv, outs[1], outs[0]});
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const int64_t heads = ctx->saved_data["heads"].toInt();
    return {attn_bf16_bwd(grads[0].contiguous(), saved[0], saved[2], saved[1],
                          heads),
            torch::Tensor()};
  }
};

// Fused LayerNorm. Saved for the backward: the input, the forward's row
// statistics and the weight; the output is not kept.
struct LayerNormFn : public torch::autograd::Function<LayerNormFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor w, torch::Tensor b, double eps) {
    auto outs = ln_fwd(x, w, b, eps);  // (y, row_stats)
    ctx->save_for_backward({x, outs[1], w});
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    auto g = ln_bwd(grads[0].contiguous(), saved[0], saved[1], saved[2]);
    return {g[0], g[1], g[2], torch::Tensor()};
  }
};

// s = x + residual, y = LayerNorm(s), both returned. The backward re-reads s
// (saved with the statistics and the weight) and folds the gradient arriving
// at s into dx; ONE dx tensor is the gradient of x and of the residual.
struct AddLayerNormFn : public torch::autograd::Function<AddLayerNormFn> {
  static variable_list forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor r, torch::Tensor w,
                               torch::Tensor b, double eps) {
    auto outs = ln_fwd(x, w, b, eps, r);  // (s, y, row_stats)
    ctx->save_for_backward({outs[0], outs[2], w});
    ctx->set_materialize_grads(false);
    return {outs[0], outs[1]};
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto& ds = grads[0];
    const auto& dy = grads[1];
    if (!dy.defined())  // only s was used: the add's own backward
      return {ds, ds, torch::Tensor(), torch::Tensor(), torch::Tensor()};
    auto saved = ctx->get_saved_variables();
    auto g = ln_bwd(dy.contiguous(), saved[0], saved[1], saved[2],
                    ds.defined()
                        ? c10::optional<torch::Tensor>(ds.contiguous())
                        : c10::nullopt);
    return {g[0], g[0], g[1], g[2], torch::Tensor()};
  }
};

// z = act(batch_norm(x) + residual) in training mode. Saved for the backward:
// x, col_stats, the weight and, with ReLU, the output z, whose sign is the
// mask; no mask tensor exists. The running statistics and the batch counter
// are updated in place by the forward's second launch. Every tensor argument
// is a defined tensor: without a residual (add false) or a counter (count
// false) the caller passes a placeholder that is not looked at.
struct BatchNormActFn : public torch::autograd::Function<BatchNormActFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor residual, torch::Tensor weight,
                               torch::Tensor bias, torch::Tensor running_mean,
                               torch::Tensor running_var,
                               torch::Tensor batches, bool add, bool count,
                               bool relu, double momentum, double eps) {
    auto opt = [](bool given, const torch::Tensor& t) {
      return given ? c10::optional<torch::Tensor>(t) : c10::nullopt;
    };
    auto outs = bn_fwd(x, weight, bias, running_mean, running_var,
                       /*training=*/true, momentum, eps, relu,
                       opt(add, residual),
                       opt(count, batches));  // (z, col_stats)
    if (relu) ctx->save_for_backward({x, outs[1], weight, outs[0]});
    else ctx->save_for_backward({x, outs[1], weight});
    ctx->saved_data["add"] = add;
    return outs[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const bool add = ctx->saved_data["add"].toBool();
    auto g = bn_bwd(grads[0].contiguous(), saved[0], saved[1], saved[2],
                    saved.size() > 3 ? c10::optional<torch::Tensor>(saved[3])
                                     : c10::nullopt,
                    add);  // (dx, dgamma, dbeta[, dresidual])
    return {g[0], add ? g[3] : torch::Tensor(), g[1], g[2], torch::Tensor(),
            torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

// The two GEMMs that turn the gradient arriving at h into the gradients of a
// linear layer's input, weight and bias; what is not needed is not computed.
variable_list linear_grads(AutogradContext* ctx, const torch::Tensor& dh,
                           const torch::Tensor& x, const torch::Tensor& w,
                           int first) {
  torch::Tensor dx, dw, db;
  if (ctx->needs_input_grad(first + 1) || ctx->needs_input_grad(first + 2)) {
    auto g = gemm_tn(dh, x);
    dw = g[0], db = g[1];
  }
  if (ctx->needs_input_grad(first)) dx = gemm_nn(dh, w);
  return {dx, dw, db};
}

// gelu(x w^T + b) on the tiled GEMMs: the bias add and GELU ride in the
// forward GEMM's epilogue. The backward has no second weight to fold gelu'
// into, so dh = da * gelu'(h) is one elementwise HIP kernel (gelu_grad_mul)
// ahead of TN and NN. Saved: x, w and h, the linear output.
struct LinearGeluFn : public torch::autograd::Function<LinearGeluFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor w, torch::Tensor b) {
    auto outs = gemm_nt(x, w, b, /*gelu=*/true);  // (h, a)
    ctx->save_for_backward({x, w, outs[0]});
    return outs[1];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const auto &x = saved[0], &w = saved[1], &h = saved[2];
    auto dh = gelu_grad_mul(grads[0].contiguous(), h);
    return linear_grads(ctx, dh, x, w, 0);
  }
};

// Linear -> GELU -> Linear. Forward: NT+GELU, NT+bias. Backward: TN(dy, a),
// NN+GELU'(dy, w2, h), TN(dh, x), NN(dh, w1): six GEMM launches and no
// elementwise kernel. Saved: x, h, a and the weights.
struct MlpFn : public torch::autograd::Function<MlpFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor w1, torch::Tensor b1,
                               torch::Tensor w2, torch::Tensor b2) {
    auto ha = gemm_nt(x, w1, b1, /*gelu=*/true);  // (h, a)
    ctx->save_for_backward({x, ha[0], ha[1], w1, w2});
    return gemm_nt(ha[1], w2, b2)[0];
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const auto &x = saved[0], &h = saved[1], &a = saved[2], &w1 = saved[3],
               &w2 = saved[4];
    auto dy = grads[0].contiguous();
    torch::Tensor dw2, db2;
    if (ctx->needs_input_grad(3) || ctx->needs_input_grad(4)) {
      auto g = gemm_tn(dy, a);
      dw2 = g[0], db2 = g[1];
    }
    variable_list first = {torch::Tensor(), torch::Tensor(), torch::Tensor()};
    if (ctx->needs_input_grad(0) || ctx->needs_input_grad(1) ||
        ctx->needs_input_grad(2))
      first = linear_grads(ctx, gemm_nn(dy, w2, h), x, w1, 0);
    return {first[0], first[1], first[2], dw2, db2};
  }
};

// y = conv2d(x, weight) on the implicit-GEMM kernels. `x` is the 2-D
// channels-last matrix, `weight` the parameter [Cout, Cin, k, k] (or its
// autocast copy) that receives the gradient, `wp` the same values packed as
// [Cout, k*k, Cin], which the kernels read; it takes no gradient. Saved: x
// and wp. dW is stored in weight's layout and dtype by the kernels.
struct Conv2dFn : public torch::autograd::Function<Conv2dFn> {
  static torch::Tensor forward(AutogradContext* ctx, torch::Tensor x,
                               torch::Tensor weight, torch::Tensor wp,
                               int64_t N, int64_t H, int64_t W,
                               int64_t stride) {
    TORCH_CHECK(weight.dim() == 4 && wp.dim() == 3 &&
                    weight.size(0) == wp.size(0) &&
                    weight.size(1) == wp.size(2) &&
                    weight.size(2) * weight.size(3) == wp.size(1) &&
                    weight.size(2) == weight.size(3),
                "conv2d_autograd: wp must be weight packed as "
                "[Cout, k*k, Cin]");
    auto y = conv2d_fwd(x, wp, N, H, W, stride);
    ctx->save_for_backward({x, wp});
    ctx->saved_data["dims"] = std::vector<int64_t>{N, H, W, stride,
                                                   weight.size(2)};
    ctx->saved_data["bf16"] = weight.scalar_type() == at::kBFloat16;
    return y;
  }

  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    const auto &x = saved[0], &wp = saved[1];
    const auto d = ctx->saved_data["dims"].toIntVector();
    auto dy = grads[0].contiguous();
    torch::Tensor dx, dw;
    if (ctx->needs_input_grad(0))
      dx = conv2d_bwd_input(dy, wp, d[0], d[1], d[2], d[3]);
    if (ctx->needs_input_grad(1)) {
      dw = torch::empty(
          {wp.size(0), wp.size(2), d[4], d[4]},
          wp.options().dtype(ctx->saved_data["bf16"].toBool() ? at::kBFloat16
                                                              : at::kFloat));
      conv2d_bwd_weight(dy, x, d[0], d[1], d[2], d[4], d[3], dw);
    }
    return {dx, dw, torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor(), torch::Tensor()};
  }
};

}  // namespace

torch::Tensor conv2d_autograd(torch::Tensor x, torch::Tensor weight,
                              torch::Tensor wp, int64_t N, int64_t H,
                              int64_t W, int64_t stride) {
  return Conv2dFn::apply(x, weight, wp, N, H, W, stride);
}

torch::Tensor mlp_autograd(torch::Tensor x, torch::Tensor w1, torch::Tensor b1,
                           torch::Tensor w2, torch::Tensor b2) {
  return MlpFn::apply(x, w1, b1, w2, b2);
}

torch::Tensor linear_gelu_autograd(torch::Tensor x, torch::Tensor w,
                                   torch::Tensor b) {
  return LinearGeluFn::apply(x, w, b);
}

torch::Tensor layer_norm_autograd(torch::Tensor x, torch::Tensor weight,
                                  torch::Tensor bias, double eps) {
  return LayerNormFn::apply(x, weight, bias, eps);
}

std::vector<torch::Tensor> add_layer_norm_autograd(torch::Tensor x,
                                                   torch::Tensor residual,
                                                   torch::Tensor weight,
                                                   torch::Tensor bias,
                                                   double eps) {
  return AddLayerNormFn::apply(x, residual, weight, bias, eps);
}

torch::Tensor batch_norm_act_autograd(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var,
    c10::optional<torch::Tensor> residual, bool relu, bool training,
    double momentum, double eps,
    c10::optional<torch::Tensor> num_batches_tracked) {
  if (training)
    return BatchNormActFn::apply(
        x, residual.has_value() ? *residual : x, weight, bias, running_mean,
        running_var,
        num_batches_tracked.has_value() ? *num_batches_tracked : running_mean,
        residual.has_value(), num_batches_tracked.has_value(), relu, momentum,
        eps);
  // evaluation: one launch from the running statistics, and no backward
  const bool wants_grad =
      torch::GradMode::is_enabled() &&
      (x.requires_grad() || weight.requires_grad() || bias.requires_grad() ||
       (residual.has_value() && residual->requires_grad()));
  TORCH_CHECK(!wants_grad,
              "batch_norm_act: gradients in evaluation mode (training=False) "
              "are not supported; run under torch.no_grad()");
  return bn_fwd(x, weight, bias, running_mean, running_var, false, momentum,
                eps, relu, residual)[0];
}

torch::Tensor linear_autograd(torch::Tensor x, torch::Tensor w,
                              c10::optional<torch::Tensor> b) {
  return LinearFn::apply(x, w, b.has_value() ? *b : torch::Tensor());
}

torch::Tensor mse_autograd(torch::Tensor y, torch::Tensor t) {
  return MseFn::apply(y, t);
}

torch::Tensor ce_autograd(torch::Tensor y, torch::Tensor t) {
  return CeFn::apply(y, t);
}

torch::Tensor cei_autograd(torch::Tensor logits, torch::Tensor labels,
                           double label_smoothing, int64_t ignore_index,
                           const std::string& reduction) {
  return CeiFn::apply(logits, labels, label_smoothing, ignore_index,
                      reduction);
}

torch::Tensor attention_autograd(torch::Tensor qkv, int64_t heads,
                                 const std::string& matrix) {
  TORCH_CHECK(matrix == "f32" || matrix == "bf16",
              "attention_autograd: matrix must be 'f32' or 'bf16', got '",
              matrix, "'");
  return matrix == "bf16" ? AttnBf16Fn::apply(qkv, heads)
                          : AttnFn::apply(qkv, heads);
}

}  // namespace mi355x
