// Python bindings for the mi355x_ddp native layer (kernels + RCCL comm).
#include <torch/extension.h>

#include <functional>
#include <memory>
#include <utility>
#include <vector>

#include "ops.h"
#include "p2p_mesh.h"
#include "rccl_comm.h"
#include "reducer_core.h"
#include "shard_run.h"

namespace mi355x {
// autograd_ops.hip
torch::Tensor linear_autograd(torch::Tensor x, torch::Tensor w,
                              c10::optional<torch::Tensor> b);
torch::Tensor mse_autograd(torch::Tensor y, torch::Tensor t);
torch::Tensor ce_autograd(torch::Tensor y, torch::Tensor t);

// The run tracker behind PersistentToyStep: shard_run.h's OrderedRuns over
// the pointer-level launchers, toy_multistep_launch at world 1 and
// toy_multistep_mesh_launch with a mesh. It defers two kinds of run, the
// index run of the shard-bound protocol and the tensor run of step(x, t),
// and OrderedRuns keeps them in submission order. Everything is validated
// where a run STARTS (bind_shard; the first tensor of a tensor run), so a
// launch is pointer arithmetic plus the kernel dispatch and cannot be
// refused: with a mesh, no sequence range is taken for a launch that does
// not happen. step_shard(i) is a few integer operations.
// The recorder variant has the same trackers and entry points but only notes
// its launches and touches no GPU API, so the schedule, the ordering and the
// host-loop cost are testable without a GPU.
class ToyShardRun : public std::enable_shared_from_this<ToyShardRun> {
  struct Noted {
    bool tensors;
    int64_t first, n;  // first step, or the first span's x address
  };

 public:
  using Runs = OrderedRuns<std::function<void(int64_t, int64_t)>,
                           std::function<void(const Span&, int64_t)>>;

  // With a mesh every rank must issue the same launches in the same order,
  // so the schedule may depend on the submitted steps alone: no ramp, which
  // starts at whichever flush a rank happens to make.
  ToyShardRun(torch::Tensor flat_param, torch::Tensor loss_out, bool use_mse,
              int64_t w_off, int64_t b_off, double lr, int64_t max_defer,
              int64_t ramp_first, double growth, P2pMesh* mesh)
      : param_(std::move(flat_param)), loss_(std::move(loss_out)),
        mesh_(mesh), use_mse_(use_mse), w_off_((int)w_off),
        b_off_((int)b_off), lr_((float)lr),
        runs_([this](int64_t first, int64_t n) {
                const int64_t esz = bf16_ ? 2 : 4;
                launch(xs_ + first * B_ * K_ * esz, ts_ + first * B_ * esz,
                       B_, K_, n);
              },
              [this](const Span& f, int64_t n) {
                launch(reinterpret_cast<const char*>(f.x),
                       reinterpret_cast<const char*>(f.t), (int)f.rows,
                       (int)f.cols, n);
              },
              max_defer, ramp_first, growth) {
    TORCH_CHECK(param_.is_cuda() && param_.is_contiguous(),
                "ToyShardRun: flat_param must be a contiguous device tensor");
    const auto dt = param_.scalar_type();
    TORCH_CHECK(dt == at::kFloat || dt == at::kBFloat16,
                "ToyShardRun: flat_param must be f32 or bf16, got ", dt);
    bf16_ = dt == at::kBFloat16;
    TORCH_CHECK(lr_ > 0.f, "ToyShardRun applies SGD in-kernel: lr must be > 0");
    TORCH_CHECK(w_off >= 0 && b_off >= 0 && b_off < param_.numel() &&
                    w_off < param_.numel(),
                "ToyShardRun: w_off/b_off outside flat_param");
    lossp_ = toy_loss_ptr(loss_);
    TORCH_CHECK(lossp_ == nullptr || (loss_.is_cuda() &&
                                      loss_.device() == param_.device()),
                "ToyShardRun: loss_out must be on flat_param's device");
    TORCH_CHECK(mesh_ == nullptr || ramp_first == 0,
                "ToyShardRun: a mesh run takes no launch ramp (ramp_first 0)");
  }

  // recorder
  ToyShardRun(int64_t steps_bound, int64_t max_defer, int64_t ramp_first,
              double growth)
      : recorder_(true),
        runs_([this](int64_t first, int64_t n) {
                noted_.push_back({false, first, n});
              },
              [this](const Span& f, int64_t n) {
                noted_.push_back({true, (int64_t)f.x, n});
              },
              max_defer, ramp_first, growth) {
    runs_.bind(steps_bound);
  }

  ToyShardRun(const ToyShardRun&) = delete;
  ToyShardRun& operator=(const ToyShardRun&) = delete;

  void bind_shard(torch::Tensor xs, torch::Tensor ts, int64_t batch) {
    TORCH_CHECK(!recorder_, "a recorder binds step counts: use bind_steps");
    TORCH_CHECK(batch >= 1, "bind_shard: batch must be >= 1");
    const ToyDims d = check("bind_shard", xs, ts, batch);
    runs_.bind(d.S);  // what is pending runs first, on the OLD shard
    shard_x_ = std::move(xs);
    shard_t_ = std::move(ts);
    xs_ = static_cast<const char*>(shard_x_.data_ptr());
    ts_ = static_cast<const char*>(shard_t_.data_ptr());
    B_ = d.B;
    K_ = d.K;
  }

  void bind_steps(int64_t steps_bound) {
    TORCH_CHECK(recorder_, "bind_steps is the recorder's bind");
    runs_.bind(steps_bound);
  }

  // One step on the batch (x, t): it extends the pending tensor run when it
  // is the next [rows, K] slice of the same buffers, else it is validated
  // (the recorder only asks for contiguous tensors), what is pending is
  // launched, and it starts a new run and is kept alive for it.
  void step_tensors(torch::Tensor x, torch::Tensor t) {
    TORCH_CHECK(x.is_contiguous() && t.is_contiguous(),
                "step_tensors: x and t must be contiguous");
    const Span s = span_of(x, t);
    const bool extends = runs_.continues(s);
    if (!extends && !recorder_ && check("step", x, t, -1).S == 0)
      return;  // no rows
    runs_.step_span(s);  // launches what is pending unless `s` extends it
    if (!extends) {  // after that launch: it read the tensors let go here
      first_x_ = std::move(x);
      first_t_ = std::move(t);
    }
  }

  Runs& runs() { return runs_; }
  auto& tracker() { return runs_.index(); }

  pybind11::list launches() const {
    pybind11::list out;
    for (const Noted& l : noted_)
      out.append(l.tensors ? pybind11::make_tuple("t", l.first, l.n)
                           : pybind11::make_tuple(l.first, l.n));
    return out;
  }

 private:
  static Span span_of(const torch::Tensor& x, const torch::Tensor& t) {
    Span s;
    s.x = reinterpret_cast<uintptr_t>(x.data_ptr());
    s.t = reinterpret_cast<uintptr_t>(t.data_ptr());
    s.x_bytes = (int64_t)x.nbytes();
    s.t_bytes = (int64_t)t.nbytes();
    s.rows = x.dim() == 2 ? x.size(0) : -1;
    s.cols = x.dim() == 2 ? x.size(1) : -1;
    s.dtype = (int64_t)x.scalar_type() * 256 + (int64_t)t.scalar_type();
    s.x_buf = x.storage().unsafeGetStorageImpl();
    s.t_buf = t.storage().unsafeGetStorageImpl();
    return s;
  }

  // the entry points' own validator (toy_kernels.hip), once per run
  ToyDims check(const char* who, const torch::Tensor& x,
                const torch::Tensor& t, int64_t batch) const {
    const ToyDims d = toy_check_args(who, x, t, param_, nullptr, false, loss_,
                                     w_off_, b_off_, batch);
    if (mesh_ != nullptr) toy_check_mesh_args(who, d, *mesh_);
    return d;
  }

  // n >= 1 steps of validated [B, K] tiles from x and t
  void launch(const char* x, const char* t, int B, int K, int64_t n) {
    if (mesh_ != nullptr)
      toy_multistep_mesh_launch(x, t, param_.data_ptr(), lossp_, use_mse_,
                                w_off_, b_off_, lr_, B, (int)n, bf16_, *mesh_);
    else
      toy_multistep_launch(x, t, param_.data_ptr(), lossp_, use_mse_, w_off_,
                           b_off_, lr_, B, K, (int)n, bf16_);
  }

  torch::Tensor param_, loss_;
  torch::Tensor shard_x_, shard_t_;  // the bound shard, kept alive
  torch::Tensor first_x_, first_t_;  // the tensor run's first batch, likewise
  P2pMesh* mesh_ = nullptr;          // not owned: the binding keeps it alive
  const char* xs_ = nullptr;
  const char* ts_ = nullptr;
  float* lossp_ = nullptr;
  bool use_mse_ = true, bf16_ = false, recorder_ = false;
  int w_off_ = 0, b_off_ = 0, B_ = 0, K_ = 0;
  float lr_ = 0.f;
  std::vector<Noted> noted_;
  Runs runs_;  // last: its launch callables use the members above
};

// step_shard as a bare METH_O C function whose self is a capsule owning a
// shared_ptr to the run: the per-step call pays neither pybind11's
// dispatcher nor a Python frame. No pybind translation here, so C++
// exceptions are turned into Python ones by hand.
static const char* const kRunCapsule = "mi355x_ddp._C.ToyShardRun";

static PyObject* shard_run_step_slow(ToyShardRun& run, PyObject* arg);

static PyObject* shard_run_step(PyObject* self, PyObject* arg) {
  auto* sp = static_cast<std::shared_ptr<ToyShardRun>*>(
      PyCapsule_GetPointer(self, kRunCapsule));
  if (sp == nullptr) return nullptr;
  // all but one step in a threshold's worth only extend the pending run:
  // that needs no exception handling at all
  if (PyLong_Check(arg)) {
    int overflow = 0;
    const long long i = PyLong_AsLongLongAndOverflow(arg, &overflow);
    if (!overflow && (*sp)->tracker().extend(i)) Py_RETURN_NONE;
  }
  return shard_run_step_slow(**sp, arg);
}

static PyObject* shard_run_step_slow(ToyShardRun& run, PyObject* arg) {
  HANDLE_TH_ERRORS
  if (!PyLong_Check(arg)) {
    PyErr_Format(PyExc_TypeError,
                 "step_shard() takes an int batch index, not %.200s",
                 Py_TYPE(arg)->tp_name);
    return nullptr;
  }
  int overflow = 0;
  const long long i = PyLong_AsLongLongAndOverflow(arg, &overflow);
  if (i == -1 && PyErr_Occurred()) return nullptr;
  try {
    if (overflow) throw std::out_of_range("step index does not fit 64 bits");
    run.tracker().step(i);
  } catch (const std::out_of_range& e) {
    PyErr_SetString(PyExc_IndexError, e.what());
    return nullptr;
  }
  Py_RETURN_NONE;
  END_HANDLE_TH_ERRORS
}

static PyMethodDef kShardRunStepDef = {
    "step_shard", shard_run_step, METH_O,
    "step_shard(i): run step i of the bound shard (deferred; see flush)"};

static pybind11::object shard_run_step_fn(ToyShardRun& run) {
  auto* sp = new std::shared_ptr<ToyShardRun>(run.shared_from_this());
  PyObject* cap = PyCapsule_New(sp, kRunCapsule, [](PyObject* c) {
    delete static_cast<std::shared_ptr<ToyShardRun>*>(
        PyCapsule_GetPointer(c, kRunCapsule));
  });
  if (cap == nullptr) {
    delete sp;
    throw pybind11::error_already_set();
  }
  PyObject* fn = PyCFunction_New(&kShardRunStepDef, cap);
  Py_DECREF(cap);  // the function object owns it now
  if (fn == nullptr) throw pybind11::error_already_set();
  return pybind11::reinterpret_steal<pybind11::object>(fn);
}
}  // namespace mi355x

namespace py = pybind11;

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native kernels and RCCL communicator for mi355x_ddp";

  // pop HIP's latched per-thread error (e.g. hipErrorStreamCaptureInvalidated
  // after a failed graph capture) so eager fallback paths can proceed
  m.def("clear_hip_errors", [] { (void)hipGetLastError(); });

  m.def("linear_fwd", &mi355x::linear_fwd, py::arg("x"), py::arg("w"),
        py::arg("bias") = c10::nullopt);
  m.def("linear_bwd_weight", &mi355x::linear_bwd_weight, py::arg("x"),
        py::arg("dy"), py::arg("dw"), py::arg("db"),
        py::arg("accumulate") = false);
  m.def("linear_bwd_input", &mi355x::linear_bwd_input);
  m.def("gemm_bf16", &mi355x::gemm_bf16, py::arg("x"), py::arg("w"),
        py::arg("bias") = c10::nullopt);
  m.def("ce_fwd", &mi355x::ce_fwd);
  m.def("ce_bwd", &mi355x::ce_bwd, py::arg("probs"), py::arg("t"),
        py::arg("tsum"), py::arg("grad_scale"),
        py::arg("gout") = c10::nullopt);
  m.def("mse_fwd", &mi355x::mse_fwd);
  m.def("mse_bwd", &mi355x::mse_bwd, py::arg("y"), py::arg("t"),
        py::arg("grad_scale"), py::arg("gout") = c10::nullopt);
  m.def("sgd_flat", &mi355x::sgd_flat, py::arg("param_flat"),
        py::arg("grad_flat"), py::arg("lr"), py::arg("zero_grad") = true,
        py::arg("grad_scale") = c10::nullopt);
  m.def("sgd_momentum_flat", &mi355x::sgd_momentum_flat,
        py::arg("param_flat"), py::arg("grad_flat"), py::arg("buf"),
        py::arg("lr"), py::arg("momentum") = 0.0,
        py::arg("weight_decay") = 0.0, py::arg("nesterov") = false,
        py::arg("zero_grad") = true, py::arg("grad_scale") = c10::nullopt);
  m.def("adamw_tick", &mi355x::adamw_tick, py::arg("step_state"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"));
  m.def("adamw_flat", &mi355x::adamw_flat, py::arg("param_flat"),
        py::arg("grad_flat"), py::arg("exp_avg"), py::arg("exp_avg_sq"),
        py::arg("step_state"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("decay_mask") = c10::nullopt, py::arg("zero_grad") = true,
        py::arg("grad_scale") = c10::nullopt);
  m.def("sumsq_slots", &mi355x::sumsq_slots, py::arg("numel"));
  m.def("grad_sumsq_flat", &mi355x::grad_sumsq_flat, py::arg("grad_flat"),
        py::arg("partials"));
  m.def("clip_coef", &mi355x::clip_coef, py::arg("partials"),
        py::arg("clip_state"), py::arg("max_norm"));
  m.def("build_copy_plan",
        [](const std::vector<torch::Tensor>& tensors,
           const std::vector<int64_t>& offsets, int device) {
          return mi355x::build_copy_plan(tensors, offsets,
                                         torch::Device(torch::kCUDA, device));
        });
  m.def("flatten_into", &mi355x::flatten_into, py::arg("bucket"),
        py::arg("plan"), py::arg("total_blocks"), py::arg("zero_src") = false);
  m.def("unflatten_from", &mi355x::unflatten_from);
  m.def("toy_fused_fwd_bwd", &mi355x::toy_fused_fwd_bwd, py::arg("x"),
        py::arg("t"), py::arg("param_flat"), py::arg("grad_flat"),
        py::arg("loss_out"), py::arg("use_mse") = true,
        py::arg("w_off") = 0, py::arg("b_off") = 0, py::arg("lr") = 0.0);
  m.def("toy_multistep_mesh", &mi355x::toy_multistep_mesh, py::arg("x"),
        py::arg("t"), py::arg("param_flat"), py::arg("loss_out"),
        py::arg("use_mse"), py::arg("w_off"), py::arg("b_off"),
        py::arg("lr"), py::arg("batch"), py::arg("mesh"));
  m.def("epoch_shard", &mi355x::epoch_shard, py::arg("X"), py::arg("T"),
        py::arg("seed"), py::arg("rank"), py::arg("world"));
  m.def("epoch_shard_multi", &mi355x::epoch_shard_multi, py::arg("X"),
        py::arg("T"), py::arg("seed0"), py::arg("epochs"), py::arg("rank"),
        py::arg("world"));
  m.def("toy_multistep", &mi355x::toy_multistep, py::arg("x"), py::arg("t"),
        py::arg("param_flat"), py::arg("loss_out"), py::arg("use_mse") = true,
        py::arg("w_off") = 0, py::arg("b_off") = 0, py::arg("lr") = 0.0,
        py::arg("batch") = 32);
  // fp32 (32|64, 20) multi-step kernel selector: "chain" (default) | "mfma"
  m.def("set_toy_multistep_impl", &mi355x::set_toy_multistep_impl,
        py::arg("name"));
  m.def("get_toy_multistep_impl", &mi355x::get_toy_multistep_impl);
  m.def("set_toy_multistep_chain_depth",
        &mi355x::set_toy_multistep_chain_depth, py::arg("depth"));

  // The persistent engine's run tracker. step_shard is a bare C function,
  // fetched once and called per step; the rest is cold.
  py::class_<mi355x::ToyShardRun, std::shared_ptr<mi355x::ToyShardRun>>(
      m, "ToyShardRun")
      .def(py::init<torch::Tensor, torch::Tensor, bool, int64_t, int64_t,
                    double, int64_t, int64_t, double, mi355x::P2pMesh*>(),
           py::arg("flat_param"), py::arg("loss_out"), py::arg("use_mse"),
           py::arg("w_off"), py::arg("b_off"), py::arg("lr"),
           py::arg("max_defer"), py::arg("ramp_first"), py::arg("growth"),
           py::arg("mesh") = nullptr,
           // the run holds a non-owning P2pMesh*: keep the mesh alive with it
           py::keep_alive<1, 11>())
      .def_static("recorder",
                  [](int64_t steps_bound, int64_t max_defer,
                     int64_t ramp_first, double growth) {
                    return std::make_shared<mi355x::ToyShardRun>(
                        steps_bound, max_defer, ramp_first, growth);
                  },
                  py::arg("steps_bound"), py::arg("max_defer"),
                  py::arg("ramp_first"), py::arg("growth"))
      .def("bind_shard", &mi355x::ToyShardRun::bind_shard, py::arg("xs"),
           py::arg("ts"), py::arg("batch"))
      .def("bind_steps", &mi355x::ToyShardRun::bind_steps,
           py::arg("steps_bound"))
      .def("step_tensors", &mi355x::ToyShardRun::step_tensors, py::arg("x"),
           py::arg("t"))
      .def("flush", [](mi355x::ToyShardRun& r) { r.runs().flush(); })
      .def("launch_pending",
           [](mi355x::ToyShardRun& r) { r.runs().launch_pending(); })
      .def_property_readonly("step_shard", &mi355x::shard_run_step_fn)
      .def_property_readonly(
          "launch_count",
          [](mi355x::ToyShardRun& r) { return r.runs().launch_count(); })
      .def_property_readonly(
          "max_defer",
          [](mi355x::ToyShardRun& r) { return r.tracker().max_defer(); })
      .def_property_readonly(
          "pending",
          [](mi355x::ToyShardRun& r) { return r.tracker().pending(); })
      .def_property_readonly(
          "pending_tensors",
          [](mi355x::ToyShardRun& r) { return r.runs().spans().pending(); })
      .def_property_readonly(
          "threshold",
          [](mi355x::ToyShardRun& r) { return r.tracker().threshold(); })
      // the recorder's launches in order: (first_step, n_steps) of an index
      // run, ("t", first x address, n_steps) of a tensor run
      .def_property_readonly("launches", &mi355x::ToyShardRun::launches);

  py::class_<mi355x::P2pMesh>(m, "P2pMesh")
      .def(py::init<int, int, int>(), py::arg("rank"), py::arg("world"),
           py::arg("device"))
      .def("handle_bytes",
           [](const mi355x::P2pMesh& m_) { return py::bytes(m_.handle_bytes()); })
      .def("connect",
           [](mi355x::P2pMesh& m_, const std::vector<py::bytes>& hs) {
             std::vector<std::string> v(hs.begin(), hs.end());
             m_.connect(v);
           })
      .def("all_reduce_avg_inline", &mi355x::P2pMesh::all_reduce_avg_inline)
      .def("check", &mi355x::P2pMesh::check)
      .def_property_readonly("rank", &mi355x::P2pMesh::rank)
      .def_property_readonly("world", &mi355x::P2pMesh::world);

  // C++ autograd Functions (whole fwd/bwd chain stays out of Python)
  m.def("linear_autograd", &mi355x::linear_autograd, py::arg("x"),
        py::arg("w"), py::arg("bias") = c10::nullopt);
  m.def("mse_autograd", &mi355x::mse_autograd);
  m.def("ce_autograd", &mi355x::ce_autograd);

  py::class_<mi355x::ReducerCore, std::shared_ptr<mi355x::ReducerCore>>(
      m, "ReducerCore")
      .def(py::init([](std::vector<std::vector<torch::Tensor>> params,
                       std::vector<std::vector<torch::Tensor>> views,
                       std::vector<torch::Tensor> flats,
                       mi355x::RcclComm* comm) {
             return std::make_shared<mi355x::ReducerCore>(
                 std::move(params), std::move(views), std::move(flats), comm);
           }),
           py::arg("bucket_params"), py::arg("bucket_views"),
           py::arg("bucket_flat_grads"), py::arg("comm") = nullptr,
           // the core holds a non-owning RcclComm*: keep the comm alive as
           // long as the core (nurse the adapter's lifetime from C++ side)
           py::keep_alive<1, 5>())
      .def("attach_hooks", &mi355x::ReducerCore::attach_hooks)
      .def("detach_hooks", &mi355x::ReducerCore::detach_hooks)
      .def("finalize", &mi355x::ReducerCore::finalize,
           py::call_guard<py::gil_scoped_release>())
      .def("set_skip_comm", &mi355x::ReducerCore::set_skip_comm)
      .def_property_readonly("steps", &mi355x::ReducerCore::steps)
      .def_property_readonly("unfenced", &mi355x::ReducerCore::unfenced);

  py::class_<mi355x::RcclComm>(m, "RcclComm")
      .def(py::init<const std::string&, int, int, int>(), py::arg("unique_id"),
           py::arg("rank"), py::arg("world"), py::arg("device"),
           py::call_guard<py::gil_scoped_release>())
      .def_static("make_unique_id", [] {
        return py::bytes(mi355x::RcclComm::make_unique_id());
      })
      .def_property_readonly("rank", &mi355x::RcclComm::rank)
      .def_property_readonly("world", &mi355x::RcclComm::world)
      .def("all_reduce_avg", &mi355x::RcclComm::all_reduce_avg)
      .def("all_reduce_avg_inline", &mi355x::RcclComm::all_reduce_avg_inline)
      .def("broadcast", &mi355x::RcclComm::broadcast)
      .def("join_compute", &mi355x::RcclComm::join_compute)
      .def("barrier", &mi355x::RcclComm::barrier,
           py::call_guard<py::gil_scoped_release>());
}
