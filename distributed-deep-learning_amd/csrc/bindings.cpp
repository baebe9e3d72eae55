// Python bindings of the native extension ``_C`` (kernels launch on torch's current HIP
// stream so they compose with RCCL collectives and hipGraph capture).
#include <torch/extension.h>
#include <pybind11/stl.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>

#include <memory>
#include <string>
#include <vector>

#include "kernels/api.h"
#include "kernels/fake_rccl.h"
#include "kernels/stamps.h"
#include "runtime/mailbox.h"

namespace py = pybind11;

namespace {

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_f32_cuda(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// The optimizer of a Python call as an OptimSpec (kernels/ps_bank.h), in true doubles or with lr,
// b1 and b2 rounded to float32 first (`f32`); its refusals as torch errors under `tag`.  The
// decay is upd_decay(lr, weight_decay): rounded to float here, once.
ddl::OptimSpec spec_of(const char* tag, int64_t kind, double lr, double b1, double b2, double eps,
                       double mu, double scale, double weight_decay, bool nesterov,
                       bool f32 = false) {
  try {
    const float e = (float)eps, m = (float)mu, s = (float)scale;
    const float decay = ddl::upd_decay(lr, weight_decay);
    return f32 ? ddl::OptimSpec::from_float32((int)kind, lr, b1, b2, e, m, s, decay, nesterov)
               : ddl::OptimSpec::from_doubles((int)kind, lr, b1, b2, e, m, s, decay, nesterov);
  } catch (const std::invalid_argument& e) {
    TORCH_CHECK(false, tag, ": ", e.what());
  }
}
// The rule alone where the call carries its step size and its decay lr * wd ready-made (a double:
// the product with 1 is exact, so upd_decay rounds it as it stands)
ddl::UpdRule rule_of(int64_t kind, double b1, double b2, double eps, double mu, double scale,
                     double decay, bool nesterov) {
  return spec_of("update", kind, 1.0, b1, b2, eps, mu, scale, decay, nesterov).rule;
}

// [(ps id, params, m, v | None, t)] as hosted PS states; the tensors go to `keep`
std::vector<ddl::AsyncPsState> ps_states(py::list ps, std::vector<at::Tensor>& keep,
                                         bool need_v = false) {
  std::vector<ddl::AsyncPsState> st;
  auto ptr = [&](py::handle h, const char* name) {
    at::Tensor x = h.cast<at::Tensor>();
    check_f32_cuda(x, name);
    keep.push_back(x);
    return x.data_ptr<float>();
  };
  for (auto item : ps) {
    auto t = item.cast<py::tuple>();
    TORCH_CHECK(!need_v || !t[3].is_none(), "in-line applies are Adam: v required");
    st.push_back({t[0].cast<int>(), ptr(t[1], "ps params"), ptr(t[2], "m"),
                  t[3].is_none() ? nullptr : ptr(t[3], "v"), t[4].cast<int64_t>()});
  }
  return st;
}
// [(lo, hi)] element ranges
std::vector<std::pair<int64_t, int64_t>> index_ranges(py::list ranges) {
  std::vector<std::pair<int64_t, int64_t>> rg;
  for (auto r : ranges) {
    auto t = r.cast<py::tuple>();
    rg.emplace_back(t[0].cast<int64_t>(), t[1].cast<int64_t>());
  }
  return rg;
}

// One update of a flat span under rule `kind` of update.h (copy: m and v may be None; momentum:
// v may be).  The step size rides beside it: Adam's lr_t, or the learning rate.  `decay` is the
// decoupled weight decay's lr * wd, as a double.
struct FlatUpdate {
  ddl::UpdRule rule;
  ddl::UpdSpan span;
  const float* g;
  int64_t n;
  FlatUpdate(int64_t kind, at::Tensor w, at::Tensor gt, c10::optional<at::Tensor> m,
             c10::optional<at::Tensor> v, double b1, double b2, double eps, double mu,
             double scale, double decay = 0.0, bool nesterov = false)
      : rule(rule_of(kind, b1, b2, eps, mu, scale, decay, nesterov)), n(w.numel()) {
    TORCH_CHECK((m || kind == ddl::kUpdCopy) && (v || kind != ddl::kUpdAdam),
                "update: optimizer state missing");
    auto ptr = [&](const at::Tensor& t, const char* name) {
      check_f32_cuda(t, name);
      TORCH_CHECK(t.numel() == n, "update: size mismatch");
      return t.data_ptr<float>();
    };
    span.w = ptr(w, "w");
    g = ptr(gt, "g");
    if (m) span.m = ptr(*m, "m");
    if (v) span.v = ptr(*v, "v");
  }
};

void update_flat(int64_t kind, at::Tensor w, at::Tensor g, c10::optional<at::Tensor> m,
                 c10::optional<at::Tensor> v, double step, double b1, double b2, double eps,
                 double mu, double scale, double decay, bool nesterov) {
  const FlatUpdate u(kind, w, g, m, v, b1, b2, eps, mu, scale, decay, nesterov);
  ddl::launch_update(u.rule, (float)step, u.span, u.g, u.n, cur_stream());
}
void adam_flat(at::Tensor w, at::Tensor g, at::Tensor m, at::Tensor v, double lr_t, double b1,
               double b2, double eps, double scale) {
  update_flat(ddl::kUpdAdam, w, g, m, v, lr_t, b1, b2, eps, 0.0, scale, 0.0, false);
}
void momentum_flat(at::Tensor w, at::Tensor g, at::Tensor m, double lr, double mu, double scale) {
  update_flat(ddl::kUpdMomentum, w, g, m, c10::nullopt, lr, 0.0, 0.0, 0.0, mu, scale, 0.0, false);
}

// Clip by global norm (kernels/clip.hip).  ranges: [(lo, n)] element ranges of grads, at most 16.
ddl::ClipRanges clip_table(const at::Tensor& grads, const std::vector<std::pair<int64_t, int64_t>>& ranges) {
  check_f32_cuda(grads, "grads");
  return ddl::make_clip_ranges(ranges, std::max<int64_t>(grads.numel(), 1));
}
// A runner's clipping site: the table plus scratch tensors it keeps alive (out: 2 floats)
struct PyClipSite {
  ddl::ClipSite site;
  std::vector<at::Tensor> keep;
  void set(double max_norm, const at::Tensor& grads,
           const std::vector<std::pair<int64_t, int64_t>>& ranges, at::Tensor out) {
    TORCH_CHECK(max_norm >= 0.0, "set_clip: negative max_norm");
    site = ddl::ClipSite();
    keep.clear();
    if (max_norm == 0.0) return;
    check_f32_cuda(out, "out");
    TORCH_CHECK(out.numel() >= 2, "set_clip: out holds {norm, coef}");
    site.ranges = clip_table(grads, ranges);
    site.max_norm = (float)max_norm;
    TORCH_CHECK(site.max_norm > 0.f, "set_clip: max_norm rounds to 0 in float32");
    at::Tensor part = at::empty({std::max(site.ranges.nchunks, 1)}, grads.options().dtype(at::kDouble));
    at::Tensor ticket = at::zeros({1}, grads.options().dtype(at::kInt));
    site.out2 = out.data_ptr<float>();
    site.partials = part.data_ptr<double>();
    site.ticket = ticket.data_ptr<int>();
    keep = {out, part, ticket};
  }
};

// Stand-alone: out <- {norm, coef}, grads scaled in place (no host sync).  The arrival ticket is
// one zeroed word per device, left zero by every call: calls on one device must be ordered (one
// stream at a time).
void clip_grads(at::Tensor grads, std::vector<std::pair<int64_t, int64_t>> ranges, double max_norm,
                at::Tensor out, int64_t max_grid) {
  TORCH_CHECK(max_norm > 0.0 && (float)max_norm > 0.f, "clip_grads: max_norm must be positive");
  check_f32_cuda(out, "out");
  TORCH_CHECK(out.numel() >= 2, "clip_grads: out holds {norm, coef}");
  const ddl::ClipRanges t = clip_table(grads, ranges);
  c10::hip::HIPGuard guard(grads.device().index());
  // (never destroyed: a device tensor must not outlive into static destruction)
  static std::vector<at::Tensor>& tickets = *new std::vector<at::Tensor>(64);
  const int dev = grads.device().index();
  TORCH_CHECK(dev >= 0 && dev < 64, "clip_grads: device index");
  if (!tickets[dev].defined()) tickets[dev] = at::zeros({1}, grads.options().dtype(at::kInt));
  at::Tensor part = at::empty({std::max(t.nchunks, 1)}, grads.options().dtype(at::kDouble));
  ddl::launch_clip(t, grads.data_ptr<float>(), (float)max_norm, out.data_ptr<float>(),
                   part.data_ptr<double>(), tickets[dev].data_ptr<int>(), cur_stream(),
                   (int)max_grid);
}

// Gradient accumulation (kernels/accum.hip).  acc: the fp32 accumulator, the size of grads and at
// the same offset from a 16-byte boundary.
void check_accum_pair(const at::Tensor& grads, const at::Tensor& acc) {
  check_f32_cuda(grads, "grads");
  check_f32_cuda(acc, "acc");
  TORCH_CHECK(acc.numel() == grads.numel(), "accum: acc must have the size of grads");
  TORCH_CHECK(acc.device() == grads.device(), "accum: acc and grads on different devices");
  TORCH_CHECK(acc.data_ptr<float>() != grads.data_ptr<float>(), "accum: acc is grads");
  TORCH_CHECK(((reinterpret_cast<uintptr_t>(acc.data_ptr<float>()) ^
                reinterpret_cast<uintptr_t>(grads.data_ptr<float>())) & 15) == 0,
              "accum: acc and grads differ in 16-byte alignment");
}
// A runner's accumulation site: the table, K and the accumulator it keeps alive
struct PyAccumSite {
  ddl::AccumSite site;
  at::Tensor keep;
  void set(int64_t k, const at::Tensor& grads,
           const std::vector<std::pair<int64_t, int64_t>>& ranges,
           c10::optional<at::Tensor> acc) {
    TORCH_CHECK(k >= 1 && k <= (1 << 20), "set_accum: K must be at least 1");
    site = ddl::AccumSite();
    keep = at::Tensor();
    if (k == 1) return;
    TORCH_CHECK(acc.has_value(), "set_accum: K > 1 needs an accumulator");
    check_accum_pair(grads, *acc);
    site.ranges = clip_table(grads, ranges);
    site.k = (int)k;
    site.acc = acc->data_ptr<float>();
    keep = *acc;
  }
};

// Stand-alone: one pass of mode 0 (acc := grads), 1 (acc += grads) or 2 (grads := (acc + grads) *
// (float)(1 / k)) over `ranges` (no host sync, no allocation)
void accum_grads(at::Tensor grads, at::Tensor acc, std::vector<std::pair<int64_t, int64_t>> ranges,
                 int64_t mode, int64_t k, int64_t max_grid) {
  TORCH_CHECK(k >= 2 && k <= (1 << 20), "accum_grads: K must be at least 2");
  TORCH_CHECK(mode >= 0 && mode <= 2, "accum_grads: mode 0 (first), 1 (add) or 2 (finish)");
  check_accum_pair(grads, acc);
  const ddl::ClipRanges t = clip_table(grads, ranges);
  c10::hip::HIPGuard guard(grads.device().index());
  ddl::launch_accum(t, grads.data_ptr<float>(), acc.data_ptr<float>(), (int)mode, (int)k,
                    cur_stream(), (int)max_grid);
}

// One training batch (kernels/batch.hip): rows [0, b) of xb and yb from the resident training set,
// shuffled and / or shifted (no host sync, no allocation); rows from b on keep their contents
void assemble_batch(at::Tensor x_train, at::Tensor y_train, at::Tensor xb, at::Tensor yb,
                    int64_t b, int64_t base, int64_t key, int64_t key_shift, int64_t s,
                    bool shuffle) {
  check_f32_cuda(x_train, "x_train");
  check_f32_cuda(xb, "xb");
  auto check_labels = [](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.dim() == 1,
                name, " must be a contiguous int64 GPU vector");
  };
  check_labels(y_train, "y_train");
  check_labels(yb, "yb");
  TORCH_CHECK(x_train.dim() == 2 && x_train.size(1) == 784 && xb.dim() == 2 && xb.size(1) == 784,
              "assemble_batch: x_train and xb must be [rows, 784]");
  const int64_t n = x_train.size(0);
  TORCH_CHECK(y_train.size(0) == n, "assemble_batch: y_train must have a label per training row");
  TORCH_CHECK(n >= 1 && n <= INT32_MAX, "assemble_batch: training rows in 1..2^31 - 1");
  TORCH_CHECK(b >= 1 && b <= xb.size(0) && b <= yb.size(0),
              "assemble_batch: xb and yb must hold the batch");
  TORCH_CHECK(base >= 0 && base + b <= n, "assemble_batch: the batch lies outside the training rows");
  TORCH_CHECK(s >= 0 && s <= 8, "assemble_batch: shift in 0..8");
  TORCH_CHECK(key >= 0 && key <= 0xFFFFFFFFLL && key_shift >= 0 && key_shift <= 0xFFFFFFFFLL,
              "assemble_batch: keys are 32-bit");
  TORCH_CHECK(x_train.device() == xb.device() && y_train.device() == xb.device() &&
              yb.device() == xb.device(), "assemble_batch: tensors on different devices");
  // apart: the training set is read while the batch is written
  const char* t0 = reinterpret_cast<const char*>(x_train.data_ptr<float>());
  const char* d0 = reinterpret_cast<const char*>(xb.data_ptr<float>());
  TORCH_CHECK(d0 + 4 * xb.numel() <= t0 || t0 + 4 * x_train.numel() <= d0,
              "assemble_batch: xb overlaps x_train");
  const char* l0 = reinterpret_cast<const char*>(y_train.data_ptr<int64_t>());
  const char* m0 = reinterpret_cast<const char*>(yb.data_ptr<int64_t>());
  TORCH_CHECK(m0 + 8 * yb.numel() <= l0 || l0 + 8 * n <= m0, "assemble_batch: yb overlaps y_train");
  c10::hip::HIPGuard guard(xb.device().index());
  ddl::launch_assemble_batch(x_train.data_ptr<float>(), y_train.data_ptr<int64_t>(), n,
                             xb.data_ptr<float>(), yb.data_ptr<int64_t>(), (int)b, base,
                             (uint32_t)key, (uint32_t)key_shift, (int)s, shuffle, cur_stream());
}

// Python-facing wrapper of ddl::Engine: owns the workspace tensor.
class PyEngine {
 public:
  PyEngine(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, int64_t max_batch,
           int64_t train_batch, double keep_prob)
      : params_(params), grads_(grads) {
    TORCH_CHECK(params.size() == 14 && grads.size() == 14, "need 14 parameter/gradient tensors");
    for (int i = 0; i < 14; ++i) {
      check_f32_cuda(params[i], "param");
      check_f32_cuda(grads[i], "grad");
      e_.P[i] = params[i].data_ptr<float>();
      e_.G[i] = grads[i].data_ptr<float>();
    }
    device_ = params[0].device();
    e_.max_batch = (int)std::max(max_batch, train_batch);
    e_.train_batch = (int)train_batch;
    set_keep_prob(keep_prob);
    realloc();
  }

  // Tile configs of the training step or of the eval forward (no split-K, large batch chunks; no
  // slab needed).  Accepted: a config the op has an instantiation of, or a special one, which
  // falls back where the op has none (the defaults hold those): effective_cfg() tells
  void set_cfgs(std::vector<int64_t> c, bool train) {
    TORCH_CHECK((int)c.size() == ddl::OP_COUNT, "expected ", (int)ddl::OP_COUNT, " tile configs");
    for (int i = 0; i < ddl::OP_COUNT; ++i)
      TORCH_CHECK(c[i] >= 0 && c[i] <= ddl::CFG_KW16 && ddl::cfg_accepted(i, (int)c[i], train),
                  "tile config out of range");
    int* dst = train ? e_.sched.cfg : e_.sched.eval_cfg;
    for (int i = 0; i < ddl::OP_COUNT; ++i) dst[i] = (int)c[i];
    if (train) realloc();
  }
  void set_cfg(std::vector<int64_t> c) { set_cfgs(c, true); }
  void set_eval_cfg(std::vector<int64_t> c) { set_cfgs(c, false); }
  std::vector<int64_t> get_cfg() const { return vec(e_.sched.cfg); }
  std::vector<int64_t> get_eval_cfg() const { return vec(e_.sched.eval_cfg); }
  // the configs that really run (kernels/schedule.h effective_cfg)
  std::vector<int64_t> effective(bool train) const {
    auto c = vec(train ? e_.sched.cfg : e_.sched.eval_cfg);
    for (int i = 0; i < ddl::OP_COUNT; ++i) c[i] = ddl::effective_cfg(i, (int)c[i], train);
    return c;
  }
  static std::vector<int64_t> vec(const int (&a)[ddl::OP_COUNT]) {
    return std::vector<int64_t>(a, a + ddl::OP_COUNT);
  }
  // the side stream exists only in the (slower, A/B) two-stream mode: every extra HIP stream
  // competes for the GPU_MAX_HW_QUEUES hardware queues
  void set_concurrent(bool on) {
    if (on) {
      c10::hip::HIPGuard guard(device_.index());
      e_.init_streams();
    }
    e_.sched.concurrent = on;
  }
  void set_dual(bool on) { e_.sched.dual = on; }
  // the same update as a one-piece optimizer tail that no launch takes: Engine::flush_tail's
  // stand-alone launch (tests)
  void flush_update_tail(int64_t kind, at::Tensor w, at::Tensor g, c10::optional<at::Tensor> m,
                         c10::optional<at::Tensor> v, double step, double b1, double b2,
                         double eps, double mu, double scale, double decay, bool nesterov) {
    queue_update_tail(kind, w, g, m, v, step, b1, b2, eps, mu, scale, decay, nesterov);
    e_.flush_tail(cur_stream());
  }
  // the same one-piece tail left pending: the next launch that carries a tail takes it, or the
  // next flush_tail launches it (tests; the tensors must outlive that launch)
  void queue_update_tail(int64_t kind, at::Tensor w, at::Tensor g, c10::optional<at::Tensor> m,
                         c10::optional<at::Tensor> v, double step, double b1, double b2,
                         double eps, double mu, double scale, double decay, bool nesterov) {
    const FlatUpdate u(kind, w, g, m, v, b1, b2, eps, mu, scale, decay, nesterov);
    e_.flush_tail(cur_stream());
    ddl::UpdPiece q;
    q.w = u.span.w; q.g = u.g; q.m = u.span.m; q.v = u.span.v;
    q.n = u.n;
    q.step = (float)step;
    e_.tail.rule = u.rule;
    e_.tail.add_piece(q);
    e_.tail.finish();
  }
  // host counters of the dispatch branches (kernels/schedule.h enum Branch), by name in enum order
  py::dict dispatch_hits() const {
    py::dict d;
    for (int b = 0; b < ddl::BR_COUNT; ++b) d[ddl::branch_name(b)] = e_.branch_hits[b];
    return d;
  }
  void reset_dispatch_hits() {
    for (int& h : e_.branch_hits) h = 0;
  }
  void set_wide_thr(int64_t t) {
    e_.sched.wide_thr = (int)std::max<int64_t>(1, t);
    for (int i = 0; i < ddl::OP_COUNT; ++i) e_.sched.wide[i] = e_.sched.wide_thr;
  }
  // per-op split-K reduce threshold: z > wide[op] -> separate reduce kernel, else in-launch
  void set_wide(std::vector<int64_t> w) {
    TORCH_CHECK((int)w.size() == ddl::OP_COUNT, "expected ", (int)ddl::OP_COUNT, " thresholds");
    for (int i = 0; i < ddl::OP_COUNT; ++i) e_.sched.wide[i] = (int)std::max<int64_t>(1, w[i]);
  }
  std::vector<int64_t> get_wide() const { return vec(e_.sched.wide); }
  // bit op: the dual launch of op's layer dispatches its second problem first
  void set_dual_bfirst(int64_t m) { e_.sched.dual_bfirst = (int)m; }
  int64_t get_dual_bfirst() const { return e_.sched.dual_bfirst; }

  void set_keep_prob(double keep) {
    const double rate = 1.0 - keep;
    e_.thr24 = (uint32_t)std::llround(rate * 16777216.0);
    e_.inv_keep = keep > 0.0 ? (float)(1.0 / keep) : 0.f;
  }

  void set_splits(std::vector<int64_t> s) {
    TORCH_CHECK((int)s.size() == ddl::OP_COUNT, "expected ", (int)ddl::OP_COUNT, " split factors");
    for (int i = 0; i < ddl::OP_COUNT; ++i) e_.sched.splits[i] = (int)std::max<int64_t>(1, s[i]);
    realloc();
  }
  std::vector<int64_t> get_splits() const { return vec(e_.sched.splits); }
  void forward(at::Tensor x, at::Tensor seed, bool train) {
    check_x(x);
    e_.forward(x.data_ptr<float>(), (int)x.size(0), seed_ptr(seed), train, cur_stream());
  }
  void backward_segment(int64_t s, at::Tensor x, at::Tensor labels, at::Tensor seed) {
    check_x(x);
    TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_cuda(), "labels must be int64 GPU");
    e_.backward_segment((int)s, x.data_ptr<float>(), labels.data_ptr<int64_t>(), (int)x.size(0),
                        seed_ptr(seed), cur_stream());
  }
  void run_op(int64_t op, at::Tensor x, at::Tensor seed, bool train) {
    check_x(x);
    e_.run_op((int)op, x.data_ptr<float>(), (int)x.size(0), seed_ptr(seed), train, cur_stream());
  }
  void zero_correct() {
    TORCH_CHECK(hipMemsetAsync(e_.correct, 0, sizeof(int), cur_stream()) == hipSuccess);
  }
  void eval_count(at::Tensor x, at::Tensor labels) {
    check_x(x);
    e_.eval_count(x.data_ptr<float>(), labels.data_ptr<int64_t>(), (int)x.size(0), cur_stream());
  }
  void head_fwd(at::Tensor labels, int64_t B) {
    ddl::launch_head_fwd(e_.h2, e_.P[12], e_.P[13], labels.data_ptr<int64_t>(), (int)B, e_.dlog,
                         e_.loss, nullptr, cur_stream());
  }

  // Views of internal buffers (testing / debugging).  Shapes are for batch B.
  at::Tensor buffer(const std::string& name, int64_t B) {
    auto f = at::TensorOptions().dtype(at::kFloat).device(device_);
    auto u8 = at::TensorOptions().dtype(at::kByte).device(device_);
    auto i32 = at::TensorOptions().dtype(at::kInt).device(device_);
    // maps stored with the 2-pixel zero halo (layers.h kHalo): the interior view
    // ("p1+halo" etc.: the whole stored map, border included)
    const bool whole = name.size() > 5 && name.compare(name.size() - 5, 5, "+halo") == 0;
    const std::string base_name = whole ? name.substr(0, name.size() - 5) : name;
    auto halo = [&](float* p, int64_t h, int64_t c) {
      auto t = torch::from_blob(p, {B, h + 4, h + 4, c}, f);
      return whole ? t : t.narrow(1, 2, h).narrow(2, 2, h);
    };
    if (whole && base_name == "p1") return halo(e_.p1, 14, 32);
    if (whole && base_name == "p2") return halo(e_.p2, 7, 64);
    if (whole && base_name == "p3") return halo(e_.p3, 4, 128);
    if (whole && base_name == "d4") return halo(e_.d4, 4, 256);
    if (whole && base_name == "d3") return halo(e_.d3, 7, 128);
    if (whole && base_name == "d2") return halo(e_.d2, 14, 64);
    if (name == "p1") return halo(e_.p1, 14, 32);
    if (name == "p2") return halo(e_.p2, 7, 64);
    if (name == "p3") return halo(e_.p3, 4, 128);
    if (name == "p4") return torch::from_blob(e_.p4, {B, 1024}, f);
    if (name == "h1") return torch::from_blob(e_.h1, {B, 1024}, f);
    if (name == "h2") return torch::from_blob(e_.h2, {B, 512}, f);
    if (name == "dlog") return torch::from_blob(e_.dlog, {B, 10}, f);
    if (name == "loss") return torch::from_blob(e_.loss, {B}, f);
    if (name == "dpre2fc") return torch::from_blob(e_.dpre2fc, {B, 512}, f);
    if (name == "dpre1fc") return torch::from_blob(e_.dpre1fc, {B, 1024}, f);
    if (name == "d4") return halo(e_.d4, 4, 256);
    if (name == "d3") return halo(e_.d3, 7, 128);
    if (name == "d2") return halo(e_.d2, 14, 64);
    if (name == "d1") return torch::from_blob(e_.d1, {B, 28, 28, 32}, f);
    if (name == "c1") return torch::from_blob(e_.c1, {B, 14, 14, 32}, u8);
    if (name == "c2") return torch::from_blob(e_.c2, {B, 7, 7, 64}, u8);
    if (name == "c3") return torch::from_blob(e_.c3, {B, 4, 4, 128}, u8);
    if (name == "c4") return torch::from_blob(e_.c4, {B, 1024}, u8);
    if (name == "correct") return torch::from_blob(e_.correct, {1}, i32);
    TORCH_CHECK(false, "unknown buffer ", name);
  }

  int64_t max_batch() const { return e_.max_batch; }
  ddl::Engine* raw() { return &e_; }
  // a runner's micro-batch, checked: the pointers and B
  struct Batch {
    const float* x;
    const int64_t* labels;
    int B;
  };
  Batch batch(const at::Tensor& x, const at::Tensor& labels) {
    check_x(x);
    TORCH_CHECK(labels.scalar_type() == at::kLong && labels.is_cuda(), "labels must be int64 GPU");
    TORCH_CHECK(labels.numel() == x.size(0), "labels/batch size mismatch");
    return {x.data_ptr<float>(), labels.data_ptr<int64_t>(), (int)x.size(0)};
  }
  int64_t workspace_bytes() const { return (int64_t)e_.workspace_bytes(); }
  static std::vector<int64_t> op_shape(int64_t op, int64_t B) {
    int M, N, K;
    ddl::Engine::op_shape((int)op, (int)B, &M, &N, &K);
    return {M, N, K};
  }

 private:
  void realloc() {
    e_.slab_floats = e_.slab_floats_needed(e_.train_batch);
    const size_t bytes = e_.workspace_bytes();
    // zeroed once: the split-K arrival tickets must start at 0 (reducers re-arm them)
    ws_ = at::zeros({(int64_t)bytes}, at::TensorOptions().dtype(at::kByte).device(device_));
    e_.bind_workspace(ws_.data_ptr());
  }
  void check_x(const at::Tensor& x) {
    check_f32_cuda(x, "x");
    TORCH_CHECK(x.dim() == 2 && x.size(1) == 784, "x must be [B,784]");
    TORCH_CHECK(x.size(0) <= e_.max_batch, "batch ", x.size(0), " exceeds engine max_batch ",
                e_.max_batch);
  }
  static const uint32_t* seed_ptr(const at::Tensor& s) {
    if (!s.defined() || s.numel() == 0) return nullptr;
    TORCH_CHECK(s.is_cuda() && s.scalar_type() == at::kInt, "seed must be an int32 GPU tensor");
    return reinterpret_cast<const uint32_t*>(s.data_ptr<int32_t>());
  }

  ddl::Engine e_;
  std::vector<at::Tensor> params_, grads_;
  at::Tensor ws_;
  at::Device device_{at::kCPU};
};

// What the wrappers of the two xGMI exchanges P (PeerExchange, AsyncPeer) share: the buffers and
// the IPC life cycle (handles out, every rank's handles in), each call on the parameters' device.
template <class P>
class PyPeerBase {
 public:
  PyPeerBase(at::Tensor params, at::Tensor grads) : params_(params), grads_(grads) {
    check_f32_cuda(params, "params");
    check_f32_cuda(grads, "grads");
    TORCH_CHECK(params.numel() == grads.numel(), "params/grads size mismatch");
  }
  py::bytes handle() const {
    c10::hip::HIPGuard guard(device());
    return py::bytes(p_->handle());
  }
  void open(std::vector<std::string> handles) {
    c10::hip::HIPGuard guard(device());
    p_->open(handles);
  }
  void unmap_peers() {
    c10::hip::HIPGuard guard(device());
    py::gil_scoped_release nogil;
    p_->unmap_peers();
  }
  void close() {
    c10::hip::HIPGuard guard(device());
    py::gil_scoped_release nogil;
    p_->close();
  }
  int error() const { return p_->error(); }
  P* raw() { return p_.get(); }
  int device() const { return params_.device().index(); }

 protected:
  at::Tensor params_, grads_;
  std::unique_ptr<P> p_;
};

// xGMI peer exchange of the native sync step (kernels/xgmi.hip)
class PyPeer : public PyPeerBase<ddl::PeerExchange> {
 public:
  PyPeer(at::Tensor params, at::Tensor grads, int64_t world, int64_t rank, py::list buckets,
         int64_t max_slices, int64_t repl_bucket)
      : PyPeerBase(params, grads) {
    // each bucket: (lo, hi) — an equal-chunk bucket — or (runs, state_offs, owner) — an owner
    // bucket of a tensor-granular plan (kernels/api.h XgmiBucketSpec)
    std::vector<ddl::XgmiBucketSpec> bk;
    for (auto b : buckets) {
      auto t = b.cast<py::tuple>();
      ddl::XgmiBucketSpec sp;
      if (t.size() == 3) {
        for (auto r : t[0].cast<py::list>()) {
          auto rr = r.cast<py::tuple>();
          sp.runs.emplace_back(rr[0].cast<int64_t>(), rr[1].cast<int64_t>());
        }
        sp.state_offs = t[1].cast<std::vector<int64_t>>();
        sp.owner = t[2].cast<int>();
      } else {
        sp.runs.emplace_back(t[0].cast<int64_t>(), t[1].cast<int64_t>());
      }
      bk.push_back(sp);
    }
    c10::hip::HIPGuard guard(params.device().index());
    p_ = std::make_unique<ddl::PeerExchange>(params.data_ptr<float>(), grads.data_ptr<float>(),
                                             params.numel(), (int)world, (int)rank, bk,
                                             (int)max_slices, (int)repl_bucket);
  }
  // One bucket's exchange kernel on the current stream, as the runner launches it but with no
  // READY gate ahead: the kernels alone, on any small plan (tests/test_exchange_kernels_gpu.py).
  // kind: update.h's rule kind; step: Adam's lr_t, or the learning rate.  m and v are this rank's
  // state of the bucket (an owner bucket: the PS's, indexed by the runs' state offsets) and may be
  // None where the rule, or a rank that does not own the bucket, has none.
  void launch(int64_t bucket, int64_t epoch, int64_t kind, c10::optional<at::Tensor> m,
              c10::optional<at::Tensor> v, double step, double b1, double b2, double eps,
              double mu, double scale, double coef, bool final_wait, double decay,
              bool nesterov) {
    TORCH_CHECK(bucket >= 0 && bucket < p_->num_buckets(), "bucket out of range");
    ddl::XgmiUpdate u;
    u.rule = rule_of(kind, b1, b2, eps, mu, scale, decay, nesterov);
    u.step = (float)step;
    u.coef = (float)coef;
    auto state = [&](const at::Tensor& t, const char* name) {
      check_f32_cuda(t, name);
      TORCH_CHECK(t.device() == params_.device(), name, " must be on the parameters' device");
      TORCH_CHECK(t.numel() >= p_->state_extent((int)bucket), name,
                  " is shorter than the bucket's state");
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0, name,
                  " must be 16-B aligned");
      return t.data_ptr<float>();
    };
    if (m) u.m = state(*m, "m");
    if (v) u.v = state(*v, "v");
    c10::hip::HIPGuard guard(params_.device().index());
    p_->launch((int)bucket, (uint32_t)epoch, u, final_wait, cur_stream());
  }
  std::vector<int64_t> nslices() const {
    std::vector<int64_t> v;
    for (int b = 0; b < p_->num_buckets(); ++b) v.push_back(p_->nslices(b));
    return v;
  }
  // -1: equal-chunk bucket; else the rank hosting the owner bucket's PS
  int owner(int64_t b) const {
    TORCH_CHECK(b >= 0 && b < p_->num_buckets(), "bucket out of range");
    return p_->owner((int)b);
  }
};

// asynchronous PS over xGMI peer memory (kernels/xgmi_async.hip); kernels on the current stream
class PyAsyncPeer : public PyPeerBase<ddl::AsyncPeer> {
 public:
  PyAsyncPeer(at::Tensor params, at::Tensor grads, int64_t world, int64_t rank, py::list ranges,
              std::vector<int64_t> hosts, int64_t max_slices)
      : PyPeerBase(params, grads) {
    std::vector<int> h(hosts.begin(), hosts.end());
    c10::hip::HIPGuard guard(params.device().index());
    p_ = std::make_unique<ddl::AsyncPeer>(params.data_ptr<float>(), grads.data_ptr<float>(),
                                          params.numel(), (int)world, (int)rank,
                                          index_ranges(ranges), h, (int)max_slices);
  }
  void push_all(int64_t epoch, double coef) { p_->push_all((uint32_t)epoch, (float)coef, cur_stream()); }
  void attach_done(std::string name, bool create) { p_->attach_done(name, create); }
  bool wait_done(int64_t epoch, double timeout_s) {
    py::gil_scoped_release nogil;
    return p_->wait_done((uint32_t)epoch, timeout_s);
  }
  // opt: update.h's rule kind (0 Adam: the step size is lr_t; 1 momentum: lr; 2 self-test).
  // (both step sizes stay in the Python-facing signature: parallel/async_xgmi.py is unchanged)
  void apply(int64_t ps, int64_t worker, int64_t epoch, int64_t opt, at::Tensor ps_params,
             c10::optional<at::Tensor> m, c10::optional<at::Tensor> v, double lr_t, double b1,
             double b2, double eps, double lr, double mu, double scale, double weight_decay,
             bool nesterov) {
    check_f32_cuda(ps_params, "ps_params");
    const ddl::OptimSpec s =
        spec_of("apply", opt, lr, b1, b2, eps, mu, scale, weight_decay, nesterov);
    ddl::XgmiUpdate u;
    u.rule = s.rule;
    u.step = s.step_for((float)lr_t);
    if (m) { check_f32_cuda(*m, "m"); u.m = m->data_ptr<float>(); }
    if (v) { check_f32_cuda(*v, "v"); u.v = v->data_ptr<float>(); }
    p_->apply((int)ps, (int)worker, (uint32_t)epoch, u, ps_params.data_ptr<float>(), cur_stream());
  }
  const at::Tensor& grads() const { return grads_; }
};

// native PS service thread of the async xGMI exchange
class PyAsyncService {
 public:
  // ps: list of (ps id, params, m, v | None, t)
  PyAsyncService(PyAsyncPeer& peer, int64_t world, py::list ps, int64_t opt,
                 double lr, double b1, double b2, double eps, double mu, double scale,
                 int64_t epoch0, bool provenance, double weight_decay, bool nesterov) {
    svc_ = std::make_unique<ddl::AsyncService>(
        peer.raw(), (int)world, peer.device(), ps_states(ps, keep_),
        spec_of("async service", opt, lr, b1, b2, eps, mu, scale, weight_decay, nesterov,
                /*f32=*/true),
        (uint32_t)epoch0, provenance);
  }
  void start(int64_t expected) { svc_->start(expected); }
  void join() {
    py::gil_scoped_release nogil;
    svc_->join();
  }
  int64_t t(int64_t ps) const { return svc_->t((int)ps); }
  int64_t served() const { return svc_->served(); }
  void pause() {
    py::gil_scoped_release nogil;
    svc_->pause();
  }
  void resume() { svc_->resume(); }
  std::vector<std::array<int64_t, 4>> provenance() const { return svc_->provenance(); }
  std::string mode() const { return svc_->mode(); }

 private:
  std::vector<at::Tensor> keep_;
  std::unique_ptr<ddl::AsyncService> svc_;
};

// asynchronous PS over point-to-point RCCL sessions (kernels/rccl_async.hip)
class PyRcclAsync {
 public:
  // ps: list of (ps id, private params, m, v | None, t); ranges: [(lo, hi)] per PS
  PyRcclAsync(at::Tensor params, at::Tensor grads, int64_t world, int64_t rank, py::list ranges,
              std::vector<int64_t> hosts, py::list ps, int64_t opt, double lr, double b1,
              double b2, double eps, double mu, bool self_sessions, double weight_decay,
              bool nesterov)
      : params_(params), grads_(grads) {
    check_f32_cuda(params, "params");
    check_f32_cuda(grads, "grads");
    std::vector<int> h(hosts.begin(), hosts.end());
    c10::hip::HIPGuard guard(params.device().index());
    // (opt: Adam, else momentum; scale 1: the workers push unscaled gradients)
    r_ = std::make_unique<ddl::RcclAsync>(
        params.data_ptr<float>(), grads.data_ptr<float>(), (int)world, (int)rank,
        params.device().index(), index_ranges(ranges), h, ps_states(ps, keep_),
        spec_of("rccl async", opt == 0 ? ddl::kUpdAdam : ddl::kUpdMomentum, lr, b1, b2, eps, mu,
                1.0, weight_decay, nesterov),
        self_sessions);
  }
  void init_comm(py::bytes id) {
    std::string s = id;
    TORCH_CHECK(s.size() == 128, "RCCL unique id must be 128 bytes");
    py::gil_scoped_release nogil;  // collective
    r_->init_comm(s.data());
  }
  void attach_shm(std::string job, bool create) { r_->attach_shm(job, create); }
  void open_boxes(bool own) { r_->open_boxes(own); }
  void start(int64_t expected, bool provenance) { r_->start(expected, provenance); }
  void push_pull() {
    hipStream_t st = cur_stream();
    py::gil_scoped_release nogil;
    r_->push_pull(st);
  }
  void join() {
    py::gil_scoped_release nogil;
    r_->join();
  }
  void pause() {
    py::gil_scoped_release nogil;
    r_->pause();
  }
  void resume() { r_->resume(); }
  int64_t t(int64_t ps) const { return r_->t((int)ps); }
  void set_t(int64_t ps, int64_t t) { r_->set_t((int)ps, t); }
  int64_t served() const { return r_->served(); }
  std::vector<std::array<int64_t, 4>> provenance() const { return r_->provenance(); }

 private:
  at::Tensor params_, grads_;
  std::vector<at::Tensor> keep_;
  std::unique_ptr<ddl::RcclAsync> r_;
};

// native async worker step (kernels/async_runner.hip)
class PyAsyncRunner {
 public:
  PyAsyncRunner(PyEngine& eng, PyAsyncPeer& peer, int64_t world, int64_t rank,
                std::vector<int64_t> seg_of_ps, int64_t epoch0)
      : eng_(eng), grads_(peer.grads()) {
    std::vector<int> seg(seg_of_ps.begin(), seg_of_ps.end());
    c10::hip::HIPGuard guard(peer.device());
    r_ = std::make_unique<ddl::AsyncRunner>(eng.raw(), peer.raw(), (int)world, (int)rank,
                                            peer.device(), seg, (uint32_t)epoch0);
  }
  // step() or accumulate() of the native runner on one checked micro-batch
  using Micro = void (ddl::AsyncRunner::*)(const float*, const int64_t*, int, uint32_t,
                                           hipStream_t, double);
  void micro(Micro f, const at::Tensor& x, const at::Tensor& labels, int64_t seed,
             double timeout_s) {
    const PyEngine::Batch b = eng_.batch(x, labels);
    hipStream_t st = cur_stream();
    py::gil_scoped_release nogil;  // the host wait for the previous round
    (r_.get()->*f)(b.x, b.labels, b.B, (uint32_t)(seed & 0xFFFFFFFF), st, timeout_s);
  }
  void step(at::Tensor x, at::Tensor labels, int64_t seed, double timeout_s) {
    micro(&ddl::AsyncRunner::step, x, labels, seed, timeout_s);
  }
  // a non-final micro-batch of an accumulated round (set_accum)
  void accumulate(at::Tensor x, at::Tensor labels, int64_t seed, double timeout_s) {
    micro(&ddl::AsyncRunner::accumulate, x, labels, seed, timeout_s);
  }
  void finish(double timeout_s) {
    py::gil_scoped_release nogil;
    r_->finish(timeout_s);
  }
  int64_t epoch() const { return r_->epoch(); }
  void set_use_tail(bool on) { r_->set_use_tail(on); }
  void set_gate(bool on) { r_->set_gate(on); }
  // clip every round's gradient by its global norm before it is pushed / applied (max_norm 0: off)
  void set_clip(double max_norm, std::vector<std::pair<int64_t, int64_t>> ranges, at::Tensor out) {
    clip_.set(max_norm, grads_, ranges, out);
    r_->set_clip(clip_.site);
  }
  // every round's gradient is the mean over k micro-batches: k - 1 accumulate(), then step()
  void set_accum(int64_t k, std::vector<std::pair<int64_t, int64_t>> ranges,
                 c10::optional<at::Tensor> acc) {
    accum_.set(k, grads_, ranges, acc);
    r_->set_accum(accum_.site);
  }
  // ps: list of (ps id, private params, m, v, t), every PS (W = 1, Adam)
  void set_inline(py::list ps, double lr, double b1, double b2, double eps, double scale,
                  bool provenance, double weight_decay) {
    r_->set_inline(ps_states(ps, keep_, /*need_v=*/true),
                   spec_of("set_inline", ddl::kUpdAdam, lr, b1, b2, eps, 0.0, scale, weight_decay,
                           false, /*f32=*/true),
                   provenance);
  }
  bool inline_on() const { return r_->inline_on(); }
  int64_t inline_t(int64_t ps) const { return r_->inline_t((int)ps); }
  void inline_sync_ps() { r_->inline_sync_ps(cur_stream()); }
  std::vector<std::array<int64_t, 4>> inline_provenance() const { return r_->inline_provenance(); }
  int64_t update_launches() const { return r_->update_launches(); }

 private:
  PyEngine& eng_;
  at::Tensor grads_;
  PyClipSite clip_;
  PyAccumSite accum_;
  std::vector<at::Tensor> keep_;
  std::unique_ptr<ddl::AsyncRunner> r_;
};

class PyRunner {
 public:
  PyRunner(PyEngine& eng, at::Tensor params, at::Tensor grads, int64_t world, int64_t rank)
      : eng_(eng), params_(params), grads_(grads), world_(world) {
    check_f32_cuda(params, "params");
    check_f32_cuda(grads, "grads");
    TORCH_CHECK(params.numel() == grads.numel(), "params/grads size mismatch");
    r_ = std::make_unique<ddl::SyncRunner>(eng.raw(), params.data_ptr<float>(),
                                           grads.data_ptr<float>(), (int)world, (int)rank);
  }
  static py::bytes unique_id() {
    char id[128];
    ddl::SyncRunner::unique_id(id);
    return py::bytes(id, 128);
  }
  static std::string probe() { return ddl::SyncRunner::probe(); }
  void init_comm(py::bytes id, bool force) {
    std::string s = id;
    TORCH_CHECK(s.size() == 128, "RCCL unique id must be 128 bytes");
    py::gil_scoped_release nogil;  // collective: blocks until every rank joins
    r_->init_comm(s.data(), force);
  }
  bool has_comm() const { return r_->has_comm(); }
  void set_peer(PyPeer& p) {
    peer_keep_ = &p;
    r_->set_peer(p.raw());
  }
  // all buckets with w := sum over ranks of g (the xGMI self-test; blocks until done)
  void peer_selftest_step() {
    py::gil_scoped_release nogil;
    r_->peer_selftest_step(cur_stream());
    (void)hipStreamSynchronize(cur_stream());
  }
  // units: list of (seg, kind, host, ps, [(lo, hi, state_off)], m|None, v|None, shard|None
  //                 [, bucket])
  void set_units(py::list units) {
    std::vector<ddl::RunnerUnit> out;
    keep_.clear();
    const int64_t n = params_.numel();
    for (auto item : units) {
      auto t = item.cast<py::tuple>();
      TORCH_CHECK(t.size() == 8 || t.size() == 9, "unit tuple must have 8 or 9 fields");
      ddl::RunnerUnit u;
      u.seg = t[0].cast<int>();
      u.kind = t[1].cast<int>();
      u.host = t[2].cast<int>();
      u.ps = t[3].cast<int>();
      auto opt_ptr = [&](py::handle h, int64_t need, const char* what) -> float* {
        if (h.is_none()) return nullptr;
        at::Tensor x = h.cast<at::Tensor>();
        check_f32_cuda(x, what);
        TORCH_CHECK(x.numel() >= need, what, " too small");
        keep_.push_back(x);
        return x.data_ptr<float>();
      };
      int64_t need_state = 0, need_shard = 0;
      if (t.size() == 9) u.bucket = t[8].cast<int>();
      // an xGMI OWNER bucket (tensor-granular plan): its owner updates the whole unit
      const bool owner_bucket = u.kind == ddl::RunnerUnit::XGMI && r_->peer() &&
                                u.bucket >= 0 && u.bucket < r_->peer()->num_buckets() &&
                                r_->peer()->owner(u.bucket) >= 0;
      for (auto r : t[4].cast<py::list>()) {
        auto rr = r.cast<py::tuple>();
        ddl::RunnerRange range{rr[0].cast<int64_t>(), rr[1].cast<int64_t>(), rr[2].cast<int64_t>()};
        TORCH_CHECK(0 <= range.lo && range.lo <= range.hi && range.hi <= n, "range out of bounds");
        int64_t len = range.hi - range.lo;
        if (u.kind == ddl::RunnerUnit::RS ||
            (u.kind == ddl::RunnerUnit::XGMI && !owner_bucket)) {  // (AR and
          // XGMI_REPL update the whole range on every rank: state for all of it)
          // reduce-scatter: this rank updates (and needs state / a shard buffer for) 1/W of it;
          // a remainder would silently get no exchange and no update
          TORCH_CHECK(len % world_ == 0, "RS unit range [", range.lo, ", ", range.hi,
                      ") is not divisible by the world size ", world_);
          len /= world_;
          if (u.kind == ddl::RunnerUnit::RS) need_shard = std::max(need_shard, len);
        }
        need_state = std::max(need_state, range.state_off + len);
        u.ranges.push_back(range);
      }
      u.m = opt_ptr(t[5], need_state, "m");
      u.v = opt_ptr(t[6], need_state, "v");
      u.shard = opt_ptr(t[7], need_shard, "shard");
      out.push_back(std::move(u));
    }
    r_->set_units(out);
  }
  void set_optimizer(int64_t kind, double lr, double b1, double b2, double eps, double mu,
                     double weight_decay, bool nesterov) {
    r_->set_optimizer(
        spec_of("set_optimizer", kind, lr, b1, b2, eps, mu, 1.0, weight_decay, nesterov));
  }
  void set_scale(double grad_scale, double coef) { r_->set_scale((float)grad_scale, (float)coef); }
  // clip the step's gradient by its global norm; out: {norm, coef} after each step (max_norm 0: off)
  void set_clip(double max_norm, std::vector<std::pair<int64_t, int64_t>> ranges, at::Tensor out) {
    clip_.set(max_norm, grads_, ranges, out);
    r_->set_clip(clip_.site);
  }
  // every step's gradient is the mean over k micro-batches: k - 1 accumulate(), then step()
  void set_accum(int64_t k, std::vector<std::pair<int64_t, int64_t>> ranges,
                 c10::optional<at::Tensor> acc) {
    accum_.set(k, grads_, ranges, acc);
    r_->set_accum(accum_.site);
  }
  // a non-final micro-batch of an accumulated step (set_accum)
  void accumulate(at::Tensor x, at::Tensor labels, int64_t seed) {
    const PyEngine::Batch b = eng_.batch(x, labels);
    r_->accumulate(b.x, b.labels, b.B, (uint32_t)(seed & 0xFFFFFFFF), cur_stream());
  }
  void set_local_on_main(bool on) { r_->set_local_on_main(on); }
  void set_last_on_main(bool on) { r_->set_last_on_main(on); }
  void set_ready_flags(int64_t mode) { r_->set_ready_flags((int)mode); }
  void set_use_tail(bool on) { r_->set_use_tail(on); }
  void set_final_in_reduce(bool on) { r_->set_final_in_reduce(on); }
  void set_tail_cfg(int64_t first, int64_t f4) { r_->set_tail_cfg((int)first, (int)f4); }
  int64_t update_launches() const { return r_->update_launches(); }
  void step(at::Tensor x, at::Tensor labels, int64_t seed, std::vector<double> lr_t) {
    const PyEngine::Batch b = eng_.batch(x, labels);
    lr_.assign(lr_t.begin(), lr_t.end());
    if (lr_.empty()) lr_.push_back(0.f);
    r_->step(b.x, b.labels, b.B, (uint32_t)(seed & 0xFFFFFFFF), lr_.data(), cur_stream());
  }
  std::string async_error() { return r_->async_error(); }
  void abort() { r_->abort(); }
  void close() {
    py::gil_scoped_release nogil;
    r_->close();
  }
  py::tuple selftest() {
    std::string why;
    bool ok;
    {
      py::gil_scoped_release nogil;
      ok = r_->selftest(&why);
    }
    return py::make_tuple(ok, why);
  }

 private:
  PyEngine& eng_;
  at::Tensor params_, grads_;
  std::vector<at::Tensor> keep_;
  std::vector<float> lr_;
  PyClipSite clip_;
  PyAccumSite accum_;
  std::unique_ptr<ddl::SyncRunner> r_;
  int64_t world_;
  PyPeer* peer_keep_ = nullptr;
};

// ---- the fake RCCL behind rccl_api.h's override seam (kernels/fake_rccl.hip; tests only) --------
std::vector<at::Tensor>& fake_rccl_keep() {
  static std::vector<at::Tensor> keep;  // (buffers the fake holds raw pointers into)
  return keep;
}
std::vector<at::Tensor>& fake_rccl_step_keep() {
  static std::vector<at::Tensor> keep;
  return keep;
}

int64_t& fake_rccl_world() {
  static int64_t w = 0;
  return w;
}

void fake_rccl_install(int64_t world, int64_t rank, at::Tensor params, at::Tensor grads,
                       std::vector<at::Tensor> shards, c10::optional<at::Tensor> seen) {
  check_f32_cuda(params, "params");
  check_f32_cuda(grads, "grads");
  ddl::fake_rccl::Config c;
  c.world = (int)world, c.rank = (int)rank;
  c.params = {params.data_ptr<float>(), params.numel()};
  c.grads = {grads.data_ptr<float>(), grads.numel()};
  std::vector<at::Tensor> keep{params, grads};
  for (auto& s : shards) {
    check_f32_cuda(s, "shard");
    c.shards.push_back({s.data_ptr<float>(), s.numel()});
    keep.push_back(s);
  }
  if (seen.has_value()) {
    check_f32_cuda(*seen, "seen");
    TORCH_CHECK(seen->numel() == grads.numel(), "seen: the gradient buffer's length");
    c.seen = seen->data_ptr<float>();
    keep.push_back(*seen);
  }
  ddl::fake_rccl::install(c);
  fake_rccl_world() = world;
  fake_rccl_keep() = keep;
  fake_rccl_step_keep().clear();
}

void fake_rccl_remove() {
  ddl::fake_rccl::remove();
  fake_rccl_keep().clear();
  fake_rccl_step_keep().clear();
}

void fake_rccl_set_step(at::Tensor peer_grads, at::Tensor params_next) {
  check_f32_cuda(peer_grads, "peer_grads");
  check_f32_cuda(params_next, "params_next");
  TORCH_CHECK(!fake_rccl_keep().empty(), "fake RCCL not installed");
  const int64_t total = fake_rccl_keep()[0].numel();
  TORCH_CHECK(peer_grads.dim() == 2 && peer_grads.size(0) == fake_rccl_world() &&
                  peer_grads.size(1) == total && params_next.numel() == total,
              "peer_grads [W, total] and params_next [total]");
  ddl::fake_rccl::set_step(peer_grads.data_ptr<float>(), params_next.data_ptr<float>());
  fake_rccl_step_keep() = {peer_grads, params_next};
}

int fake_rccl_code(const std::string& name, const std::vector<const char*>& names) {
  for (size_t i = 0; i < names.size(); ++i)
    if (name == names[i]) return (int)i;
  TORCH_CHECK(false, "fake RCCL: unknown name '", name, "'");
  return -1;
}

py::list fake_rccl_calls() {
  py::list out;
  for (const auto& c : ddl::fake_rccl::calls())
    out.append(py::make_tuple(c.op, c.buf, c.off, c.count, c.root, c.stream, c.depth, c.rbuf,
                              c.roff));
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "ddl_amd native extension: gfx950 HIP kernels + C++ runtime";
  m.def("adam_flat", &adam_flat, "Fused TF1 Adam on a flat shard",
        py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("lr_t"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("scale") = 1.0);
  m.def("momentum_flat", &momentum_flat, "Fused momentum SGD on a flat shard");
  m.def("update_flat", &update_flat, "One update of a flat shard under rule `kind` (update.h)",
        py::arg("kind"), py::arg("w"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("step"),
        py::arg("b1") = 0.0, py::arg("b2") = 0.0, py::arg("eps") = 0.0, py::arg("mu") = 0.0,
        py::arg("scale") = 1.0, py::arg("decay") = 0.0, py::arg("nesterov") = false);
  m.def("clip_grads", &clip_grads,
        "Clip grads in place by the global norm over `ranges` [(lo, n)]; out <- {norm, coef}",
        py::arg("grads"), py::arg("ranges"), py::arg("max_norm"), py::arg("out"),
        py::arg("max_grid") = 0);
  m.def("accum_grads", &accum_grads,
        "One accumulation pass over `ranges` [(lo, n)]: mode 0 acc := grads, 1 acc += grads, "
        "2 grads := (acc + grads) * float32(1 / k)",
        py::arg("grads"), py::arg("acc"), py::arg("ranges"), py::arg("mode"), py::arg("k"),
        py::arg("max_grid") = 0);
  m.def("assemble_batch", &assemble_batch,
        "Rows [0, b) of xb [>= b,784] and yb [>= b] from the training set: row i is training row "
        "perm(base + i; N, key) (base + i unshuffled), translated by its draw in [-s, s]^2",
        py::arg("x_train"), py::arg("y_train"), py::arg("xb"), py::arg("yb"), py::arg("b"),
        py::arg("base"), py::arg("key"), py::arg("key_shift"), py::arg("s"), py::arg("shuffle"));
  m.attr("CLIP_CHUNK") = (int)ddl::kClipChunk;
  m.attr("CLIP_SLOTS") = (int)ddl::kClipSlots;
  m.def("upd_decay", [](double lr, double weight_decay) {
          return (double)ddl::upd_decay(lr, weight_decay);
        }, "The decoupled weight decay's factor lr * wd as every rule carries it (float32, widened)");
  m.def("adam_step_size", [](double lr, double b1, double b2, int64_t t) {
          return (double)ddl::adam_step_size(lr, b1, b2, t);
        }, "TF1 Adam's lr_t at step t as the native runtime forms it (float32, returned widened)");
  // per-block timestamps of the split-K dual launches (kernels/stamps.h; a build with
  // DDL_STAMPS=1 records them, the default build records nothing)
  m.def("stamps_enabled", []() { return (bool)DDL_STAMPS; });
  m.def("stamps_begin", [](int64_t cap) {
    ddl::StampState& s = ddl::stamp_state();
    if (s.buf) (void)hipFree(s.buf);
    s.buf = nullptr;
    s.cap = s.next = 0;
    s.log.clear();
    if (cap <= 0) return;
    TORCH_CHECK(hipMalloc(&s.buf, (size_t)cap * 64) == hipSuccess, "stamp buffer");
    TORCH_CHECK(hipMemset(s.buf, 0, (size_t)cap * 64) == hipSuccess, "stamp buffer");
    s.cap = cap;
  });
  m.def("stamps_end", []() {
    ddl::StampState& s = ddl::stamp_state();
    TORCH_CHECK(hipDeviceSynchronize() == hipSuccess, "stamps: device sync");
    at::Tensor out = at::empty({(int64_t)s.next, 8}, at::kLong);
    if (s.next)
      TORCH_CHECK(hipMemcpy(out.data_ptr(), s.buf, (size_t)s.next * 64, hipMemcpyDeviceToHost) ==
                      hipSuccess, "stamps: copy");
    std::vector<std::vector<int64_t>> log;
    for (const auto& r : s.log) log.push_back({r.off, r.nblocks, r.sub, r.gx, r.gy, r.gz});
    if (s.buf) (void)hipFree(s.buf);
    s.buf = nullptr;
    s.cap = s.next = 0;
    s.log.clear();
    return std::make_pair(out, log);
  });
  m.def("mfma_peak", [](at::Tensor out, int64_t blocks, int64_t iters, int64_t kind) {
    check_f32_cuda(out, "out");
    TORCH_CHECK(out.numel() >= blocks * 64, "out too small");
    ddl::launch_mfma_peak(out.data_ptr<float>(), (int)blocks, (int)iters, cur_stream(), (int)kind);
  }, "diagnostic: per iteration 2 chains of v_mfma_f32_32x32x2_f32 (kind 0) or 4 of "
     "v_mfma_f32_16x16x4_f32 (kind 1), the same FLOPs", py::arg("out"), py::arg("blocks"),
     py::arg("iters"), py::arg("kind") = 0);
  m.def("gemm_nomem", [](at::Tensor out, at::Tensor slab, int64_t M, int64_t N, int64_t K,
                         int64_t splits) {
    ddl::launch_gemm_nomem(out.data_ptr<float>(), (int)M, (int)N, (int)K, (int)splits,
                           slab.data_ptr(), nullptr, cur_stream());
  }, "diagnostic: engine GEMM structure with register-only operand loads");
  m.def("xcd_sweep", [](at::Tensor a, c10::optional<at::Tensor> want, at::Tensor out) {
    check_f32_cuda(a, "a");
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kInt && out.numel() >= 2, "out: 2 int32");
    if (want) {
      check_f32_cuda(*want, "want");
      TORCH_CHECK(want->numel() == a.numel(), "want: same size as a");
    }
    ddl::launch_xcd_sweep(a.data_ptr<float>(), want ? want->data_ptr<float>() : nullptr,
                          a.numel(), out.data_ptr<int>(), cur_stream());
  }, "xGMI self-test probe: every XCD reads (warms) every line of a, or counts mismatches "
     "against want into out[0]", py::arg("a"), py::arg("want"), py::arg("out"));
  m.attr("OP_COUNT") = (int)ddl::OP_COUNT;

  py::class_<PyEngine>(m, "Engine")
      .def(py::init<std::vector<at::Tensor>, std::vector<at::Tensor>, int64_t, int64_t, double>(),
           py::arg("params"), py::arg("grads"), py::arg("max_batch"), py::arg("train_batch"),
           py::arg("keep_prob"))
      .def("set_keep_prob", &PyEngine::set_keep_prob)
      .def("set_splits", &PyEngine::set_splits)
      .def("get_splits", &PyEngine::get_splits)
      .def("set_cfg", &PyEngine::set_cfg)
      .def("get_cfg", &PyEngine::get_cfg)
      .def("set_eval_cfg", &PyEngine::set_eval_cfg)
      .def("get_eval_cfg", &PyEngine::get_eval_cfg)
      .def("effective_cfg", [](const PyEngine& e) { return e.effective(true); })
      .def("effective_eval_cfg", [](const PyEngine& e) { return e.effective(false); })
      .def_static("op_has_cfg", [](int op, int cfg, bool train) {
        return ddl::op_has_cfg(op, cfg, train);
      })
      .def("set_concurrent", &PyEngine::set_concurrent)
      .def("set_dual", &PyEngine::set_dual)
      .def("flush_update_tail", &PyEngine::flush_update_tail, py::arg("kind"), py::arg("w"),
           py::arg("g"), py::arg("m"), py::arg("v"), py::arg("step"), py::arg("b1"), py::arg("b2"),
           py::arg("eps"), py::arg("mu"), py::arg("scale"), py::arg("decay") = 0.0,
           py::arg("nesterov") = false)
      .def("queue_update_tail", &PyEngine::queue_update_tail, py::arg("kind"), py::arg("w"),
           py::arg("g"), py::arg("m"), py::arg("v"), py::arg("step"), py::arg("b1"), py::arg("b2"),
           py::arg("eps"), py::arg("mu"), py::arg("scale"), py::arg("decay") = 0.0,
           py::arg("nesterov") = false)
      .def("dispatch_hits", &PyEngine::dispatch_hits)
      .def("reset_dispatch_hits", &PyEngine::reset_dispatch_hits)
      .def("set_fc_wgrad_defer", [](PyEngine& e, bool on) { e.raw()->sched.fc_wgrad_defer = on; })
      .def("fc_wgrad_defer", [](PyEngine& e) { return e.raw()->sched.fc_wgrad_defer; })
      .def("set_conv1_direct", [](PyEngine& e, bool on) { e.raw()->sched.conv1_direct = on; })
      .def("conv1_direct", [](PyEngine& e) { return e.raw()->sched.conv1_direct; })
      .def("set_conv1_wgrad_direct", [](PyEngine& e, bool on) { e.raw()->sched.conv1_wgrad_direct = on; })
      .def("conv1_wgrad_direct", [](PyEngine& e) { return e.raw()->sched.conv1_wgrad_direct; })
      .def("set_wide_thr", &PyEngine::set_wide_thr)
      .def("set_wide", &PyEngine::set_wide)
      .def("set_dual_bfirst", &PyEngine::set_dual_bfirst)
      .def("get_dual_bfirst", &PyEngine::get_dual_bfirst)
      .def("get_wide", &PyEngine::get_wide)
      .def("forward", &PyEngine::forward, py::arg("x"), py::arg("seed"), py::arg("train"))
      .def("backward_segment", &PyEngine::backward_segment)
      .def("run_op", &PyEngine::run_op)
      .def("zero_correct", &PyEngine::zero_correct)
      .def("eval_count", &PyEngine::eval_count)
      .def("head_fwd", &PyEngine::head_fwd)
      .def("buffer", &PyEngine::buffer)
      .def("max_batch", &PyEngine::max_batch)
      .def("workspace_bytes", &PyEngine::workspace_bytes)
      .def_static("op_shape", &PyEngine::op_shape);

  py::class_<PyRunner>(m, "SyncRunner")
      .def(py::init<PyEngine&, at::Tensor, at::Tensor, int64_t, int64_t>(), py::arg("engine"),
           py::arg("params"), py::arg("grads"), py::arg("world"), py::arg("rank"),
           py::keep_alive<1, 2>())
      .def_static("unique_id", &PyRunner::unique_id)
      .def_static("probe", &PyRunner::probe)
      .def("init_comm", &PyRunner::init_comm, py::arg("id"), py::arg("force") = false)
      .def("has_comm", &PyRunner::has_comm)
      .def("set_units", &PyRunner::set_units)
      .def("set_optimizer", &PyRunner::set_optimizer, py::arg("kind"), py::arg("lr"),
           py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("mu"),
           py::arg("weight_decay") = 0.0, py::arg("nesterov") = false)
      .def("set_scale", &PyRunner::set_scale)
      .def("set_clip", &PyRunner::set_clip, py::arg("max_norm"), py::arg("ranges"), py::arg("out"))
      .def("set_accum", &PyRunner::set_accum, py::arg("k"), py::arg("ranges"), py::arg("acc"))
      .def("accumulate", &PyRunner::accumulate, py::arg("x"), py::arg("labels"), py::arg("seed"))
      .def("set_local_on_main", &PyRunner::set_local_on_main)
      .def("set_last_on_main", &PyRunner::set_last_on_main)
      .def("set_use_tail", &PyRunner::set_use_tail)
      .def("set_ready_flags", &PyRunner::set_ready_flags)
      .def("set_final_in_reduce", &PyRunner::set_final_in_reduce)
      .def("update_launches", &PyRunner::update_launches,
           "Stand-alone optimizer kernel launches issued for the most recent step()")
      .def("set_tail_cfg", &PyRunner::set_tail_cfg)
      .def("step", &PyRunner::step)
      .def("selftest", &PyRunner::selftest)
      .def("set_peer", &PyRunner::set_peer, py::keep_alive<1, 2>())
      .def("peer_selftest_step", &PyRunner::peer_selftest_step)
      .def("async_error", &PyRunner::async_error)
      .def("abort", &PyRunner::abort)
      .def("close", &PyRunner::close);

  py::class_<PyAsyncPeer>(m, "AsyncPeer")
      .def(py::init<at::Tensor, at::Tensor, int64_t, int64_t, py::list, std::vector<int64_t>,
                    int64_t>(),
           py::arg("params"), py::arg("grads"), py::arg("world"), py::arg("rank"),
           py::arg("ranges"), py::arg("hosts"), py::arg("max_slices") = 512)
      .def("handle", &PyAsyncPeer::handle)
      .def("open", &PyAsyncPeer::open)
      .def("push_all", &PyAsyncPeer::push_all)
      .def("attach_done", &PyAsyncPeer::attach_done)
      .def("wait_done", &PyAsyncPeer::wait_done)
      .def("apply", &PyAsyncPeer::apply, py::arg("ps"), py::arg("worker"), py::arg("epoch"),
           py::arg("opt"), py::arg("ps_params"), py::arg("m"), py::arg("v"), py::arg("lr_t"),
           py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("lr"), py::arg("mu"),
           py::arg("scale"), py::arg("weight_decay") = 0.0, py::arg("nesterov") = false)
      .def("unmap_peers", &PyAsyncPeer::unmap_peers)
      .def("close", &PyAsyncPeer::close)
      .def("error", &PyAsyncPeer::error);

  py::class_<PyAsyncService>(m, "AsyncService")
      .def(py::init<PyAsyncPeer&, int64_t, py::list, int64_t, double, double, double,
                    double, double, double, int64_t, bool, double, bool>(),
           py::arg("peer"), py::arg("world"), py::arg("ps"), py::arg("opt"), py::arg("lr"),
           py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("mu"), py::arg("scale"),
           py::arg("epoch0"), py::arg("provenance"), py::arg("weight_decay") = 0.0,
           py::arg("nesterov") = false, py::keep_alive<1, 2>())
      .def("start", &PyAsyncService::start)
      .def("join", &PyAsyncService::join)
      .def("t", &PyAsyncService::t)
      .def("pause", &PyAsyncService::pause)
      .def("resume", &PyAsyncService::resume)
      .def("served", &PyAsyncService::served)
      .def("provenance", &PyAsyncService::provenance)
      .def("mode", &PyAsyncService::mode);

  py::class_<PyRcclAsync>(m, "RcclAsync")
      .def(py::init<at::Tensor, at::Tensor, int64_t, int64_t, py::list, std::vector<int64_t>,
                    py::list, int64_t, double, double, double, double, double, bool, double,
                    bool>(),
           py::arg("params"), py::arg("grads"), py::arg("world"), py::arg("rank"),
           py::arg("ranges"), py::arg("hosts"), py::arg("ps"), py::arg("opt"), py::arg("lr"),
           py::arg("b1"), py::arg("b2"), py::arg("eps"), py::arg("mu"), py::arg("self_sessions"),
           py::arg("weight_decay") = 0.0, py::arg("nesterov") = false)
      .def("init_comm", &PyRcclAsync::init_comm)
      .def("attach_shm", &PyRcclAsync::attach_shm)
      .def("open_boxes", &PyRcclAsync::open_boxes)
      .def("start", &PyRcclAsync::start)
      .def("push_pull", &PyRcclAsync::push_pull)
      .def("join", &PyRcclAsync::join)
      .def("pause", &PyRcclAsync::pause)
      .def("resume", &PyRcclAsync::resume)
      .def("t", &PyRcclAsync::t)
      .def("set_t", &PyRcclAsync::set_t)
      .def("served", &PyRcclAsync::served)
      .def("provenance", &PyRcclAsync::provenance);

  py::class_<PyAsyncRunner>(m, "AsyncRunner")
      .def(py::init<PyEngine&, PyAsyncPeer&, int64_t, int64_t, std::vector<int64_t>, int64_t>(),
           py::arg("engine"), py::arg("peer"), py::arg("world"), py::arg("rank"),
           py::arg("seg_of_ps"), py::arg("epoch0"),
           py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
      .def("step", &PyAsyncRunner::step)
      .def("finish", &PyAsyncRunner::finish)
      .def("epoch", &PyAsyncRunner::epoch)
      .def("set_use_tail", &PyAsyncRunner::set_use_tail)
      .def("set_gate", &PyAsyncRunner::set_gate)
      .def("set_clip", &PyAsyncRunner::set_clip, py::arg("max_norm"), py::arg("ranges"),
           py::arg("out"))
      .def("set_accum", &PyAsyncRunner::set_accum, py::arg("k"), py::arg("ranges"),
           py::arg("acc"))
      .def("accumulate", &PyAsyncRunner::accumulate, py::arg("x"), py::arg("labels"),
           py::arg("seed"), py::arg("timeout_s") = 600.0)
      .def("set_inline", &PyAsyncRunner::set_inline, py::arg("ps"), py::arg("lr"), py::arg("b1"),
           py::arg("b2"), py::arg("eps"), py::arg("scale"), py::arg("provenance"),
           py::arg("weight_decay") = 0.0)
      .def("inline_on", &PyAsyncRunner::inline_on)
      .def("inline_t", &PyAsyncRunner::inline_t)
      .def("inline_sync_ps", &PyAsyncRunner::inline_sync_ps)
      .def("inline_provenance", &PyAsyncRunner::inline_provenance)
      .def("update_launches", &PyAsyncRunner::update_launches,
           "Stand-alone optimizer kernel launches issued for the most recent in-line step()");

  py::class_<PyPeer>(m, "PeerExchange")
      .def(py::init<at::Tensor, at::Tensor, int64_t, int64_t, py::list, int64_t, int64_t>(),
           py::arg("params"), py::arg("grads"), py::arg("world"), py::arg("rank"),
           py::arg("buckets"), py::arg("max_slices") = 128, py::arg("repl_bucket") = -1)
      .def("handle", &PyPeer::handle)
      .def("open", &PyPeer::open)
      .def("error", &PyPeer::error)
      .def("nslices", &PyPeer::nslices)
      .def("owner", &PyPeer::owner)
      .def("launch", &PyPeer::launch, py::arg("bucket"), py::arg("epoch"), py::arg("kind"),
           py::arg("m"), py::arg("v"), py::arg("step"), py::arg("b1"), py::arg("b2"),
           py::arg("eps"), py::arg("mu"), py::arg("scale"), py::arg("coef"),
           py::arg("final_wait"), py::arg("decay") = 0.0, py::arg("nesterov") = false)
      .def("unmap_peers", &PyPeer::unmap_peers)
      .def("close", &PyPeer::close);

  py::class_<ddl::ShmMailbox>(m, "ShmMailbox")
      .def(py::init<const std::string&, int64_t, bool>(), py::arg("name"), py::arg("capacity"),
           py::arg("create"))
      .def("push", &ddl::ShmMailbox::push, py::call_guard<py::gil_scoped_release>())
      .def("pop", &ddl::ShmMailbox::pop, py::call_guard<py::gil_scoped_release>())
      .def("size", &ddl::ShmMailbox::size)
      .def("capacity", &ddl::ShmMailbox::capacity)
      .def("unlink", &ddl::ShmMailbox::unlink);

  // the fake RCCL of the rank tests (kernels/fake_rccl.hip): install / remove the override table
  m.def("fake_rccl_install", &fake_rccl_install, py::arg("world"), py::arg("rank"),
        py::arg("params"), py::arg("grads"), py::arg("shards"), py::arg("seen") = py::none(),
        "Configure the fake RCCL and put its table into the RCCL seam (refused while a "
        "SyncRunner holds a communicator)");
  m.def("fake_rccl_remove", &fake_rccl_remove, "Take the fake RCCL's table out of the seam");
  m.def("rccl_overridden", [] { return ddl::fake_rccl::overridden(); });
  m.def("fake_rccl_set_step", &fake_rccl_set_step, py::arg("peer_grads"), py::arg("params_next"));
  m.def("fake_rccl_set_peers", [](const std::string& n) {
    ddl::fake_rccl::set_peers(fake_rccl_code(n, {"table", "pattern"}));
  });
  m.def("fake_rccl_set_fault", [](const std::string& n) {
    ddl::fake_rccl::set_fault(fake_rccl_code(
        n, {"none", "rs_next_chunk", "ag_skip", "reduce_drop_peer", "bcast_skip"}));
  });
  m.def("fake_rccl_clear", &ddl::fake_rccl::clear);
  m.def("fake_rccl_calls", &fake_rccl_calls,
        "(op, buffer, offset, count, root, stream, group depth, recv buffer, recv offset)");
  m.def("fake_rccl_violations", &ddl::fake_rccl::violations);
  m.def("fake_rccl_group_depth", &ddl::fake_rccl::group_depth);
}
