// Adam / AdamW (optim/adamw.py): one launch updates every tensor of a param group.
//   adam_step       : p, exp_avg, exp_avg_sq of up to LARGE_MAXT tensors by common.h adam_rule,
//                     predicated on found_inf read ON DEVICE, the unscale folded in
//                     (grad_scale), the rate optionally device-resident (lr_dev, optim/lr.py),
//                     the gradient optionally times a device-resident clipping coefficient
//                     (clip_coef, csrc/kernels/clip.hip grad_norm)
//   nonfinite_check : found_inf |= any(!isfinite(g)); reads the gradients, never writes them
//   adam_table      : the device tensor table of a group of more than MAXT tensors
//
// The step count t of the bias corrections lives on the device, one float32 word per param
// group: a by-value count would be frozen into a captured graph, as a by-value learning rate
// is (optim/lr.py).  Every workgroup reads the word before anything else and updates with
// t = word + 1; a launch that found_inf does not skip advances the word once, after every
// workgroup has read it: each workgroup takes a ticket when it is done, and the one that takes
// the last ticket stores word + 1 and resets the ticket word.  No workgroup waits for another
// (no grid barrier, no residency requirement): a workgroup that has not started has not taken
// its ticket, so the last ticket cannot be taken before every workgroup has read the word.
//
// Work: the tensors' 16-byte granules, concatenated (each tensor rounded up to whole granules),
// in fixed chunks of ADAM_THR * U granules that the workgroups walk grid-stride, so ResNet-50's
// 161 mostly tiny tensors do not cost a workgroup each.  The last granule of a tensor whose
// numel is not a multiple of 4, and every granule of a tensor with a pointer that is not
// 16-byte aligned, moves per element (kernels/multi_tensor.h, shared with clip.hip).
#include "kernels/multi_tensor.h"

namespace dpa {
namespace adam {

// Device table (int64): [0] n, [1] total granules, then off[n+1] | numel[n] | p[n] | g[n] | m[n] | v[n]
__global__ void __launch_bounds__(64) adam_table_kernel(int64_t* __restrict__ table, int n, int s, int e, AdamList c,
                                                        long long off_s, long long total) {
  // entries [s, e) of the table from a by-value chunk (graph-capturable, no host copy)
  const int k = threadIdx.x;
  int64_t* off = table + 2;
  if (k == 0 && s == 0) { table[0] = n; table[1] = total; }
  if (k == 0 && e == n) off[n] = total;
  if (k < e - s) {
    const int t = s + k;
    off[t] = off_s + c.off[k];
    off[n + 1 + t] = c.numel[k];
    off[2 * n + 1 + t] = reinterpret_cast<int64_t>(c.p[k]);
    off[3 * n + 1 + t] = reinterpret_cast<int64_t>(c.g[k]);
    off[4 * n + 1 + t] = reinterpret_cast<int64_t>(c.m[k]);
    off[5 * n + 1 + t] = reinterpret_cast<int64_t>(c.v[k]);
  }
}

// 1 - lr*wd from a device-resident rate: the product rounded, then the difference
__device__ __forceinline__ float decay_of(float lr, float wd) {
#pragma clang fp contract(off)
  return 1.f - lr * wd;
}

// w1 = 1 - beta1 and w2 = 1 - beta2 are rounded from the host's doubles, as the Python scalars
// torch hands to _foreach_lerp_ / _foreach_addcmul_ are (1.f - (float)beta2 would be off by 3e-5
// of itself at beta2 = 0.999)
struct AdamHyper {
  float inv_lr, decay_mul, beta1, beta2, w1, w2, eps, wd;
  int decoupled, maximize;
};

// U granules per lane and chunk; NT: exp_avg / exp_avg_sq loads non-temporal; CLIP: the unscaled
// gradient times clip_coef[0], the two products rounded one after the other -- what unscale_
// followed by clip.scale_ stores.  A template flag, not a null test, and the word is the last
// argument, behind `grid`: the unclipped instantiations are instruction for instruction the
// kernels measured in profiles/adamw_step_ab.txt (no argument of theirs moved).
template <bool TABLE, int U, bool NT, bool CLIP>
__global__ void __launch_bounds__(ADAM_THR)
adam_kernel(AdamList L, const int64_t* __restrict__ table, float* step_word, unsigned* ticket, AdamHyper h,
            const float* __restrict__ found_inf, const float* __restrict__ grad_scale,
            const float* __restrict__ lr_dev, int grid, const float* __restrict__ clip_coef) {
  __shared__ Staged S;
  const int tid = threadIdx.x;
  // the step count first: an atomic load, so it is made once, here, before this workgroup's
  // ticket (the barrier below waits for every wave's copy of it)
  const float step0 = __hip_atomic_load(step_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float inv_lr = h.inv_lr, decay_mul = h.decay_mul;
  if (lr_dev != nullptr) {
    const float lr = lr_dev[0];
    inv_lr = 1.f / lr;
    decay_mul = decay_of(lr, h.wd);
  }
  // a skipped step: every workgroup returns (found_inf is not written by this launch), no
  // ticket is taken, p / m / v and the step word stay as they are
  if (found_inf != nullptr && found_inf[0] != 0.f) return;
  const float gs = grad_scale != nullptr ? 1.f / grad_scale[0] : 1.f;
  float cf = 1.f;  // a skipped step has returned above: whatever the word holds then is not read
  if constexpr (CLIP) cf = clip_coef[0];
  int n;
  long long total;
  stage<TABLE>(S, L, table, n, total, false);
  AdamCoef c;
  c.decay_mul = decay_mul; c.wd = h.wd; c.w1 = h.w1; c.beta2 = h.beta2; c.w2 = h.w2;
  c.eps = h.eps; c.decoupled = h.decoupled; c.maximize = h.maximize;
  __syncthreads();
  adam_bias(step0 + 1.f, inv_lr, h.beta1, h.beta2, c);
  constexpr long long CH = (long long)ADAM_THR * U;
  int t = 0;
  for (long long base = (long long)blockIdx.x * CH + tid; base - tid < total; base += (long long)grid * CH) {
    f32x4 pv[U], gv[U], mv[U], vv[U];
    int tt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long gi = base + (long long)u * ADAM_THR;
      tt[u] = -1;
      if (gi < total) {
        while (S.off[t + 1] <= gi) ++t;
        tt[u] = t;
        const long long o = (gi - S.off[t]) * 4, rem = S.numel[t] - o;
        const bool vec = S.vec[t];
        gv[u] = load4<false>(S.g[t] + o, rem, vec);
        pv[u] = load4<false>(S.p[t] + o, rem, vec);
        mv[u] = load4<NT>(S.m[t] + o, rem, vec);
        vv[u] = load4<NT>(S.v[t] + o, rem, vec);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tu = tt[u];
      if (tu < 0) continue;
      const long long o = (base + (long long)u * ADAM_THR - S.off[tu]) * 4, rem = S.numel[tu] - o;
      const bool vec = S.vec[tu];
      f32x4 pn = pv[u], mn = mv[u], vn = vv[u];
      f32x4 gu = unscaled(gv[u], gs);
      if constexpr (CLIP) gu = unscaled(gu, cf);
      adam_rule4(pn, gu, mn, vn, c);
      store4(S.m[tu] + o, rem, vec, mn);
      store4(S.v[tu] + o, rem, vec, vn);
      store4(S.p[tu] + o, rem, vec, pn);
    }
  }
  // the ticket: the last of the launch's `grid` workgroups advances the count
  // (no ticket word: the count stays -- what the advance costs is measured against this)
  if (tid == 0 && ticket != nullptr) {
    // relaxed: the only access the ticket orders is this workgroup's read of the count, whose
    // value had arrived before the barrier above; a release here writes the XCD's L2 back at
    // the end of every workgroup (+96 us on ResNet-50's set, profiles/adamw_step_ab.txt)
    const unsigned k = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == (unsigned)grid - 1u) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(step_word, step0 + 1.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

constexpr int CHECK_U = 4;

template <bool TABLE>
__global__ void __launch_bounds__(ADAM_THR)
nonfinite_check_kernel(AdamList L, const int64_t* __restrict__ table, float* __restrict__ found_inf, int grid) {
  __shared__ Staged S;
  const int tid = threadIdx.x;
  int n;
  long long total;
  stage<TABLE>(S, L, table, n, total, true);
  __syncthreads();
  constexpr long long CH = (long long)ADAM_THR * CHECK_U;
  bool bad = false;
  int t = 0;
  for (long long base = (long long)blockIdx.x * CH + tid; base - tid < total; base += (long long)grid * CH) {
    f32x4 gv[CHECK_U];
#pragma unroll
    for (int u = 0; u < CHECK_U; ++u) {
      const long long gi = base + (long long)u * ADAM_THR;
      gv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (gi < total) {
        while (S.off[t + 1] <= gi) ++t;
        const long long o = (gi - S.off[t]) * 4;
        gv[u] = load4<false>(S.g[t] + o, S.numel[t] - o, S.vec[t]);
      }
    }
#pragma unroll
    for (int u = 0; u < CHECK_U; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) bad |= !isfinite(gv[u][j]);
  }
  if (__any(bad) && (tid & 63) == 0) found_inf[0] = 1.f;  // every writer stores the same value
}

// Device table of a group of up to LARGE_MAXT tensors: written by by-value upload launches
// (one per MAXT tensors), so building it is stream-ordered and graph-capturable.
at::Tensor adam_table(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, std::vector<at::Tensor> ms,
                      std::vector<at::Tensor> vs) {
  const size_t n = params.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)LARGE_MAXT, "adam_table: 1..", LARGE_MAXT, " tensors");
  TORCH_CHECK(grads.size() == n && ms.size() == n && vs.size() == n, "adam_table: four lists of one length");
  auto table = at::empty({(int64_t)(2 + (n + 1) + 5 * n)}, params[0].options().dtype(at::kLong));
  long long total = 0;
  for (size_t i = 0; i < n; ++i) total += (params[i].numel() + 3) / 4;
  long long off_s = 0;
  for (size_t s = 0; s < n; s += MAXT) {
    const size_t e = std::min(n, s + MAXT);
    const AdamList c = list_of(params, grads, ms, vs, s, e);
    hipLaunchKernelGGL(adam_table_kernel, dim3(1), dim3(64), 0, cur_stream(), table.data_ptr<int64_t>(), (int)n,
                       (int)s, (int)e, c, off_s, total);
    DPA_CHECK_LAUNCH();
    off_s += c.off[c.n];
  }
  return table;
}

// Kernel variant, measured in profiles/adamw_step_ab.txt: non-temporal exp_avg / exp_avg_sq loads
// (ResNet-50's set: 155.0 against 165.3 us at 2 granules per lane; the ConvNet's: no difference),
// and the granules per lane and chunk: 2 once that fills the grid (ResNet-50: 155.0 us, 1: 156.7,
// 4: 179.5), else 1 for twice the workgroups (the ConvNet: 5.8 us, 2: 7.1, 4: 9.6).  0 = that rule.
static bool g_nt = true;
static int g_u = 0;
void set_variant(bool nt, int64_t u) {
  TORCH_CHECK(u == 0 || u == 1 || u == 2 || u == 4, "adam.set_variant: 0 (by size), 1, 2 or 4 granules per lane");
  g_nt = nt;
  g_u = (int)u;
}

void adam_step(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, std::vector<at::Tensor> ms,
               std::vector<at::Tensor> vs, at::Tensor step_word, double lr, double beta1, double beta2, double eps,
               double wd, bool decoupled, bool maximize, c10::optional<at::Tensor> found_inf,
               c10::optional<at::Tensor> grad_scale, c10::optional<at::Tensor> lr_dev,
               c10::optional<at::Tensor> ticket, c10::optional<at::Tensor> table, int64_t total_granules,
               c10::optional<at::Tensor> clip_coef) {
  check_f32(step_word);
  TORCH_CHECK(step_word.numel() == 1, "adam_step: step_word is one f32 word");
  unsigned* tk = nullptr;  // None: the count is not advanced (measurements only)
  if (ticket.has_value()) {
    DPA_CHECK_INPUT(*ticket);
    TORCH_CHECK(ticket->scalar_type() == at::kInt && ticket->numel() == 1 && ticket->device() == step_word.device(),
                "adam_step: ticket is one zero-initialised int32 word on the step word's device");
    tk = reinterpret_cast<unsigned*>(ticket->data_ptr<int>());
  }
  const float* fi = opt_word(found_inf, step_word, "found_inf");
  const float* gsp = opt_word(grad_scale, step_word, "grad_scale");
  const float* lrp = opt_word(lr_dev, step_word, "lr_dev");
  const float* ccp = opt_word(clip_coef, step_word, "clip_coef");
  AdamList L{};
  const int64_t* tab = nullptr;
  long long total;
  if (table.has_value()) {
    check_table(*table);
    TORCH_CHECK(table->device() == step_word.device() && total_granules >= 0, "adam_step: table and its granule count");
    tab = table->data_ptr<int64_t>();
    total = total_granules;  // only sizes the grid: the kernel reads the table's own count
  } else {
    const size_t n = params.size();
    TORCH_CHECK(n >= 1 && n <= (size_t)MAXT, "adam_step: 1..", MAXT, " tensors by value (more: adam_table)");
    TORCH_CHECK(grads.size() == n && ms.size() == n && vs.size() == n, "adam_step: four lists of one length");
    TORCH_CHECK(params[0].device() == step_word.device(), "adam_step: step_word on the parameters' device");
    L = list_of(params, grads, ms, vs, 0, n);
    total = L.off[L.n];
  }
  // the scalar of torch's _foreach_mul_(params, 1 - lr*wd): a Python double, rounded once
  const AdamHyper h{(float)(1.0 / lr), (float)(1.0 - lr * wd), (float)beta1, (float)beta2, (float)(1.0 - beta1),
                    (float)(1.0 - beta2), (float)eps, (float)wd,
                    (int)decoupled, (int)maximize};
  auto launch = [&](auto kern, int u) {
    const int grid = grid_for(total, (long long)ADAM_THR * u);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab, step_word.data_ptr<float>(), tk, h,
                       fi, gsp, lrp, grid, ccp);
  };
  const int gu = g_u != 0 ? g_u : (total >= (long long)grid_cap() * ADAM_THR * 2 ? 2 : 1);
  auto pick = [&](auto table_c, auto clip_c) {
    constexpr bool T = decltype(table_c)::value, CL = decltype(clip_c)::value;
    if (g_nt) {
      if (gu == 1) launch(adam_kernel<T, 1, true, CL>, 1);
      else if (gu == 2) launch(adam_kernel<T, 2, true, CL>, 2);
      else launch(adam_kernel<T, 4, true, CL>, 4);
    } else {
      if (gu == 1) launch(adam_kernel<T, 1, false, CL>, 1);
      else if (gu == 2) launch(adam_kernel<T, 2, false, CL>, 2);
      else launch(adam_kernel<T, 4, false, CL>, 4);
    }
  };
  auto pick_clip = [&](auto table_c) {
    if (ccp != nullptr) pick(table_c, std::true_type{}); else pick(table_c, std::false_type{});
  };
  if (tab != nullptr) pick_clip(std::true_type{}); else pick_clip(std::false_type{});
  DPA_CHECK_LAUNCH();
}

void nonfinite_check(std::vector<at::Tensor> grads, at::Tensor found_inf, c10::optional<at::Tensor> table,
                     int64_t total_granules) {
  check_f32(found_inf);
  TORCH_CHECK(found_inf.numel() == 1, "nonfinite_check: found_inf is one f32 word");
  AdamList L{};
  const int64_t* tab = nullptr;
  long long total;
  if (table.has_value()) {
    check_table(*table);
    TORCH_CHECK(table->device() == found_inf.device() && total_granules >= 0,
                "nonfinite_check: table and its granule count");
    tab = table->data_ptr<int64_t>();
    total = total_granules;
  } else {
    TORCH_CHECK(grads.size() >= 1 && grads.size() <= (size_t)MAXT, "nonfinite_check: 1..", MAXT,
                " tensors by value (more: adam_table)");
    TORCH_CHECK(grads[0].device() == found_inf.device(), "nonfinite_check: found_inf on the gradients' device");
    L = list_of({}, grads, {}, {}, 0, grads.size());
    total = L.off[L.n];
  }
  const int grid = grid_for(total, (long long)ADAM_THR * CHECK_U);
  if (tab != nullptr)
    hipLaunchKernelGGL(nonfinite_check_kernel<true>, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab,
                       found_inf.data_ptr<float>(), grid);
  else
    hipLaunchKernelGGL(nonfinite_check_kernel<false>, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab,
                       found_inf.data_ptr<float>(), grid);
  DPA_CHECK_LAUNCH();
}

}  // namespace adam

void register_adam(pybind11::module& m) {
  namespace py = pybind11;
  auto s = m.def_submodule("adam", "multi-tensor Adam / AdamW kernels with a device-resident step count");
  s.def("adam_step", &adam::adam_step, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("step_word"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("weight_decay"), py::arg("decoupled"), py::arg("maximize"),
        py::arg("found_inf") = py::none(), py::arg("grad_scale") = py::none(), py::arg("lr_dev") = py::none(),
        py::kw_only(), py::arg("ticket"), py::arg("table") = py::none(), py::arg("total_granules") = 0,
        py::arg("clip_coef") = py::none());
  s.def("nonfinite_check", &adam::nonfinite_check, py::arg("grads"), py::arg("found_inf"),
        py::arg("table") = py::none(), py::arg("total_granules") = 0);
  s.def("adam_table", &adam::adam_table, py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"));
  s.def("set_variant", &adam::set_variant, py::arg("nt_loads"), py::arg("granules_per_lane"));
  s.attr("MAXT") = adam::MAXT;
  s.attr("LARGE_MAXT") = adam::LARGE_MAXT;
}

}  // namespace dpa
