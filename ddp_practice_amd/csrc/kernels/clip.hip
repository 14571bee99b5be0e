// Global-norm gradient clipping (optim/clip.py, optim/adamw.py): the norm of every gradient of
// a step in one read-only launch whose result is two device words, and the consumer that reads
// them -- the Adam update (adam.hip clip_coef) or, for any other optimizer, scale_.
//   grad_norm : out[0] = ||g||_2 over up to LARGE_MAXT tensors, out[1] = the clipping
//               coefficient min(1, max_norm / (norm + 1e-6)) with torch's roundings; optionally
//               of the unscaled gradients (grad_scale) and with nonfinite_check's found_inf
//   scale_    : g *= coef[0] in place; every workgroup returns at once when the word is 1.f
//
// The gradients are walked in adam.hip's granule space (kernels/multi_tensor.h) in chunks of
// ADAM_THR * NORM_U granules.  The sum of squares of ONE CHUNK is one fp32 partial, whichever
// workgroup computes it: the lane's 4 * NORM_U squares in index order, group_sum<64>, the four
// waves in wave order.  The partials go to partials[chunk] write-through (handoff.h st_wt);
// the workgroup that takes the launch's last ticket reads them all (ld_wt), adds them in a
// fixed order in float64 and rounds once.  So the result does not depend on the grid, no
// workgroup waits for another, and there is no float atomic and no fence (the hand-off is
// handoff.h's: write-through rows, one relaxed ticket per workgroup behind every wave's drain).
#include "kernels/handoff.h"
#include "kernels/multi_tensor.h"

namespace dpa {
namespace clip {

using adam::ADAM_THR;
using adam::AdamList;
using adam::LARGE_MAXT;
using adam::MAXT;
using adam::StagedGrads;

constexpr int NORM_U = 4;  // granules per lane and chunk: nonfinite_check's, whose pass this replaces
constexpr long long CHUNK = (long long)ADAM_THR * NORM_U;
constexpr int WAVES = ADAM_THR / 64;

// multi_tensor.h's load4 / store4 on global addresses.  The staged pointers come out of LDS as
// generic ones, and a flat load counts on the LDS counter too: the table reads of the next
// granule (S.off, S.numel) then wait for it, one memory latency per granule.  Gradients are
// device memory, so the accesses here are global ones and a lane's granules are in flight together
// (read off the ISA; on ResNet-50's set the norm launch measured 46.9 us before and 46.3 us after).
typedef const __attribute__((address_space(1))) f32x4* gload4_t;
typedef const __attribute__((address_space(1))) float* gload1_t;
typedef __attribute__((address_space(1))) f32x4* gstore4_t;
typedef __attribute__((address_space(1))) float* gstore1_t;
__device__ __forceinline__ f32x4 load4g(const float* p, long long rem, bool vec) {
  if (rem >= 4 && vec) return *(gload4_t)p;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < rem) v[j] = ((gload1_t)p)[j];
  return v;
}
__device__ __forceinline__ void store4g(float* p, long long rem, bool vec, f32x4 v) {
  if (rem >= 4 && vec) { *(gstore4_t)p = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < rem) ((gstore1_t)p)[j] = v[j];
}

// x * x, rounded on its own (no fma with the running sum)
__device__ __forceinline__ float square(float x) {
#pragma clang fp contract(off)
  return x * x;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// torch's clip coefficient from the norm: Tensor.__rdiv__ is reciprocal() * other, and
// clamp(max=1) keeps a NaN
__device__ __forceinline__ float coef_of(float norm, float max_norm) {
#pragma clang fp contract(off)
  const float c = (1.f / (norm + 1e-6f)) * max_norm;
  return c > 1.f ? 1.f : c;
}

template <bool TABLE>
__global__ void __launch_bounds__(ADAM_THR)
grad_norm_kernel(AdamList L, const int64_t* __restrict__ table, float max_norm, float* __restrict__ out,
                 float* partials, unsigned* ticket, const float* __restrict__ grad_scale,
                 float* __restrict__ found_inf, long long nchunks, int grid) {
  __shared__ StagedGrads S;
  __shared__ float s_wave[2][WAVES];
  __shared__ double s_fin[ADAM_THR];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const float gs = grad_scale != nullptr ? 1.f / grad_scale[0] : 1.f;
  int n;
  long long total;
  adam::stage_grads<TABLE>(S, L, table, n, total);
  __syncthreads();
  bool bad = false;
  int t = 0, par = 0;
  // nchunks is the host's count (it sized `partials`); the table's own total only bounds the loads
  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += grid, par ^= 1) {
    const long long base = chunk * CHUNK + tid;
    f32x4 gv[NORM_U];
#pragma unroll
    for (int u = 0; u < NORM_U; ++u) {
      const long long gi = base + (long long)u * ADAM_THR;
      gv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (gi < total) {
        while (S.off[t + 1] <= gi) ++t;
        const long long o = (gi - S.off[t]) * 4;
        gv[u] = load4g(S.g[t] + o, S.numel[t] - o, S.vec[t]);
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < NORM_U; ++u) {
      const f32x4 x = grad_scale != nullptr ? adam::unscaled(gv[u], gs) : gv[u];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bad |= !isfinite(gv[u][j]);
        acc = add_rn(acc, square(x[j]));
      }
    }
    acc = group_sum<64>(acc);
    if ((tid & 63) == 0) s_wave[par][tid >> 6] = acc;
    // one barrier per chunk: the next chunk writes the other half of s_wave, and the one after
    // that is behind the next barrier, which lane 0 joins only after this read
    __syncthreads();
    if (tid == 0) {
      float p = s_wave[par][0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) p = add_rn(p, s_wave[par][w]);
      st_wt(partials + chunk, p);
    }
  }
  if (found_inf != nullptr && __any(bad) && (tid & 63) == 0) found_inf[0] = 1.f;  // every writer stores the same value
  if (!last_arriver(ticket, (unsigned)grid, &s_flag)) return;
  // the last arriver: lane-strided sums of the partials, then a fixed tree, in float64
  // (FIN_U loads in flight per lane: one after the other, each waited for, they were a chain of
  // 25 memory latencies on ResNet-50's 6,250 chunks; the order of the adds is the same, and a
  // lane past the end adds +0)
  constexpr int FIN_U = 8;
  double d = 0.0;
  for (long long i = tid; i < nchunks; i += (long long)FIN_U * ADAM_THR) {
    float v[FIN_U];
#pragma unroll
    for (int k = 0; k < FIN_U; ++k) {  // clamped index, unconditional load: no branch between the loads
      const long long idx = i + (long long)k * ADAM_THR;
      v[k] = ld_wt(partials + (idx < nchunks ? idx : 0));
    }
#pragma unroll
    for (int k = 0; k < FIN_U; ++k) d += (i + (long long)k * ADAM_THR < nchunks) ? (double)v[k] : 0.0;
  }
  s_fin[tid] = d;
  __syncthreads();
#pragma unroll
  for (int w = ADAM_THR / 2; w > 0; w >>= 1) {
    if (tid < w) s_fin[tid] += s_fin[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const float norm = sqrtf((float)s_fin[0]);  // the sum rounded once to fp32, then the root's rounding
    out[0] = norm;
    out[1] = coef_of(norm, max_norm);
  }
}

template <bool TABLE>
__global__ void __launch_bounds__(ADAM_THR)
scale_kernel(AdamList L, const int64_t* __restrict__ table, const float* __restrict__ coef, int grid) {
  __shared__ StagedGrads S;
  const int tid = threadIdx.x;
  // the word first: a step that does not clip costs one load per workgroup
  const float c = coef[0];
  if (c == 1.f) return;
  int n;
  long long total;
  adam::stage_grads<TABLE>(S, L, table, n, total);
  __syncthreads();
  int t = 0;
  for (long long base = (long long)blockIdx.x * CHUNK + tid; base - tid < total; base += (long long)grid * CHUNK) {
    f32x4 gv[NORM_U];
    int tt[NORM_U];
#pragma unroll
    for (int u = 0; u < NORM_U; ++u) {
      const long long gi = base + (long long)u * ADAM_THR;
      tt[u] = -1;
      if (gi < total) {
        while (S.off[t + 1] <= gi) ++t;
        tt[u] = t;
        const long long o = (gi - S.off[t]) * 4;
        gv[u] = load4g(S.g[t] + o, S.numel[t] - o, S.vec[t]);
      }
    }
#pragma unroll
    for (int u = 0; u < NORM_U; ++u) {
      const int tu = tt[u];
      if (tu < 0) continue;
      const long long o = (base + (long long)u * ADAM_THR - S.off[tu]) * 4;
      store4g(S.g[tu] + o, S.numel[tu] - o, S.vec[tu], adam::unscaled(gv[u], c));
    }
  }
}

// 0: adam.hip's cap (8 workgroups per CU); n: at most n workgroups (tests and measurements: the
// norm must not depend on it)
static int g_grid_cap = 0;
void set_grid_cap(int64_t n) {
  TORCH_CHECK(n >= 0 && n <= (1 << 20), "clip.set_grid_cap: 0 (default) or a workgroup count");
  g_grid_cap = (int)n;
}
static int grid_of(long long nchunks) {
  const long long cap = g_grid_cap > 0 ? g_grid_cap : adam::grid_cap();
  return (int)std::max<long long>(1, std::min(nchunks, cap));
}

// the gradients of a launch: by value, or the g column of an adam_table
static long long grads_of(const std::vector<at::Tensor>& grads, const c10::optional<at::Tensor>& table,
                          int64_t total_granules, const at::Tensor& like, const char* who, AdamList& L,
                          const int64_t*& tab) {
  if (table.has_value()) {
    adam::check_table(*table);
    TORCH_CHECK(table->device() == like.device() && total_granules >= 0, who, ": table and its granule count");
    tab = table->data_ptr<int64_t>();
    return total_granules;
  }
  TORCH_CHECK(grads.size() >= 1 && grads.size() <= (size_t)MAXT, who, ": 1..", MAXT,
              " tensors by value (more: adam_table)");
  for (const auto& g : grads) TORCH_CHECK(g.device() == like.device(), who, ": every tensor on one device");
  L = adam::list_of({}, grads, {}, {}, 0, grads.size());
  tab = nullptr;
  return L.off[L.n];
}

void grad_norm(std::vector<at::Tensor> grads, double max_norm, at::Tensor out, at::Tensor partials,
               at::Tensor ticket, c10::optional<at::Tensor> grad_scale, c10::optional<at::Tensor> found_inf,
               c10::optional<at::Tensor> table, int64_t total_granules) {
  adam::check_f32(out);
  adam::check_f32(partials);
  DPA_CHECK_INPUT(ticket);
  TORCH_CHECK(out.numel() == 2, "grad_norm: out is two f32 words (norm, coefficient)");
  TORCH_CHECK(ticket.scalar_type() == at::kInt && ticket.numel() == 1 && ticket.device() == out.device() &&
                  partials.device() == out.device(),
              "grad_norm: ticket is one zero-initialised int32 word, partials f32, on out's device");
  const float* gsp = adam::opt_word(grad_scale, out, "grad_scale");
  float* fi = const_cast<float*>(adam::opt_word(found_inf, out, "found_inf"));
  AdamList L{};
  const int64_t* tab = nullptr;
  const long long total = grads_of(grads, table, total_granules, out, "grad_norm", L, tab);
  const long long nchunks = std::max<long long>(1, (total + CHUNK - 1) / CHUNK);
  TORCH_CHECK(partials.numel() >= nchunks, "grad_norm: partials holds ", partials.numel(), " words, the gradients ",
              nchunks, " chunks");
  const int grid = grid_of(nchunks);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab, (float)max_norm,
                       out.data_ptr<float>(), partials.data_ptr<float>(),
                       reinterpret_cast<unsigned*>(ticket.data_ptr<int>()), gsp, fi, nchunks, grid);
  };
  if (tab != nullptr) launch(grad_norm_kernel<true>); else launch(grad_norm_kernel<false>);
  DPA_CHECK_LAUNCH();
}

void scale_(std::vector<at::Tensor> grads, at::Tensor coef, c10::optional<at::Tensor> table,
            int64_t total_granules) {
  adam::check_f32(coef);
  TORCH_CHECK(coef.numel() == 1, "scale_: coef is one f32 word");
  AdamList L{};
  const int64_t* tab = nullptr;
  const long long total = grads_of(grads, table, total_granules, coef, "scale_", L, tab);
  const int grid = grid_of(std::max<long long>(1, (total + CHUNK - 1) / CHUNK));
  if (tab != nullptr)
    hipLaunchKernelGGL(scale_kernel<true>, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab,
                       coef.data_ptr<float>(), grid);
  else
    hipLaunchKernelGGL(scale_kernel<false>, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab,
                       coef.data_ptr<float>(), grid);
  DPA_CHECK_LAUNCH();
}

}  // namespace clip

void register_clip(pybind11::module& m) {
  namespace py = pybind11;
  auto s = m.def_submodule("clip", "global-norm gradient clipping: a grid-independent norm launch and its consumers");
  s.def("grad_norm", &clip::grad_norm, py::arg("grads"), py::arg("max_norm"), py::arg("out"), py::arg("partials"),
        py::arg("ticket"), py::arg("grad_scale") = py::none(), py::arg("found_inf") = py::none(),
        py::arg("table") = py::none(), py::arg("total_granules") = 0);
  s.def("scale_", &clip::scale_, py::arg("grads"), py::arg("coef"), py::arg("table") = py::none(),
        py::arg("total_granules") = 0);
  s.def("set_grid_cap", &clip::set_grid_cap, py::arg("n"));
  s.attr("U") = clip::NORM_U;
  s.attr("THR") = clip::ADAM_THR;
}

}  // namespace dpa
