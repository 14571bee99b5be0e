// Gradient accumulation (optim/accum.py): one launch folds every fresh gradient of a micro-step
// into its float32 accumulator.
//   accumulate  : rows (acc, grad, numel) of up to LARGE_MAXT float32 tensors, in one of four
//                 modes passed by value:
//                   FIRST  acc = g            (the accumulator is never zero-filled)
//                   ADD    acc = acc + g
//                   LAST   g   = (acc + g) * c, acc not written (12 B per element)
//                   SCALE  g   = g * c          (a window of a single micro-step)
//                 The sum and the product of LAST round separately, as torch's
//                 `(acc + g) * c` does.
//   accum_table : the device row table of more than MAXT rows
//
// The micro-step's position in its window is known on the host when the launch is issued, and
// a captured window holds one node per micro-step with its mode baked in: no device counter,
// no ticket, no atomics, no workgroup waits for another.  Non-finite values propagate by
// arithmetic alone (inf + x = inf, inf + -inf = nan), so the update's found_inf check sees them.
//
// Work: multi_tensor.h's granule space over the rows, in chunks of ADAM_THR * U granules walked
// grid-stride.  A tail granule and every granule of a row whose acc or grad is not 16-byte
// aligned move per element (load4 / store4).
#include "kernels/multi_tensor.h"

namespace dpa {
namespace accum {

using adam::ADAM_THR;
using adam::LARGE_MAXT;
using adam::MAXT;
using adam::load4;
using adam::store4;

enum Mode : int { FIRST = 0, ADD = 1, LAST = 2, SCALE = 3 };

// <= MAXT rows by value; off: prefix sum of granules
struct AccList {
  int n;
  long long off[MAXT + 1];
  long long numel[MAXT];
  float* a[MAXT];  // accumulator
  float* g[MAXT];  // gradient
};

// The rows of a launch in LDS, from the by-value list or the device table
// (int64: [0] n, [1] total granules, then off[n+1] | numel[n] | a[n] | g[n]).
struct StagedAcc {
  long long off[LARGE_MAXT + 1];
  long long numel[LARGE_MAXT];
  float* a[LARGE_MAXT];
  float* g[LARGE_MAXT];
  unsigned char vec[LARGE_MAXT];  // both pointers 16-byte aligned: granules move as one access
};

template <bool TABLE>
__device__ __forceinline__ void stage_rows(StagedAcc& S, const AccList& L, const int64_t* __restrict__ table, int& n,
                                           long long& total) {
  const int tid = threadIdx.x;
  if (TABLE) {
    n = (int)table[0];
    total = table[1];
    const int64_t* off = table + 2;
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = off[n + 1 + t];
      const int64_t a = off[2 * n + 1 + t], g = off[3 * n + 1 + t];
      S.a[t] = reinterpret_cast<float*>(a);
      S.g[t] = reinterpret_cast<float*>(g);
      S.vec[t] = ((a | g) & 15) == 0;
    }
  } else {
    n = L.n;
    total = L.off[L.n];
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = L.off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = L.numel[t];
      S.a[t] = L.a[t];
      S.g[t] = L.g[t];
      S.vec[t] = ((reinterpret_cast<uintptr_t>(L.a[t]) | reinterpret_cast<uintptr_t>(L.g[t])) & 15) == 0;
    }
  }
}

__global__ void __launch_bounds__(64) accum_table_kernel(int64_t* __restrict__ table, int n, int s, int e, AccList c,
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
    off[2 * n + 1 + t] = reinterpret_cast<int64_t>(c.a[k]);
    off[3 * n + 1 + t] = reinterpret_cast<int64_t>(c.g[k]);
  }
}

// (acc + g) * c: the sum and the product rounded one after the other, never contracted
__device__ __forceinline__ f32x4 mean_rule4(f32x4 a, f32x4 g, float c) {
#pragma clang fp contract(off)
  const f32x4 s = a + g;
  return s * c;
}
__device__ __forceinline__ f32x4 sum_rule4(f32x4 a, f32x4 g) { return a + g; }

// U granules per lane and chunk; NT: non-temporal loads of the accumulator (read once and
// written once per micro-step, as adam.hip's moments).  Both are measured choices
// (profiles/accum_ab.txt), set by set_variant for the measurement and the tests.
template <bool TABLE, int U, bool NT>
__global__ void __launch_bounds__(ADAM_THR)
accum_kernel(AccList L, const int64_t* __restrict__ table, int mode, float c, int grid) {
  __shared__ StagedAcc S;
  const int tid = threadIdx.x;
  int n;
  long long total;
  stage_rows<TABLE>(S, L, table, n, total);
  __syncthreads();
  constexpr long long CH = (long long)ADAM_THR * U;
  int t = 0;
  for (long long base = (long long)blockIdx.x * CH + tid; base - tid < total; base += (long long)grid * CH) {
    f32x4 av[U], gv[U];
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
        // FIRST and SCALE do not read the accumulator: it holds nothing yet
        if (mode == ADD || mode == LAST) av[u] = load4<NT>(S.a[t] + o, rem, vec);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tu = tt[u];
      if (tu < 0) continue;
      const long long o = (base + (long long)u * ADAM_THR - S.off[tu]) * 4, rem = S.numel[tu] - o;
      if (mode == FIRST) store4(S.a[tu] + o, rem, S.vec[tu], gv[u]);
      else if (mode == ADD) store4(S.a[tu] + o, rem, S.vec[tu], sum_rule4(av[u], gv[u]));
      else if (mode == LAST) store4(S.g[tu] + o, rem, S.vec[tu], mean_rule4(av[u], gv[u], c));
      else store4(S.g[tu] + o, rem, S.vec[tu], adam::unscaled(gv[u], c));
    }
  }
}

// ---------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------
static long long check_row(const at::Tensor& a, const at::Tensor& g, const char* who) {
  adam::check_f32(a);
  adam::check_f32(g);
  TORCH_CHECK(a.numel() == g.numel() && a.device() == g.device(), who,
              ": an accumulator and its gradient differ in size or device");
  TORCH_CHECK(a.numel() == 0 || a.data_ptr() != g.data_ptr(), who, ": an accumulator aliases its gradient");
  return (long long)a.numel();
}

static AccList list_of(const std::vector<at::Tensor>& accs, const std::vector<at::Tensor>& grads, size_t s, size_t e,
                       const char* who) {
  AccList L{};
  L.n = (int)(e - s);
  L.off[0] = 0;
  for (size_t i = s; i < e; ++i) {
    const int k = (int)(i - s);
    L.numel[k] = check_row(accs[i], grads[i], who);
    L.a[k] = accs[i].data_ptr<float>();
    L.g[k] = grads[i].data_ptr<float>();
    L.off[k + 1] = L.off[k] + (L.numel[k] + 3) / 4;
  }
  return L;
}

// Device table of up to LARGE_MAXT rows, written by by-value upload launches (one per MAXT rows)
at::Tensor accum_table(std::vector<at::Tensor> accs, std::vector<at::Tensor> grads) {
  const size_t n = accs.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)LARGE_MAXT, "accum_table: 1..", LARGE_MAXT, " rows");
  TORCH_CHECK(grads.size() == n, "accum_table: two lists of one length");
  auto table = at::empty({(int64_t)(2 + (n + 1) + 3 * n)}, accs[0].options().dtype(at::kLong));
  long long total = 0;
  for (size_t i = 0; i < n; ++i) total += ((long long)accs[i].numel() + 3) / 4;
  long long off_s = 0;
  for (size_t s = 0; s < n; s += MAXT) {
    const size_t e = std::min(n, s + MAXT);
    const AccList c = list_of(accs, grads, s, e, "accum_table");
    for (size_t i = s; i < e; ++i)
      TORCH_CHECK(accs[i].device() == table.device(), "accum_table: every row on one device");
    hipLaunchKernelGGL(accum_table_kernel, dim3(1), dim3(64), 0, cur_stream(), table.data_ptr<int64_t>(), (int)n,
                       (int)s, (int)e, c, off_s, total);
    DPA_CHECK_LAUNCH();
    off_s += c.off[c.n];
  }
  TORCH_CHECK(off_s == total, "accum_table: granule count");
  return table;
}

// Kernel variant (tests and measurements, profiles/accum_ab.txt): the granules per lane and
// chunk (0 = adam.hip's rule: 2 once that fills the grid, else 1 for twice the workgroups)
// and whether the accumulator is loaded non-temporally.
static int g_u = 0;
static bool g_nt = false;
void set_variant(int64_t u, bool nt) {
  TORCH_CHECK(u == 0 || u == 1 || u == 2 || u == 4, "accum.set_variant: 0 (by size), 1, 2 or 4 granules per lane");
  g_u = (int)u;
  g_nt = nt;
}

void accumulate(std::vector<at::Tensor> accs, std::vector<at::Tensor> grads, int64_t mode, double c,
                c10::optional<at::Tensor> table, int64_t total_granules) {
  TORCH_CHECK(mode >= FIRST && mode <= SCALE, "accumulate: mode 0 (first), 1 (add), 2 (last) or 3 (scale)");
  AccList L{};
  const int64_t* tab = nullptr;
  long long total;
  if (table.has_value()) {
    DPA_CHECK_INPUT(*table);
    TORCH_CHECK(table->scalar_type() == at::kLong && table->numel() >= 6 && total_granules >= 0,
                "accumulate: table from accum_table, and its granule count");
    tab = table->data_ptr<int64_t>();
    total = total_granules;  // only sizes the grid: the kernel reads the table's own count
  } else {
    const size_t n = accs.size();
    TORCH_CHECK(n >= 1 && n <= (size_t)MAXT, "accumulate: 1..", MAXT, " rows by value (more: accum_table)");
    TORCH_CHECK(grads.size() == n, "accumulate: two lists of one length");
    L = list_of(accs, grads, 0, n, "accumulate");
    for (size_t i = 0; i < n; ++i)
      TORCH_CHECK(accs[i].device() == accs[0].device(), "accumulate: every row on one device");
    total = L.off[L.n];
  }
  auto launch = [&](auto kern, int u) {
    const int grid = adam::grid_for(total, (long long)ADAM_THR * u);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab, (int)mode, (float)c, grid);
  };
  const int gu = g_u != 0 ? g_u : (total >= (long long)adam::grid_cap() * ADAM_THR * 2 ? 2 : 1);
  auto pick = [&](auto table_c, auto nt_c) {
    constexpr bool T = decltype(table_c)::value;
    constexpr bool N = decltype(nt_c)::value;
    if (gu == 1) launch(accum_kernel<T, 1, N>, 1);
    else if (gu == 2) launch(accum_kernel<T, 2, N>, 2);
    else launch(accum_kernel<T, 4, N>, 4);
  };
  if (tab != nullptr) {
    if (g_nt) pick(std::true_type{}, std::true_type{}); else pick(std::true_type{}, std::false_type{});
  } else {
    if (g_nt) pick(std::false_type{}, std::true_type{}); else pick(std::false_type{}, std::false_type{});
  }
  DPA_CHECK_LAUNCH();
}

}  // namespace accum

void register_accum(pybind11::module& m) {
  namespace py = pybind11;
  auto s = m.def_submodule("accum", "multi-tensor gradient accumulation into float32 accumulators");
  s.def("accumulate", &accum::accumulate, py::arg("accs"), py::arg("grads"), py::arg("mode"), py::arg("c") = 1.0,
        py::arg("table") = py::none(), py::arg("total_granules") = 0);
  s.def("accum_table", &accum::accum_table, py::arg("accs"), py::arg("grads"));
  s.def("set_variant", &accum::set_variant, py::arg("granules_per_lane"), py::arg("nontemporal") = false);
  s.attr("FIRST") = (int)accum::FIRST;
  s.attr("ADD") = (int)accum::ADD;
  s.attr("LAST") = (int)accum::LAST;
  s.attr("SCALE") = (int)accum::SCALE;
  s.attr("MAXT") = accum::MAXT;
  s.attr("LARGE_MAXT") = accum::LARGE_MAXT;
  s.attr("THR") = accum::ADAM_THR;
}

}  // namespace dpa
