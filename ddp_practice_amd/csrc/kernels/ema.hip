// Exponential moving average of a model's weights (optim/ema.py): one launch updates every
// shadow tensor.
//   ema_update : rows (shadow, source, words, kind) of up to LARGE_MAXT tensors; kind average:
//                shadow = lerp(shadow, source, w) by common.h lerp_rule (float32); kind copy: the
//                source's 4-byte words stored into the shadow, no arithmetic on them (float
//                buffers without use_buffers, integer buffers always; an int64 scalar is two words)
//   ema_table  : the device row table of more than MAXT rows
//
// The update count n_averaged lives on the device, an int64 word as in torch's AveragedModel:
// a host branch on it (torch's `copy_param = bool(n_averaged == 0)`) is frozen into a captured
// graph.  Every workgroup reads the word before anything else: 0 makes every row a copy (the
// first update), and with warm-up the lerp weight is computed from it (common.h
// ema_warmup_weight).  The word is advanced as adam.hip advances its step count: each workgroup
// takes a ticket when it is done, and the one that takes the launch's last ticket stores n + 1
// and resets the ticket word.  No workgroup waits for another (no grid barrier, no fence, no
// residency requirement): a workgroup that has not started has not taken its ticket, so the
// last ticket cannot be taken before every workgroup has read the word.
//
// Work: multi_tensor.h's granule space over the rows' 4-byte words, in chunks of ADAM_THR * U
// granules walked grid-stride.  A tail granule and every granule of a row whose shadow or source
// is not 16-byte aligned move per word (load4 / store4).
#include "kernels/multi_tensor.h"

namespace dpa {
namespace ema {

using adam::ADAM_THR;
using adam::LARGE_MAXT;
using adam::MAXT;
using adam::load4;
using adam::store4;

// <= MAXT rows by value; off: prefix sum of granules, numel: 4-byte words
struct EmaList {
  int n;
  long long off[MAXT + 1];
  long long numel[MAXT];
  float* s[MAXT];        // shadow
  const float* x[MAXT];  // source
  unsigned char copy[MAXT];
};

// The rows of a launch in LDS, from the by-value list or the device table
// (int64: [0] n, [1] total granules, then off[n+1] | numel[n] | s[n] | x[n] | copy[n]).
struct StagedEma {
  long long off[LARGE_MAXT + 1];
  long long numel[LARGE_MAXT];
  float* s[LARGE_MAXT];
  const float* x[LARGE_MAXT];
  unsigned char copy[LARGE_MAXT];
  unsigned char vec[LARGE_MAXT];  // both pointers 16-byte aligned: granules move as one access
};

template <bool TABLE>
__device__ __forceinline__ void stage_rows(StagedEma& S, const EmaList& L, const int64_t* __restrict__ table, int& n,
                                           long long& total) {
  const int tid = threadIdx.x;
  if (TABLE) {
    n = (int)table[0];
    total = table[1];
    const int64_t* off = table + 2;
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = off[n + 1 + t];
      const int64_t s = off[2 * n + 1 + t], x = off[3 * n + 1 + t];
      S.s[t] = reinterpret_cast<float*>(s);
      S.x[t] = reinterpret_cast<const float*>(x);
      S.copy[t] = off[4 * n + 1 + t] != 0;
      S.vec[t] = ((s | x) & 15) == 0;
    }
  } else {
    n = L.n;
    total = L.off[L.n];
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = L.off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = L.numel[t];
      S.s[t] = L.s[t];
      S.x[t] = L.x[t];
      S.copy[t] = L.copy[t];
      S.vec[t] = ((reinterpret_cast<uintptr_t>(L.s[t]) | reinterpret_cast<uintptr_t>(L.x[t])) & 15) == 0;
    }
  }
}

__global__ void __launch_bounds__(64) ema_table_kernel(int64_t* __restrict__ table, int n, int s, int e, EmaList c,
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
    off[2 * n + 1 + t] = reinterpret_cast<int64_t>(c.s[k]);
    off[3 * n + 1 + t] = reinterpret_cast<int64_t>(c.x[k]);
    off[4 * n + 1 + t] = c.copy[k];
  }
}

// U granules per lane and chunk.  Non-temporal loads of the shadows (read once and written once per
// step, as adam.hip's moments) were measured and were not faster -- ResNet-50's set 72.04 us against
// 71.95 us plain, the ConvNet's 5.10 against 4.80 us (profiles/ema_ab.txt) -- so the loads are plain.
template <bool TABLE, int U>
__global__ void __launch_bounds__(ADAM_THR)
ema_kernel(EmaList L, const int64_t* __restrict__ table, long long* count, unsigned* ticket, float w, float decay,
           int warmup, int grid) {
  __shared__ StagedEma S;
  const int tid = threadIdx.x;
  // the count first: an atomic load, so it is made once, here, before this workgroup's ticket
  // (the barrier below waits for every wave's copy of it)
  const long long n0 = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int n;
  long long total;
  stage_rows<TABLE>(S, L, table, n, total);
  __syncthreads();
  const bool first = n0 == 0;  // the first update copies every row
  const float we = (warmup && !first) ? ema_warmup_weight(n0, decay, w) : w;
  constexpr long long CH = (long long)ADAM_THR * U;
  int t = 0;
  for (long long base = (long long)blockIdx.x * CH + tid; base - tid < total; base += (long long)grid * CH) {
    f32x4 sv[U], xv[U];
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
        xv[u] = load4<false>(S.x[t] + o, rem, vec);
        // a copied granule does not read the shadow: its words are only moved, never computed with
        if (!(first || S.copy[t])) sv[u] = load4<false>(S.s[t] + o, rem, vec);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tu = tt[u];
      if (tu < 0) continue;
      const long long o = (base + (long long)u * ADAM_THR - S.off[tu]) * 4, rem = S.numel[tu] - o;
      f32x4 r = xv[u];
      if (!(first || S.copy[tu])) r = lerp_rule4(sv[u], xv[u], we);
      store4(S.s[tu] + o, rem, S.vec[tu], r);
    }
  }
  // the ticket: the last of the launch's `grid` workgroups advances the count (relaxed: the only
  // access it orders is this workgroup's read of the count, which arrived before the barrier above)
  if (tid == 0) {
    const unsigned k = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == (unsigned)grid - 1u) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(count, n0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------
// a row's tensors: dense, contiguous, same dtype and size, whole 4-byte words; an averaged row float32
static long long check_row(const at::Tensor& s, const at::Tensor& x, bool copy, const char* who) {
  DPA_CHECK_INPUT(s);
  DPA_CHECK_INPUT(x);
  TORCH_CHECK(s.scalar_type() == x.scalar_type() && s.numel() == x.numel() && s.device() == x.device(), who,
              ": a shadow and its source differ in dtype, size or device");
  TORCH_CHECK(copy || s.scalar_type() == at::kFloat, who, ": an averaged row is float32");
  const long long bytes = (long long)s.numel() * (long long)s.element_size();
  TORCH_CHECK(bytes % 4 == 0 && reinterpret_cast<uintptr_t>(s.data_ptr()) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 4 == 0,
              who, ": rows are whole, 4-byte aligned 4-byte words");
  TORCH_CHECK(s.numel() == 0 || s.data_ptr() != x.data_ptr(), who, ": a shadow aliases its source");
  return bytes / 4;
}

static EmaList list_of(const std::vector<at::Tensor>& shadows, const std::vector<at::Tensor>& sources,
                       const std::vector<bool>& copy, size_t s, size_t e, const char* who) {
  EmaList L{};
  L.n = (int)(e - s);
  L.off[0] = 0;
  for (size_t i = s; i < e; ++i) {
    const int k = (int)(i - s);
    L.numel[k] = check_row(shadows[i], sources[i], copy[i], who);
    L.s[k] = reinterpret_cast<float*>(shadows[i].data_ptr());
    L.x[k] = reinterpret_cast<const float*>(sources[i].data_ptr());
    L.copy[k] = copy[i] ? 1 : 0;
    L.off[k + 1] = L.off[k] + (L.numel[k] + 3) / 4;
  }
  return L;
}

// Device table of up to LARGE_MAXT rows, written by by-value upload launches (one per MAXT rows)
at::Tensor ema_table(std::vector<at::Tensor> shadows, std::vector<at::Tensor> sources, std::vector<bool> copy) {
  const size_t n = shadows.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)LARGE_MAXT, "ema_table: 1..", LARGE_MAXT, " rows");
  TORCH_CHECK(sources.size() == n && copy.size() == n, "ema_table: three lists of one length");
  auto table = at::empty({(int64_t)(2 + (n + 1) + 4 * n)}, shadows[0].options().dtype(at::kLong));
  long long total = 0;
  for (size_t i = 0; i < n; ++i)
    total += ((long long)shadows[i].numel() * (long long)shadows[i].element_size() / 4 + 3) / 4;
  long long off_s = 0;
  for (size_t s = 0; s < n; s += MAXT) {
    const size_t e = std::min(n, s + MAXT);
    const EmaList c = list_of(shadows, sources, copy, s, e, "ema_table");
    for (size_t i = s; i < e; ++i)
      TORCH_CHECK(shadows[i].device() == table.device(), "ema_table: every row on one device");
    hipLaunchKernelGGL(ema_table_kernel, dim3(1), dim3(64), 0, cur_stream(), table.data_ptr<int64_t>(), (int)n,
                       (int)s, (int)e, c, off_s, total);
    DPA_CHECK_LAUNCH();
    off_s += c.off[c.n];
  }
  TORCH_CHECK(off_s == total, "ema_table: granule count");
  return table;
}

// Kernel variant (tests and measurements, profiles/ema_ab.txt): the granules per lane and chunk.
// 0 = adam.hip's rule: 2 once that fills the grid (ResNet-50's set: 69.9-73.6 us over 1 / 2 / 4 in two
// runs, in no consistent order), else 1 for twice the workgroups (the ConvNet's: 4.6 us, 2: 5.1, 4: 6.7).
static int g_u = 0;
void set_variant(int64_t u) {
  TORCH_CHECK(u == 0 || u == 1 || u == 2 || u == 4, "ema.set_variant: 0 (by size), 1, 2 or 4 granules per lane");
  g_u = (int)u;
}

void ema_update(std::vector<at::Tensor> shadows, std::vector<at::Tensor> sources, std::vector<bool> copy,
                at::Tensor count, at::Tensor ticket, double weight, double decay, bool warmup,
                c10::optional<at::Tensor> table, int64_t total_granules) {
  DPA_CHECK_INPUT(count);
  DPA_CHECK_INPUT(ticket);
  TORCH_CHECK(count.scalar_type() == at::kLong && count.numel() == 1, "ema_update: n_averaged is one int64 word");
  TORCH_CHECK(ticket.scalar_type() == at::kInt && ticket.numel() == 1 && ticket.device() == count.device(),
              "ema_update: ticket is one zero-initialised int32 word on the count's device");
  EmaList L{};
  const int64_t* tab = nullptr;
  long long total;
  if (table.has_value()) {
    DPA_CHECK_INPUT(*table);
    TORCH_CHECK(table->scalar_type() == at::kLong && table->numel() >= 7 && table->device() == count.device() &&
                    total_granules >= 0, "ema_update: table from ema_table, and its granule count");
    tab = table->data_ptr<int64_t>();
    total = total_granules;  // only sizes the grid: the kernel reads the table's own count
  } else {
    const size_t n = shadows.size();
    TORCH_CHECK(n >= 1 && n <= (size_t)MAXT, "ema_update: 1..", MAXT, " rows by value (more: ema_table)");
    TORCH_CHECK(sources.size() == n && copy.size() == n, "ema_update: three lists of one length");
    L = list_of(shadows, sources, copy, 0, n, "ema_update");
    for (size_t i = 0; i < n; ++i)
      TORCH_CHECK(shadows[i].device() == count.device(), "ema_update: n_averaged on the rows' device");
    total = L.off[L.n];
  }
  auto launch = [&](auto kern, int u) {
    const int grid = adam::grid_for(total, (long long)ADAM_THR * u);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(ADAM_THR), 0, cur_stream(), L, tab,
                       reinterpret_cast<long long*>(count.data_ptr<int64_t>()),
                       reinterpret_cast<unsigned*>(ticket.data_ptr<int>()), (float)weight, (float)decay,
                       (int)warmup, grid);
  };
  const int gu = g_u != 0 ? g_u : (total >= (long long)adam::grid_cap() * ADAM_THR * 2 ? 2 : 1);
  auto pick = [&](auto table_c) {
    constexpr bool T = decltype(table_c)::value;
    if (gu == 1) launch(ema_kernel<T, 1>, 1);
    else if (gu == 2) launch(ema_kernel<T, 2>, 2);
    else launch(ema_kernel<T, 4>, 4);
  };
  if (tab != nullptr) pick(std::true_type{}); else pick(std::false_type{});
  DPA_CHECK_LAUNCH();
}

}  // namespace ema

void register_ema(pybind11::module& m) {
  namespace py = pybind11;
  auto s = m.def_submodule("ema", "multi-tensor weight averaging with a device-resident update count");
  s.def("ema_update", &ema::ema_update, py::arg("shadows"), py::arg("sources"), py::arg("copy"),
        py::arg("n_averaged"), py::arg("ticket"), py::arg("weight"), py::arg("decay"), py::arg("warmup") = false,
        py::arg("table") = py::none(), py::arg("total_granules") = 0);
  s.def("ema_table", &ema::ema_table, py::arg("shadows"), py::arg("sources"), py::arg("copy"));
  s.def("set_variant", &ema::set_variant, py::arg("granules_per_lane"));
  s.attr("MAXT") = ema::MAXT;
  s.attr("LARGE_MAXT") = ema::LARGE_MAXT;
  s.attr("THR") = ema::ADAM_THR;
}

}  // namespace dpa
