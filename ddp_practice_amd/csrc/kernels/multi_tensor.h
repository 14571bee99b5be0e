// The multi-tensor granule space of adam.hip and clip.hip: the tensors' 16-byte granules,
// concatenated (each tensor rounded up to whole granules), in fixed chunks of ADAM_THR * U
// granules that the workgroups walk grid-stride.  Up to MAXT tensors travel by value, up to
// LARGE_MAXT through a device table (adam.hip adam_table).  The last granule of a tensor whose
// numel is not a multiple of 4, and every granule of a tensor with a pointer that is not
// 16-byte aligned, moves per element; lanes past a tensor's end read +0 and are not written.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "kernels/amp_step.h"

namespace dpa {
namespace adam {

using opt::MAXT;
constexpr int LARGE_MAXT = 512;  // == optim.hip's: one bound for every tensor table of the package
constexpr int ADAM_THR = 256;

// <= MAXT tensors by value; off: prefix sum of granules
struct AdamList {
  int n;
  long long off[MAXT + 1];
  long long numel[MAXT];
  float* p[MAXT];
  float* g[MAXT];
  float* m[MAXT];
  float* v[MAXT];
};

// The tensor list of a launch in LDS, from the by-value list or the device table
// (int64: [0] n, [1] total granules, then off[n+1] | numel[n] | p[n] | g[n] | m[n] | v[n]).
struct Staged {
  long long off[LARGE_MAXT + 1];
  long long numel[LARGE_MAXT];
  float* p[LARGE_MAXT];
  float* g[LARGE_MAXT];
  float* m[LARGE_MAXT];
  float* v[LARGE_MAXT];
  unsigned char vec[LARGE_MAXT];  // all four pointers 16-byte aligned: granules move as one access
};

template <bool TABLE>
__device__ __forceinline__ void stage(Staged& S, const AdamList& L, const int64_t* __restrict__ table, int& n,
                                      long long& total, bool grads_only) {
  const int tid = threadIdx.x;
  if (TABLE) {
    n = (int)table[0];
    total = table[1];
    const int64_t* off = table + 2;
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = off[n + 1 + t];
      const int64_t p = off[2 * n + 1 + t], g = off[3 * n + 1 + t], m = off[4 * n + 1 + t], v = off[5 * n + 1 + t];
      S.p[t] = reinterpret_cast<float*>(p);
      S.g[t] = reinterpret_cast<float*>(g);
      S.m[t] = reinterpret_cast<float*>(m);
      S.v[t] = reinterpret_cast<float*>(v);
      S.vec[t] = ((grads_only ? g : (p | g | m | v)) & 15) == 0;
    }
  } else {
    n = L.n;
    total = L.off[L.n];
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = L.off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = L.numel[t];
      S.p[t] = L.p[t];
      S.g[t] = L.g[t];
      S.m[t] = L.m[t];
      S.v[t] = L.v[t];
      const uintptr_t a = reinterpret_cast<uintptr_t>(L.g[t]);
      const uintptr_t b = reinterpret_cast<uintptr_t>(L.p[t]) | reinterpret_cast<uintptr_t>(L.m[t]) |
                          reinterpret_cast<uintptr_t>(L.v[t]);
      S.vec[t] = ((grads_only ? a : (a | b)) & 15) == 0;
    }
  }
}

// The gradients of a launch only (clip.hip): a third of Staged's LDS.
struct StagedGrads {
  long long off[LARGE_MAXT + 1];
  long long numel[LARGE_MAXT];
  float* g[LARGE_MAXT];
  unsigned char vec[LARGE_MAXT];
};

template <bool TABLE>
__device__ __forceinline__ void stage_grads(StagedGrads& S, const AdamList& L, const int64_t* __restrict__ table,
                                            int& n, long long& total) {
  const int tid = threadIdx.x;
  if (TABLE) {
    n = (int)table[0];
    total = table[1];
    const int64_t* off = table + 2;
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = off[n + 1 + t];
      const int64_t g = off[3 * n + 1 + t];
      S.g[t] = reinterpret_cast<float*>(g);
      S.vec[t] = (g & 15) == 0;
    }
  } else {
    n = L.n;
    total = L.off[L.n];
    for (int t = tid; t <= n; t += ADAM_THR) S.off[t] = L.off[t];
    for (int t = tid; t < n; t += ADAM_THR) {
      S.numel[t] = L.numel[t];
      S.g[t] = L.g[t];
      S.vec[t] = (reinterpret_cast<uintptr_t>(L.g[t]) & 15) == 0;
    }
  }
}

// One granule: `rem` = elements from p to the tensor's end (>= 1); lanes past it read 0 and
// are not written.
template <bool NT>
__device__ __forceinline__ f32x4 load4(const float* p, long long rem, bool vec) {
  if (rem >= 4 && vec) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return *reinterpret_cast<const f32x4*>(p);
  }
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < rem) v[j] = p[j];
  return v;
}
__device__ __forceinline__ void store4(float* p, long long rem, bool vec, f32x4 v) {
  if (rem >= 4 && vec) { *reinterpret_cast<f32x4*>(p) = v; return; }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < rem) p[j] = v[j];
}

// g * (1/scale), rounded on its own: what unscale_check_kernel (optim.hip) stores
__device__ __forceinline__ f32x4 unscaled(f32x4 g, float gs) {
#pragma clang fp contract(off)
  return g * gs;
}

// ---------------------------------------------------------------------------
// Host helpers
// ---------------------------------------------------------------------------
inline void check_f32(const at::Tensor& t) {
  DPA_CHECK_INPUT(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat, "optimizer tensors must be f32");
}

inline const float* opt_word(const c10::optional<at::Tensor>& w, const at::Tensor& like, const char* what) {
  if (!w.has_value()) return nullptr;
  check_f32(*w);
  TORCH_CHECK(w->numel() == 1 && w->device() == like.device(), what, ": one f32 word on the parameters' device");
  return w->data_ptr<float>();
}

// Workgroups of a launch over `total` granules in chunks of `chunk`: one per chunk up to 8 per CU
inline int grid_cap() {
  static const int cap = [] {
    int dev = 0, cus = 0;
    DPA_CHECK_HIP(hipGetDevice(&dev));
    DPA_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return std::max(1, resident_cus(cus)) * 8;
  }();
  return cap;
}
inline int grid_for(long long total, long long chunk) {
  return (int)std::max<long long>(1, std::min<long long>((total + chunk - 1) / chunk, grid_cap()));
}

// the by-value list of tensors [s, e); lists other than grads may be empty (gradient readers)
inline AdamList list_of(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                        const std::vector<at::Tensor>& ms, const std::vector<at::Tensor>& vs, size_t s, size_t e) {
  AdamList L{};
  L.n = (int)(e - s);
  L.off[0] = 0;
  for (size_t i = s; i < e; ++i) {
    const int k = (int)(i - s);
    check_f32(grads[i]);
    L.numel[k] = grads[i].numel();
    L.g[k] = grads[i].data_ptr<float>();
    if (!params.empty()) {
      check_f32(params[i]); check_f32(ms[i]); check_f32(vs[i]);
      TORCH_CHECK(params[i].numel() == L.numel[k] && ms[i].numel() == L.numel[k] && vs[i].numel() == L.numel[k],
                  "adam: a parameter, its gradient and its state differ in size");
      TORCH_CHECK(params[i].device() == grads[i].device() && ms[i].device() == grads[i].device() &&
                      vs[i].device() == grads[i].device(), "adam: tensors on one device");
      L.p[k] = params[i].data_ptr<float>();
      L.m[k] = ms[i].data_ptr<float>();
      L.v[k] = vs[i].data_ptr<float>();
    }
    L.off[k + 1] = L.off[k] + (L.numel[k] + 3) / 4;
  }
  return L;
}

inline void check_table(const at::Tensor& table) {
  DPA_CHECK_INPUT(table);
  TORCH_CHECK(table.scalar_type() == at::kLong && table.numel() >= 9, "adam: table from adam_table");
}

}  // namespace adam
}  // namespace dpa
