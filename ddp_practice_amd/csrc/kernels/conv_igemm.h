// Shared by the implicit-GEMM convolution translation units: conv_igemm.hip (forward /
// data gradients + fused BN statistics) and conv_wgrad.hip (weight gradients).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include "common.h"
#include "kernels/handoff.h"

namespace dpa {
namespace igemm {

constexpr int THR = 256;
constexpr int BK = 64;   // reduction elements per K-step

struct Geom {
  int N, H, W, C, OH, OW, K, R, S, stride, pad;
  long long M;  // N*OH*OW
  int accumulate = 0;  // conv_fwd: y += conv(x, w) (a residual gradient already in y)
  long long cls_rows = 0;  // MODE_S2T: pixel tiles per output parity class
  const void* aux = nullptr;  // conv_fwd epilogue: y[n][oh][ow] += aux[n][oh/2][ow/2] at even (oh, ow)
};

// Loader modes of the implicit-GEMM kernels:
//   MODE_GEN  one filter tap x 64 input channels per K-step (C % 64 == 0);
//   MODE_STEM the 7x7 / stride-2 stem on a 4-channel (3 + one zero) NHWC image: K is
//             the flattened (r, s, c) space padded to 8 x 8 x 4 = 256 (4 K-steps), a
//             16-B chunk is two horizontally adjacent taps x 4 channels (two 8-B loads);
//             the packed filter is [K][8][8][4] with zeros in the padding;
//   MODE_S2T  the data gradient of a 3x3 / stride-2 / pad-1 conv (a transposed conv):
//             dx is split by output parity (py, px) into four stride-1 sub-convolutions
//             of dy with 1, 2, 2 and 4 of the taps -- no zero-inserted dy, no wasted MFMA
//             -- each written with stride 2 into dx; filter = the flipped transpose.
constexpr int MODE_GEN = 0, MODE_STEM = 1, MODE_S2T = 2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

// XCD-aware tile order: the hardware deals workgroup i to XCD i % 8; remap so that
// consecutive logical tiles -- the channel tiles of one pixel tile, which read the same
// activation rows -- run on one XCD and share its L2 (bijective for any grid)
__device__ __forceinline__ unsigned xcd_tile() {
  const unsigned nwg = gridDim.x, hw = blockIdx.x;
  const unsigned q8 = nwg / 8, r8 = nwg % 8, xcd = hw % 8, slot = hw / 8;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

// one global_load_lds_dwordx4: 16 B per lane from `src` (per lane) to dst + 16 * lane (dst
// wave-uniform).  A non-template device function: called directly inside the kernel
// template, hipcc's host pass fails to instantiate it and emits no launch stub (undefined
// __device_stub__ at load time).
typedef __attribute__((address_space(3))) void* lds_vptr;
__device__ __forceinline__ void glds16(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds(src, (lds_vptr)dst, 16, 0, 0);
}

// 16 zero bytes: the LDS-DMA source of padding taps and out-of-range rows (a DMA cannot
// zero-fill; its per-lane source address can point here instead).  One per translation unit.
static __device__ __attribute__((aligned(16))) unsigned char g_zero16[16] = {0};

// A run-time setting: read once from its environment variable (unset: `def`), changed by
// its *_config binding.  `norm(v, keep)` is the one validation step of both: the value to
// hold for a requested v, `keep` when v is not acceptable (the environment keeps the
// default, set() leaves the setting alone -- the bindings' "negative = leave alone").
// flag: an on / off setting, off when the variable starts with '0'.
struct Knob {
  const char* env;
  long long def;
  long long (*norm)(long long v, long long keep);
  bool flag = false;
  bool read = false;
  long long v = 0;
  long long get() {
    if (!read) {
      const char* e = std::getenv(env);
      v = e == nullptr ? def : norm(flag ? (long long)(e[0] != '0') : std::atoll(e), def);
      read = true;
    }
    return v;
  }
  long long set(long long nv) {  // -> the previous value
    const long long prev = get();
    v = norm(nv, prev);
    return prev;
  }
};
inline long long knob_nonneg(long long v, long long keep) { return v >= 0 ? v : keep; }
inline long long knob_onoff(long long v, long long keep) { return v >= 0 ? (v ? 1 : 0) : keep; }
inline long long knob_any(long long v, long long) { return v; }

// Table-driven launches: Var<...> names one instantiated kernel variant by its integer
// template arguments; for_variant() hands each variant of a list to `f` until one returns
// true (f compares the variant with the configuration picked at run time and launches it).
template <int... I>
struct Var {
  static constexpr int n = sizeof...(I);
  static constexpr int v[n] = {I...};
  static bool is(std::initializer_list<int> c) { return c.size() == (size_t)n && std::equal(c.begin(), c.end(), v); }
};
template <typename... V, typename F>
bool for_variant(std::tuple<V...>, F&& f) {
  return (f(V{}) || ...);
}

// Which variants the last conv_fwd / conv_wgrad call launched (host bookkeeping only, read by
// the last_launch() binding: the tests assert the variant a case was designed to reach).
// A call launches at most a conv kernel and a statistics-tree kernel.  Forward and backward
// calls come from different threads (autograd's device thread): one lock around the record.
struct LaunchRec {
  const char* family;
  const char* dtype;
  int n;
  int v[8];
};
struct LaunchLog {
  std::mutex mu;
  int n = 0;
  LaunchRec rec[2];
  void clear() {
    std::lock_guard<std::mutex> lk(mu);
    n = 0;
  }
};
LaunchLog& launch_log();  // conv_igemm.hip
template <typename V>
inline void note_launch(const char* family, const char* dtype) {
  static_assert(V::n <= 8, "LaunchRec holds 8 template arguments");
  LaunchLog& L = launch_log();
  std::lock_guard<std::mutex> lk(L.mu);
  if (L.n >= 2) return;
  LaunchRec& r = L.rec[L.n++];
  r.family = family;
  r.dtype = dtype;
  r.n = V::n;
  std::copy(V::v, V::v + V::n, r.v);
}
// the template arguments of every variant of a list, generated from the tuple itself
template <typename... V>
std::vector<std::vector<int64_t>> variant_list(std::tuple<V...>) {
  return {std::vector<int64_t>(V::v, V::v + V::n)...};
}
inline const char* dtype_name(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16 ? "bf16" : "f16"; }

inline Geom geom(const at::Tensor& x, const at::Tensor& w, int stride, int pad) {
  // x: [N, C, H, W] channels_last; w: [K, C, R, S] channels_last (= [K][R][S][C] in memory)
  Geom g;
  g.N = (int)x.size(0); g.C = (int)x.size(1); g.H = (int)x.size(2); g.W = (int)x.size(3);
  g.K = (int)w.size(0); g.R = (int)w.size(2); g.S = (int)w.size(3);
  g.stride = stride; g.pad = pad;
  g.OH = (g.H + 2 * pad - g.R) / stride + 1;
  g.OW = (g.W + 2 * pad - g.S) / stride + 1;
  g.M = (long long)g.N * g.OH * g.OW;
  return g;
}

inline bool supported(int64_t C, int64_t K) { return C % BK == 0 && K % 64 == 0; }

// conv_wgrad.hip (bound in register_conv_igemm)
int64_t wgrad_config(int64_t glds);
int64_t wgrad_waves_config(int64_t w);
int64_t wgrad_fixup_config(int64_t maxsp);
int64_t wgrad_splits(int64_t M, int64_t K, int64_t C, int64_t R, int64_t S);
std::vector<std::vector<int64_t>> wgrad_variants(bool glds);  // WgradVariants / WgradGldsVariants
std::vector<int64_t> conv_wgrad(at::Tensor dy, at::Tensor x, at::Tensor grad, int64_t stride, int64_t pad,
                                at::Tensor slab, int64_t mode, bool reduce);
void wgrad_reduce_batch(std::vector<at::Tensor> slabs, std::vector<at::Tensor> grads,
                        std::vector<std::vector<int64_t>> geos);

}  // namespace igemm
}  // namespace dpa
