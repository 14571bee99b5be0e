// Pointwise (1x1, stride 1, bias-free) convolution of NHWC bf16 / fp16 activations with the
// fp32 master weight [K][C][1][1] read and rounded in-kernel: forward, data gradient and
// weight gradient on MFMA with fp32 accumulation, for C and K multiples of 8 in 8..1024 and
// any P = N*H*W >= 1.  The shapes the implicit-GEMM kernel refuses (C or K no multiple of 64):
// the narrow MobileNet widths (ops/conv_pw.py, models/resnet.py::_conv).
//
// Forward and data gradient: pw_kernel<T, TRANS, MULTI>
//   Both are out[P][Nc] = A[P][Kc] * B: forward A = x rows, B[k][n] = W[n][k] (Kc = C,
//   Nc = K); data gradient A = dy rows, B[k][n] = W[k][n] (Kc = K, Nc = C, TRANS).  The
//   transpose happens while the fp32 weight is staged into LDS, not in a launch of its own.
//   instruction  v_mfma_f32_16x16x32_{bf16,f16} (common.h MM<T>) with the weights on the A
//                side and the pixels on the B side: lane l supplies the 8 K-consecutive
//                elements 8 * (l / 16) .. + 7 of pixel l % 16, which is one 16-B channel
//                granule of one NHWC row, loaded from global memory straight into the operand
//                registers.  Activations never touch LDS and the tile loop has no barrier
//                (single-chunk regime).  A lane's four results are four consecutive channels
//                of one pixel: one 8-B store.
//   work split   256 threads; a pixel tile is TP = 128 rows: wave v owns rows 32v .. 32v+31
//                as two MFMA pixel tiles, so one LDS read of a weight fragment feeds two
//                instructions.  A workgroup owns `nb` output channels (grid.y blocks) and
//                walks `per` consecutive pixel tiles (1..16, about 1024 workgroups remain).
//   LDS          only the converted weight block: nb rows of kcp + 8 elements (kcp = the
//                staged depth rounded up to 32; the 8 make the row stride 4 or 20 dwords mod
//                32, so the 16-B reads of 16 consecutive rows fall in different banks).  At
//                most SLAB = 30,720 elements = 61,440 B (dynamic, sized per launch: a narrow
//                conv takes a few KB and the occupancy is the registers'; the largest leaves
//                room for two workgroups per CU, as conv_group.hip's 63,312 B).
//   regimes      Kc <= KCH = 256 (MULTI = false): the whole depth is staged ONCE per workgroup,
//                nb = min(Nc, what fits: 30,720 / (kcp + 8) rows, in 16s), and a tile's
//                activation fragments (at most 8 K-steps x 2 pixel tiles = 64 registers) stay
//                in registers while the wave loops over all nb channels: each activation
//                row is read once per channel block.  One block (rows read exactly once)
//                while Nc <= 768 at Kc <= 32, 416 at 64, 288 at 96, 224 at 128, 112 at 256.
//                Kc > 256 (MULTI = true): nb = 64, the depth is walked in 256-deep chunks
//                and the chunk's weights are restaged per tile (two barriers per chunk) with the
//                64 x 2 accumulators (32 registers) kept across chunks; the activation rows
//                are re-read once per 64-channel block.  These are the rare wide shapes
//                (e.g. 264 .. 1016 channels next to a count that is no multiple of 64).
//                The restaging reads as many L2 bytes per tile as the tile's activations at
//                Kc = 1024, so `per` amortises nothing in this regime; keeping the
//                accumulators across tiles instead was not built.  Measured at one shape
//                only (520 -> 264, 14 x 14, batch 128: forward 0.75x of torch.mm, the conv a
//                tie); 256 -> 120 (single-stage, two channel blocks) loses as a conv and is
//                routed back (profiles/pwconv_bench.txt).  Nothing else above 192 channels
//                was timed: the wide end is correct (tests) but not tuned.
//   tails        a 32-deep K-step beyond Kc (Kc % 32 = 8, 16, 24): the activation granule is
//                not loaded (zero fragment) and the weight tile is zero-filled; a 16-channel
//                tile beyond Nc (Nc % 16 = 8) is masked at the store; pixel rows >= P are
//                clamped on load and masked on store.
//   not done     no prefetch of the next tile's fragments (it would double the 64 fragment
//                registers), no BN statistics in the epilogue, no GradTap / BNTap hand-off.
//
// Weight gradient: wgrad_kernel<T> + reduce_kernel.  dW[K][C] = sum_p dy[p][K] * x[p][C].
//   work split   256 threads; a workgroup owns one 64 x 64 (K block, C block) of the output
//                and a contiguous pixel range (the split) that it walks in chunks of
//                WP = 128 pixels; wave v owns K rows 16v .. 16v+15 x all 64 C columns: four
//                accumulators (16 registers) kept across the range.
//   LDS          the chunk of dy and of x, pixel-major, 128 pixels x 80 elements (64 + 16
//                pad: 40 dwords, so the four pixel rows of a transposed read start 8 banks
//                apart) each: 40,960 B.  Channel granules beyond K / C and pixels beyond
//                the range are written as zeros, never read from memory.
//   MFMA         per 32 pixels one dy fragment and four x fragments, both read transposed with
//                ds_read_b64_tr_b16 (the fragment layout of conv_wgrad.hip / conv_group.hip).
//   partials     one fp32 [K][C] block per split in slab[split]; reduce_kernel<G> sums the
//                splits in a fixed order (G lanes per element, each in index order over its
//                stride-G splits, then a fixed lane tree) straight into the fp32 OIHW
//                gradient: no atomics, no cast pass, the same bits from the same inputs.
//                wgrad_splits keeps about 1024 workgroups and caps the partials (written and
//                read back) at the activation bytes, the rule of conv_group.hip.
//   not built    a register-prefetched or double-buffered chunk, and 32- or 96-wide blocks: the
//                weight gradient alone loses to the split-K library GEMM at 8 -> 16 (mostly
//                zero tiles) and 96 -> 96 (one and a half blocks, dy staged twice), where
//                the conv as a whole still wins (profiles/pwconv_bench.txt).
#include "common.h"

#include <map>
#include <mutex>
#include <string>

namespace dpa {
namespace pwconv {

constexpr int TP = 128;       // pixel rows per tile (4 waves x 2 MFMA pixel tiles)
constexpr int KCH = 256;      // staged depth per chunk
constexpr int NKS = KCH / 32; // K-steps per chunk
constexpr int SLAB = 30720;   // weight slab, elements
constexpr int NBM = 64;       // channel block of the chunked regime and of the weight gradient
constexpr int WP = 128;       // weight gradient: pixels per chunk
constexpr int WS = 80;        // weight gradient: LDS pixel stride, elements

typedef unsigned short lds_t;
typedef __attribute__((ext_vector_type(4))) short v4s;
typedef __attribute__((ext_vector_type(8))) short v8s;

struct Dims {
  int P, Kc, Nc;      // pixel rows, reduction depth, output channels of the GEMM
  int nb, stride;     // channels per workgroup (a multiple of 16), slab row stride (elements)
  int tiles, per;     // pixel tiles (fwd / dgrad) or pixel chunks (wgrad); per workgroup
};

template <typename T>
__device__ __forceinline__ unsigned short bits(float v) {
  return __builtin_bit_cast(unsigned short, MM<T>::cv(v));
}

// nb rows x kcp columns of the slab from depth k0: slab[n][k] = B[k0 + k][n0 + n], zeros beyond
// Kc and Nc.  Forward B[k][n] = w[n * Kc + k]; TRANS B[k][n] = w[k * Nc + n].  float4 reads
// along the weight's contiguous side (Kc, Nc multiples of 8: a float4 is all in or all out).
template <typename T, bool TRANS>
__device__ __forceinline__ void stage_weights(lds_t* slab, const float* __restrict__ w, const Dims& d, int n0, int k0,
                                              int kcp) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if constexpr (!TRANS) {
    const int kq = kcp >> 2;
    for (int i = threadIdx.x; i < d.nb * kq; i += 256) {
      const int n = i / kq, k = 4 * (i - n * kq);
      f32x4 v = z;
      if (n0 + n < d.Nc && k0 + k < d.Kc) v = *reinterpret_cast<const f32x4*>(w + (size_t)(n0 + n) * d.Kc + k0 + k);
      const u16x4 o = {bits<T>(v[0]), bits<T>(v[1]), bits<T>(v[2]), bits<T>(v[3])};
      *reinterpret_cast<u16x4*>(slab + n * d.stride + k) = o;
    }
  } else {
    const int nq = d.nb >> 2;
    for (int i = threadIdx.x; i < kcp * nq; i += 256) {
      const int k = i / nq, n = 4 * (i - k * nq);
      f32x4 v = z;
      if (n0 + n < d.Nc && k0 + k < d.Kc) v = *reinterpret_cast<const f32x4*>(w + (size_t)(k0 + k) * d.Nc + n0 + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) slab[(n + j) * d.stride + k] = bits<T>(v[j]);
    }
  }
}

// four consecutive channels of one pixel
template <typename T>
__device__ __forceinline__ void store4(T* p, f32x4 a) {
  const u16x4 v = {bits<T>(a[0]), bits<T>(a[1]), bits<T>(a[2]), bits<T>(a[3])};
  *reinterpret_cast<u16x4*>(p) = v;
}

// The fragments of the wave's two pixel tiles for the K-steps of [k0, k0 + 32 * NKS): granule
// k0 + 32 * ks + 8 * q of rows r0 and r1 (already clamped to P - 1); zeros beyond Kc.
template <typename T>
__device__ __forceinline__ void load_frags(typename MM<T>::frag (&xf)[NKS][2], const T* __restrict__ a, const Dims& d,
                                           size_t r0, size_t r1, int k0, int q) {
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int kg = k0 + 32 * ks + 8 * q;
    u16x8 v0 = z, v1 = z;
    if (kg < d.Kc) {
      v0 = *reinterpret_cast<const u16x8*>(a + r0 * d.Kc + kg);
      v1 = *reinterpret_cast<const u16x8*>(a + r1 * d.Kc + kg);
    }
    xf[ks][0] = __builtin_bit_cast(typename MM<T>::frag, v0);
    xf[ks][1] = __builtin_bit_cast(typename MM<T>::frag, v1);
  }
}

// ---- forward / data gradient ----------------------------------------------------------------
template <typename T, bool TRANS, bool MULTI>
__global__ __launch_bounds__(256) void pw_kernel(const T* __restrict__ a, const float* __restrict__ w,
                                                 T* __restrict__ out, Dims d) {
  extern __shared__ __attribute__((aligned(16))) lds_t slab_[];
  const T* slab = reinterpret_cast<const T*>(slab_);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int n0 = blockIdx.y * d.nb;
  const int t1 = min(d.tiles, ((int)blockIdx.x + 1) * d.per);
  typename MM<T>::frag xf[NKS][2];
  if constexpr (!MULTI) {
    const int kcp = d.stride - 8;  // Kc rounded up to 32
    stage_weights<T, TRANS>(slab_, w, d, n0, 0, kcp);
    __syncthreads();
    for (int t = blockIdx.x * d.per; t < t1; ++t) {
      const int p0 = t * TP + 32 * wv + li, p1 = p0 + 16;
      load_frags<T>(xf, a, d, (size_t)min(p0, d.P - 1), (size_t)min(p1, d.P - 1), 0, q);
      for (int nt = 0; 16 * nt < d.nb; ++nt) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        const T* wrow = slab + (16 * nt + li) * d.stride + 8 * q;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
          if (32 * ks < kcp) {
            const auto wf = MM<T>::ld(wrow + 32 * ks);
            acc0 = MM<T>::mma(wf, xf[ks][0], acc0);
            acc1 = MM<T>::mma(wf, xf[ks][1], acc1);
          }
        const int c = n0 + 16 * nt + 4 * q;
        if (c < d.Nc) {
          if (p0 < d.P) store4<T>(out + (size_t)p0 * d.Nc + c, acc0);
          if (p1 < d.P) store4<T>(out + (size_t)p1 * d.Nc + c, acc1);
        }
      }
    }
  } else {
    for (int t = blockIdx.x * d.per; t < t1; ++t) {
      const int p0 = t * TP + 32 * wv + li, p1 = p0 + 16;
      f32x4 acc[NBM / 16][2] = {};
      for (int k0 = 0; k0 < d.Kc; k0 += KCH) {
        const int kcp = (min(KCH, d.Kc - k0) + 31) & ~31;
        load_frags<T>(xf, a, d, (size_t)min(p0, d.P - 1), (size_t)min(p1, d.P - 1), k0, q);
        __syncthreads();  // the previous chunk is read
        stage_weights<T, TRANS>(slab_, w, d, n0, k0, kcp);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
          if (32 * ks < kcp) {
#pragma unroll
            for (int nt = 0; nt < NBM / 16; ++nt) {
              const auto wf = MM<T>::ld(slab + (16 * nt + li) * d.stride + 32 * ks + 8 * q);
              acc[nt][0] = MM<T>::mma(wf, xf[ks][0], acc[nt][0]);
              acc[nt][1] = MM<T>::mma(wf, xf[ks][1], acc[nt][1]);
            }
          }
      }
#pragma unroll
      for (int nt = 0; nt < NBM / 16; ++nt) {
        const int c = n0 + 16 * nt + 4 * q;
        if (c < d.Nc) {
          if (p0 < d.P) store4<T>(out + (size_t)p0 * d.Nc + c, acc[nt][0]);
          if (p1 < d.P) store4<T>(out + (size_t)p1 * d.Nc + c, acc[nt][1]);
        }
      }
    }
  }
}

// ---- weight gradient ------------------------------------------------------------------------
// WP pixels from p0 x 64 channels from c0 of a [P][C] row matrix, zeros beyond p1 and C.
template <typename T>
__device__ __forceinline__ void stage_rows(lds_t* lds, const T* __restrict__ src, int C, int c0, int p0, int p1) {
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = threadIdx.x; i < WP * 8; i += 256) {
    const int p = i >> 3, g = i & 7;
    u16x8 v = z;
    if (p0 + p < p1 && c0 + 8 * g < C) v = *reinterpret_cast<const u16x8*>(src + (size_t)(p0 + p) * C + c0 + 8 * g);
    *reinterpret_cast<u16x8*>(lds + p * WS + 8 * g) = v;
  }
}

// A lane's 8 consecutive pixels of channel ch + (lane & 15): two transposed reads of 4 pixel
// rows x 16 channels; the lane supplies the address of pixel (lane & 15) >> 2 (and + 4),
// channels ch + 4 * (lane & 3) (conv_group.hip trfrag).
template <typename T>
__device__ __forceinline__ typename MM<T>::frag trfrag(const lds_t* first, int lane) {
  const int gi = lane & 15;
  const lds_t* a0 = first + (gi >> 2) * WS + 4 * (gi & 3);
  const lds_t* a1 = a0 + 4 * WS;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a0);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a1);
  const v8s v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename MM<T>::frag, v);
}

// d.Kc = K (dy channels), d.Nc = C (x channels); grid (splits, K blocks, C blocks)
template <typename T>
__global__ __launch_bounds__(256) void wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                    float* __restrict__ slab, Dims d) {
  __shared__ __attribute__((aligned(16))) lds_t dt[WP * WS];
  __shared__ __attribute__((aligned(16))) lds_t xt[WP * WS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane >> 4, li = lane & 15;
  const int o0 = blockIdx.y * NBM, c0 = blockIdx.z * NBM;
  const int pbeg = min(d.P, (int)blockIdx.x * d.per * WP), pend = min(d.P, pbeg + d.per * WP);
  f32x4 acc[4] = {};
  for (int p0 = pbeg; p0 < pend; p0 += WP) {
    __syncthreads();  // the previous chunk is read
    stage_rows<T>(dt, dy, d.Kc, o0, p0, pend);
    stage_rows<T>(xt, x, d.Nc, c0, p0, pend);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WP / 32; ++kk) {
      if (p0 + 32 * kk >= pend) break;
      const int pix = 32 * kk + 8 * grp;  // the lane group's 8 pixels
      const auto af = trfrag<T>(dt + pix * WS + 16 * wv, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = MM<T>::mma(af, trfrag<T>(xt + pix * WS + 16 * nt, lane), acc[nt]);
    }
  }
  // D[o][c]: row o = 4 * grp + j, column c = li
  float* dst = slab + (size_t)blockIdx.x * d.Kc * d.Nc;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int c = c0 + 16 * nt + li;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + 16 * wv + 4 * grp + j;
      if (o < d.Kc && c < d.Nc) dst[(size_t)o * d.Nc + c] = acc[nt][j];
    }
  }
}

// grad[i] = the sum of slab[sp][i] over the splits in a fixed order: lane g of an aligned group of
// G lanes sums splits g, g + G, g + 2G, ... in index order, 16 loads in flight at a time
// (common.h slab_colsum), and the G lane sums are combined by the fixed DPP tree (group_sum<G>).
// G = 1: plain index order.  A narrow conv has about 1000 splits of a few hundred elements, which
// one lane per element would walk as about 1000 dependent loads.
template <int G>
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ slab, float* __restrict__ grad, int n,
                                                     int splits) {
  const int i = (blockIdx.x * 256 + threadIdx.x) / G, g = threadIdx.x % G;
  float a = slab_colsum<G>(slab, splits, n, i, g);  // (0 for i >= n; every lane stays for the tree)
  if constexpr (G > 1) a = group_sum<G>(a);
  if (i < n && g == 0) grad[i] = a;
}

// ---- host ----------------------------------------------------------------------------------
static bool supported(int64_t C, int64_t K) {
  return C >= 8 && K >= 8 && C <= 1024 && K <= 1024 && C % 8 == 0 && K % 8 == 0;
}

// Which kernels ran since clear_launches(): family -> (C, K), dtype, calls.  Host bookkeeping
// only; forward and backward come from different threads (autograd's).
struct Rec {
  int C = 0, K = 0;
  const char* dtype = "";
  int calls = 0;
};
static std::mutex g_mu;
static std::map<std::string, Rec> g_log;
static void note(const char* family, int C, int K, const at::Tensor& t) {
  std::lock_guard<std::mutex> lk(g_mu);
  Rec& r = g_log[family];
  r.C = C;
  r.K = K;
  r.dtype = t.scalar_type() == at::kBFloat16 ? "bf16" : "f16";
  ++r.calls;
}
static std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> last_launch() {
  std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> out;
  std::lock_guard<std::mutex> lk(g_mu);
  for (const auto& kv : g_log)
    out[kv.first] = std::make_tuple(std::vector<int64_t>{kv.second.C, kv.second.K}, std::string(kv.second.dtype),
                                    (int64_t)kv.second.calls);
  return out;
}
static void clear_launches() {
  std::lock_guard<std::mutex> lk(g_mu);
  g_log.clear();
}

static void check_act(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4, name, ": a 4-d HIP tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf, name, ": bf16 or fp16");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), name, ": channels_last");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, ": 16-byte aligned");
}
// x: [N, C, H, W], y: [N, K, H, W], w: fp32 [K, C, 1, 1]; returns (P, C, K)
static std::tuple<int, int, int> shape(const at::Tensor& x, const at::Tensor& y, const at::Tensor& w) {
  check_act(x, "x");
  check_act(y, "y");
  TORCH_CHECK(x.scalar_type() == y.scalar_type(), "conv_pw: one activation dtype");
  TORCH_CHECK(x.device() == y.device() && x.device() == w.device(), "conv_pw: one device");
  const int64_t C = x.size(1), K = y.size(1);
  TORCH_CHECK(supported(C, K), "conv_pw: unsupported C / K ", C, " / ", K);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous() && w.dim() == 4 && w.size(0) == K &&
                  w.size(1) == C && w.size(2) == 1 && w.size(3) == 1 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "conv_pw: fp32 contiguous 16-byte aligned weight [K, C, 1, 1]");
  TORCH_CHECK(x.size(0) >= 1 && x.size(2) >= 1 && x.size(3) >= 1, "conv_pw: empty input");
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(2) == x.size(2) && y.size(3) == x.size(3), "conv_pw: output shape");
  TORCH_CHECK(x.numel() < (1ll << 31) && y.numel() < (1ll << 31), "conv_pw: activation of 2^31 elements or more");
  return std::make_tuple((int)(x.size(0) * x.size(2) * x.size(3)), (int)C, (int)K);
}

// bf16 / fp16 only: check_act has refused everything else
#define PWCONV_DISPATCH(t, ...)                                                \
  do {                                                                         \
    if ((t).scalar_type() == at::kBFloat16) { typedef __hip_bfloat16 T; __VA_ARGS__; } \
    else { typedef __half T; __VA_ARGS__; }                                    \
  } while (0)

template <typename T>
static void launch_gemm(const at::Tensor& a, const at::Tensor& w, at::Tensor& out, bool trans, dim3 grid,
                        const Dims& d) {
  const bool multi = d.Kc > KCH;
  auto k = trans ? (multi ? pw_kernel<T, true, true> : pw_kernel<T, true, false>)
                 : (multi ? pw_kernel<T, false, true> : pw_kernel<T, false, false>);
  const size_t lds = (size_t)d.nb * d.stride * sizeof(lds_t);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, cur_stream(), dptr<const T>(a), dptr<const float>(w), dptr<T>(out), d);
}

// out[P][Nc] = a[P][Kc] * B: the regime, the channel block, `per` tiles per workgroup so that
// about 1024 workgroups remain (at most 16 tiles share one staging of the weights)
static Dims plan(int P, int Kc, int Nc) {
  Dims d;
  d.P = P; d.Kc = Kc; d.Nc = Nc;
  if (Kc <= KCH) {
    d.stride = ceil_to(Kc, 32) + 8;
    d.nb = std::min(ceil_to(Nc, 16), SLAB / d.stride / 16 * 16);
  } else {
    d.stride = KCH + 8;
    d.nb = NBM;  // (the kernel's channel-tile loop is unrolled over all 64; rows beyond Nc are zeros)
  }
  d.tiles = (P + TP - 1) / TP;
  const long long blocks = (Nc + d.nb - 1) / d.nb;
  d.per = (int)std::min<long long>(16, std::max<long long>(1, d.tiles * blocks / 1024));
  return d;
}
static void gemm(const at::Tensor& a, const at::Tensor& w, at::Tensor& out, int P, int Kc, int Nc, bool trans) {
  const Dims d = plan(P, Kc, Nc);
  const dim3 grid((unsigned)((d.tiles + d.per - 1) / d.per), (unsigned)((Nc + d.nb - 1) / d.nb));
  PWCONV_DISPATCH(a, launch_gemm<T>(a, w, out, trans, grid, d));
  DPA_CHECK_LAUNCH();
}
// pixel tiles one workgroup of the forward (Kc = C, Nc = K) or data gradient (Kc = K, Nc = C) walks
static int64_t tiles_per_workgroup(int64_t P, int64_t Kc, int64_t Nc) {
  TORCH_CHECK(P >= 1 && P < (1ll << 31) && supported(Kc, Nc), "conv_pw: unsupported P / Kc / Nc");
  return plan((int)P, (int)Kc, (int)Nc).per;
}

// output channels one workgroup of the forward / data gradient owns (grid.y = ceil(Nc / this))
static int64_t channel_block(int64_t Kc, int64_t Nc) {
  TORCH_CHECK(supported(Kc, Nc), "conv_pw: unsupported Kc / Nc");
  return plan(1, (int)Kc, (int)Nc).nb;
}

static void fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y) {
  const auto [P, C, K] = shape(x, y, w);
  note("fwd", C, K, x);
  gemm(x, w, y, P, C, K, false);
}

static void dgrad(const at::Tensor& dy, const at::Tensor& w, at::Tensor& dx) {
  const auto [P, C, K] = shape(dx, dy, w);
  note("dgrad", C, K, dy);
  gemm(dy, w, dx, P, K, C, true);
}

// Pixel splits of the weight gradient over P pixel rows: about 1024 workgroups, every split at
// least one 128-pixel chunk, and the partials (written and read back) at most about the
// activation bytes the kernel reads.
static int64_t wgrad_splits(int64_t P, int64_t K, int64_t C) {
  const int64_t chunks = (P + WP - 1) / WP, blocks = ((K + NBM - 1) / NBM) * ((C + NBM - 1) / NBM);
  const int64_t act = P * 2 * (K + C), part = 2 * 4 * K * C;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>({chunks, 1024 / blocks + 1, act / part}));
  const int64_t per = (chunks + want - 1) / want;
  return (chunks + per - 1) / per;
}

static void wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& grad, at::Tensor& slab) {
  const auto [P, C, K] = shape(x, dy, grad);
  Dims d;
  d.P = P; d.Kc = K; d.Nc = C; d.nb = NBM; d.stride = WS;
  d.tiles = (P + WP - 1) / WP;
  const int64_t splits = wgrad_splits(P, K, C), n = grad.numel();
  d.per = (int)((d.tiles + splits - 1) / splits);
  TORCH_CHECK(slab.is_cuda() && slab.device() == x.device() && slab.scalar_type() == at::kFloat &&
                  slab.is_contiguous() && slab.numel() >= splits * n,
              "conv_pw: wgrad workspace of ", splits * n, " floats");
  note("wgrad", C, K, dy);
  const dim3 grid((unsigned)splits, (unsigned)((K + NBM - 1) / NBM), (unsigned)((C + NBM - 1) / NBM));
  PWCONV_DISPATCH(dy, hipLaunchKernelGGL((wgrad_kernel<T>), grid, dim3(256), 0, cur_stream(), dptr<const T>(dy),
                                         dptr<const T>(x), dptr<float>(slab), d));
  DPA_CHECK_LAUNCH();
  // lanes per element: at most 16 splits per lane while the launch stays above the partials' size
  const int G = splits <= 16 ? 1 : splits <= 64 ? 4 : splits <= 256 ? 16 : 64;
  auto rk = G == 1 ? reduce_kernel<1> : G == 4 ? reduce_kernel<4> : G == 16 ? reduce_kernel<16> : reduce_kernel<64>;
  hipLaunchKernelGGL(rk, dim3((unsigned)((n * G + 255) / 256)), dim3(256), 0, cur_stream(), dptr<const float>(slab),
                     dptr<float>(grad), (int)n, (int)splits);
  DPA_CHECK_LAUNCH();
}

static std::pair<int, int> tile() { return std::make_pair(TP, NBM); }

}  // namespace pwconv

void register_conv_pw(pybind11::module& m) {
  auto s = m.def_submodule("conv_pw", "pointwise 1x1 NHWC convolution on MFMA (activations global -> operand registers)");
  s.def("supported", &pwconv::supported);
  s.def("fwd", &pwconv::fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"));
  s.def("dgrad", &pwconv::dgrad, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("dx"));
  s.def("wgrad", &pwconv::wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("grad"), pybind11::arg("slab"));
  s.def("wgrad_splits", &pwconv::wgrad_splits, pybind11::arg("P"), pybind11::arg("K"), pybind11::arg("C"));
  s.def("tiles_per_workgroup", &pwconv::tiles_per_workgroup, pybind11::arg("P"), pybind11::arg("Kc"),
        pybind11::arg("Nc"));
  s.def("channel_block", &pwconv::channel_block, pybind11::arg("Kc"), pybind11::arg("Nc"));
  s.def("tile", &pwconv::tile, "(pixel rows of a tile, output-channel block of the chunked regime and the weight gradient)");
  s.def("last_launch", &pwconv::last_launch);
  s.def("clear_launches", &pwconv::clear_launches);
  s.attr("K_CHUNK") = pwconv::KCH;
}

}  // namespace dpa
