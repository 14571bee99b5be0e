// Depthwise 5x5 convolution (padding 2, stride 1 or 2, K == C == groups, channel multiplier 1,
// C any multiple of 8) of NHWC bf16 / fp16 activations with the fp32 master weight [C][1][5][5]:
// forward, data gradient and weight gradient.  MnasNet's 5x5 depthwise convs
// (models/mnasnet.py, ops/conv_dw.py); the 3x3 family is conv_dw.hip, the shared granule
// helpers conv_dw_gran.h.
//
// Why not conv_dw.hip with other constants
//   25 multiply-adds per element moved instead of 9: by the public peak figures the vector fp32
//   rate is now within a factor of two of the bytes, so what the inner loop issues matters
//   (measured: profiles/dwconv5_bench.txt; at most 10.6 TFMA/s and 2.7 TB/s, neither peak).  And
//   a granule thread (8 channels) would keep 25 x 8 = 200 fp32 weights (or 200 weight-gradient
//   accumulators) beside its window: no room in 256 VGPRs.
//
// Weights: HALF-GRANULE threads.  A thread owns 4 channels (8 B of a pixel) of one output
//   column and walks down rows; its 25 x 4 weights are loaded once from the fp32 master, rounded
//   to the compute dtype and kept as fp32 in 100 VGPRs, as 50 channel pairs.  Chosen over
//   packed 16-bit pairs (an unpack per use inside a VALU-bound loop), over a filter-row-at-a-time
//   schedule (the input tile read five times from LDS) and over weights in LDS (50 extra 16-B
//   reads per 200 FMAs: not built, not measured).  The same split gives the weight gradient
//   100 accumulators per thread, which fit; its 25 taps are therefore NOT split over threads: the
//   channels are.  Every instantiation takes 168..250 VGPRs and no scratch: two workgroups per
//   CU by registers (three for the stride-2 data gradient), whatever the LDS would allow
//   (profiles/dwconv5_resources.txt; the unrolled walks issue their LDS reads up front).
// Inner product: packed.  Every operand is a float2 of two adjacent channels and every
//   multiply-add is __builtin_elementwise_fma on float2, which the compiler emits as
//   v_pk_fma_f32 (counts per kernel in profiles/dwconv5_resources.txt): one rounding per
//   channel, exactly as fmaf, so the outputs do not depend on the packing.  An 8-B LDS read
//   yields two such pairs after the bf16 shift / mask (fp16: v_cvt_f32_f16).
//
// Common to the three operations (the 3x3 family's conventions)
//   * A workgroup (256 threads) owns a channel block of 64 channels = 16 half-granules; lanes
//     0..15 of every 16 read one pixel's 128 B.  The last block of a C that is no multiple of 64
//     is masked by granule (C is a multiple of 8: half-granules are live in pairs).
//   * LDS tile: the input tile with its halo of 2, pixel-major, staged once by 16-B global loads
//     (stage_tile); halo outside the image and masked granules are zeros.  Pixel stride 72 elements.
//   * A workgroup walks `per` consecutive tiles (1..16, about 1024 workgroups remain).
//
// Forward, and the stride-1 data gradient (the same kernel on dy with the flipped filter):
// fwd_kernel<T, S, DGRAD>
//   work split   stride 1: output tile 8 rows x 16 columns; thread = half-granule x column,
//                walking all 8 rows.  stride 2: 8 rows x 8 columns; 2 row groups of 4 rows.
//   LDS          ((TH-1)S+5) x ((TW-1)S+5) pixels x 144 B: 12 x 20 = 34,560 B at stride 1,
//                19 x 19 = 51,984 B at stride 2 (four / three workgroups per CU by LDS; two by VGPRs).
//   registers    an input row is read once (five 8-B reads: the five filter columns) and feeds
//                the accumulators of every output row it touches (at most 5 live at stride 1, 3
//                at stride 2).  8-B LDS reads per output half-granule: 12 * 5 / 8 = 7.5 at
//                stride 1, 11 * 5 / 4 = 13.75 at stride 2, for 50 packed FMAs.
//
// Stride-2 data gradient: dgrad2_kernel<T>, the output-parity decomposition.
//   dx[ih][iw] = sum over (r, s) with ih + 2 - r and iw + 2 - s even of
//                dy[(ih + 2 - r) / 2][(iw + 2 - s) / 2] * w[r][s]: even rows take r = 0, 2, 4, odd
//                rows r = 1, 3, the same for columns: 9, 6, 6 or 4 taps, none on an inserted zero.
//   work split   dx tile 16 x 16; wave v owns the 8 columns of parity v & 1 and the 8 rows of
//                half v >> 1; a lane is half-granule x one of 4 column slots and walks its 8 rows
//                for two columns in turn.  The column parity is uniform per wave; the row walk
//                keeps a rolling window of three dy rows: the even dx row 2k takes r = 4, 2, 0 of
//                dy rows k - 1, k, k + 1, the odd row 2k + 1 takes r = 3, 1 of rows k, k + 1.
//   LDS          the 10 x 10 dy pixels the tile reads: 14,400 B.
//
// Weight gradient: wgrad_kernel<T, S> + reduce_kernel
//   work split   as the forward (same tiles, thread = half-granule x column x row group); a
//                workgroup owns one channel block and a contiguous range of output tiles (the
//                pixel split); every thread keeps 25 x 4 fp32 accumulators across them.
//   LDS          the x tile (as the forward) + the dy tile: 34,560 + 18,432 = 52,992 B at
//                stride 1, 51,984 + 9,216 = 61,200 B at stride 2: two workgroups per CU either way.
//   reduction    the 16 threads of a half-granule, in a fixed order: lanes l ^ 16, ^ 32
//                (permlane swaps, common.h) inside the wave, then waves 0..3 in index order
//                through LDS.  The workgroup writes its fp32 [channels][25] slice of slab[split];
//                reduce_kernel sums the splits in index order straight into the fp32
//                [C, 1, 5, 5] gradient: no atomics, the same bits on the same inputs.
//                wgrad_splits: about 1024 workgroups, partials at most the activation bytes.
#include "conv_dw_gran.h"

#include <map>
#include <mutex>
#include <string>

namespace dpa {
namespace dwconv5 {

using dwconv::CB;
using dwconv::NG;
using dwconv::PS;
using dwconv::lds_t;
using dwconv::stage_tile;

constexpr int NH = 2 * NG;  // half-granules (4 channels, 8 B) per channel block
constexpr int KS = 5, NT = KS * KS, PAD = 2;
constexpr int DXT = 16;          // stride-2 data gradient: dx tile side
constexpr int DD = DXT / 2 + 2;  // ... and the dy pixels under it, per side

template <int S> struct Tile;  // output tile per stride (NH * TW * row groups = 256 threads)
template <> struct Tile<1> { static constexpr int TH = 8, TW = 16; };
template <> struct Tile<2> { static constexpr int TH = 8, TW = 8; };

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef f32x2 half_t[2];  // a half-granule in registers: channel pairs (0, 1) and (2, 3)

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// ---- half-granules -------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void unpack4(u32x2 v, half_t& f);
template <> __device__ __forceinline__ void unpack4<__hip_bfloat16>(u32x2 v, half_t& f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    f[i][0] = __builtin_bit_cast(float, v[i] << 16);
    f[i][1] = __builtin_bit_cast(float, v[i] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void unpack4<__half>(u32x2 v, half_t& f) {
  typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
  const f16x4 h = __builtin_bit_cast(f16x4, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i >> 1][i & 1] = (float)h[i];
}
template <typename T> __device__ __forceinline__ void ld_half(const lds_t* p, half_t& f) {
  unpack4<T>(*reinterpret_cast<const u32x2*>(p), f);
}
// four fp32 values -> one rounding each -> one 8-B store
template <typename T> __device__ __forceinline__ void st_half(T* p, const half_t& f) {
  typedef typename MM<T>::elem E;
  u16x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const E e = MM<T>::cv(f[i >> 1][i & 1]);
    v[i] = __builtin_bit_cast(unsigned short, e);
  }
  *reinterpret_cast<u16x4*>(p) = v;
}

// The half-granule's 4 x 25 fp32 weights (100 contiguous floats from channel c, 400 B: 16-B
// aligned), rounded to T, as wr[tap][pair]; FLIP: tap 24 - tap (the stride-1 data gradient).
// A masked half-granule reads nothing.
template <typename T, bool FLIP>
__device__ __forceinline__ void load_weights(half_t (&wr)[NT], const float* __restrict__ w, int c, bool live) {
  float flat[4 * NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) v = reinterpret_cast<const f32x4*>(w + (size_t)c * NT)[i];
    flat[4 * i] = v[0]; flat[4 * i + 1] = v[1]; flat[4 * i + 2] = v[2]; flat[4 * i + 3] = v[3];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int tap = 0; tap < NT; ++tap) wr[FLIP ? NT - 1 - tap : tap][j >> 1][j & 1] = MM<T>::rnd(flat[j * NT + tap]);
}

struct Dims {
  int N, H, W, OH, OW, C;      // H, W: the stride-times-larger side (x, dx); OH, OW: y, dy
  int tiles_x, tiles_y, per;   // tiles per image row / column; tiles per workgroup
};

// ---- forward / stride-1 data gradient --------------------------------------------------
template <typename T, int S, bool DGRAD>
__global__ __launch_bounds__(256) void fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                  T* __restrict__ y, Dims d) {
  constexpr int TH = Tile<S>::TH, TW = Tile<S>::TW, RPT = TH * NH * TW / 256;  // rows per thread
  constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
  __shared__ __attribute__((aligned(16))) lds_t tile[IH * IW * PS];
  const int h = threadIdx.x & (NH - 1), col = (threadIdx.x / NH) % TW, row0 = (threadIdx.x / (NH * TW)) * RPT;
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = h < 2 * ng;
  half_t wr[NT];
  load_weights<T, DGRAD>(wr, w, c0 + 4 * h, live);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int oh0 = ty * TH + row0, ow = tx * TW + col;
    __syncthreads();  // the previous tile is read
    stage_tile<T, IH, IW>(tile, x, n, d.H, d.W, d.C, c0, ng, ty * TH * S - PAD, tx * TW * S - PAD);
    __syncthreads();
    if (!live || oh0 >= d.OH || ow >= d.OW) continue;  // (the barriers are above)
    half_t acc[RPT] = {};
    T* dst = y + (((size_t)n * d.OH + oh0) * d.OW + ow) * d.C + c0 + 4 * h;
#pragma unroll
    for (int i = 0; i < (RPT - 1) * S + KS; ++i) {  // the thread's input rows, top to bottom
      half_t in[KS];
      const lds_t* p = tile + ((row0 * S + i) * IW + col * S) * PS + 4 * h;
#pragma unroll
      for (int s = 0; s < KS; ++s) ld_half<T>(p + s * PS, in[s]);
#pragma unroll
      for (int r = 0; r < KS; ++r) {
        if (i - r < 0 || (i - r) % S != 0 || (i - r) / S >= RPT) continue;
        const int j = (i - r) / S;  // the output row this input row is filter row r of
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int k = 0; k < 2; ++k) acc[j][k] = fma2(in[s][k], wr[r * KS + s][k], acc[j][k]);
      }
      if (i >= KS - 1 && (i - (KS - 1)) % S == 0) {  // output row j is complete
        const int j = (i - (KS - 1)) / S;
        if (oh0 + j < d.OH) st_half<T>(dst + (size_t)j * d.OW * d.C, acc[j]);
      }
    }
  }
}

// ---- stride-2 data gradient --------------------------------------------------------------
// One lane's walk down 8 dx rows of column parity B at column slot j.  Filter column s = B + 2t
// (t = 0 .. NS-1) reads dy tile column j + 2 - t; dy tile row k + u (u = 0, 1, 2) is filter row
// 4 - 2u of the even dx row 2k and filter row 5 - 2u (u = 1, 2) of the odd row 2k + 1.
template <typename T, int B>
__device__ __forceinline__ void dgrad2_walk(const lds_t* tile, const half_t (&wr)[NT], T* dst, const Dims& d, int ih,
                                            int k0, int j) {
  constexpr int NS = B ? 2 : 3;
  half_t win[3][NS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < NS; ++t) ld_half<T>(tile + ((k0 + u) * DD + j + 2 - t) * PS, win[u][t]);
#pragma unroll
  for (int kk = 0; kk < DXT / 4; ++kk) {
#pragma unroll
    for (int t = 0; t < NS; ++t) ld_half<T>(tile + ((k0 + kk + 2) * DD + j + 2 - t) * PS, win[2][t]);
    half_t ev = {}, od = {};
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int t = 0; t < NS; ++t)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          ev[k] = fma2(win[u][t][k], wr[(4 - 2 * u) * KS + B + 2 * t][k], ev[k]);
          if (u > 0) od[k] = fma2(win[u][t][k], wr[(5 - 2 * u) * KS + B + 2 * t][k], od[k]);
        }
    if (ih + 2 * kk < d.H) st_half<T>(dst + (size_t)(2 * kk) * d.W * d.C, ev);
    if (ih + 2 * kk + 1 < d.H) st_half<T>(dst + (size_t)(2 * kk + 1) * d.W * d.C, od);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < NS; ++t)
#pragma unroll
        for (int k = 0; k < 2; ++k) win[u][t][k] = win[u + 1][t][k];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dgrad2_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                     T* __restrict__ dx, Dims d) {
  __shared__ __attribute__((aligned(16))) lds_t tile[DD * DD * PS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane & (NH - 1), q = lane / NH;
  const int b = wv & 1, k0 = (wv >> 1) * (DXT / 4);  // column parity; first dy step of the wave's 8 dx rows
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = h < 2 * ng;
  half_t wr[NT];
  load_weights<T, false>(wr, w, c0 + 4 * h, live);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int ih = ty * DXT + 2 * k0;
    __syncthreads();
    stage_tile<T, DD, DD>(tile, dy, n, d.OH, d.OW, d.C, c0, ng, ty * (DXT / 2) - 1, tx * (DXT / 2) - 1);
    __syncthreads();
    if (!live || ih >= d.H) continue;
    for (int j = q; j < DXT / 2; j += 64 / NH) {  // the lane's two columns of its wave's parity
      const int iw = tx * DXT + 2 * j + b;
      if (iw >= d.W) break;
      T* dst = dx + (((size_t)n * d.H + ih) * d.W + iw) * d.C + c0 + 4 * h;
      if (b) dgrad2_walk<T, 1>(tile + 4 * h, wr, dst, d, ih, k0, j);  // (uniform per wave)
      else dgrad2_walk<T, 0>(tile + 4 * h, wr, dst, d, ih, k0, j);
    }
  }
}

// ---- weight gradient -----------------------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(256) void wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                    float* __restrict__ slab, Dims d) {
  constexpr int TH = Tile<S>::TH, TW = Tile<S>::TW, RPT = TH * NH * TW / 256;
  constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
  static_assert(IH * IW * PS * sizeof(lds_t) >= 4 * NH * 4 * NT * sizeof(float), "the wave partials reuse the x tile");
  __shared__ __attribute__((aligned(16))) lds_t xt[IH * IW * PS];
  __shared__ __attribute__((aligned(16))) lds_t dt[TH * TW * PS];
  const int h = threadIdx.x & (NH - 1), col = (threadIdx.x / NH) % TW, row0 = (threadIdx.x / (NH * TW)) * RPT;
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = h < 2 * ng;
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  half_t acc[NT] = {};
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    __syncthreads();
    stage_tile<T, IH, IW>(xt, x, n, d.H, d.W, d.C, c0, ng, ty * TH * S - PAD, tx * TW * S - PAD);
    stage_tile<T, TH, TW>(dt, dy, n, d.OH, d.OW, d.C, c0, ng, ty * TH, tx * TW);
    __syncthreads();
    if (!live || ty * TH + row0 >= d.OH || tx * TW + col >= d.OW) continue;  // (only zeros of dy there)
    half_t dv[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) ld_half<T>(dt + ((row0 + j) * TW + col) * PS + 4 * h, dv[j]);
#pragma unroll
    for (int i = 0; i < (RPT - 1) * S + KS; ++i) {
      half_t in[KS];
      const lds_t* p = xt + ((row0 * S + i) * IW + col * S) * PS + 4 * h;
#pragma unroll
      for (int s = 0; s < KS; ++s) ld_half<T>(p + s * PS, in[s]);
#pragma unroll
      for (int r = 0; r < KS; ++r) {
        if (i - r < 0 || (i - r) % S != 0 || (i - r) / S >= RPT) continue;
        const int j = (i - r) / S;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int k = 0; k < 2; ++k) acc[r * KS + s][k] = fma2(dv[j][k], in[s][k], acc[r * KS + s][k]);
      }
    }
  }
  // the 16 threads of a half-granule, in a fixed order: lanes ^ 16, ^ 32, then waves 0..3
  __syncthreads();  // every lane is here (the lane swaps read them all), the x tile is read
  float* red = reinterpret_cast<float*>(xt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int tap = 0; tap < NT; ++tap)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = xor32_sum(xor16_sum(acc[tap][c >> 1][c & 1]));
      if (lane < NH) red[(wv * NH + lane) * 4 * NT + c * NT + tap] = v;
    }
  __syncthreads();
  constexpr int WS = NH * 4 * NT;  // floats per wave
  float* out = slab + ((size_t)blockIdx.x * d.C + c0) * NT;  // [channel][tap] of this split
  for (int i = threadIdx.x; i < ng * 8 * NT; i += 256)
    out[i] = ((red[i] + red[WS + i]) + red[2 * WS + i]) + red[3 * WS + i];
}

// grad[i] = slab[0][i] + slab[1][i] + ... in that order
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ slab, float* __restrict__ grad, int n,
                                                     int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = slab[i];
  for (int sp = 1; sp < splits; ++sp) a += slab[(size_t)sp * n + i];
  grad[i] = a;
}

// ---- host ----------------------------------------------------------------------------------
static bool supported(int64_t C, int64_t K, int64_t groups) { return C == K && groups == C && C >= 8 && C % 8 == 0; }

// Which kernels ran since clear_launches(): family -> (stride, C), dtype, calls.  Host
// bookkeeping only; forward and backward come from different threads (autograd's).
struct Rec {
  int stride = 0, C = 0;
  const char* dtype = "";
  int calls = 0;
};
static std::mutex g_mu;
static std::map<std::string, Rec> g_log;
static void note(const char* family, int stride, int C, const at::Tensor& t) {
  std::lock_guard<std::mutex> lk(g_mu);
  Rec& r = g_log[family];
  r.stride = stride;
  r.C = C;
  r.dtype = t.scalar_type() == at::kBFloat16 ? "bf16" : "f16";
  ++r.calls;
}
static std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> last_launch() {
  std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> out;
  std::lock_guard<std::mutex> lk(g_mu);
  for (const auto& kv : g_log)
    out[kv.first] = std::make_tuple(std::vector<int64_t>{kv.second.stride, kv.second.C},
                                    std::string(kv.second.dtype), (int64_t)kv.second.calls);
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
// big: [N, C, H, W] (x / dx), small: [N, C, OH, OW] (y / dy), w: fp32 [C, 1, 5, 5]
static Dims dims(const at::Tensor& big, const at::Tensor& small, const at::Tensor& w, int64_t stride) {
  check_act(big, "x");
  check_act(small, "y");
  TORCH_CHECK(big.scalar_type() == small.scalar_type(), "conv_dw5: one activation dtype");
  TORCH_CHECK(big.device() == small.device() && big.device() == w.device(), "conv_dw5: one device");
  TORCH_CHECK(stride == 1 || stride == 2, "conv_dw5: stride 1 or 2");
  const int64_t C = big.size(1);
  TORCH_CHECK(w.dim() == 4 && supported(C, w.size(0), C), "conv_dw5: unsupported C / K ", C, " / ", w.size(0));
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous() && w.size(1) == 1 &&
                  w.size(2) == KS && w.size(3) == KS && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "conv_dw5: fp32 contiguous 16-byte aligned weight [C, 1, 5, 5]");
  Dims d;
  d.N = (int)big.size(0); d.C = (int)C; d.H = (int)big.size(2); d.W = (int)big.size(3);
  d.OH = (d.H - 1) / (int)stride + 1; d.OW = (d.W - 1) / (int)stride + 1;
  TORCH_CHECK(d.N >= 1 && d.H >= 1 && d.W >= 1, "conv_dw5: empty input");
  TORCH_CHECK(small.size(0) == d.N && small.size(1) == C && small.size(2) == d.OH && small.size(3) == d.OW,
              "conv_dw5: output shape");
  TORCH_CHECK(big.numel() < (1ll << 31), "conv_dw5: activation of 2^31 elements or more");
  return d;
}
static int64_t blocks_of(int64_t C) { return (C + CB - 1) / CB; }
// tiles of th x tw over an oh x ow image; `per` tiles per workgroup so that about 1024
// workgroups remain (at most 16 tiles share one load of the weights)
static dim3 tile_grid(Dims& d, int oh, int ow, int th, int tw) {
  d.tiles_y = (oh + th - 1) / th;
  d.tiles_x = (ow + tw - 1) / tw;
  const long long total = (long long)d.N * d.tiles_y * d.tiles_x, blocks = blocks_of(d.C);
  d.per = (int)std::min<long long>(16, std::max<long long>(1, total * blocks / 1024));
  return dim3((unsigned)((total + d.per - 1) / d.per), (unsigned)blocks);
}

template <typename T>
static void launch_fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y, int stride, bool dgrad, dim3 grid,
                       const Dims& d) {
  auto k = dgrad ? fwd_kernel<T, 1, true> : stride == 1 ? fwd_kernel<T, 1, false> : fwd_kernel<T, 2, false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, cur_stream(), dptr<const T>(x), dptr<const float>(w), dptr<T>(y), d);
}

static void fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y, int64_t stride) {
  Dims d = dims(x, y, w, stride);
  const dim3 grid = stride == 1 ? tile_grid(d, d.OH, d.OW, Tile<1>::TH, Tile<1>::TW)
                                : tile_grid(d, d.OH, d.OW, Tile<2>::TH, Tile<2>::TW);
  note("fwd5", (int)stride, d.C, x);
  DWCONV_DISPATCH(x, launch_fwd<T>(x, w, y, (int)stride, false, grid, d));
  DPA_CHECK_LAUNCH();
}

static void dgrad(const at::Tensor& dy, const at::Tensor& w, at::Tensor& dx, int64_t stride) {
  Dims d = dims(dx, dy, w, stride);
  note("dgrad5", (int)stride, d.C, dy);
  if (stride == 1) {
    const dim3 grid = tile_grid(d, d.H, d.W, Tile<1>::TH, Tile<1>::TW);
    DWCONV_DISPATCH(dy, launch_fwd<T>(dy, w, dx, 1, true, grid, d));
  } else {
    const dim3 grid = tile_grid(d, d.H, d.W, DXT, DXT);
    DWCONV_DISPATCH(dy, hipLaunchKernelGGL((dgrad2_kernel<T>), grid, dim3(256), 0, cur_stream(), dptr<const T>(dy),
                                           dptr<const float>(w), dptr<T>(dx), d));
  }
  DPA_CHECK_LAUNCH();
}

// Pixel splits of the weight gradient of an [N, C, OH, OW] output gradient: about 1024
// workgroups, every split at least one output tile, and the partials (written and read back)
// at most about the activation bytes the kernel reads.
static int64_t wgrad_splits(int64_t N, int64_t OH, int64_t OW, int64_t C, int64_t stride) {
  const int64_t th = stride == 1 ? Tile<1>::TH : Tile<2>::TH, tw = stride == 1 ? Tile<1>::TW : Tile<2>::TW;
  const int64_t total = N * ((OH + th - 1) / th) * ((OW + tw - 1) / tw), blocks = blocks_of(C);
  const int64_t act = N * OH * OW * 2 * CB * (1 + stride * stride), part = 2 * 4 * CB * NT;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>({total, 1024 / blocks + 1, act / part}));
  const int64_t per = (total + want - 1) / want;
  return (total + per - 1) / per;
}

static void wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& grad, int64_t stride, at::Tensor& slab) {
  Dims d = dims(x, dy, grad, stride);
  const int th = stride == 1 ? Tile<1>::TH : Tile<2>::TH, tw = stride == 1 ? Tile<1>::TW : Tile<2>::TW;
  d.tiles_y = (d.OH + th - 1) / th;
  d.tiles_x = (d.OW + tw - 1) / tw;
  const int64_t total = (int64_t)d.N * d.tiles_y * d.tiles_x;
  const int64_t splits = wgrad_splits(d.N, d.OH, d.OW, d.C, stride), n = grad.numel();
  d.per = (int)((total + splits - 1) / splits);
  TORCH_CHECK(slab.is_cuda() && slab.device() == x.device() && slab.scalar_type() == at::kFloat &&
                  slab.is_contiguous() && slab.numel() >= splits * n,
              "conv_dw5: wgrad workspace of ", splits * n, " floats");
  note("wgrad5", (int)stride, d.C, dy);
  const dim3 grid((unsigned)splits, (unsigned)blocks_of(d.C));
  DWCONV_DISPATCH(dy, hipLaunchKernelGGL((stride == 1 ? wgrad_kernel<T, 1> : wgrad_kernel<T, 2>), grid, dim3(256), 0,
                                         cur_stream(), dptr<const T>(dy), dptr<const T>(x), dptr<float>(slab), d));
  DPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cur_stream(),
                     dptr<const float>(slab), dptr<float>(grad), (int)n, (int)splits);
  DPA_CHECK_LAUNCH();
}

static std::pair<int, int> tile(int64_t stride) {
  return stride == 1 ? std::make_pair(Tile<1>::TH, Tile<1>::TW) : std::make_pair(Tile<2>::TH, Tile<2>::TW);
}

}  // namespace dwconv5

void register_conv_dw5(pybind11::module& m) {
  auto s = m.def_submodule("conv_dw5", "depthwise 5x5 NHWC convolution (VALU, packed fp32, one 8-B half-granule per thread)");
  s.def("supported", &dwconv5::supported);
  s.def("fwd", &dwconv5::fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"), pybind11::arg("stride"));
  s.def("dgrad", &dwconv5::dgrad, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("dx"),
        pybind11::arg("stride"));
  s.def("wgrad", &dwconv5::wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("grad"),
        pybind11::arg("stride"), pybind11::arg("slab"));
  s.def("wgrad_splits", &dwconv5::wgrad_splits);
  s.def("tile", &dwconv5::tile, "(rows, columns) of the output tile at a stride");
  s.def("last_launch", &dwconv5::last_launch);
  s.def("clear_launches", &dwconv5::clear_launches);
}

}  // namespace dpa
