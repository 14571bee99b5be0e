// Grouped 3x3 convolution (padding 1, stride 1 or 2, C == K, Cg = C / groups in
// {4, 8, 16, 32}, C a multiple of 64) of NHWC bf16 / fp16 activations with fp32 master
// weights [K][Cg][3][3]: forward, data gradient and weight gradient on MFMA with fp32
// accumulation.  ResNeXt's 3x3 convolutions (models/resnet.py, ops/conv_group.py).
//
// Common to the three operations
//   * Channel blocks, not groups.  A workgroup owns 32 consecutive channels: because C == K
//     and Cg divides 32, outputs [32b, 32b+32) read exactly inputs [32b, 32b+32), and one
//     filter tap is a 32 x 32 product with a block-diagonal weight (8 / 4 / 2 / 1 groups,
//     exact zeros elsewhere).  A pixel's 32 channels are 64 contiguous bytes = four 16-B
//     granules, which is one v_mfma_f32_16x16x32_{bf16,f16} operand row per lane.
//   * Instruction: the 16x16x32 form (common.h MM<T>), not 32x32x16: its operand is one
//     16-B LDS read per lane straight from a pixel row, and a lane's four results are four
//     consecutive channels of one pixel (one 8-B store).  The multiply-by-zero waste is
//     32 / Cg; 16-channel blocks for Cg <= 16 (half the waste) were NOT built or measured:
//     they halve the bytes per pixel row to 32 and double the workgroups that stage the
//     same halo, and the op is bandwidth-bound (profiles/gconv_bench.txt).
//   * LDS activation tiles are pixel-major with a pixel stride of PS = 40 elements (80 B,
//     the 64 B of data + 16 B): 16 lanes reading 16 consecutive pixels (stride 1) or every
//     second pixel (stride 2) then start in different banks (20 / 40 dwords apart instead
//     of 16 / 32).  The halo outside the image is written as zeros, never read from memory.
//   * Weights: every workgroup reads its block's fp32 master slice (32 * Cg * 9 floats),
//     rounds it and scatters it into LDS as nine 32 x 32 tiles (18 KB, zeros written once).
//     No per-step pack launch and no WeightPack entry.  A workgroup walks `per` consecutive
//     tiles (1..16, chosen so that about 1024 workgroups remain) to spread that staging.
//     A pre-packed buffer was not measured.
//
// Forward, and the stride-1 data gradient (the same kernel on dy with the transposed,
// spatially flipped block): fwd_kernel<T, S, DGRAD>
//   work split   256 threads; output tile 8 rows x 16 pixels of one image x 32 channels;
//                wave v owns rows 2v, 2v+1: 2 pixel tiles x 2 channel halves.
//   LDS          weights 9 x 32 x 32 (18,432 B) + input tile with halo, (7S+3) x (15S+3)
//                pixels x 80 B: 14,400 B at stride 1, 44,880 B at stride 2 (63,312 B in
//                all: two workgroups per CU; a 4-row tile for stride 2 was not measured).
//   MFMA         A = weights [channel][32 inputs], B = pixels; 9 taps x 4 instructions per
//                wave and tile; 4 accumulators = 16 registers.  The 9 taps are shifted reads
//                of the one LDS tile.  Rows below the image are skipped per wave.
//
// Stride-2 data gradient: dgrad2_kernel<T>.  Chosen: the output-parity decomposition of
// the dense kernels (dgrad_s2), but inside one workgroup instead of four sub-launches:
// a dx tile is 8 rows x 32 columns, and an MFMA pixel tile is the 16 pixels of one row
// with one column parity, so all 16 share their valid taps (1, 2, 2 or 4 of the 9) and
// their dy reads are 16 consecutive pixels.  Rejected: the gather form over a zero-upsampled
// halo tile, which multiplies by inserted zeros for 27 of every 36 tap-pixels.
//   work split   256 threads; wave v owns dx rows 2v (even: r = 1) and 2v+1 (odd: r = 0, 2)
//                with both column parities: 9 taps per wave, the same for every wave.
//   LDS          weights 18,432 B + the 5 x 17 dy pixels the tile reads (6,800 B).
//   MFMA         9 taps x 2 channel halves per wave and tile; 8 accumulators = 32 registers.
//
// Weight gradient: wgrad_kernel<T, S, FULL> + reduce_kernel
//   work split   192 threads: wave v owns filter row r = v (3 taps), so the 9 taps x 16
//                accumulator registers are split evenly (4 waves over 9 taps are not).
//                A workgroup owns one channel block and a contiguous range of 8 x 16
//                output tiles (the pixel split) and keeps its accumulators across them.
//   LDS          x tile with halo (as the forward) + the dy tile, 128 pixels x 80 B:
//                24,640 B at stride 1, 55,120 B at stride 2.
//   MFMA         per tap a 32 x 32 product dy^T x with 32 pixels per step; both operands are
//                pixel-major in LDS and read transposed with ds_read_b64_tr_b16 (the fragment
//                layout of conv_wgrad.hip).  Cg <= 16: only the two diagonal 16 x 16 tiles
//                (FULL = false, 24 accumulator registers), Cg = 32: all four (48).
//   partials     each workgroup writes its fp32 [32][Cg][3][3] slice of slab[split]; only
//                the diagonal Cg x Cg blocks are stored.  reduce_kernel sums the splits in
//                index order straight into the fp32 OIHW gradient: no atomics, no cast pass.
//                The split count keeps about 1024 workgroups but caps the partials at
//                the activation bytes (wgrad_splits).  Capped at a quarter of them, the Cg = 32
//                shapes ran on 64 / 192 workgroups: 188.5 / 141.7 us against 53.5 / 93.1 us
//                (profiles/gconv_bench.txt).
// No identity-block GradTap / BNTap hand-off and no BN statistics in the epilogue.
#include "common.h"

#include <map>
#include <mutex>
#include <string>

namespace dpa {
namespace gconv {

constexpr int CB = 32;   // channels per workgroup
constexpr int TH = 8;    // output tile rows
constexpr int TW = 16;   // output tile pixels per row (one MFMA pixel tile)
constexpr int PS = 40;   // LDS pixel stride, elements
constexpr int WL = 9 * CB * CB;  // weight tiles, elements

typedef unsigned short lds_t;  // LDS arrays are raw 16-bit words (T has constructors)
typedef __attribute__((ext_vector_type(4))) short v4s;
typedef __attribute__((ext_vector_type(8))) short v8s;

// ---- staging ---------------------------------------------------------------------------
// The block's 32 * cg * 9 fp32 weights -> nine [32][32] tiles of T.  Forward: tile[tap][o][c];
// TRANS (data gradient): tile[tap'][c][o] with tap' = 8 - tap when FLIP (stride 1: the
// gradient as a forward conv of dy) or tap' = tap (stride 2: taps addressed directly).
template <typename T, int NT, bool TRANS, bool FLIP>
__device__ __forceinline__ void stage_weights(T* wl, const float* __restrict__ w, int c0, int cg) {
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < WL / 8; i += NT) reinterpret_cast<u16x8*>(wl)[i] = z;
  __syncthreads();
  const int per = cg * 9, total = CB * per;
  const float* src = w + (size_t)c0 * per;
  typedef typename MM<T>::elem E;
  for (int i = threadIdx.x; i < total; i += NT) {
    const int ol = i / per, rem = i - ol * per, ci = rem / 9, tap = rem - ci * 9;
    const int cl = (ol / cg) * cg + ci;
    T* dst = TRANS ? wl + ((FLIP ? 8 - tap : tap) * CB + cl) * CB + ol : wl + (tap * CB + ol) * CB + cl;
    *reinterpret_cast<E*>(dst) = MM<T>::cv(src[i]);
  }
}

// RH x RW pixels x 32 channels of image n from (h0, w0), zeros outside [0, H) x [0, W).
template <typename T, int NT, int RH, int RW>
__device__ __forceinline__ void stage_tile(T* lds, const T* __restrict__ src, int n, int H, int W, int C, int c0,
                                           int h0, int w0) {
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int i = threadIdx.x; i < RH * RW * 4; i += NT) {
    const int p = i >> 2, g = i & 3;
    const int h = h0 + p / RW, x = w0 + p % RW;
    u16x8 v = z;
    if ((unsigned)h < (unsigned)H && (unsigned)x < (unsigned)W)
      v = *reinterpret_cast<const u16x8*>(src + (((size_t)n * H + h) * W + x) * C + c0 + 8 * g);
    *reinterpret_cast<u16x8*>(lds + p * PS + 8 * g) = v;
  }
}

// four consecutive channels of one pixel
template <typename T>
__device__ __forceinline__ void store4(T* p, f32x4 a) {
  typedef typename MM<T>::elem E;
  const E e0 = MM<T>::cv(a[0]), e1 = MM<T>::cv(a[1]), e2 = MM<T>::cv(a[2]), e3 = MM<T>::cv(a[3]);
  const u16x4 v = {__builtin_bit_cast(unsigned short, e0), __builtin_bit_cast(unsigned short, e1),
                   __builtin_bit_cast(unsigned short, e2), __builtin_bit_cast(unsigned short, e3)};
  *reinterpret_cast<u16x4*>(p) = v;
}

struct Dims {
  int N, H, W, OH, OW, C, cg;  // H, W: the stride-times-larger side (x, dx); OH, OW: y, dy
  int tiles_x, tiles_y, per;   // tiles per image row / column; tiles per workgroup
};

// ---- forward / stride-1 data gradient --------------------------------------------------
template <typename T, int S, bool DGRAD>
__global__ __launch_bounds__(256) void fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                  T* __restrict__ y, Dims d) {
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  __shared__ __attribute__((aligned(16))) lds_t wl_[WL];
  __shared__ __attribute__((aligned(16))) lds_t tile_[IH * IW * PS];
  T* wl = reinterpret_cast<T*>(wl_);
  T* tile = reinterpret_cast<T*>(tile_);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * CB;
  stage_weights<T, 256, DGRAD, DGRAD>(wl, w, c0, d.cg);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int oh0 = ty * TH, ow0 = tx * TW;
    __syncthreads();  // the weights are staged / the previous tile is read
    stage_tile<T, 256, IH, IW>(tile, x, n, d.H, d.W, d.C, c0, oh0 * S - 1, ow0 * S - 1);
    __syncthreads();
    const int row = 2 * wv;
    if (oh0 + row >= d.OH) continue;  // (uniform per wave; the barriers are above)
    f32x4 acc[2][2] = {};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int r = tap / 3, s = tap % 3;
      const auto a0 = MM<T>::ld(wl + (tap * CB + li) * CB + 8 * q);
      const auto a1 = MM<T>::ld(wl + (tap * CB + 16 + li) * CB + 8 * q);
      const auto b0 = MM<T>::ld(tile + ((row * S + r) * IW + li * S + s) * PS + 8 * q);
      const auto b1 = MM<T>::ld(tile + (((row + 1) * S + r) * IW + li * S + s) * PS + 8 * q);
      acc[0][0] = MM<T>::mma(a0, b0, acc[0][0]);
      acc[1][0] = MM<T>::mma(a1, b0, acc[1][0]);
      acc[0][1] = MM<T>::mma(a0, b1, acc[0][1]);
      acc[1][1] = MM<T>::mma(a1, b1, acc[1][1]);
    }
    const int ow = ow0 + li;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int oh = oh0 + row + nt;
      if (oh < d.OH && ow < d.OW) {
        T* dst = y + (((size_t)n * d.OH + oh) * d.OW + ow) * d.C + c0 + 4 * q;
        store4<T>(dst, acc[0][nt]);
        store4<T>(dst + 16, acc[1][nt]);
      }
    }
  }
}

// ---- stride-2 data gradient --------------------------------------------------------------
// dx[ih][iw] = sum over (r, s) with ih + 1 - r and iw + 1 - s even of
//              dy[(ih + 1 - r) / 2][(iw + 1 - s) / 2] * w[r][s]
template <typename T>
__global__ __launch_bounds__(256) void dgrad2_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                     T* __restrict__ dx, Dims d) {
  constexpr int DH = TH / 2 + 1, DW = TW + 1;  // dy pixels under an 8 x 32 dx tile
  __shared__ __attribute__((aligned(16))) lds_t wl_[WL];
  __shared__ __attribute__((aligned(16))) lds_t tile_[DH * DW * PS];
  T* wl = reinterpret_cast<T*>(wl_);
  T* tile = reinterpret_cast<T*>(tile_);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, q = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * CB;
  stage_weights<T, 256, true, false>(wl, w, c0, d.cg);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int ih0 = ty * TH, iw0 = tx * 2 * TW;
    __syncthreads();
    stage_tile<T, 256, DH, DW>(tile, dy, n, d.OH, d.OW, d.C, c0, ih0 / 2, iw0 / 2);
    __syncthreads();
    if (ih0 + 2 * wv >= d.H) continue;
    f32x4 acc[2][2][2] = {};  // [channel half][row parity a][column parity b]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if ((a + 1 - r) & 1) continue;
        const int lrow = (2 * wv + a + 1 - r) / 2;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            if ((b + 1 - s) & 1) continue;
            const int tap = r * 3 + s;
            const auto a0 = MM<T>::ld(wl + (tap * CB + li) * CB + 8 * q);
            const auto a1 = MM<T>::ld(wl + (tap * CB + 16 + li) * CB + 8 * q);
            const auto bb = MM<T>::ld(tile + (lrow * DW + (b + 1 - s) / 2 + li) * PS + 8 * q);
            acc[0][a][b] = MM<T>::mma(a0, bb, acc[0][a][b]);
            acc[1][a][b] = MM<T>::mma(a1, bb, acc[1][a][b]);
          }
      }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ih = ih0 + 2 * wv + a, iw = iw0 + b + 2 * li;
        if (ih < d.H && iw < d.W) {
          T* dst = dx + (((size_t)n * d.H + ih) * d.W + iw) * d.C + c0 + 4 * q;
          store4<T>(dst, acc[0][a][b]);
          store4<T>(dst + 16, acc[1][a][b]);
        }
      }
  }
}

// ---- weight gradient -----------------------------------------------------------------------
// A lane's 8 consecutive pixels (p, p+1, .., p+7 of the lane group's run) of channel
// ch + (lane & 15): two transposed reads of 4 pixel rows x 16 channels; the lane supplies
// the address of pixel (lane & 15) >> 2 (and + 4), channels ch + 4 * (lane & 3).
// `step`: elements between consecutive pixels of the run.
template <typename T>
__device__ __forceinline__ typename MM<T>::frag trfrag(const T* first, int step, int lane) {
  const int gi = lane & 15;
  const T* a0 = first + (gi >> 2) * step + 4 * (gi & 3);
  const T* a1 = a0 + 4 * step;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a0);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a1);
  const v8s v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename MM<T>::frag, v);
}

template <typename T, int S, bool FULL>
__global__ __launch_bounds__(192) void wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                    float* __restrict__ slab, Dims d) {
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3, NN = FULL ? 2 : 1;
  __shared__ __attribute__((aligned(16))) lds_t xt_[IH * IW * PS];
  __shared__ __attribute__((aligned(16))) lds_t dt_[TH * TW * PS];
  T* xt = reinterpret_cast<T*>(xt_);
  T* dt = reinterpret_cast<T*>(dt_);
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6, grp = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * CB;
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  f32x4 acc[3][2][NN] = {};  // [s][dy half][x half (FULL) / the same half]
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int oh0 = ty * TH, ow0 = tx * TW;
    __syncthreads();
    stage_tile<T, 192, IH, IW>(xt, x, n, d.H, d.W, d.C, c0, oh0 * S - 1, ow0 * S - 1);
    stage_tile<T, 192, TH, TW>(dt, dy, n, d.OH, d.OW, d.C, c0, oh0, ow0);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TH / 2; ++kk) {  // 32 output pixels: rows 2kk, 2kk+1
      if (oh0 + 2 * kk >= d.OH) break;
      const int prow = 2 * kk + (grp >> 1), pcol = 8 * (grp & 1);  // the lane group's 8 pixels
      typename MM<T>::frag A[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) A[mt] = trfrag<T>(dt + (prow * TW + pcol) * PS + 16 * mt, PS, lane);
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const T* xp = xt + ((prow * S + r) * IW + pcol * S + s) * PS;
        if constexpr (FULL) {
          const auto b0 = trfrag<T>(xp, S * PS, lane);
          const auto b1 = trfrag<T>(xp + 16, S * PS, lane);
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            acc[s][mt][0] = MM<T>::mma(A[mt], b0, acc[s][mt][0]);
            acc[s][mt][NN - 1] = MM<T>::mma(A[mt], b1, acc[s][mt][NN - 1]);
          }
        } else {
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
            acc[s][mt][0] = MM<T>::mma(A[mt], trfrag<T>(xp + 16 * mt, S * PS, lane), acc[s][mt][0]);
        }
      }
    }
  }
  // D[o][c]: row o = 4 * grp + j, column c = li; only the diagonal Cg x Cg blocks exist
  float* out = slab + ((size_t)blockIdx.x * d.C + c0) * d.cg * 9;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nn = 0; nn < NN; ++nn) {
        const int nt = FULL ? nn : mt;
        const int cl = 16 * nt + li;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ol = 16 * mt + 4 * grp + j;
          if (ol / d.cg == cl / d.cg) out[(ol * d.cg + cl % d.cg) * 9 + r * 3 + s] = acc[s][mt][nn][j];
        }
      }
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
static bool supported(int64_t C, int64_t K, int64_t groups) {
  if (C != K || groups <= 1 || C % 64 != 0 || C % groups != 0) return false;
  const int64_t cg = C / groups;
  return cg == 4 || cg == 8 || cg == 16 || cg == 32;
}

// Which kernels ran since clear_launches(): family -> (stride, Cg), dtype, calls.  Host
// bookkeeping only; forward and backward come from different threads (autograd's).
struct Rec {
  int stride = 0, cg = 0;
  const char* dtype = "";
  int calls = 0;
};
static std::mutex g_mu;
static std::map<std::string, Rec> g_log;
static void note(const char* family, int stride, int cg, const at::Tensor& t) {
  std::lock_guard<std::mutex> lk(g_mu);
  Rec& r = g_log[family];
  r.stride = stride;
  r.cg = cg;
  r.dtype = t.scalar_type() == at::kBFloat16 ? "bf16" : "f16";
  ++r.calls;
}
static std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> last_launch() {
  std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> out;
  std::lock_guard<std::mutex> lk(g_mu);
  for (const auto& kv : g_log)
    out[kv.first] = std::make_tuple(std::vector<int64_t>{kv.second.stride, kv.second.cg},
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
// big: [N, C, H, W] (x / dx), small: [N, C, OH, OW] (y / dy), w: fp32 [C, Cg, 3, 3]
static Dims dims(const at::Tensor& big, const at::Tensor& small, const at::Tensor& w, int64_t stride,
                 int64_t groups) {
  check_act(big, "x");
  check_act(small, "y");
  TORCH_CHECK(big.scalar_type() == small.scalar_type(), "conv_group: one activation dtype");
  TORCH_CHECK(stride == 1 || stride == 2, "conv_group: stride 1 or 2");
  const int64_t C = big.size(1);
  TORCH_CHECK(supported(C, w.size(0), groups), "conv_group: unsupported C / K / groups ", C, " / ", w.size(0),
              " / ", groups);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous() && w.dim() == 4 &&
                  w.size(1) == C / groups && w.size(2) == 3 && w.size(3) == 3,
              "conv_group: fp32 contiguous weight [C, C / groups, 3, 3]");
  Dims d;
  d.N = (int)big.size(0); d.C = (int)C; d.H = (int)big.size(2); d.W = (int)big.size(3);
  d.OH = (d.H - 1) / (int)stride + 1; d.OW = (d.W - 1) / (int)stride + 1;
  d.cg = (int)(C / groups);
  TORCH_CHECK(d.N >= 1 && d.H >= 1 && d.W >= 1, "conv_group: empty input");
  TORCH_CHECK(small.size(0) == d.N && small.size(1) == C && small.size(2) == d.OH && small.size(3) == d.OW,
              "conv_group: output shape");
  TORCH_CHECK(big.numel() < (1ll << 31), "conv_group: activation of 2^31 elements or more");
  return d;
}
// tiles of th x tw over an oh x ow image; `per` tiles per workgroup so that about 1024
// workgroups remain (at most 16 tiles share one staging of the weights)
static dim3 tile_grid(Dims& d, int oh, int ow, int th, int tw) {
  d.tiles_y = (oh + th - 1) / th;
  d.tiles_x = (ow + tw - 1) / tw;
  const long long total = (long long)d.N * d.tiles_y * d.tiles_x, blocks = d.C / CB;
  d.per = (int)std::min<long long>(16, std::max<long long>(1, total * blocks / 1024));
  return dim3((unsigned)((total + d.per - 1) / d.per), (unsigned)blocks);
}

// bf16 / fp16 only: check_act has refused everything else
#define GCONV_DISPATCH(t, ...)                                                 \
  do {                                                                         \
    if ((t).scalar_type() == at::kBFloat16) { typedef __hip_bfloat16 T; __VA_ARGS__; } \
    else { typedef __half T; __VA_ARGS__; }                                    \
  } while (0)

template <typename T>
static void launch_fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y, int stride, bool dgrad, dim3 grid,
                       const Dims& d) {
  auto k = dgrad ? fwd_kernel<T, 1, true> : stride == 1 ? fwd_kernel<T, 1, false> : fwd_kernel<T, 2, false>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, cur_stream(), dptr<const T>(x), dptr<const float>(w), dptr<T>(y), d);
}

static void fwd(const at::Tensor& x, const at::Tensor& w, at::Tensor& y, int64_t stride, int64_t groups) {
  Dims d = dims(x, y, w, stride, groups);
  const dim3 grid = tile_grid(d, d.OH, d.OW, TH, TW);
  note("fwd", (int)stride, d.cg, x);
  GCONV_DISPATCH(x, launch_fwd<T>(x, w, y, (int)stride, false, grid, d));
  DPA_CHECK_LAUNCH();
}

static void dgrad(const at::Tensor& dy, const at::Tensor& w, at::Tensor& dx, int64_t stride, int64_t groups) {
  Dims d = dims(dx, dy, w, stride, groups);
  note("dgrad", (int)stride, d.cg, dy);
  if (stride == 1) {
    const dim3 grid = tile_grid(d, d.H, d.W, TH, TW);
    GCONV_DISPATCH(dy, launch_fwd<T>(dy, w, dx, 1, true, grid, d));
  } else {
    const dim3 grid = tile_grid(d, d.H, d.W, TH, 2 * TW);
    GCONV_DISPATCH(dy, hipLaunchKernelGGL((dgrad2_kernel<T>), grid, dim3(256), 0, cur_stream(), dptr<const T>(dy),
                                          dptr<const float>(w), dptr<T>(dx), d));
  }
  DPA_CHECK_LAUNCH();
}

// Pixel splits of the weight gradient of an [N, C, OH, OW] output gradient: about 1024
// workgroups, every split at least one 8 x 16 tile, and the partials (written and read back)
// at most about the activation bytes the kernel reads.
static int64_t wgrad_splits(int64_t N, int64_t OH, int64_t OW, int64_t C, int64_t cg, int64_t stride) {
  const int64_t total = N * ((OH + TH - 1) / TH) * ((OW + TW - 1) / TW), blocks = C / CB;
  const int64_t act = N * OH * OW * 2 * CB * (1 + stride * stride), part = 2 * 4 * CB * cg * 9;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>({total, 1024 / blocks + 1, act / part}));
  const int64_t per = (total + want - 1) / want;
  return (total + per - 1) / per;
}

template <typename T>
static void launch_wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& slab, int stride, bool full,
                         dim3 grid, const Dims& d) {
  auto k = stride == 1 ? (full ? wgrad_kernel<T, 1, true> : wgrad_kernel<T, 1, false>)
                       : (full ? wgrad_kernel<T, 2, true> : wgrad_kernel<T, 2, false>);
  hipLaunchKernelGGL(k, grid, dim3(192), 0, cur_stream(), dptr<const T>(dy), dptr<const T>(x), dptr<float>(slab), d);
}

static void wgrad(const at::Tensor& dy, const at::Tensor& x, at::Tensor& grad, int64_t stride, int64_t groups,
                  at::Tensor& slab) {
  Dims d = dims(x, dy, grad, stride, groups);
  d.tiles_y = (d.OH + TH - 1) / TH;
  d.tiles_x = (d.OW + TW - 1) / TW;
  const int64_t total = (int64_t)d.N * d.tiles_y * d.tiles_x;
  const int64_t splits = wgrad_splits(d.N, d.OH, d.OW, d.C, d.cg, stride), n = grad.numel();
  d.per = (int)((total + splits - 1) / splits);
  TORCH_CHECK(slab.is_cuda() && slab.scalar_type() == at::kFloat && slab.is_contiguous() &&
                  slab.numel() >= splits * n, "conv_group: wgrad workspace of ", splits * n, " floats");
  note("wgrad", (int)stride, d.cg, dy);
  const dim3 grid((unsigned)splits, (unsigned)(d.C / CB));
  const bool full = d.cg == 32;
  GCONV_DISPATCH(dy, launch_wgrad<T>(dy, x, slab, (int)stride, full, grid, d));
  DPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cur_stream(),
                     dptr<const float>(slab), dptr<float>(grad), (int)n, (int)splits);
  DPA_CHECK_LAUNCH();
}

}  // namespace gconv

void register_conv_group(pybind11::module& m) {
  auto s = m.def_submodule("conv_group", "grouped 3x3 NHWC convolution on MFMA (32-channel block-diagonal tiles)");
  s.def("supported", &gconv::supported);
  s.def("fwd", &gconv::fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"), pybind11::arg("stride"),
        pybind11::arg("groups"));
  s.def("dgrad", &gconv::dgrad, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("dx"), pybind11::arg("stride"),
        pybind11::arg("groups"));
  s.def("wgrad", &gconv::wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("grad"),
        pybind11::arg("stride"), pybind11::arg("groups"), pybind11::arg("slab"));
  s.def("wgrad_splits", &gconv::wgrad_splits);
  s.def("last_launch", &gconv::last_launch);
  s.def("clear_launches", &gconv::clear_launches);
  s.attr("TILE_H") = gconv::TH;
  s.attr("TILE_W") = gconv::TW;
}

}  // namespace dpa
