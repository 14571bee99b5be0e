// Depthwise 3x3 convolution (padding 1, stride 1 or 2, K == C == groups, channel multiplier 1,
// C any multiple of 8) of NHWC bf16 / fp16 activations with the fp32 master weight [C][1][3][3]:
// forward, data gradient and weight gradient.  MobileNetV1's depthwise convs
// (models/mobilenet.py, ops/conv_dw.py).
//
// Why VALU and not MFMA
//   The op does 9 multiply-adds per element it moves, and every product pairs one activation
//   with one weight of the SAME channel: as a matrix product it is the diagonal of a 32 x 32
//   tile, so the block-diagonal design of conv_group.hip would multiply by 31 zeros for every
//   weight.  The bytes bound it long before the vector fp32 rate does (expected; the measured
//   figures are in profiles/dwconv_bench.txt).  The kernels use plain fmaf on fp32 values
//   unpacked from 16-B loads; the compiler chooses the instructions.
//
// Common to the three operations
//   * Granules.  8 channels of a pixel are one 16-B granule; a thread owns ONE granule of ONE
//     output column and walks DOWN rows.  A workgroup (256 threads) owns a channel block of 64
//     channels = 8 granules = 128 contiguous bytes per pixel; lanes 0..7 of every 8 read one
//     pixel's 128 B.  The last block of a C that is no multiple of 64 is masked by granule
//     (C = 32: four live granules; C = 8: one).
//   * Weights: a thread's 9 x 8 weights are loaded once from the fp32 master, rounded to the
//     compute dtype (as the library branch's weight.to(cdtype)) and kept in registers as fp32
//     for the whole walk: 72 VGPRs.  Chosen over packed 16-bit pairs (36 VGPRs and an unpack
//     per use) because every instantiation fits the 256 VGPRs of two workgroups per CU
//     without scratch (139..234, profiles/dwconv_resources.txt: the unrolled walks issue their
//     LDS reads up front); packed pairs were not built.
//   * LDS tile: the input tile with its halo, pixel-major, staged once by 16-B global loads;
//     the halo outside the image (and masked granules) are written as zeros, never read from
//     memory.  Pixel stride PS = 72 elements (144 B = the 128 B of data + 16 B), so eight
//     consecutive pixels start 36 dwords apart instead of 32.
//   * A workgroup walks `per` consecutive tiles (1..16, so that about 1024 workgroups remain)
//     to amortise the weight load, as the grouped kernels do.
//
// Forward, and the stride-1 data gradient (the same kernel on dy with the flipped filter):
// fwd_kernel<T, S, DGRAD>
//   work split   stride 1: output tile 8 rows x 16 columns; thread = granule x column x one
//                of 2 row groups, walking 4 rows.  stride 2: 8 rows x 8 columns; 4 row groups
//                of 2 rows.  (16 columns at stride 2 need an 80,784-B tile: one workgroup per CU.)
//   LDS          (7S+3) x ((TW-1)S+3) pixels x 144 B: 10 x 18 = 25,920 B at stride 1,
//                17 x 17 = 41,616 B at stride 2: three workgroups per CU by LDS.
//   registers    an input row is read once (three granules: the left, centre and right
//                column) and feeds the accumulators of every output row it touches, so the walk
//                reads 3 (stride 1) or 6 (stride 2) granules per output granule plus the
//                two / one rows of window fill per walk: 4.5 and 7.5 in all, not 9.
//                Products and sums in fp32, one rounding at the 16-B store.
//
// Stride-2 data gradient: dgrad2_kernel<T>, the output-parity decomposition.
//   dx[ih][iw] = sum over (r, s) with ih + 1 - r and iw + 1 - s even of
//                dy[(ih + 1 - r) / 2][(iw + 1 - s) / 2] * w[r][s]: 1, 2, 2 or 4 taps by parity.
//   work split   dx tile 16 x 16; wave v owns the 8 columns of parity v & 1 and the 8 rows of
//                half v >> 1; a lane is granule x column.  The column parity is uniform per
//                wave (the taps s are chosen by a wave-uniform branch), and the row walk
//                alternates the row parity: an even row takes r = 1 of the current dy row, an
//                odd row r = 2 of the current and r = 0 of the next, which then becomes the
//                current one.  No multiply by an inserted zero.
//   LDS          only the 9 x 9 dy pixels the tile reads: 11,664 B.
//
// Weight gradient: wgrad_kernel<T, S> + reduce_kernel
//   work split   as the forward (same tiles, same thread = granule x column x row group); a
//                workgroup owns one channel block and a contiguous range of output tiles (the
//                pixel split) and every thread keeps 9 x 8 fp32 accumulators across them.
//   LDS          the x tile (as the forward) + the dy tile (zeros outside the image, so no
//                masks in the loop): 25,920 + 18,432 = 44,352 B at stride 1, 41,616 + 9,216 =
//                50,832 B at stride 2: three workgroups per CU by LDS.
//   reduction    the 32 threads of a granule are summed in a fixed order: lanes l, l ^ 8
//                (DPP row rotate), ^ 16, ^ 32 (permlane swaps, common.h) inside the wave, then
//                waves 0..3 in index order through LDS.  The workgroup writes its fp32
//                [channels][9] slice of slab[split]; reduce_kernel sums the splits in index
//                order straight into the fp32 [C, 1, 3, 3] gradient: no atomics, no cast pass,
//                the same bits on the same inputs.  wgrad_splits keeps about 1024 workgroups and
//                caps the partials at the activation bytes, as the grouped one.
// No BN statistics in the epilogue (the following BN takes its own pass) and no tap hand-off.
#include "conv_dw_gran.h"

#include <map>
#include <mutex>
#include <string>

namespace dpa {
namespace dwconv {

constexpr int DXT = 16;  // stride-2 data gradient: dx tile side
constexpr int DD = DXT / 2 + 1;  // ... and the dy pixels under it, per side

template <int S> struct Tile;  // output tile per stride (NG * TW * row groups = 256 threads)
template <> struct Tile<1> { static constexpr int TH = 8, TW = 16; };
template <> struct Tile<2> { static constexpr int TH = 8, TW = 8; };

// The granule's 8 x 9 fp32 weights (72 contiguous floats from channel c), rounded to T, as
// wr[tap][channel]; FLIP: tap 8 - tap (the stride-1 data gradient).  A masked granule reads
// nothing.
template <typename T, bool FLIP>
__device__ __forceinline__ void load_weights(float (&wr)[9][8], const float* __restrict__ w, int c, bool live) {
  float flat[72];
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) v = reinterpret_cast<const f32x4*>(w + (size_t)c * 9)[i];  // 288 B per granule: 16-B aligned
    flat[4 * i] = v[0]; flat[4 * i + 1] = v[1]; flat[4 * i + 2] = v[2]; flat[4 * i + 3] = v[3];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) wr[FLIP ? 8 - tap : tap][j] = MM<T>::rnd(flat[j * 9 + tap]);
}

struct Dims {
  int N, H, W, OH, OW, C;      // H, W: the stride-times-larger side (x, dx); OH, OW: y, dy
  int tiles_x, tiles_y, per;   // tiles per image row / column; tiles per workgroup
};

// ---- forward / stride-1 data gradient --------------------------------------------------
template <typename T, int S, bool DGRAD>
__global__ __launch_bounds__(256) void fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                  T* __restrict__ y, Dims d) {
  constexpr int TH = Tile<S>::TH, TW = Tile<S>::TW, RPT = TH * NG * TW / 256;  // rows per thread
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  __shared__ __attribute__((aligned(16))) lds_t tile[IH * IW * PS];
  const int g = threadIdx.x & 7, col = (threadIdx.x >> 3) % TW, row0 = (threadIdx.x / (NG * TW)) * RPT;
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = g < ng;
  float wr[9][8];
  load_weights<T, DGRAD>(wr, w, c0 + 8 * g, live);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int oh0 = ty * TH + row0, ow = tx * TW + col;
    __syncthreads();  // the previous tile is read
    stage_tile<T, IH, IW>(tile, x, n, d.H, d.W, d.C, c0, ng, ty * TH * S - 1, tx * TW * S - 1);
    __syncthreads();
    if (!live || oh0 >= d.OH || ow >= d.OW) continue;  // (the barriers are above)
    float acc[RPT][8] = {};
    T* dst = y + (((size_t)n * d.OH + oh0) * d.OW + ow) * d.C + c0 + 8 * g;
#pragma unroll
    for (int i = 0; i < (RPT - 1) * S + 3; ++i) {  // the thread's input rows, top to bottom
      float in[3][8];
      const lds_t* p = tile + ((row0 * S + i) * IW + col * S) * PS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) ld_gran<T>(p + s * PS, in[s]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if (i - r < 0 || (i - r) % S != 0 || (i - r) / S >= RPT) continue;
        const int j = (i - r) / S;  // the output row this input row is filter row r of
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[j][c] = fmaf(in[s][c], wr[r * 3 + s][c], acc[j][c]);
      }
      if (i >= 2 && (i - 2) % S == 0) {  // output row j is complete
        const int j = (i - 2) / S;
        if (oh0 + j < d.OH) st_gran<T>(dst + (size_t)j * d.OW * d.C, acc[j]);
      }
    }
  }
}

// ---- stride-2 data gradient --------------------------------------------------------------
// One lane's walk down 8 dx rows of column parity B: dy column j (s = 1) for B = 0; dy columns
// j (s = 2) and j + 1 (s = 0) for B = 1.
template <typename T, int B>
__device__ __forceinline__ void dgrad2_walk(const lds_t* tile, const float (&wr)[9][8], T* dst, const Dims& d,
                                            int ih, int k0, int j) {
  constexpr int NS = B ? 2 : 1;
  float cur[NS][8], nxt[NS][8];
#pragma unroll
  for (int t = 0; t < NS; ++t) ld_gran<T>(tile + (k0 * DD + j + t) * PS, cur[t]);
#pragma unroll
  for (int kk = 0; kk < DXT / 4; ++kk) {
#pragma unroll
    for (int t = 0; t < NS; ++t) ld_gran<T>(tile + ((k0 + kk + 1) * DD + j + t) * PS, nxt[t]);
    float ev[8] = {}, od[8] = {};
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      const int s = B ? (t ? 0 : 2) : 1;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        ev[c] = fmaf(cur[t][c], wr[3 + s][c], ev[c]);  // even row: r = 1
        od[c] = fmaf(cur[t][c], wr[6 + s][c], od[c]);  // odd row: r = 2 of this dy row ...
        od[c] = fmaf(nxt[t][c], wr[s][c], od[c]);      // ... and r = 0 of the next
      }
    }
    if (ih + 2 * kk < d.H) st_gran<T>(dst + (size_t)(2 * kk) * d.W * d.C, ev);
    if (ih + 2 * kk + 1 < d.H) st_gran<T>(dst + (size_t)(2 * kk + 1) * d.W * d.C, od);
#pragma unroll
    for (int t = 0; t < NS; ++t)
#pragma unroll
      for (int c = 0; c < 8; ++c) cur[t][c] = nxt[t][c];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dgrad2_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                     T* __restrict__ dx, Dims d) {
  __shared__ __attribute__((aligned(16))) lds_t tile[DD * DD * PS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane & 7, j = lane >> 3;
  const int b = wv & 1, k0 = (wv >> 1) * (DXT / 4);  // column parity; first dy row of the wave's 8 dx rows
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = g < ng;
  float wr[9][8];
  load_weights<T, false>(wr, w, c0 + 8 * g, live);
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    const int ih = ty * DXT + 2 * k0, iw = tx * DXT + 2 * j + b;
    __syncthreads();
    stage_tile<T, DD, DD>(tile, dy, n, d.OH, d.OW, d.C, c0, ng, ty * (DXT / 2), tx * (DXT / 2));
    __syncthreads();
    if (!live || ih >= d.H || iw >= d.W) continue;
    T* dst = dx + (((size_t)n * d.H + ih) * d.W + iw) * d.C + c0 + 8 * g;
    if (b) dgrad2_walk<T, 1>(tile + 8 * g, wr, dst, d, ih, k0, j);  // (uniform per wave)
    else dgrad2_walk<T, 0>(tile + 8 * g, wr, dst, d, ih, k0, j);
  }
}

// ---- weight gradient -----------------------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(256) void wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                    float* __restrict__ slab, Dims d) {
  constexpr int TH = Tile<S>::TH, TW = Tile<S>::TW, RPT = TH * NG * TW / 256;
  constexpr int IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3;
  static_assert(IH * IW * PS * sizeof(lds_t) >= 4 * NG * 72 * sizeof(float), "the wave partials reuse the x tile");
  __shared__ __attribute__((aligned(16))) lds_t xt[IH * IW * PS];
  __shared__ __attribute__((aligned(16))) lds_t dt[TH * TW * PS];
  const int g = threadIdx.x & 7, col = (threadIdx.x >> 3) % TW, row0 = (threadIdx.x / (NG * TW)) * RPT;
  const int c0 = blockIdx.y * CB, ng = min(NG, (d.C - c0) >> 3);
  const bool live = g < ng;
  const int per_img = d.tiles_y * d.tiles_x, total = d.N * per_img;
  const int t1 = min(total, ((int)blockIdx.x + 1) * d.per);
  float acc[9][8] = {};
  for (int t = blockIdx.x * d.per; t < t1; ++t) {
    const int n = t / per_img, rem = t - n * per_img, ty = rem / d.tiles_x, tx = rem - ty * d.tiles_x;
    __syncthreads();
    stage_tile<T, IH, IW>(xt, x, n, d.H, d.W, d.C, c0, ng, ty * TH * S - 1, tx * TW * S - 1);
    stage_tile<T, TH, TW>(dt, dy, n, d.OH, d.OW, d.C, c0, ng, ty * TH, tx * TW);
    __syncthreads();
    if (!live || ty * TH + row0 >= d.OH || tx * TW + col >= d.OW) continue;  // (only zeros of dy there)
    float dv[RPT][8];
#pragma unroll
    for (int j = 0; j < RPT; ++j) ld_gran<T>(dt + ((row0 + j) * TW + col) * PS + 8 * g, dv[j]);
#pragma unroll
    for (int i = 0; i < (RPT - 1) * S + 3; ++i) {
      float in[3][8];
      const lds_t* p = xt + ((row0 * S + i) * IW + col * S) * PS + 8 * g;
#pragma unroll
      for (int s = 0; s < 3; ++s) ld_gran<T>(p + s * PS, in[s]);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        if (i - r < 0 || (i - r) % S != 0 || (i - r) / S >= RPT) continue;
        const int j = (i - r) / S;
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[r * 3 + s][c] = fmaf(dv[j][c], in[s][c], acc[r * 3 + s][c]);
      }
    }
  }
  // the 32 threads of a granule, in a fixed order: lanes ^ 8, ^ 16, ^ 32, then waves 0..3
  __syncthreads();  // every lane is here (the DPP reads need them all), the x tile is read
  float* red = reinterpret_cast<float*>(xt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = acc[tap][c];
      v += dpp_mov<0x128>(v);  // row_ror:8: lane ^ 8 of the 16-lane row
      v = xor32_sum(xor16_sum(v));
      if (lane < NG) red[(wv * NG + lane) * 72 + c * 9 + tap] = v;
    }
  __syncthreads();
  float* out = slab + ((size_t)blockIdx.x * d.C + c0) * 9;  // [channel][tap] of this split
  for (int i = threadIdx.x; i < ng * 72; i += 256)
    out[i] = ((red[i] + red[NG * 72 + i]) + red[2 * NG * 72 + i]) + red[3 * NG * 72 + i];
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
// big: [N, C, H, W] (x / dx), small: [N, C, OH, OW] (y / dy), w: fp32 [C, 1, 3, 3]
static Dims dims(const at::Tensor& big, const at::Tensor& small, const at::Tensor& w, int64_t stride) {
  check_act(big, "x");
  check_act(small, "y");
  TORCH_CHECK(big.scalar_type() == small.scalar_type(), "conv_dw: one activation dtype");
  TORCH_CHECK(big.device() == small.device() && big.device() == w.device(), "conv_dw: one device");
  TORCH_CHECK(stride == 1 || stride == 2, "conv_dw: stride 1 or 2");
  const int64_t C = big.size(1);
  TORCH_CHECK(w.dim() == 4 && supported(C, w.size(0), C), "conv_dw: unsupported C / K ", C, " / ", w.size(0));
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.is_contiguous() && w.size(1) == 1 &&
                  w.size(2) == 3 && w.size(3) == 3 && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
              "conv_dw: fp32 contiguous 16-byte aligned weight [C, 1, 3, 3]");
  Dims d;
  d.N = (int)big.size(0); d.C = (int)C; d.H = (int)big.size(2); d.W = (int)big.size(3);
  d.OH = (d.H - 1) / (int)stride + 1; d.OW = (d.W - 1) / (int)stride + 1;
  TORCH_CHECK(d.N >= 1 && d.H >= 1 && d.W >= 1, "conv_dw: empty input");
  TORCH_CHECK(small.size(0) == d.N && small.size(1) == C && small.size(2) == d.OH && small.size(3) == d.OW,
              "conv_dw: output shape");
  TORCH_CHECK(big.numel() < (1ll << 31), "conv_dw: activation of 2^31 elements or more");
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
  note("fwd", (int)stride, d.C, x);
  DWCONV_DISPATCH(x, launch_fwd<T>(x, w, y, (int)stride, false, grid, d));
  DPA_CHECK_LAUNCH();
}

static void dgrad(const at::Tensor& dy, const at::Tensor& w, at::Tensor& dx, int64_t stride) {
  Dims d = dims(dx, dy, w, stride);
  note("dgrad", (int)stride, d.C, dy);
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
  const int64_t act = N * OH * OW * 2 * CB * (1 + stride * stride), part = 2 * 4 * CB * 9;
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
              "conv_dw: wgrad workspace of ", splits * n, " floats");
  note("wgrad", (int)stride, d.C, dy);
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

}  // namespace dwconv

void register_conv_dw(pybind11::module& m) {
  auto s = m.def_submodule("conv_dw", "depthwise 3x3 NHWC convolution (VALU, one 16-B granule per thread)");
  s.def("supported", &dwconv::supported);
  s.def("fwd", &dwconv::fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"), pybind11::arg("stride"));
  s.def("dgrad", &dwconv::dgrad, pybind11::arg("dy"), pybind11::arg("w"), pybind11::arg("dx"),
        pybind11::arg("stride"));
  s.def("wgrad", &dwconv::wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("grad"),
        pybind11::arg("stride"), pybind11::arg("slab"));
  s.def("wgrad_splits", &dwconv::wgrad_splits);
  s.def("tile", &dwconv::tile, "(rows, columns) of the output tile at a stride");
  s.def("last_launch", &dwconv::last_launch);
  s.def("clear_launches", &dwconv::clear_launches);
}

}  // namespace dpa
