// NHWC implicit-GEMM convolution on MFMA for the ResNet-50 stress config
// (BASELINE.json config 5; the reference has no ResNet, its conv semantics are
// torch's: /root/reference/ddp_main.py:83-93 trains the ConvNet with nn.Conv2d).
//
//   y[p][k] = sum_{r,s,c} x[n][oh*st+r-pad][ow*st+s-pad][c] * w[k][r][s][c]
//   (p = (n, oh, ow): GEMM M = N*OH*OW pixels, N = Cout, K = R*S*C)
//
// with the BatchNorm statistics of the (storage-rounded) output produced in the
// epilogue -- per channel sum(y - shift), sum((y - shift)^2) around the running
// mean, the layout ops/bn_nhwc.py's kernels consume -- so a BN after a conv
// needs no separate statistics pass over the activation.
//
// Geometry (MI355X, 64-wide waves, 160 KB LDS):
//   * workgroup = 4 waves, tile 128 pixels x BN (64|128) channels, K-step 64
//     (one filter tap (r,s) x 64 input channels: C % 64 == 0);
//   * operands staged global -> registers -> LDS (double-buffered, one barrier
//     per K-step), 16-B chunks, rows of 64 bf16 with the chunk index XOR-swizzled
//     by (row & 7): the MFMA fragment reads (ds_read_b128) are at most 2-way;
//   * MFMA orientation: A = weights (rows = output channels), B = pixels, so a
//     lane's accumulator holds 4 CONSECUTIVE channels of one pixel
//     (C/D map: row = 4*(lane>>4) + j, col = lane & 15): the BN sums reduce over
//     lanes only, and the rounded tile is staged through LDS so it leaves as
//     whole-row 16-B stores;
//   * XCD-aware workgroup order (the channel tiles of one pixel tile share an L2);
//   * the pixel tile's im2col addresses (n, ih0, iw0) are computed once per
//     workgroup; padding / ragged M are zero-filled in the loader.
#include <map>
#include <string>

#include "comm/xgmi.h"
#include "kernels/conv_igemm.h"

namespace dpa {
namespace igemm {

constexpr int BM = 128;  // pixels per workgroup
constexpr int SHIFT_OFF = 4;  // stats layout of bn_nhwc.hip: [2C] = rows, shift at [2C+4 ...)

__device__ __forceinline__ int swz(int row, int chunk) { return row * BK + ((chunk ^ (row & 7)) << 3); }

// Statistics tree (all in the conv launch, deterministic: fixed-order sums):
// every workgroup writes its [2][BN] partial row for its channel tile; the last
// arriver of each group of G1 pixel tiles (ticket) sums the group's rows into a
// level-2 row; the last level-2 arriver sums those and writes the final stats.
// Tickets are re-armed by their last arriver (graph replays need no reset).
constexpr int G1 = 32;

struct StatArgs {
  float* part;        // [nct][rows][2*BN] level 1, then [nct][NG][2*BN] level 2
  unsigned* tickets;  // [nct][NG] + [nct], zero-initialised
  float* stats;       // [3K+4]
  const float* shift; // running mean (the sums are taken around it)
  int64_t* nbt;       // num_batches_tracked (bumped once) or null
  int defer;          // 1: level-1 rows only (plain stores, no ticket), stat_tree_kernel follows
  // backward statistics of the BatchNorm whose output gradient this conv produces
  // (conv_glds_kernel BS > 0): stats = out [S1 | S2], plus dbeta = S1, dgamma = S2
  float* dgamma = nullptr;
  float* dbeta = nullptr;
  int bwd = 0;
  // SyncBN: the finishers of the deferred tree (stat_sum1_kernel / stat_tree_kernel) exchange
  // their slices through this site (comm/xsite.h positioned form) -- the statistics leave
  // the launch already global, no all-reduce launch follows.  dgamma / dbeta stay local.
  xgmi::XSite xs;
};

// BS (conv_glds_kernel): the output is the gradient dy of a BatchNorm's output; the epilogue
// also takes that BN's backward sums S1 = sum dz, S2 = sum dz * xhat (dz = dy * relu'),
// as the separate bn_nhwc bwd_stats pass would (csrc/kernels/bn_nhwc.hip):
//   BS_Y:   ReLU mask from the BN's output y (a residual was added); the gradient is
//           accumulated onto the tapped residual gradient (Geom.accumulate)
//   BS_REC: ReLU mask recomputed from x (fma(x, gamma*invstd, beta - mean*gamma*invstd) > 0)
constexpr int BS_NONE = 0, BS_Y = 1, BS_REC = 2;
template <typename T>
struct BwdStatArgs {
  const T* x = nullptr;         // the BN's input (this conv's gradient layout [M][K])
  const T* y = nullptr;         // BS_Y: the BN's output
  const float* save = nullptr;  // mean[K], invstd[K] of the forward
  const float* gamma = nullptr;
  const float* beta = nullptr;
};

// dst[0, W) = sum over rows g < n of src[g*W + .] in row order (W = 2*BN <= 256 floats;
// src read with write-through loads; dst written write-through when `wt`): lane owns a
// column, THR/W row groups, combined in group order via scr
template <int W>
__device__ __forceinline__ void sum_rows(const float* __restrict__ src, int n, float* __restrict__ dst, float* scr,
                                         bool wt) {
  constexpr int RG = THR / W;
  const int col = threadIdx.x % W, rg = threadIdx.x / W;
  float acc = 0.f;
  for (int g0 = rg; g0 < n; g0 += 8 * RG) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int gg = g0 + u * RG;
      v[u] = ld_wt(src + (long long)(gg < n ? gg : 0) * W + col);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (g0 + u * RG < n) acc += v[u];
  }
  scr[rg * W + col] = acc;
  __syncthreads();
  if ((int)threadIdx.x < W) {
    float t = 0.f;
    for (int r = 0; r < RG; ++r) t += scr[r * W + threadIdx.x];
    if (wt) st_wt(dst + threadIdx.x, t); else dst[threadIdx.x] = t;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// The tile epilogue of conv_fwd_kernel and conv_glds_kernel, and the statistics tree they
// share with stat_tree_kernel.  A workgroup of NT threads holds a BPX-pixel x BN-channel
// tile: lane (fr, fq) of a wave holds channels cw + 16a + 4fq + j of pixel pw + 16b + fr.
// The rounded tile goes through LDS ([pixel][channel], rows padded by 16 B: the 8-byte
// writes of a 16-pixel column are conflict-free) and leaves as whole 16-B chunks,
// consecutive lanes along a pixel's channels (full rows per store).
template <int BN>
struct Epi {
  static constexpr int RS = BN + 8;   // LDS row stride (elements)
  static constexpr int CPR = BN / 8;  // 16-B chunks per pixel row
};

// accumulators -> the LDS tile (cw, pw: this wave's first channel / pixel of the tile)
template <typename T, int BN, int CT, int PT>
__device__ __forceinline__ void stage_tile(T* tile, const f32x4 (&acc)[CT][PT], int cw, int pw, int fr, int fq) {
#pragma unroll
  for (int a = 0; a < CT; ++a) {
    const int cl = cw + a * 16 + 4 * fq;
#pragma unroll
    for (int b = 0; b < PT; ++b) {
      const int pl = pw + b * 16 + fr;
      T v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = Cvt<T>::from_f(acc[a][b][j]);
      *reinterpret_cast<u16x4*>(tile + pl * Epi<BN>::RS + cl) = *reinterpret_cast<const u16x4*>(v);
    }
  }
}

// Output stores: whole 16-B chunks, consecutive lanes along a pixel's channels;
// y (+)= tile (+ aux at the even pixels): the tile comes from LDS already rounded to T
// (stage_tile), old + aux + tile is summed in fp32 and rounded again -- two roundings on
// the accumulate / aux paths, one otherwise.  MODE_S2T writes
// parity class (py, px) with stride 2.  OLDPRE: the accumulated-onto chunk of pass `it` was
// prefetched by the kernel (old_of(it)) instead of being read here; stored(it, raw) sees
// every stored chunk (the BN-backward sums of conv_glds_kernel).
template <typename T, int BPX, int BN, int NT, int MODE, bool OLDPRE, typename OldFn, typename StoredFn>
__device__ __forceinline__ void store_tile(const T* tile, T* __restrict__ y, const Geom& g, long long p0, int k0,
                                           int py, int px, OldFn&& old_of, StoredFn&& stored) {
  constexpr int RS = Epi<BN>::RS, CPR = Epi<BN>::CPR, RPI = NT / CPR;  // RPI: pixel rows per pass
  const int tid = threadIdx.x, ch = tid % CPR;
  const T* aux = reinterpret_cast<const T*>(g.aux);
#pragma unroll
  for (int it = 0; it < BPX / RPI; ++it) {
    const int pl = it * RPI + tid / CPR;
    const long long p = p0 + pl;
    if (p < g.M) {
      long long op = p;  // output pixel
      int oh = 0, ow = 0, n = 0;
      if (MODE == MODE_S2T || aux != nullptr) {
        ow = (int)(p % g.OW);
        const long long t = p / g.OW;
        oh = (int)(t % g.OH);
        n = (int)(t / g.OH);
      }
      if constexpr (MODE == MODE_S2T) op = ((long long)n * (2 * g.OH) + 2 * oh + py) * (2 * g.OW) + 2 * ow + px;
      f32x4* dst = reinterpret_cast<f32x4*>(y + op * g.K + k0 + ch * 8);
      f32x4 raw = *reinterpret_cast<const f32x4*>(tile + pl * RS + ch * 8);
      const bool add_aux = aux != nullptr && !(oh & 1) && !(ow & 1);
      if (g.accumulate || add_aux) {
        f32x4 old = {0.f, 0.f, 0.f, 0.f}, ax = {0.f, 0.f, 0.f, 0.f};
        if constexpr (OLDPRE) old = old_of(it);
        else if (g.accumulate) old = *dst;
        if (add_aux)
          ax = *reinterpret_cast<const f32x4*>(
              aux + (((long long)n * (g.OH >> 1) + (oh >> 1)) * (g.OW >> 1) + (ow >> 1)) * g.K + k0 + ch * 8);
        const T* a = reinterpret_cast<const T*>(&old);
        const T* e = reinterpret_cast<const T*>(&ax);
        T* b = reinterpret_cast<T*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          b[j] = Cvt<T>::from_f(Cvt<T>::to_f(a[j]) + Cvt<T>::to_f(e[j]) + Cvt<T>::to_f(b[j]));
      }
      *dst = raw;
      stored(it, raw);
    }
  }
}

// Each lane's sums of its fixed 8-channel chunk over its rows of the tile: the rounded
// values around the shift sh (the running mean), rows past the ragged end masked out
template <typename T, int BPX, int BN, int NT>
__device__ __forceinline__ void tile_col_sums(const T* tile, int plast, const float (&sh)[8], float (&s1)[8],
                                              float (&s2)[8]) {
  constexpr int RS = Epi<BN>::RS, CPR = Epi<BN>::CPR, RPI = NT / CPR;
  const int tid = threadIdx.x, ch = tid % CPR;
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  // unconditional reads of clamped rows (a per-row guard was a branch + wait per row)
  f32x4 raw[BPX / RPI];
#pragma unroll
  for (int it = 0; it < BPX / RPI; ++it)
    raw[it] = *reinterpret_cast<const f32x4*>(tile + min(it * RPI + tid / CPR, plast) * RS + ch * 8);
#pragma unroll
  for (int it = 0; it < BPX / RPI; ++it) {
    const float m = it * RPI + tid / CPR <= plast ? 1.f : 0.f;
    const T* e = reinterpret_cast<const T*>(&raw[it]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = (Cvt<T>::to_f(e[j]) - sh[j]) * m;
      s1[j] += d;
      s2[j] = fmaf(d, d, s2[j]);
    }
  }
}

// The per-lane column sums -> red[wave][2][BN]: xor-reduced over the lanes of a wave that
// share the chunk (the row bits of the lane index), then an LDS-only barrier:
// __syncthreads() is a workgroup fence whose vmcnt(0) would wait here for the whole output
// tile's stores to drain (~30 us on a 56x56 x 256 conv)
template <int BN>
__device__ __forceinline__ void reduce_cols(float (&s1)[8], float (&s2)[8], float (*red)[2][BN]) {
  constexpr int CPR = Epi<BN>::CPR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ch = tid % CPR;
#pragma unroll
  for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s1[j] += __shfl_xor(s1[j], o);
      s2[j] += __shfl_xor(s2[j], o);
    }
  if (lane < CPR)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wave][0][ch * 8 + j] = s1[j];
      red[wave][1][ch * 8 + j] = s2[j];
    }
  lds_barrier();
}

// red summed over the NW waves in wave order -> this pixel tile's level-1 row: plain stores
// (the tree runs in a launch after this one) or write-through (the in-launch tree)
template <int BN, int NW>
__device__ __forceinline__ void write_level1(const float (*red)[2][BN], float* row, bool wt) {
  for (int t = threadIdx.x; t < 2 * BN; t += 64 * NW) {
    const int q = t / BN, c = t % BN;
    float v = red[0][q][c];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[w][q][c];
    if (wt) st_wt(row + t, v); else row[t] = v;
  }
}

// The tree above the level-1 rows of channel tile bn (THR threads; rows pixel tiles in NG
// groups of G1).  Level 2: this workgroup sums group grp's gsz rows into the group's level-2
// row and is ticketed; true in the last of the channel tile's NG arrivals.
struct Tree {
  float *lvl1, *lvl2;  // this channel tile's level-1 / level-2 rows
  int NG;
  template <int BN>
  __device__ __forceinline__ static Tree of(const StatArgs& sa, int nct, int bn, long long rows) {
    const int NG = (int)((rows + G1 - 1) / G1);
    return {sa.part + (long long)bn * rows * (2 * BN),
            sa.part + (long long)nct * rows * (2 * BN) + (long long)bn * NG * (2 * BN), NG};
  }
};
template <int BN>
__device__ __forceinline__ bool tree_level2(const StatArgs& sa, const Tree& t, int nct, int bn, int grp, int gsz,
                                            float* scr, int* s_flag) {
  sum_rows<2 * BN>(t.lvl1 + (long long)grp * G1 * (2 * BN), gsz, t.lvl2 + (long long)grp * (2 * BN), scr, true);
  return last_arriver(sa.tickets + nct * t.NG + bn, (unsigned)t.NG, s_flag);
}
// tot = [sum | sumsq] of channel tile bn -> the final statistics [s1 | s2 | count | shift]
template <int BN>
__device__ __forceinline__ void write_stats(const StatArgs& sa, int K, int bn, const float* tot, float count) {
  const int k0 = bn * BN, tid = threadIdx.x;
  for (int t = tid; t < BN; t += THR) {
    sa.stats[k0 + t] = tot[t];
    sa.stats[K + k0 + t] = tot[BN + t];
    sa.stats[2 * K + SHIFT_OFF + k0 + t] = sa.shift[k0 + t];
  }
  if (bn == 0 && tid == 0) {
    sa.stats[2 * K] = count;
    if (sa.nbt != nullptr) sa.nbt[0] = sa.nbt[0] + 1;
  }
}
// The in-launch tree of a conv workgroup that was the last of its level-1 group
template <int BN>
__device__ __forceinline__ void tree_in_launch(const StatArgs& sa, const Geom& g, int nct, int bn, long long rows,
                                               int grp, int gsz, float* scr, float* tot, int* s_flag) {
  const Tree t = Tree::of<BN>(sa, nct, bn, rows);
  if (!tree_level2<BN>(sa, t, nct, bn, grp, gsz, scr, s_flag)) return;
  sum_rows<2 * BN>(t.lvl2, t.NG, tot, scr, false);
  write_stats<BN>(sa, g.K, bn, tot, (float)g.M);
}

// slab: [gridDim(pixel tiles)][2][K] partial statistics (null: none)
template <typename T, int BN, int MODE = MODE_GEN>
__global__ void __launch_bounds__(THR)
conv_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, StatArgs sa, Geom g) {
  using MMT = MM<T>;
  typedef typename MMT::frag frag;
  constexpr int CT = BN / 32;         // 16-channel tiles per wave (2 channel-waves)
  constexpr int PT = 4;               // 16-pixel tiles per wave (64 pixels)
  constexpr int BLD = BN / 32;        // B (weight) 16-B chunks per thread per K-step
  __shared__ __attribute__((aligned(16))) T lds[2][(BM + BN) * BK];
  __shared__ __attribute__((aligned(16))) float red[4][2][BN];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave & 1, wc = wave >> 1;  // pixel half, channel half
  const int nct = g.K / BN;
  const unsigned lid = xcd_tile();  // the nct channel tiles of one pixel tile share an L2
  const long long bm_all = lid / nct;
  const int bn = (int)(lid % nct);
  int cls = 0;  // MODE_S2T: output parity class (py, px)
  long long bm = bm_all;
  if constexpr (MODE == MODE_S2T) {
    cls = (int)(bm_all / g.cls_rows);
    bm = bm_all - (long long)cls * g.cls_rows;
  }
  const int py = cls >> 1, px = cls & 1;
  const int nsx = px ? 2 : 1;  // MODE_S2T: column taps of this class
  const long long p0 = bm * BM;
  const int k0 = bn * BN;
  const int cpt = MODE == MODE_STEM ? 1 : g.C / BK;
  const int KT = MODE == MODE_STEM ? 4 : (MODE == MODE_S2T ? (py ? 2 : 1) * nsx : g.R * g.S) * cpt;
  // loader geometry: chunk cc of rows rr + 32 i
  const int cc = tid & 7, rr = tid >> 3;
  long long xb[4];
  int ih0[4], iw0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long p = p0 + rr + 32 * i;
    if (p < g.M) {
      const int ow = (int)(p % g.OW);
      const long long t = p / g.OW;
      const int oh = (int)(t % g.OH);
      const int n = (int)(t / g.OH);
      xb[i] = (long long)n * g.H * g.W * g.C;
      ih0[i] = MODE == MODE_S2T ? oh : oh * g.stride - g.pad;
      iw0[i] = MODE == MODE_S2T ? ow : ow * g.stride - g.pad;
    } else {
      xb[i] = -1;
      ih0[i] = iw0[i] = 0;
    }
  }
  const long long wrow = MODE == MODE_STEM ? 256 : (long long)g.R * g.S * g.C;
  f32x4 rx[4], rw[BLD];
  auto gload = [&](int kt) {
    long long woff;  // this K-step's offset inside a filter row
    if constexpr (MODE == MODE_STEM) {
      const int r = 2 * kt + (cc >> 2), s = (cc & 3) * 2;  // taps (r, s) and (r, s + 1)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ih = ih0[i] + r, iw = iw0[i] + s;
        const bool rok = xb[i] >= 0 && r < 7 && (unsigned)ih < (unsigned)g.H;
        const T* px_ = x + xb[i] + ((long long)ih * g.W + iw) * 4;
        f32x2 lo = {0.f, 0.f}, hi = {0.f, 0.f};
        if (rok && (unsigned)iw < (unsigned)g.W) lo = *reinterpret_cast<const f32x2*>(px_);
        if (rok && s + 1 < 7 && (unsigned)(iw + 1) < (unsigned)g.W) hi = *reinterpret_cast<const f32x2*>(px_ + 4);
        rx[i] = f32x4{lo[0], lo[1], hi[0], hi[1]};
      }
      woff = (long long)kt * BK + cc * 8;
    } else if constexpr (MODE == MODE_S2T) {
      const int t = kt / cpt, c0 = (kt - t * cpt) * BK + cc * 8;
      const int ri = t / nsx, si = t - ri * nsx;
      const int r = py ? (ri ? 2 : 0) : 1, s = px ? (si ? 2 : 0) : 1;  // forward-filter tap
      const int dh = (py && !ri) ? 1 : 0, dw = (px && !si) ? 1 : 0;    // dy row / col offset
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ih = ih0[i] + dh, iw = iw0[i] + dw;
        const bool ok = xb[i] >= 0 && ih < g.H && iw < g.W;
        rx[i] = ok ? *reinterpret_cast<const f32x4*>(x + xb[i] + ((long long)ih * g.W + iw) * g.C + c0)
                   : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      woff = (long long)(8 - (r * 3 + s)) * g.C + c0;  // flipped filter: tap 8 - (3r + s)
    } else {
      const int rs = kt / cpt, c0 = (kt - rs * cpt) * BK + cc * 8;
      const int r = rs / g.S, s = rs - r * g.S;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ih = ih0[i] + r, iw = iw0[i] + s;
        const bool ok = xb[i] >= 0 && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
        rx[i] = ok ? *reinterpret_cast<const f32x4*>(x + xb[i] + ((long long)ih * g.W + iw) * g.C + c0)
                   : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      woff = (long long)kt * BK + cc * 8;
    }
#pragma unroll
    for (int i = 0; i < BLD; ++i)
      rw[i] = *reinterpret_cast<const f32x4*>(w + (long long)(k0 + rr + 32 * i) * wrow + woff);
  };
  auto lstore = [&](int buf) {
    T* A = lds[buf];           // weights: rows [0, BN)
    T* B = lds[buf] + BN * BK;  // pixels:  rows [0, BM)
#pragma unroll
    for (int i = 0; i < BLD; ++i) *reinterpret_cast<f32x4*>(A + swz(rr + 32 * i, cc)) = rw[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(B + swz(rr + 32 * i, cc)) = rx[i];
  };
  f32x4 acc[CT][PT];
#pragma unroll
  for (int a = 0; a < CT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the statistics' shift (running mean) for this lane's epilogue chunk, loaded with tile 0:
  // loaded after the K loop it cost every workgroup a dependent global-load latency
  float shp[8];
  if (sa.part != nullptr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) shp[j] = sa.shift[k0 + (tid % (BN / 8)) * 8 + j];
  }
  gload(0);
  lstore(0);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) gload(kt + 1);
    const T* A = lds[buf];
    const T* B = lds[buf] + BN * BK;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag fa[CT], fb[PT];
#pragma unroll
      for (int a = 0; a < CT; ++a)
        fa[a] = *reinterpret_cast<const frag*>(A + swz(wc * (BN / 2) + a * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int b = 0; b < PT; ++b)
        fb[b] = *reinterpret_cast<const frag*>(B + swz(wp * 64 + b * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int b = 0; b < PT; ++b) acc[a][b] = MMT::mma(fa[a], fb[b], acc[a][b]);
    }
    if (kt + 1 < KT) lstore(buf ^ 1);
    __syncthreads();
  }
  // epilogue: lane holds channels k0 + wc*BN/2 + 16a + 4fq + j of pixel p0 + wp*64 + 16b + fr
  T* tile = lds[0];
  stage_tile<T, BN>(tile, acc, wc * (BN / 2), wp * 64, fr, fq);
  __syncthreads();
  // With statistics, each lane first sums its fixed 8-channel chunk over its rows of
  // the tile (the rounded values, around the running mean) and the workgroup's partial
  // row goes out (write-through) and is ticketed BEFORE the output stores are issued:
  // the ticket's store drain then never waits for the output tile.
  const bool stats = sa.part != nullptr;
  auto store = [&]() {
    store_tile<T, BM, BN, THR, MODE, false>(tile, y, g, p0, k0, py, px, [](int) { return f32x4{0.f, 0.f, 0.f, 0.f}; },
                                            [](int, const f32x4&) {});
  };
  // Without statistics, or with the tree deferred to stat_tree_kernel, the stores leave
  // first and drain while the sums are taken from the tile still in LDS (the barrier
  // after the sums is LDS-only: __syncthreads() would wait for the stores); with the
  // in-launch tree they follow the ticket, whose vmcnt(0) must not wait for the tile.
  const bool stores_first = !stats || sa.defer;
  if (stores_first) store();
  bool last1 = false;
  long long rows = 0;
  int grp = 0, gsz = 0;
  if (stats) {
    float s1[8], s2[8];
    tile_col_sums<T, BM, BN, THR>(tile, (int)min((long long)BM, g.M - p0) - 1, shp, s1, s2);
    reduce_cols<BN>(s1, s2, red);
    rows = (g.M + BM - 1) / BM;
    float* lvl1 = sa.part + (long long)bn * rows * (2 * BN);
    write_level1<BN, 4>(red, lvl1 + bm * (2 * BN), !sa.defer);
    if (!sa.defer) {
      grp = (int)(bm / G1);
      gsz = (int)min((long long)G1, rows - (long long)grp * G1);
      last1 = last_arriver(sa.tickets + bn * (int)((rows + G1 - 1) / G1) + grp, (unsigned)gsz, &s_flag);
    }
  }
  if (!stores_first) store();
  if (!last1) return;
  __syncthreads();  // every lane is done with the tile: its LDS becomes the tree's scratch
  tree_in_launch<BN>(sa, g, nct, bn, rows, grp, gsz, reinterpret_cast<float*>(lds[1]), &red[0][0][0], &s_flag);
}

// ---------------------------------------------------------------------------
// Implicit-GEMM convolution with both operands staged by LDS-DMA (MODE_GEN: any R x S,
// stride, padding; C % 64 == 0).  Written first for the 1x1 convs, a plain GEMM over the
// NHWC rows (y[p][k] = sum_c x[row(p)][c] * w[k][c]; M = pixels, N = Cout, K = C) -- the
// forward of 36 of ResNet-50's 53 convs and, with the transposed filter, their data
// gradients; a K-step is one filter tap x 64 channels, a padding tap reads a zero page.
// The general kernel above is LDS-bound on these shapes: a 64 x 64
// wave tile reads 32 FLOP per LDS byte and its register-staged ds_write_b128 stores
// cost ~13 LDS cycles per KiB, so the MFMAs idle behind the LDS (2x slower than
// hipBLASLt on the deep layers, profiles/r2_conv_igemm_fwd_vs_library_bs128.txt).
// This one:
//   * BP x BN tile (256 or 128 pixels x 128 or 64 channels), 4 waves as 2 x 2, wave tile
//     BP/2 x BN/2 (128 x 64: 43 FLOP per LDS byte);
//   * operands go global -> LDS with global_load_lds_dwordx4 (no VGPRs, no ds_write):
//     one wave-instruction fills 8 rows of 128 B, lane l its row l/8 at slot l%8; the
//     XOR swizzle of the LDS image (chunk ^ row&7, the same image the general kernel
//     writes) goes on the per-lane SOURCE address, since the LDS side is lane-linear;
//   * two LDS buffers, ONE barrier per K-step: wait the landed tile (vmcnt(0)) +
//     barrier, issue tile t+1 into the other buffer, MFMA on tile t; every LDS byte
//     lives in one __shared__ array (a second __shared__ object can make hipcc wait
//     vmcnt(0) before each K-step's first LDS read, cdna_hip_programming.md §5);
//   * the epilogue of the general kernel: rounded tile staged through LDS, the next
//     BN's statistics tree, whole-row stores, accumulate / aux for the fused gradients.
template <typename T, int BP, int BN, int NS = 2, int NW = 4>
struct G1x1Lds {
  static constexpr int STAGE = (BP + BN) * BK;            // elements per buffer
  static constexpr int RS = BN + 8;                       // epilogue tile row stride
  static constexpr int TILE = BP * RS * (int)sizeof(T);   // epilogue tile bytes
  static constexpr int RED = TILE;                        // float red[4][2][BN]
  static constexpr int FLAG = RED + NW * 2 * BN * 4;      // int s_flag
  static constexpr int SCR = FLAG + 16;                   // float scr[THR]
  static constexpr int EPI = SCR + 64 * NW * 4;
  static constexpr int MAIN = NS * STAGE * (int)sizeof(T);
  static constexpr int SHIFT = MAIN > EPI ? MAIN : EPI;  // float shift[BN] (statistics only)
  static constexpr int BWC = SHIFT + BN * 4;              // float mean|invstd|gamma|beta [4][BN] (BS)
  static constexpr int BYTES = BWC + 4 * BN * 4;
};

// NS = 3 | 4 (DPA_GLDS_STAGES): three or four LDS buffers, NS - 1 tiles in flight across every barrier --
// the wait is a counted vmcnt (this wave's DMAs of the newest tile stay outstanding) and the
// barrier a raw s_barrier (__syncthreads() would add vmcnt(0)); one workgroup per CU (96 or 128 KB).
//
// NWP x NWC waves (pixels x channels; default 2 x 2 = 256 threads): the wide tiles run 8
// waves -- 256 x 128 (4 x 2) or 256 x 256 (2 x 4, wave tile 128 x 64) -- so each LDS-DMA byte
// feeds 1.33x / 2x the MFMAs of the 128 x 128 tile (its per-K-step cost is the DMA issue:
// profiles/r5b_stage_ab.txt, two or three tiles in flight gained nothing), and the second
// wave on every SIMD hides the first's fragment-read waits.  The wide variants always defer
// the statistics tree (stat_sum1_kernel / stat_tree_kernel).
template <typename T, int BP, int BN, int BS = BS_NONE, bool KXK = false, int NS = 2, int NWP = 2, int NWC = 2>
__global__ void __launch_bounds__(64 * NWP * NWC)
conv_glds_kernel(const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y, StatArgs sa, Geom g,
               BwdStatArgs<T> bs) {
  using MMT = MM<T>;
  constexpr int NW = NWP * NWC, NT = 64 * NW;  // waves, threads
  using L = G1x1Lds<T, BP, BN, NS, NW>;
  static_assert(NS == 2 || ((NS == 3 || NS == 4) && BS == BS_NONE), "3-4 stages: forward / plain data gradients only");
  static_assert(NW == 4 || BS == BS_NONE || BP == 128, "wide pixel tiles: forward / plain data gradients only");
  typedef typename MMT::frag frag;
  constexpr int CT = BN / (16 * NWC);  // 16-channel tiles per wave
  constexpr int PT = BP / (16 * NWP);  // 16-pixel tiles per wave
  constexpr int AR = BP / (8 * NW);    // pixel rows per lane per K-step (8 rows per wave-instruction)
  constexpr int WR = BN / (8 * NW);    // filter rows per lane per K-step
  static_assert(CT >= 1 && PT >= 1 && AR >= 1 && WR >= 1 && AR * 8 * NW == BP && WR * 8 * NW == BN, "tile / waves");
  // the in-launch statistics tree (sum_rows) is written for 256 threads and 2 BN <= 256
  constexpr bool kInTree = NT == THR && 2 * BN <= THR;
  __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];
  T* const lds = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave % NWP, wc = wave / NWP;
  const int nct = g.K / BN;
  const unsigned lid = xcd_tile();  // the nct channel tiles of one pixel tile share an L2
  const long long bm = lid / nct;
  const int bn = (int)(lid % nct);
  const long long p0 = bm * BP;
  const int k0 = bn * BN;
  // this lane's source rows: wave-instruction i covers rows (NW i + wave) * 8 .. + 7, the lane
  // row (lane >> 3) of them, logical chunk (lane & 7) ^ (row & 7) (row & 7 == lane >> 3).
  // KXK: a K-step is one filter tap (r, s) x 64 input channels (C % 64 == 0): the pixel's
  // input row is (n, oh*st - pad + r, ow*st - pad + s) and a padding tap reads the zero
  // page; else (1x1, pad 0) the K-steps walk the pixel's own input row (no bounds checks,
  // no per-step tap arithmetic: the general form costs the 1x1 shapes 5-12 %).
  const int lr = lane >> 3, chunk = (lane & 7) ^ lr;
  unsigned xo[AR], wo[WR];  // element offsets of the pixel rows / (n, ih0, iw0), filter rows (< 2^31)
  int ih0[AR], iw0[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    long long p = p0 + (i * NW + wave) * 8 + lr;
    p = p < g.M ? p : g.M - 1;  // ragged tail: a valid row, its output is not stored
    if constexpr (KXK) {
      const int ow = (int)(p % g.OW);
      const long long t = p / g.OW;
      const int oh = (int)(t % g.OH);
      const int n = (int)(t / g.OH);
      ih0[i] = oh * g.stride - g.pad;
      iw0[i] = ow * g.stride - g.pad;
      xo[i] = (unsigned)((((long long)n * g.H + ih0[i]) * g.W + iw0[i]) * g.C + chunk * 8);
    } else {
      long long r = p;
      if (g.stride != 1) {
        const int ow = (int)(p % g.OW);
        const long long t = p / g.OW;
        const int oh = (int)(t % g.OH);
        const int n = (int)(t / g.OH);
        r = ((long long)n * g.H + (long long)oh * g.stride) * g.W + (long long)ow * g.stride;
      }
      xo[i] = (unsigned)(r * g.C + chunk * 8);
      ih0[i] = iw0[i] = 0;
    }
  }
  const int wrow = KXK ? g.R * g.S * g.C : g.C;
#pragma unroll
  for (int i = 0; i < WR; ++i) wo[i] = (unsigned)((k0 + (i * NW + wave) * 8 + lr) * wrow + chunk * 8);
  const int cpt = g.C / BK;
  const int KT = KXK ? g.R * g.S * cpt : cpt;
  auto issue = [&](int kt, int buf) {
    T* base = lds + buf * L::STAGE;
#pragma unroll
    for (int i = 0; i < WR; ++i)
      glds16(w + wo[i] + kt * BK, base + (i * NW + wave) * 8 * BK);
    if constexpr (KXK) {
      const int rs = kt / cpt, c0 = (kt - rs * cpt) * BK;  // wave-uniform
      const int r = rs / g.S, s = rs - r * g.S;
      const int xk = (r * g.W + s) * g.C + c0;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const bool ok = (unsigned)(ih0[i] + r) < (unsigned)g.H && (unsigned)(iw0[i] + s) < (unsigned)g.W;
        glds16(ok ? (const void*)(x + (int)xo[i] + xk) : (const void*)g_zero16,
               base + (BN + (i * NW + wave) * 8) * BK);
      }
    } else {
#pragma unroll
      for (int i = 0; i < AR; ++i) glds16(x + xo[i] + kt * BK, base + (BN + (i * NW + wave) * 8) * BK);
    }
  };
  f32x4 acc[CT][PT];
#pragma unroll
  for (int a = 0; a < CT; ++a)
#pragma unroll
    for (int b = 0; b < PT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  // the statistics' shift (running mean) rides with tile 0 into LDS: loaded after the K loop
  // it cost every workgroup a dependent global-load latency in its epilogue
  if (BS == BS_NONE && sa.part != nullptr && wave == 0 && lane < BN / 4)
    glds16(sa.shift + k0 + lane * 4, reinterpret_cast<float*>(smem + L::SHIFT));
  // BS: the BN's per-channel constants ride with tile 0 too (wave w: array w), and this
  // lane's epilogue chunks of x (and y, and the accumulated-onto gradient) are loaded into
  // registers now -- they land with tile 0 instead of stalling the epilogue
  constexpr int CPR = BN / 8;     // 16-B chunks per pixel row (epilogue)
  constexpr int RPI = NT / CPR;   // pixel rows per pass
  constexpr int NIT = BS != BS_NONE ? BP / RPI : 1;
  const int ch = tid % CPR;
  f32x4 bxr[NIT], byr[NIT], bor[NIT];
  if constexpr (BS != BS_NONE) {
    if (lane < BN / 4 && (BS == BS_REC ? wave < 4 : wave < 2)) {
      const float* src = wave == 0 ? bs.save + k0 : wave == 1 ? bs.save + g.K + k0 : wave == 2 ? bs.gamma + k0
                                                                                                : bs.beta + k0;
      glds16(src + lane * 4, reinterpret_cast<float*>(smem + L::BWC) + wave * BN);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const long long pp = min(p0 + it * RPI + tid / CPR, g.M - 1);
      const long long o = pp * g.K + k0 + ch * 8;
      bxr[it] = *reinterpret_cast<const f32x4*>(bs.x + o);
      if constexpr (BS == BS_Y) {
        byr[it] = *reinterpret_cast<const f32x4*>(bs.y + o);
        bor[it] = *reinterpret_cast<const f32x4*>(y + o);  // the tapped residual gradient
      }
    }
  }
  issue(0, 0);
  if (NS >= 3 && KT > 1) issue(1, 1);
  if (NS == 4 && KT > 2) issue(2, 2);
  int buf = 0;
  for (int kt = 0; kt < KT; ++kt) {
    if constexpr (NS == 2) {
      buf = kt & 1;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of tile kt has landed
      __syncthreads();  // ... every wave's, and tile kt-1 (the other buffer) is no longer read
      if (kt + 1 < KT) issue(kt + 1, buf ^ 1);
    } else {
      // tile kt landed (the WR + AR DMAs per younger tile of this wave -- up to NS - 2 of
      // them -- may still be in flight); the barrier orders every wave's DMAs of tile kt
      // before any read, and every wave's reads of buffer (kt-1)%NS (tile kt-1, done: its
      // MFMAs have issued) before its refill with tile kt+NS-1
      if (NS == 4 && kt + 2 < KT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (WR + AR)) : "memory");
      else if (kt + 1 < KT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WR + AR) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + NS - 1 < KT) issue(kt + NS - 1, buf == 0 ? NS - 1 : buf - 1);
    }
    const T* A = lds + buf * L::STAGE;  // filter rows [0, BN)
    const T* B = A + BN * BK;           // pixel rows [0, BP)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag fa[CT], fb[PT];
#pragma unroll
      for (int a = 0; a < CT; ++a)
        fa[a] = *reinterpret_cast<const frag*>(A + swz(wc * (BN / NWC) + a * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int b = 0; b < PT; ++b)
        fb[b] = *reinterpret_cast<const frag*>(B + swz(wp * (BP / NWP) + b * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int a = 0; a < CT; ++a)
#pragma unroll
        for (int b = 0; b < PT; ++b) acc[a][b] = MMT::mma(fa[a], fb[b], acc[a][b]);
    }
    if constexpr (NS >= 3) buf = buf == NS - 1 ? 0 : buf + 1;
  }
  __syncthreads();  // the last tile is read: the buffers become the epilogue's tile
  // ---- epilogue (the shared pieces, for a BP-pixel tile) ----
  T* tile = lds;
  float(*red)[2][BN] = reinterpret_cast<float(*)[2][BN]>(smem + L::RED);
  int* s_flag = reinterpret_cast<int*>(smem + L::FLAG);
  float* scr = reinterpret_cast<float*>(smem + L::SCR);
  const float* shl = reinterpret_cast<const float*>(smem + L::SHIFT);
  stage_tile<T, BN>(tile, acc, wc * (BN / NWC), wp * (BP / NWP), fr, fq);
  __syncthreads();
  const bool stats = BS == BS_NONE && sa.part != nullptr;
  // BS: this lane's 8 channels' BN constants, and its running sums of dz, dz * xhat
  float bmu[8], bis[8], bsc[8], bsh[8], bs1[8], bs2[8];
  if constexpr (BS != BS_NONE) {
    const float* bwc = reinterpret_cast<const float*>(smem + L::BWC);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bmu[j] = bwc[ch * 8 + j];
      bis[j] = bwc[BN + ch * 8 + j];
      if (BS == BS_REC) {
        bsc[j] = bwc[2 * BN + ch * 8 + j] * bis[j];
        bsh[j] = fmaf(-bmu[j], bsc[j], bwc[3 * BN + ch * 8 + j]);
      }
      bs1[j] = bs2[j] = 0.f;
    }
  }
  auto store = [&]() {
    store_tile<T, BP, BN, NT, MODE_GEN, BS == BS_Y>(
        tile, y, g, p0, k0, 0, 0, [&](int it) { return bor[BS == BS_Y ? it : 0]; },  // prefetched with tile 0
        [&](int it, const f32x4& raw) {
          if constexpr (BS != BS_NONE) {  // the BN backward sums of the stored (rounded) gradient
            const T* d = reinterpret_cast<const T*>(&raw);
            const T* xv = reinterpret_cast<const T*>(&bxr[it]);
            const T* yv = reinterpret_cast<const T*>(&byr[it]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float xf = Cvt<T>::to_f(xv[j]);
              const bool on = BS == BS_Y ? Cvt<T>::to_f(yv[j]) > 0.f : fmaf(xf, bsc[j], bsh[j]) > 0.f;
              const float z = on ? Cvt<T>::to_f(d[j]) : 0.f;
              bs1[j] += z;
              bs2[j] = fmaf(z, (xf - bmu[j]) * bis[j], bs2[j]);
            }
          }
        });
  };
  // Without statistics, or with the tree deferred to stat_tree_kernel, the stores leave
  // first and drain while the sums are taken from the tile still in LDS; with the
  // in-launch tree they follow the ticket (its vmcnt(0) must not wait for the tile).
  const bool stores_first = !stats || sa.defer || !kInTree;
  if (stores_first) store();
  // this pixel tile's level-1 row of channel tile bn
  auto lvl1_row = [&](long long rows) { return sa.part + ((long long)bn * rows + bm) * (2 * BN); };
  if constexpr (BS != BS_NONE) {  // -> level-1 row (stat_tree_kernel follows)
    reduce_cols<BN>(bs1, bs2, red);
    write_level1<BN, NW>(red, lvl1_row((g.M + BP - 1) / BP), false);
    return;
  }
  bool last1 = false;
  long long rows = 0;
  int grp = 0, gsz = 0;
  if (stats) {
    rows = (g.M + BP - 1) / BP;
    float s1[8], s2[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[j] = shl[ch * 8 + j];
    tile_col_sums<T, BP, BN, NT>(tile, (int)min((long long)BP, g.M - p0) - 1, sh, s1, s2);
    reduce_cols<BN>(s1, s2, red);
    const bool deferred = sa.defer || !kInTree;  // the tree runs in stat_tree_kernel after this launch
    write_level1<BN, NW>(red, lvl1_row(rows), !deferred);
    if (!deferred) {
      grp = (int)(bm / G1);
      gsz = (int)min((long long)G1, rows - (long long)grp * G1);
      last1 = last_arriver(sa.tickets + bn * (int)((rows + G1 - 1) / G1) + grp, (unsigned)gsz, s_flag);
    }
  }
  if (!stores_first) store();
  if (!last1) return;
  if constexpr (kInTree) {  // (wide tiles always defer: last1 is false there)
    __syncthreads();
    tree_in_launch<BN>(sa, g, nct, bn, rows, grp, gsz, scr, &red[0][0][0], s_flag);
  }
}

// The statistics tree of a conv launch with StatArgs.defer: the conv's workgroups stored
// their level-1 partial rows with plain stores and exited (no write-through drain, no
// ticket round trip per workgroup: on a many-round grid that serial hand-off cost each
// workgroup ~3 us, ~30 us per large conv); this launch runs the same two levels --
// workgroup (bn, grp) sums its group of G1 rows into a level-2 row, the last of a
// channel tile's NG arrivals sums those into the final statistics.  Same association
// as the in-launch tree: the result is bitwise the same.
// One-level variant for grids of <= S1_MAXROWS pixel tiles (every ResNet-50 conv but the
// 56x56 ones): a
// workgroup of 1024 lanes owns S1_COLS of the 2*BN level-1 columns of one channel tile as
// 16 row groups x 64 columns, each group with every row it sums in flight (16 loads),
// combined in group order through LDS -- one dependent round trip instead of the two
// levels' three (rows, ticket, level-2 rows).  Fixed order: deterministic.
constexpr int S1_THR = 1024, S1_COLS = 64, S1_RG = S1_THR / S1_COLS, S1_MAXROWS = 1024;
// NL: loads per lane, all in flight (16: up to 256 rows; 64: up to S1_MAXROWS)
template <int BN, int NL>
__global__ void __launch_bounds__(S1_THR) stat_sum1_kernel(StatArgs sa, long long M, int BM_, int K) {
  __shared__ float part[S1_RG][S1_COLS];
  __shared__ uint32_t ep_s;
  const int nct = K / BN, bn = blockIdx.x, c0 = blockIdx.y * S1_COLS;
  const int rows = (int)((M + BM_ - 1) / BM_);
  const int col = threadIdx.x % S1_COLS, rg = threadIdx.x / S1_COLS;
  // SyncBN: every workgroup of this launch finishes 64 columns; its ticket's round trip
  // overlaps the row loads
  const bool xon = sa.xs.active();
  const int xbid = (int)(blockIdx.x + blockIdx.y * gridDim.x);
  unsigned long long tk = 0;
  if (xon && threadIdx.x == 0) tk = xgmi::xsite_ticket(sa.xs, xbid);
  const float* lvl1 = sa.part + (long long)bn * rows * (2 * BN) + c0 + col;
  float v[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int r = rg + u * S1_RG;
    v[u] = lvl1[(long long)(r < rows ? r : 0) * (2 * BN)];
  }
  float a = 0.f;
#pragma unroll
  for (int u = 0; u < NL; ++u)
    if (rg + u * S1_RG < rows) a += v[u];
  part[rg][col] = a;
  if (xon && threadIdx.x == 0) ep_s = xgmi::xsite_epoch(sa.xs, tk, xbid);
  __syncthreads();
  if (xon) xgmi::xsite_advance(sa.xs, ep_s, xbid, S1_THR);
  if (threadIdx.x >= S1_COLS) return;
  float t = 0.f;
#pragma unroll
  for (int g = 0; g < S1_RG; ++g) t += part[g][threadIdx.x];
  const int cc = c0 + threadIdx.x;  // column of [S1 | S2] (or [sum | sumsq])
  const int h = cc / BN, k = bn * BN + cc % BN;
  const bool cnt = !sa.bwd && bn == 0 && cc == 0;  // the lane that writes the row count
  float tg = t, mg = (float)M;
  if (xon) {  // local -> global (rank-ordered sums; the count too)
    const uint32_t ep = ep_s;
    xgmi::xsite_push_at(sa.xs, ep, h * K + k, t);
    if (cnt) xgmi::xsite_push_at(sa.xs, ep, 2 * K, mg);
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    unsigned polls = 0;
    bool fail = false;
    tg = xgmi::xsite_pull_at(sa.xs, ep, h * K + k, t, t0, polls, fail);
    if (cnt) mg = xgmi::xsite_pull_at(sa.xs, ep, 2 * K, mg, t0, polls, fail);
  }
  if (sa.bwd) {  // dbeta / dgamma: this rank's sums (DDP averages them); out: global
    if (h == 0) {
      sa.dbeta[k] = t;
      sa.stats[k] = tg;
    } else {
      sa.dgamma[k] = t;
      sa.stats[K + k] = tg;
    }
    return;
  }
  sa.stats[h * K + k] = tg;
  if (h == 0) sa.stats[2 * K + SHIFT_OFF + k] = sa.shift[k];
  if (cnt) {
    sa.stats[2 * K] = mg;
    if (sa.nbt != nullptr) sa.nbt[0] = sa.nbt[0] + 1;
  }
  (void)nct;
}

template <int BN>
__global__ void __launch_bounds__(THR) stat_tree_kernel(StatArgs sa, long long M, int BM_, int K) {
  __shared__ float scr[THR];
  __shared__ float tot[2 * BN + 1];  // + the row count (SyncBN exchange)
  __shared__ int s_flag;
  const int nct = K / BN;
  const long long rows = (M + BM_ - 1) / BM_;
  const int NG = (int)((rows + G1 - 1) / G1);
  const int bn = (int)(blockIdx.x / NG), grp = (int)(blockIdx.x % NG);
  const int gsz = (int)min((long long)G1, rows - (long long)grp * G1);
  const int k0 = bn * BN, tid = threadIdx.x;
  const Tree tr = Tree::of<BN>(sa, nct, bn, rows);
  if (!tree_level2<BN>(sa, tr, nct, bn, grp, gsz, scr, &s_flag)) return;
  // SyncBN: the nct finishers exchange their slices (ticket round trip behind the level-2 loads)
  const bool xon = sa.xs.active();
  unsigned long long tk = 0;
  if (xon && tid == 0) tk = xgmi::xsite_ticket(sa.xs, bn);
  sum_rows<2 * BN>(tr.lvl2, NG, tot, scr, false);
  if (sa.bwd) {  // BN backward sums: out = [S1 | S2], dbeta = S1, dgamma = S2 (bn_nhwc layout)
    for (int t = tid; t < BN; t += THR) {
      sa.dbeta[k0 + t] = tot[t];  // this rank's (DDP averages them)
      sa.dgamma[k0 + t] = tot[BN + t];
    }
    if (xon) xgmi::xsite_exchange_slice(sa.xs, tot, 2 * BN, [&](int i) { return i < BN ? k0 + i : K + k0 + i - BN; },
                                        tk, bn, THR);
    for (int t = tid; t < BN; t += THR) {
      sa.stats[k0 + t] = tot[t];
      sa.stats[K + k0 + t] = tot[BN + t];
    }
    return;
  }
  __shared__ float cnt[1];
  if (tid == 0) cnt[0] = (float)M;
  if (xon) {
    // the row count rides with finisher 0's slice (position 2K)
    const int n = 2 * BN + (bn == 0 ? 1 : 0);
    if (bn == 0 && tid == 0) tot[2 * BN] = cnt[0];
    xgmi::xsite_exchange_slice(sa.xs, tot, n, [&](int i) { return i < BN ? k0 + i : i < 2 * BN ? K + k0 + i - BN : 2 * K; },
                               tk, bn, THR);
    if (bn == 0 && tid == 0) cnt[0] = tot[2 * BN];
  }
  write_stats<BN>(sa, K, bn, tot, tid == 0 ? cnt[0] : 0.f);  // (lane 0 wrote, and writes, the count)
}

// ---------------------------------------------------------------------------
// Per-step weight packing for every implicit-GEMM conv of a network in ONE launch:
// fp32 OIHW master weights -> the compute-dtype forward filter wf[k][r][s][c] (the
// channels_last layout the kernels read) and, where a data gradient runs on the
// kernel, the flipped transposed filter wd[c][R-1-r][S-1-s][k] (for a 1x1 conv: the
// plain transpose).  64 x 64 (k, c) tiles of one tap through LDS: both writes are
// whole 128-B rows.  Table (int64, 8 per conv): src, wf, wd (0: none), K, C, R*S,
// first tile (prefix over the convs), unused.
template <typename T>
__global__ void __launch_bounds__(256)
pack_weights_kernel(const int64_t* __restrict__ table, int n) {
  __shared__ float tile[64][65];
  const long long t = blockIdx.x;
  int lo = 0, hi = n - 1;  // the conv holding tile t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[8 * mid + 6] <= t) lo = mid; else hi = mid - 1;
  }
  const int64_t* d = table + 8 * lo;
  const float* src = reinterpret_cast<const float*>(d[0]);
  T* wf = reinterpret_cast<T*>(d[1]);
  T* wd = reinterpret_cast<T*>(d[2]);
  const int K = (int)d[3], C = (int)d[4], RS = (int)d[5];
  const long long lt = t - d[6];
  const int rs = (int)(lt % RS);
  const long long kc = lt / RS;
  const int ct = C / 64, k0 = (int)(kc / ct) * 64, c0 = (int)(kc % ct) * 64;
  const int tid = threadIdx.x, cl = tid & 63, rg = tid >> 6;
  float v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = src[((long long)(k0 + rg * 16 + i) * C + c0 + cl) * RS + rs];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int kl = rg * 16 + i;
    wf[((long long)(k0 + kl) * RS + rs) * C + c0 + cl] = Cvt<T>::from_f(v[i]);
    tile[kl][cl] = v[i];
  }
  if (wd == nullptr) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = rg * 16 + i;  // lanes along k
    wd[((long long)(c0 + c) * RS + (RS - 1 - rs)) * K + k0 + cl] = Cvt<T>::from_f(tile[cl][c]);
  }
}

// Stem operands in one launch: the [N][3][H][W] image (fp32 or the compute dtype)
// -> the 4-channel NHWC image [N][H][W][4] (one 8-B store per pixel, 4th channel 0),
// and, in the trailing workgroups, the fp32 [K][3][7][7] filter -> [K][8][8][4] in the
// compute dtype with zeros in the padding (the MODE_STEM K space).
template <typename T, typename S>
__global__ void __launch_bounds__(256)
stem_pack_kernel(const S* __restrict__ x, T* __restrict__ x4, long long npix, int HW, const float* __restrict__ w,
                 T* __restrict__ w4, int K, long long xblocks) {
  if ((long long)blockIdx.x < xblocks) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const long long n = p / HW, hw = p - n * HW;
    const S* src = x + n * 3 * HW + hw;
    T v[4] = {Cvt<T>::from_f(Cvt<S>::to_f(src[0])), Cvt<T>::from_f(Cvt<S>::to_f(src[HW])),
              Cvt<T>::from_f(Cvt<S>::to_f(src[2 * HW])), Cvt<T>::from_f(0.f)};
    *reinterpret_cast<u16x4*>(x4 + p * 4) = *reinterpret_cast<const u16x4*>(v);
    return;
  }
  const int e = (int)((long long)blockIdx.x - xblocks) * 256 + threadIdx.x;
  if (e >= K * 256) return;
  const int k = e >> 8, rem = e & 255, r = rem >> 5, s = (rem >> 2) & 7, c = rem & 3;
  w4[e] = Cvt<T>::from_f(r < 7 && s < 7 && c < 3 ? w[((k * 3 + c) * 7 + r) * 7 + s] : 0.f);
}

// x: [N, 3, H, W] contiguous (fp32 / bf16 / f16); w: fp32 [K, 3, 7, 7]; x4: [N, 4, H, W]
// channels_last, w4: [K, 4, 8, 8] channels_last, both in the compute dtype.
void stem_pack(at::Tensor x, at::Tensor w, at::Tensor x4, at::Tensor w4) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4 && x.size(1) == 3, "stem_pack: x [N, 3, H, W]");
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous() && w.size(1) == 3 && w.size(2) == 7 &&
                  w.size(3) == 7, "stem_pack: fp32 [K, 3, 7, 7] filter");
  TORCH_CHECK(x4.is_contiguous(at::MemoryFormat::ChannelsLast) && x4.size(0) == x.size(0) && x4.size(1) == 4 &&
                  x4.size(2) == x.size(2) && x4.size(3) == x.size(3), "stem_pack: x4 [N, 4, H, W] channels_last");
  TORCH_CHECK(w4.is_contiguous(at::MemoryFormat::ChannelsLast) && w4.size(0) == w.size(0) && w4.size(1) == 4 &&
                  w4.size(2) == 8 && w4.size(3) == 8 && w4.scalar_type() == x4.scalar_type(), "stem_pack: w4");
  TORCH_CHECK(x4.scalar_type() == at::kBFloat16 || x4.scalar_type() == at::kHalf, "stem_pack: bf16 / f16");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == x4.scalar_type(), "stem_pack: x dtype");
  const long long HW = x.size(2) * x.size(3), npix = x.size(0) * HW;
  const int K = (int)w.size(0);
  const long long xblocks = (npix + 255) / 256, wblocks = ((long long)K * 256 + 255) / 256;
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    T* x4p = reinterpret_cast<T*>(x4.data_ptr());
    T* w4p = reinterpret_cast<T*>(w4.data_ptr());
    if (x.scalar_type() == at::kFloat)
      hipLaunchKernelGGL((stem_pack_kernel<T, float>), dim3((unsigned)(xblocks + wblocks)), dim3(256), 0,
                         cur_stream(), x.data_ptr<float>(), x4p, npix, (int)HW, w.data_ptr<float>(), w4p, K, xblocks);
    else
      hipLaunchKernelGGL((stem_pack_kernel<T, T>), dim3((unsigned)(xblocks + wblocks)), dim3(256), 0, cur_stream(),
                         reinterpret_cast<const T*>(x.data_ptr()), x4p, npix, (int)HW, w.data_ptr<float>(), w4p, K,
                         xblocks);
  };
  if (x4.scalar_type() == at::kBFloat16) launch(__hip_bfloat16{}); else launch(__half{});
  DPA_CHECK_LAUNCH();
}

void pack_weights(at::Tensor table, int64_t n, int64_t tiles, int64_t dtype_code) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong && table.numel() >= 8 * n, "pack_weights: table");
  if (tiles <= 0) return;
  if (dtype_code == 0)
    hipLaunchKernelGGL(pack_weights_kernel<__hip_bfloat16>, dim3((unsigned)tiles), dim3(256), 0, cur_stream(),
                       table.data_ptr<int64_t>(), (int)n);
  else
    hipLaunchKernelGGL(pack_weights_kernel<__half>, dim3((unsigned)tiles), dim3(256), 0, cur_stream(),
                       table.data_ptr<int64_t>(), (int)n);
  DPA_CHECK_LAUNCH();
}

LaunchLog& launch_log() {
  static LaunchLog log;
  return log;
}

static int tile_n(int64_t K) { return K % 128 == 0 ? 128 : 64; }

// 1x1 convs on conv_glds_kernel (DPA_G1X1=0: the general kernel, A/B runs); its pixel tile
// forced to 128 | 256 (DPA_G1X1_BP), or 256 from DPA_G1X1_MIN256 workgroups up (256-pixel
// tiles measured slower: off); g1x1_config switches all three at run time for tests and sweeps
static Knob k_g1x1_on{"DPA_G1X1", 1, knob_onoff, true}, k_g1x1_bp{"DPA_G1X1_BP", 0, knob_nonneg},
    k_g1x1_min256{"DPA_G1X1_MIN256", 1LL << 40, knob_nonneg};
// (on, bp, min256) -> previous; a negative argument leaves that setting alone
std::vector<int64_t> g1x1_config(int64_t on, int64_t bp, int64_t min256) {
  return {k_g1x1_on.set(on), k_g1x1_bp.set(bp), k_g1x1_min256.set(min256)};
}
static bool g1x1_enabled() { return k_g1x1_on.get() != 0; }

// LDS buffers of conv_glds_kernel (forward / plain data gradients): 2 (default), 3 or 4
// (DPA_GLDS_STAGES; glds_config(stages) at run time)
static Knob k_glds_stages{"DPA_GLDS_STAGES", 2, [](long long v, long long keep) { return v >= 2 && v <= 4 ? v : keep; }};
int64_t glds_config(int64_t stages) { return k_glds_stages.set(stages); }

// 128-channel tiles of conv_glds_kernel narrowed to 64 when the grid would have fewer than
// this many workgroups (DPA_G1X1_BN64_BELOW; 0 = never; bn64_config at run time)
static Knob k_bn64_below{"DPA_G1X1_BN64_BELOW", 0, knob_nonneg};
int64_t bn64_config(int64_t below) { return k_bn64_below.set(below); }

// KxK convs (any stride / padding) on the glds kernel too (DPA_G3X3=0: 1x1 only, A/B runs)
static Knob k_g3x3_on{"DPA_G3X3", 1, knob_onoff, true};
int64_t g3x3_config(int64_t on) { return k_g3x3_on.set(on); }
static bool g3x3_enabled() { return k_g3x3_on.get() != 0; }

// Measured and not kept (profiles/r5j_wide_ns_ab.txt): the 8-wave 128 x 128 tile with three or
// four LDS stages (two / three tiles in flight, one workgroup per CU) -- no faster even where
// the grid is one workgroup per CU anyway (512 -> 512 3x3 at 7x7: 56.1 vs 57.9 / 58.1 us),
// 23 % slower over the network: the K-loop does not wait on DMA latency (PMC,
// profiles/r5i_conv_pmc.txt: MFMA busy 27-32 %, waits at the barrier / LDS-read counters).
// Wide 8-wave tiles of conv_glds_kernel for the forward / plain data-gradient convs
// (DPA_WIDE; wide_config at run time): 0 off, 1 auto (see wide_pick), 2 force 256 x 128,
// 3 force 256 x 256, 4 force 128 x 128 on 8 waves.  Shapes a forced tile does not fit keep
// the 4-wave kernel.
static Knob k_wide{"DPA_WIDE", 1, knob_nonneg};
int64_t wide_config(int64_t m) { return k_wide.set(m); }
// -> 0 (the 4-wave 128 x 128 / x 64 tiles), 1 (256 x 128), 2 (256 x 256), 3 (128 x 128, 8 waves).
// Auto (profiles/r5c_wide_ab.txt, every ResNet-50 forward shape): 8 waves on the 128 x 128
// tile wherever Cout % 128 == 0 (the second wave on each SIMD hides the other's fragment-read
// waits: network forward convs 2459 -> 2380 us); 256 x 256 where the reduction is deep
// (C R S >= 1024) and the grid still fills the chip (>= 196 workgroups: 40.5 vs 42.9-44.3 us
// on 1024 -> 512 at 14x14).  bs: BN backward sums in the epilogue (128-pixel tiles only).
static int wide_pick(long long M, int64_t K, int64_t CRS, bool bs) {
  const long long m = k_wide.get();
  const long long r256 = (M + 255) / 256;
  const bool ok2 = !bs && K % 256 == 0 && r256 <= S1_MAXROWS;  // the deferred tree: one level at BN = 256
  const bool ok1 = K % 128 == 0;
  if (m == 2) return ok1 && !bs ? 1 : 0;
  if (m == 3) return ok2 ? 2 : 0;
  if (m == 4) return ok1 ? 3 : 0;
  if (m != 1) return 0;
  if (ok2 && CRS >= 1024 && r256 * (K / 256) >= 196) return 2;
  return ok1 ? 3 : 0;
}

// pixel tile of conv_glds_kernel: 256 when the grid still has >= min256 workgroups (default
// 2 per CU: the 96 KB of LDS leave one 256-pixel workgroup per CU), else 128 (64 KB: two
// per CU); DPA_G1X1_BP=128|256 forces one.
static int g1x1_bp(long long M, int64_t K) {
  const long long bp = k_g1x1_bp.get();
  if (bp == 128 || bp == 256) return (int)bp;
  const long long t256 = (M + 255) / 256 * (K / tile_n(K));
  return t256 >= k_g1x1_min256.get() ? 256 : 128;
}

// deferred statistics tree (StatArgs.defer + stat_tree_kernel) for grids of more than
// DPA_STAT_DEFER_MIN workgroups (several rounds per CU: the in-launch hand-off is then paid
// serially by every round); 0 = always (the default: measured 14.73 vs 14.77-14.84 ms at
// 1024), -1 = never; stat_defer_config at run time (-2 leaves it alone)
static Knob k_defer_min{"DPA_STAT_DEFER_MIN", 0, [](long long v, long long keep) { return v >= -1 ? v : keep; }};
int64_t stat_defer_config(int64_t min_blocks) { return k_defer_min.set(min_blocks); }
static bool defer_stats(long long blocks) { return k_defer_min.get() >= 0 && blocks > k_defer_min.get(); }

// The instantiated variants: stat_sum1_kernel <BN, NL>, stat_tree_kernel <BN>
using Sum1Variants = std::tuple<Var<256, 16>, Var<128, 16>, Var<64, 16>, Var<256, S1_MAXROWS / S1_RG>,
                                Var<128, S1_MAXROWS / S1_RG>, Var<64, S1_MAXROWS / S1_RG>>;
using TreeVariants = std::tuple<Var<128>, Var<64>>;

static void launch_stat_tree(StatArgs sa, long long M, int bm, int K, int BN) {
  const long long rows = (M + bm - 1) / bm, NG = (rows + G1 - 1) / G1;
  bool found;
  if (rows <= S1_MAXROWS) {  // one level: every row in flight at once (16 or 64 per lane), no ticket
    const dim3 gr((unsigned)(K / BN), (unsigned)(2 * BN / S1_COLS));
    xgmi::set_site_grid(sa.xs, (long long)gr.x * gr.y, "stat_sum1");  // SyncBN finishers: every workgroup
    const int NL = rows <= 16 * S1_RG ? 16 : S1_MAXROWS / S1_RG;
    found = for_variant(Sum1Variants{}, [&](auto v) {
      using V = decltype(v);
      if (!V::is({BN, NL})) return false;
      note_launch<V>("stat_sum1", "f32");
      hipLaunchKernelGGL((stat_sum1_kernel<V::v[0], V::v[1]>), gr, dim3(S1_THR), 0, cur_stream(), sa, M, bm, K);
      return true;
    });
  } else {
    TORCH_CHECK(BN <= 128, "stat_tree: 256-channel tiles need <= ", S1_MAXROWS, " pixel tiles");
    xgmi::set_site_grid(sa.xs, K / BN, "stat_tree");  // SyncBN finishers: the last arriver of each channel tile
    found = for_variant(TreeVariants{}, [&](auto v) {
      using V = decltype(v);
      if (!V::is({BN})) return false;
      note_launch<V>("stat_tree", "f32");
      hipLaunchKernelGGL(stat_tree_kernel<V::v[0]>, dim3((unsigned)(NG * (K / BN))), dim3(THR), 0, cur_stream(), sa, M,
                         bm, K);
      return true;
    });
  }
  TORCH_CHECK(found, "stat_tree: no kernel variant for ", BN, "-channel tiles");
  DPA_CHECK_LAUNCH();
}

// statistics workspace: level-1 + level-2 partial rows (floats) and tickets (int32)
int64_t stat_part_len(int64_t M, int64_t K) {
  const int64_t rows = (M + BM - 1) / BM, ng = (rows + G1 - 1) / G1;
  return 2 * K * (rows + ng);
}
int64_t stat_tickets_len(int64_t M, int64_t K) {
  const int64_t rows = (M + BM - 1) / BM, ng = (rows + G1 - 1) / G1;
  return (K / 64) * (ng + 1);  // 64-channel tiles at most (conv_glds_kernel may narrow 128 -> 64)
}

// The instantiated variants: conv_fwd_kernel <BN, MODE>, conv_glds_kernel
// <BP, BN, BS, KXK, NS, NWP, NWC>
using FwdVariants = std::tuple<Var<128, MODE_GEN>, Var<64, MODE_GEN>, Var<128, MODE_STEM>, Var<64, MODE_STEM>,
                               Var<128, MODE_S2T>, Var<64, MODE_S2T>>;
using GldsVariants = std::tuple<
    // 4 waves, two LDS buffers: 1x1 (pixel tile 256 | 128) and KxK
    Var<256, 128, BS_NONE, 0, 2, 2, 2>, Var<256, 64, BS_NONE, 0, 2, 2, 2>, Var<128, 128, BS_NONE, 0, 2, 2, 2>,
    Var<128, 64, BS_NONE, 0, 2, 2, 2>, Var<128, 128, BS_NONE, 1, 2, 2, 2>, Var<128, 64, BS_NONE, 1, 2, 2, 2>,
    // three / four LDS buffers
    Var<128, 128, BS_NONE, 0, 3, 2, 2>, Var<128, 64, BS_NONE, 0, 3, 2, 2>, Var<128, 128, BS_NONE, 1, 3, 2, 2>,
    Var<128, 64, BS_NONE, 1, 3, 2, 2>, Var<128, 128, BS_NONE, 0, 4, 2, 2>, Var<128, 64, BS_NONE, 0, 4, 2, 2>,
    Var<128, 128, BS_NONE, 1, 4, 2, 2>, Var<128, 64, BS_NONE, 1, 4, 2, 2>,
    // wide tiles, 8 waves
    Var<256, 128, BS_NONE, 0, 2, 4, 2>, Var<256, 128, BS_NONE, 1, 2, 4, 2>, Var<256, 256, BS_NONE, 0, 2, 2, 4>,
    Var<256, 256, BS_NONE, 1, 2, 2, 4>, Var<128, 128, BS_NONE, 0, 2, 2, 4>, Var<128, 128, BS_NONE, 1, 2, 2, 4>,
    // BN backward sums in the epilogue: 4 waves, and 128 x 128 on 8
    Var<128, 128, BS_Y, 0, 2, 2, 2>, Var<128, 64, BS_Y, 0, 2, 2, 2>, Var<128, 128, BS_Y, 0, 2, 2, 4>,
    Var<128, 128, BS_REC, 0, 2, 2, 2>, Var<128, 64, BS_REC, 0, 2, 2, 2>, Var<128, 128, BS_REC, 0, 2, 2, 4>,
    Var<128, 128, BS_REC, 1, 2, 2, 2>, Var<128, 64, BS_REC, 1, 2, 2, 2>, Var<128, 128, BS_REC, 1, 2, 2, 4>>;

// y: [N, K, OH, OW] channels_last (preallocated).  With `stats` (fp32 [3K+4], the
// bn_nhwc layout), also part / tickets (stat_part_len / stat_tickets_len; tickets
// zero-initialised once), shift (running mean) and nbt: the fused BN statistics.
//
// mode MODE_STEM: x = the stem_pack image [N, 4, H, W], w = [K, 4, 8, 8] (stride 2, pad 3,
// a 7x7 filter); mode MODE_S2T: x = dy [N, Cf, OHf, OWf] of a 3x3 / stride-2 / pad-1 conv,
// w = its flipped transposed filter [Cin, Cf, 3, 3], y = dx [N, Cin, 2 OHf, 2 OWf].
// aux (MODE_GEN, channels_last [N, K, OH/2, OW/2]): added at the even output pixels --
// a stride-2 1x1 conv's data gradient folded into this one's output.
//
// bn_x (1x1, stride 1, on conv_glds_kernel): y is the output gradient of a training BatchNorm
// whose input was bn_x; the epilogue also produces that BN's backward sums (bn_nhwc
// bwd_stats: bn_out = [S1 | S2], bn_dbeta = S1, bn_dgamma = S2) -- bn_y given: the ReLU
// mask comes from the BN's output (and y accumulates onto the tapped residual gradient,
// accumulate = true); else it is recomputed from bn_x with bn_gamma / bn_beta.  bn_save =
// the forward's [mean | invstd]; part / tickets = the statistics workspace.
void conv_fwd(at::Tensor x, at::Tensor w, at::Tensor y, int64_t stride, int64_t pad, c10::optional<at::Tensor> part,
              c10::optional<at::Tensor> tickets, c10::optional<at::Tensor> stats, c10::optional<at::Tensor> shift,
              c10::optional<at::Tensor> nbt, bool accumulate, int64_t mode, c10::optional<at::Tensor> aux,
              c10::optional<at::Tensor> bn_x, c10::optional<at::Tensor> bn_y, c10::optional<at::Tensor> bn_save,
              c10::optional<at::Tensor> bn_gamma, c10::optional<at::Tensor> bn_beta,
              c10::optional<at::Tensor> bn_out, c10::optional<at::Tensor> bn_dgamma,
              c10::optional<at::Tensor> bn_dbeta, std::shared_ptr<xgmi::XgmiComm> xc) {
  TORCH_CHECK(x.is_cuda() && w.is_cuda() && y.is_cuda(), "conv_fwd: device tensors");
  TORCH_CHECK(x.scalar_type() == w.scalar_type() && x.scalar_type() == y.scalar_type(), "conv_fwd: one dtype");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "conv_fwd: bf16 / f16");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast) && w.is_contiguous(at::MemoryFormat::ChannelsLast) &&
                  y.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv_fwd: channels_last x / w / y");
  launch_log().clear();
  const char* dn = dtype_name(x);
  Geom g = geom(x, w, (int)stride, (int)pad);
  g.accumulate = accumulate ? 1 : 0;
  TORCH_CHECK(mode == MODE_GEN || mode == MODE_STEM || mode == MODE_S2T, "conv_fwd: mode");
  if (mode == MODE_STEM) {
    TORCH_CHECK(g.C == 4 && w.size(1) == 4 && g.R == 8 && g.S == 8 && stride == 2 && pad == 3 && g.K % 64 == 0,
                "conv_fwd: stem needs the stem_pack operands (x [N,4,H,W], w [K,4,8,8]), stride 2, pad 3");
    g.R = g.S = 7;
    g.OH = (g.H + 2 * g.pad - 7) / 2 + 1;
    g.OW = (g.W + 2 * g.pad - 7) / 2 + 1;
    g.M = (long long)g.N * g.OH * g.OW;
  } else {
    TORCH_CHECK(w.size(1) == g.C && supported(g.C, g.K), "conv_fwd: needs C % 64 == 0 and Cout % 64 == 0");
  }
  if (mode == MODE_S2T) {
    TORCH_CHECK(g.R == 3 && g.S == 3 && stride == 2 && pad == 1, "conv_fwd: the S2T mode is a 3x3/s2/p1 dgrad");
    g.OH = g.H;
    g.OW = g.W;
    g.M = (long long)g.N * g.OH * g.OW;
    g.cls_rows = (g.M + BM - 1) / BM;
    TORCH_CHECK(y.size(0) == g.N && y.size(1) == g.K && y.size(2) == 2 * g.OH && y.size(3) == 2 * g.OW,
                "conv_fwd: S2T dx must be [N, Cin, 2 OHf, 2 OWf]");
    TORCH_CHECK(!stats.has_value() && !aux.has_value(), "conv_fwd: S2T has no statistics / aux");
  } else {
    TORCH_CHECK(y.size(0) == g.N && y.size(1) == g.K && y.size(2) == g.OH && y.size(3) == g.OW, "conv_fwd: y shape");
  }
  if (aux.has_value()) {
    TORCH_CHECK(mode == MODE_GEN && g.OH % 2 == 0 && g.OW % 2 == 0 && aux->scalar_type() == y.scalar_type() &&
                    aux->is_contiguous(at::MemoryFormat::ChannelsLast) && aux->size(0) == g.N &&
                    aux->size(1) == g.K && aux->size(2) == g.OH / 2 && aux->size(3) == g.OW / 2,
                "conv_fwd: aux must be [N, K, OH/2, OW/2] channels_last in y's dtype");
    g.aux = aux->data_ptr();
  }
  const bool st = stats.has_value();
  const bool bwdst = bn_x.has_value();
  TORCH_CHECK(!(st && accumulate), "conv_fwd: statistics of an accumulated output are not supported");
  if (bwdst) {
    TORCH_CHECK(mode == MODE_GEN && g.stride == 1 && g1x1_enabled() && x.numel() < (1LL << 31) &&
                    w.numel() < (1LL << 31) && ((g.R == 1 && g.S == 1 && g.pad == 0) || g3x3_enabled()),
                "conv_fwd: BN backward sums need the LDS-DMA kernel (stride 1)");
    TORCH_CHECK(bn_y.has_value() || !accumulate, "conv_fwd: recomputed-mask BN sums on an accumulated output");
    TORCH_CHECK(!st && !aux.has_value() && part.has_value() && tickets.has_value(),
                "conv_fwd: BN backward sums take part / tickets and no forward statistics / aux");
    TORCH_CHECK(accumulate == bn_y.has_value(), "conv_fwd: bn_y (ReLU after a residual) goes with accumulate");
    TORCH_CHECK(bn_save.has_value() && bn_out.has_value() && bn_dgamma.has_value() && bn_dbeta.has_value() &&
                    (bn_y.has_value() || (bn_gamma.has_value() && bn_beta.has_value())),
                "conv_fwd: BN backward sums need save / out / dgamma / dbeta (+ gamma / beta to recompute)");
    auto rows_like_y = [&](const at::Tensor& t) {
      return t.scalar_type() == y.scalar_type() && t.is_contiguous(at::MemoryFormat::ChannelsLast) &&
             t.sizes() == y.sizes();
    };
    TORCH_CHECK(rows_like_y(*bn_x) && (!bn_y.has_value() || rows_like_y(*bn_y)), "conv_fwd: bn_x / bn_y like y");
    for (const at::Tensor* t : {&*bn_save, &*bn_out})
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() >= 2 * g.K, "conv_fwd: bn f32");
    for (const at::Tensor* t : {&*bn_dgamma, &*bn_dbeta})
      TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == g.K, "conv_fwd: bn dgamma / dbeta");
    if (!bn_y.has_value())
      TORCH_CHECK(bn_gamma->scalar_type() == at::kFloat && bn_gamma->numel() == g.K && bn_beta->numel() == g.K,
                  "conv_fwd: bn gamma / beta");
    TORCH_CHECK(part->scalar_type() == at::kFloat && part->numel() >= stat_part_len(g.M, g.K) &&
                    tickets->scalar_type() == at::kInt && tickets->numel() >= stat_tickets_len(g.M, g.K),
                "conv_fwd: statistics workspace");
  }
  TORCH_CHECK(st == shift.has_value() && (bwdst || (st == part.has_value() && st == tickets.has_value())),
              "conv_fwd: part, tickets, stats and shift go together");
  StatArgs sa{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  if (st) {
    TORCH_CHECK(part->scalar_type() == at::kFloat && part->numel() >= stat_part_len(g.M, g.K), "conv_fwd: part size");
    TORCH_CHECK(tickets->scalar_type() == at::kInt && tickets->numel() >= stat_tickets_len(g.M, g.K),
                "conv_fwd: tickets size");
    TORCH_CHECK(stats->scalar_type() == at::kFloat && stats->numel() >= 3 * g.K + 4, "conv_fwd: stats size");
    TORCH_CHECK(shift->scalar_type() == at::kFloat && shift->numel() == g.K, "conv_fwd: shift size");
    sa.part = part->data_ptr<float>();
    sa.tickets = reinterpret_cast<unsigned*>(tickets->data_ptr<int>());
    sa.stats = stats->data_ptr<float>();
    sa.shift = shift->data_ptr<float>();
    sa.nbt = nbt.has_value() ? nbt->data_ptr<int64_t>() : nullptr;
  }
  // SyncBN inside the statistics finishers: they run in the deferred tree launch
  if (xc) {
    TORCH_CHECK(st || bwdst, "conv_fwd: xc (SyncBN site) goes with statistics");
    TORCH_CHECK(2 * g.K + 1 <= xgmi::kWideVals, "conv_fwd: SyncBN site row holds 2K+1 <= ", xgmi::kWideVals);
    sa.xs = xc->wide_site();
  }
  const int BN0 = tile_n(g.K);
  if (mode == MODE_GEN && g1x1_enabled() && x.numel() < (1LL << 31) && w.numel() < (1LL << 31) &&
      (g3x3_enabled() || (g.R == 1 && g.S == 1 && g.pad == 0))) {
    // the glds-staged implicit-GEMM kernel (pixel tile 256 or 128, see g1x1_bp; 64-channel
    // tiles when 128-channel ones leave the grid below DPA_G1X1_BN64_BELOW workgroups)
    const int wide = wide_pick(g.M, g.K, (int64_t)g.C * g.R * g.S, bwdst);
    int BP = (bwdst || !(g.R == 1 && g.S == 1 && g.pad == 0)) ? 128 : g1x1_bp(g.M, g.K);
    int BN = BN0 == 128 && BP == 128 && (g.M + 127) / 128 * (g.K / 128) < k_bn64_below.get() ? 64 : BN0;
    if (wide == 1 || wide == 2) BP = 256;
    if (wide == 1 || wide == 3) BN = 128;
    if (wide == 2) BN = 256;
    if (wide == 3) BP = 128;
    const long long blocks = (g.M + BP - 1) / BP * (g.K / BN);
    TORCH_CHECK(blocks < (1LL << 31), "conv_fwd: grid too large");
    sa.defer = st && (defer_stats(blocks) || xc || wide) ? 1 : 0;
    if (bwdst) {  // the BN backward sums: level-1 rows in the conv, the tree after it
      sa.part = part->data_ptr<float>();
      sa.tickets = reinterpret_cast<unsigned*>(tickets->data_ptr<int>());
      sa.stats = bn_out->data_ptr<float>();
      sa.dgamma = bn_dgamma->data_ptr<float>();
      sa.dbeta = bn_dbeta->data_ptr<float>();
      sa.bwd = 1;
      sa.defer = 1;
    }
    // the tile configuration <BP, BN, BS, KXK, NS, NWP, NWC>.  Waves: the wide tiles run 8
    // (256 x 128 as 4 x 2, the others 2 x 4).  BS_Y stays on 4 waves unless forced
    // (DPA_WIDE=4): its epilogue prefetches three operand rows, and 8 waves measured +218 us
    // over the network's 12 launches (profiles/r5d_resnet50_steady_wide.txt).  Three / four
    // LDS buffers (one workgroup per CU): the 4-wave 128-pixel tiles without BN sums.
    const bool kxk = !(g.R == 1 && g.S == 1 && g.pad == 0);  // KxK: tap-walking loader (128-pixel tiles)
    TORCH_CHECK(!(bwdst && kxk && bn_y.has_value()), "conv_fwd: KxK BN sums take the recomputed mask");
    const int BS = !bwdst ? BS_NONE : bn_y.has_value() ? BS_Y : BS_REC;
    const bool w8 = wide != 0 && !(BS == BS_Y && !(wide == 3 && k_wide.get() == 4));
    const int NWP = w8 && wide == 1 ? 4 : 2, NWC = w8 ? 8 / NWP : 2;
    const long long stages = k_glds_stages.get();
    const int NS = !wide && !bwdst && BP == 128 && (stages == 3 || stages == 4) ? (int)stages : 2;
    auto launch = [&](auto tag) {
      using T = decltype(tag);
      BwdStatArgs<T> bs;
      if (bwdst) {
        bs.x = reinterpret_cast<const T*>(bn_x->data_ptr());
        bs.y = bn_y.has_value() ? reinterpret_cast<const T*>(bn_y->data_ptr()) : nullptr;
        bs.save = bn_save->data_ptr<float>();
        bs.gamma = bn_gamma.has_value() ? bn_gamma->data_ptr<float>() : nullptr;
        bs.beta = bn_beta.has_value() ? bn_beta->data_ptr<float>() : nullptr;
      }
      return for_variant(GldsVariants{}, [&](auto v) {
        using V = decltype(v);
        if (!V::is({BP, BN, BS, kxk, NS, NWP, NWC})) return false;
        note_launch<V>("glds", dn);
        hipLaunchKernelGGL((conv_glds_kernel<T, V::v[0], V::v[1], V::v[2], V::v[3] != 0, V::v[4], V::v[5], V::v[6]>),
                           dim3((unsigned)blocks), dim3(64 * NWP * NWC), 0, cur_stream(),
                           reinterpret_cast<const T*>(x.data_ptr()), reinterpret_cast<const T*>(w.data_ptr()),
                           reinterpret_cast<T*>(y.data_ptr()), sa, g, bs);
        return true;
      });
    };
    const bool found = x.scalar_type() == at::kBFloat16 ? launch(__hip_bfloat16{}) : launch(__half{});
    TORCH_CHECK(found, "conv_fwd: no glds kernel variant for tile ", BP, " x ", BN, " (BS ", BS, ", KxK ", kxk, ", ",
                NS, " stages, ", NWP, " x ", NWC, " waves)");
    DPA_CHECK_LAUNCH();
    if (sa.defer) launch_stat_tree(sa, g.M, BP, (int)g.K, BN);
    return;
  }
  TORCH_CHECK(!bwdst, "conv_fwd: BN backward sums need the 1x1 kernel");
  const int BN = BN0;
  const long long rows = (g.M + BM - 1) / BM;
  const long long blocks = rows * (g.K / BN) * (mode == MODE_S2T ? 4 : 1);
  TORCH_CHECK(blocks < (1LL << 31), "conv_fwd: grid too large");
  sa.defer = st && (defer_stats(blocks) || xc) ? 1 : 0;
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    return for_variant(FwdVariants{}, [&](auto v) {
      using V = decltype(v);
      if (!V::is({BN, (int)mode})) return false;
      note_launch<V>("fwd", dn);
      hipLaunchKernelGGL((conv_fwd_kernel<T, V::v[0], V::v[1]>), dim3((unsigned)blocks), dim3(THR), 0, cur_stream(),
                         reinterpret_cast<const T*>(x.data_ptr()), reinterpret_cast<const T*>(w.data_ptr()),
                         reinterpret_cast<T*>(y.data_ptr()), sa, g);
      return true;
    });
  };
  const bool found = x.scalar_type() == at::kBFloat16 ? launch(__hip_bfloat16{}) : launch(__half{});
  TORCH_CHECK(found, "conv_fwd: no kernel variant for ", BN, "-channel tiles, mode ", mode);
  DPA_CHECK_LAUNCH();
  if (sa.defer) launch_stat_tree(sa, g.M, BM, (int)g.K, BN);
}

// [(family, template arguments, dtype)] of the kernels the last conv_fwd / conv_wgrad call launched
static std::vector<std::tuple<std::string, std::vector<int64_t>, std::string>> last_launch() {
  std::vector<std::tuple<std::string, std::vector<int64_t>, std::string>> out;
  LaunchLog& L = launch_log();
  std::lock_guard<std::mutex> lk(L.mu);
  for (int i = 0; i < L.n; ++i)
    out.emplace_back(L.rec[i].family, std::vector<int64_t>(L.rec[i].v, L.rec[i].v + L.rec[i].n), L.rec[i].dtype);
  return out;
}
// family -> the template arguments of every instantiated variant (from the dispatch tuples)
static std::map<std::string, std::vector<std::vector<int64_t>>> variants() {
  return {{"fwd", variant_list(FwdVariants{})},        {"glds", variant_list(GldsVariants{})},
          {"stat_sum1", variant_list(Sum1Variants{})}, {"stat_tree", variant_list(TreeVariants{})},
          {"wgrad", wgrad_variants(false)},            {"wgrad_glds", wgrad_variants(true)}};
}

}  // namespace igemm

void register_conv_igemm(pybind11::module& m) {
  auto s = m.def_submodule("conv_igemm", "NHWC implicit-GEMM convolution on MFMA (+ fused BN statistics)");
  s.def("conv_fwd", &igemm::conv_fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("y"),
        pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("part") = pybind11::none(),
        pybind11::arg("tickets") = pybind11::none(), pybind11::arg("stats") = pybind11::none(),
        pybind11::arg("shift") = pybind11::none(), pybind11::arg("nbt") = pybind11::none(),
        pybind11::arg("accumulate") = false, pybind11::arg("mode") = 0, pybind11::arg("aux") = pybind11::none(),
        pybind11::arg("bn_x") = pybind11::none(), pybind11::arg("bn_y") = pybind11::none(),
        pybind11::arg("bn_save") = pybind11::none(), pybind11::arg("bn_gamma") = pybind11::none(),
        pybind11::arg("bn_beta") = pybind11::none(), pybind11::arg("bn_out") = pybind11::none(),
        pybind11::arg("bn_dgamma") = pybind11::none(), pybind11::arg("bn_dbeta") = pybind11::none(),
        pybind11::arg("xc") = pybind11::none());
  s.def("last_launch", &igemm::last_launch);
  s.def("variants", &igemm::variants);
  s.def("supported", &igemm::supported);
  s.def("stat_part_len", &igemm::stat_part_len);
  s.def("stat_tickets_len", &igemm::stat_tickets_len);
  s.def("conv_wgrad", &igemm::conv_wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("grad"),
        pybind11::arg("stride"), pybind11::arg("pad"), pybind11::arg("slab"), pybind11::arg("mode") = 0,
        pybind11::arg("reduce") = true);
  s.def("wgrad_reduce_batch", &igemm::wgrad_reduce_batch);
  s.def("wgrad_waves_config", &igemm::wgrad_waves_config, pybind11::arg("waves") = -1);
  s.def("stem_pack", &igemm::stem_pack);
  s.attr("MODE_STEM") = igemm::MODE_STEM;
  s.attr("MODE_S2T") = igemm::MODE_S2T;
  s.def("pack_weights", &igemm::pack_weights);
  s.def("wgrad_splits", &igemm::wgrad_splits);
  s.def("wgrad_fixup_config", &igemm::wgrad_fixup_config, pybind11::arg("maxsp") = -1);
  s.def("wgrad_config", &igemm::wgrad_config, pybind11::arg("glds") = -1);
  s.def("g3x3_config", &igemm::g3x3_config, pybind11::arg("on") = -1);
  s.def("glds_config", &igemm::glds_config, pybind11::arg("stages") = -1);
  s.def("wide_config", &igemm::wide_config, pybind11::arg("mode") = -1);
  s.def("bn64_config", &igemm::bn64_config, pybind11::arg("below") = -1);
  s.def("stat_defer_config", &igemm::stat_defer_config, pybind11::arg("min_blocks") = -2);
  s.def("g1x1_config", &igemm::g1x1_config, pybind11::arg("on") = -1, pybind11::arg("bp") = -1,
        pybind11::arg("min256") = -1);
}

}  // namespace dpa
