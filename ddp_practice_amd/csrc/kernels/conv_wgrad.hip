// NHWC implicit-GEMM weight gradients on MFMA for the ResNet-50 stress config: the
// weight-gradient half of kernels/conv_igemm.hip (its header comment has the geometry the
// two halves share), a translation unit of its own so the two compile side by side.
#include "kernels/conv_igemm.h"

namespace dpa {
namespace igemm {

// ---------------------------------------------------------------------------
// Weight gradient:  dW[k][r][s][c] = sum_p dy[p][k] * x[n][oh*st+r-pad][ow*st+s-pad][c]
// GEMM M = Cout, N = R*S*C, reduction over the pixels p -- both operands are stored
// pixel-major, so they are staged in LDS as [64 pixels][cols] rows and read TRANSPOSED
// into the MFMA operands with ds_read_b64_tr_b16 (each 16-lane group: 4 pixel rows x
// 16 columns; two reads make a lane's 8 consecutive pixels).  Row chunks are XOR-
// swizzled by 2*f(row), f(row) = (row&3) | ((row>>1)&4): the 8 rows one 32-lane half
// reads map to 8 distinct chunk pairs (conflict-free with 16 chunks per row).
// Split over the pixels: S partial fp32 tiles -> wgrad_reduce_kernel, which also
// writes the fp32 OIHW gradient directly (no separate layout/cast pass).
typedef __attribute__((ext_vector_type(4))) short v4s;

// With 8 chunks per row (128-B rows: 64-channel tiles) one 32-lane half reads rows
// {0..3, 8..11} (+4, +32kk), the even ones in one bank half: their 4 chunk pairs must
// differ, so the XOR there is 2*f8(row), f8 = bit 1 | bit 3 of the row (was 2*(row&3):
// rows r and r+8 shared a pair, 2-way -- 1.6 conflict cycles per LDS instruction in the
// 64-wide wgrad kernels, profiles/r3s2l_resnet50_pmc_pass1.txt).
template <int CH>
__device__ __forceinline__ int wswz_xor(int row) {
  if constexpr (CH >= 16) return 2 * ((row & 3) | ((row >> 1) & 4));
  return 2 * (((row >> 1) & 1) | ((row >> 2) & 2));
}

template <int CH>  // 16-B chunks per LDS row
__device__ __forceinline__ int wswz(int row, int chunk) {
  return row * CH * 8 + ((chunk ^ wswz_xor<CH>(row)) << 3);
}

// transposed fragment: 8 consecutive pixel rows (32kk + 8g .. +7) of column cb + (lane & 15)
template <typename T, int CH>
__device__ __forceinline__ typename MM<T>::frag trfrag(const T* base, int kk, int cb, int lane) {
  const int grp = lane >> 4, gi = lane & 15, q = gi >> 2, pq = gi & 3;
  const int row = 32 * kk + 8 * grp + q, col = cb + 4 * pq;
  const T* a0 = base + wswz<CH>(row, col >> 3) + (col & 7);
  const T* a1 = base + wswz<CH>(row + 4, col >> 3) + (col & 7);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a0);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)a1);
  typedef __attribute__((ext_vector_type(8))) short v8s;
  const v8s v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename MM<T>::frag, v);
}

template <typename T, int BM, int BN, int MODE = MODE_GEN>
__global__ void __launch_bounds__(THR)
conv_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ slab, Geom g, int splits,
                  long long pps) {
  typedef typename MM<T>::frag frag;
  constexpr int BP = 64;                 // pixels per K-step
  constexpr int CHA = BM / 8, CHB = BN / 8;
  constexpr int LA = BP * CHA / THR, LB = BP * CHB / THR;  // 16-B loads per thread
  constexpr int MT = BM / 32, NT = BN / 32;
  __shared__ __attribute__((aligned(16))) T lds[2][BP * (BM + BN)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int RSC = MODE == MODE_STEM ? 256 : g.R * g.S * g.C;  // stem: [8][8][4] padded columns
  const int tm = g.K / BM, tn = RSC / BN, tiles = tm * tn;
  const unsigned lid = xcd_tile();
  const int sp = (int)(lid / tiles), tile = (int)(lid % tiles);
  const int k0 = (tile / tn) * BM, n0 = (tile % tn) * BN;
  const int rs = n0 / g.C, c0 = n0 - rs * g.C, fr_ = rs / g.S, fs_ = rs - fr_ * g.S;
  const long long pa = sp * pps, pb = min(g.M, pa + pps);
  const int steps = (int)((pb - pa + BP - 1) / BP);
  f32x4 ra[LA], rb[LB];
  auto gload = [&](int t) {
    const long long pbase = pa + (long long)t * BP;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int e = i * THR + tid, row = e / CHA, cc = e % CHA;
      const long long p = pbase + row;
      ra[i] = p < pb ? *reinterpret_cast<const f32x4*>(dy + p * g.K + k0 + cc * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int e = i * THR + tid, row = e / CHB, cc = e % CHB;
      const long long p = pbase + row;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (p < pb) {
        const unsigned pu = (unsigned)p, q = pu / (unsigned)g.OW;  // M < 2^31 (host check)
        const int ow = (int)(pu - q * (unsigned)g.OW);
        const unsigned n = q / (unsigned)g.OH;
        const int oh = (int)(q - n * (unsigned)g.OH);
        if constexpr (MODE == MODE_STEM) {
          // column n0 + 8cc: taps (r, s), (r, s + 1) of the [8][8][4] padded filter space
          const int col = n0 + cc * 8, r = col >> 5, s = (col >> 2) & 7;
          const int ih = oh * g.stride + r - g.pad, iw = ow * g.stride + s - g.pad;
          const bool rok = r < 7 && (unsigned)ih < (unsigned)g.H;
          const T* px_ = x + (((long long)n * g.H + ih) * g.W + iw) * 4;
          f32x2 lo = {0.f, 0.f}, hi = {0.f, 0.f};
          if (rok && (unsigned)iw < (unsigned)g.W) lo = *reinterpret_cast<const f32x2*>(px_);
          if (rok && s + 1 < 7 && (unsigned)(iw + 1) < (unsigned)g.W) hi = *reinterpret_cast<const f32x2*>(px_ + 4);
          v = f32x4{lo[0], lo[1], hi[0], hi[1]};
        } else {
          const int ih = oh * g.stride + fr_ - g.pad, iw = ow * g.stride + fs_ - g.pad;
          if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
            v = *reinterpret_cast<const f32x4*>(x + (((long long)n * g.H + ih) * g.W + iw) * g.C + c0 + cc * 8);
        }
      }
      rb[i] = v;
    }
  };
  auto lstore = [&](int buf) {
    T* A = lds[buf];
    T* B = lds[buf] + BP * BM;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int e = i * THR + tid;
      *reinterpret_cast<f32x4*>(A + wswz<CHA>(e / CHA, e % CHA)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int e = i * THR + tid;
      *reinterpret_cast<f32x4*>(B + wswz<CHB>(e / CHB, e % CHB)) = rb[i];
    }
  };
  const int grp = lane >> 4, gi = lane & 15;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (steps > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    const int buf = t & 1;
    if (t + 1 < steps) gload(t + 1);
    const T* A = lds[buf];
    const T* B = lds[buf] + BP * BM;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag fa[MT], fb[NT];
#pragma unroll
      for (int a = 0; a < MT; ++a)
        fa[a] = trfrag<T, CHA>(A, kk, wm * (BM / 2) + a * 16, lane);
#pragma unroll
      for (int b = 0; b < NT; ++b)
        fb[b] = trfrag<T, CHB>(B, kk, wn * (BN / 2) + b * 16, lane);
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = MM<T>::mma(fa[a], fb[b], acc[a][b]);
    }
    if (t + 1 < steps) lstore(buf ^ 1);
    __syncthreads();
  }
  // partial tile: C[m = k][n = (r,s,c)]; lane: col n = lane & 15, rows 4*(lane>>4) + j
  float* out = slab + (long long)sp * g.K * RSC;
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = k0 + wm * (BM / 2) + a * 16 + 4 * grp + j, n = n0 + wn * (BN / 2) + b * 16 + gi;
        out[(long long)m * RSC + n] = acc[a][b][j];
      }
}

// The same weight gradient with both operand tiles staged global -> LDS by LDS-DMA
// (MODE_GEN): no VGPR staging and no ds_write_b128 pass (the register-staged loop pays
// ~13 LDS cycles per KiB written).  A wave-instruction fills 64/CH whole rows of the
// [64 pixels][CH chunks] image, lane l row l / CH at slot l % CH; the wswz swizzle goes on
// the per-lane source address (logical chunk = slot ^ xor(row)); padding taps and pixels
// past the split's end read a 16-B zero page instead of being zero-filled by the loader.
// One barrier per 64-pixel step: wait the landed step (vmcnt(0)) + barrier, issue step
// t+1 into the other buffer, MFMA on step t (as conv_glds_kernel).

// NWM x NWN waves (default 2 x 2; 2 x 4 = 8 waves, DPA_WGRAD_WAVES=8: the second wave on
// every SIMD hides the other's transposed-read waits, as the forward's 8-wave tiles do).
// FIX (DPA_WGRAD_FIXUP_MAXSP, opt-in): the split-K reduction in this launch -- partial
// tiles stored write-through, one ticket per output tile, and the tile's last arriver sums
// the splits in split order and writes the fp32 OIHW gradient (no wgrad_reduce launch).
template <typename T, int BM, int BN, int NWM = 2, int NWN = 2, bool FIX = false>
__global__ void __launch_bounds__(64 * NWM * NWN)
conv_wgrad_glds_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ slab, Geom g,
                       int splits, long long pps, float* __restrict__ grad, unsigned* __restrict__ tickets) {
  typedef typename MM<T>::frag frag;
  constexpr int BP = 64;
  constexpr int CHA = BM / 8, CHB = BN / 8;
  constexpr int NW = NWM * NWN;
  constexpr int IA = CHA / NW, IB = CHB / NW;  // wave-instructions per wave per step
  constexpr int MT = BM / (16 * NWM), NT = BN / (16 * NWN);
  static_assert(IA >= 1 && IB >= 1 && IA * NW == CHA && IB * NW == CHB && MT >= 1 && NT >= 1, "tile / waves");
  constexpr int STAGE = BP * (BM + BN);
  __shared__ __attribute__((aligned(16))) T lds[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % NWM, wn = wave / NWM;
  const int RSC = g.R * g.S * g.C;
  const int tm = g.K / BM, tn = RSC / BN, tiles = tm * tn;
  const unsigned lid = xcd_tile();
  const int sp = (int)(lid / tiles), tile = (int)(lid % tiles);
  const int k0 = (tile / tn) * BM, n0 = (tile % tn) * BN;
  const int rs = n0 / g.C, c0 = n0 - rs * g.C, fr_ = rs / g.S, fs_ = rs - fr_ * g.S;
  const long long pa = sp * pps, pb = min(g.M, pa + pps);
  const int steps = (int)((pb - pa + BP - 1) / BP);
  const bool plain = g.R == 1 && g.S == 1 && g.stride == 1 && g.pad == 0;  // x rows = pixels
  // this lane's rows and source chunks (row = (i*4 + wave) * (64/CH) + lane / CH)
  const int ra = lane / CHA, rb = lane / CHB;
  auto issue = [&](int t, int buf) {
    T* A = lds + buf * STAGE;
    T* B = A + BP * BM;
    const long long pbase = pa + (long long)t * BP;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
      const int row = (i * NW + wave) * (64 / CHA) + ra;
      const int ck = (lane % CHA) ^ wswz_xor<CHA>(row);
      const long long p = pbase + row;
      const void* src = p < pb ? (const void*)(dy + p * g.K + k0 + ck * 8) : (const void*)g_zero16;
      glds16(src, A + (i * NW + wave) * (64 / CHA) * BM);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      const int row = (i * NW + wave) * (64 / CHB) + rb;
      const int ck = (lane % CHB) ^ wswz_xor<CHB>(row);
      const long long p = pbase + row;
      const void* src = g_zero16;
      if (p < pb) {
        if (plain) {
          src = x + p * g.C + c0 + ck * 8;
        } else {
          const unsigned pu = (unsigned)p, q = pu / (unsigned)g.OW;  // M < 2^31 (host check)
          const int ow = (int)(pu - q * (unsigned)g.OW);
          const unsigned n = q / (unsigned)g.OH;
          const int oh = (int)(q - n * (unsigned)g.OH);
          const int ih = oh * g.stride + fr_ - g.pad, iw = ow * g.stride + fs_ - g.pad;
          if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
            src = x + (((long long)n * g.H + ih) * g.W + iw) * g.C + c0 + ck * 8;
        }
      }
      glds16(src, B + (i * NW + wave) * (64 / CHB) * BN);
    }
  };
  const int grp = lane >> 4, gi = lane & 15;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (steps > 0) issue(0, 0);
  for (int t = 0; t < steps; ++t) {
    const int buf = t & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < steps) issue(t + 1, buf ^ 1);
    const T* A = lds + buf * STAGE;
    const T* B = A + BP * BM;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      frag fa[MT], fb[NT];
#pragma unroll
      for (int a = 0; a < MT; ++a)
        fa[a] = trfrag<T, CHA>(A, kk, wm * (BM / NWM) + a * 16, lane);
#pragma unroll
      for (int b = 0; b < NT; ++b)
        fb[b] = trfrag<T, CHB>(B, kk, wn * (BN / NWN) + b * 16, lane);
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = MM<T>::mma(fa[a], fb[b], acc[a][b]);
    }
  }
  float* out = slab + (long long)sp * g.K * RSC;
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = k0 + wm * (BM / NWM) + a * 16 + 4 * grp + j, n = n0 + wn * (BN / NWN) + b * 16 + gi;
        if constexpr (FIX) st_wt(out + (long long)m * RSC + n, acc[a][b][j]);
        else out[(long long)m * RSC + n] = acc[a][b][j];
      }
  if constexpr (FIX) {
    __shared__ int s_flag;
    // (last_arriver: this wave's write-through stores drained, one ticket per workgroup)
    if (!last_arriver(tickets + tile, (unsigned)splits, &s_flag)) return;
    // the tile's splits in split order, 8 loads in flight per lane; consecutive lanes take
    // consecutive columns (channels of one tap: unit-stride OIHW writes on a 1x1 conv)
    const long long plane = (long long)g.K * RSC;
    const int st = g.R * g.S;
    for (int e = tid; e < BM * BN; e += 64 * NW) {
      const int r = e / BN, cn = e - r * BN;
      const long long off = (long long)(k0 + r) * RSC + n0 + cn;
      float t = 0.f;
      int s0 = 0;
      for (; s0 + 8 <= splits; s0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld_wt(slab + (s0 + u) * plane + off);
#pragma unroll
        for (int u = 0; u < 8; ++u) t += v[u];
      }
      for (; s0 < splits; ++s0) t += ld_wt(slab + s0 * plane + off);
      const int n = n0 + cn, c = n % g.C, rs = n / g.C;  // (r*S + s)*C + c
      grad[((long long)(k0 + r) * g.C + c) * st + rs] = t;
    }
  }
}

constexpr int WR_QC = 16;  // float4 columns per wgrad_reduce_kernel workgroup

// grad[k][c][r][s] (fp32 OIHW) = sum over splits of slab[sp][k][(r*S + s)*C + c]:
// a workgroup owns 64 consecutive slab columns as 16 float4 quads x 16 split groups
// (every 4th split, fixed order, 4 loads in flight), combined through LDS in group
// order, written in the OIHW order of a [K][Cd][Rd][Sd] gradient (Cd <= C, Rd <= R,
// Sd <= S: the stem's padded columns are dropped here).
// `blk`: this workgroup's 64-column block of the [K][R*S*C] slab plane.
__device__ __forceinline__ void wgrad_reduce_block(const float* __restrict__ slab, float* __restrict__ grad,
                                                   long long blk, int splits, int K, int C, int R, int S, int Cd,
                                                   int Rd, int Sd) {
  // 16 float4 columns x 16 split groups per workgroup (was 64 x 4: a grid of ~150
  // workgroups whose lanes each waited ~6 dependent rounds of 4 loads)
  constexpr int QC = WR_QC, SG = 256 / WR_QC;
  __shared__ f32x4 part[SG][QC];
  const long long RSC = (long long)R * S * C, total = (long long)K * RSC;
  const int qd = threadIdx.x % QC, rg = threadIdx.x / QC;
  const long long col = (blk * QC + qd) * 4;  // total % 4 == 0 (C % 64 == 0)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (col < total) {
    int sp = rg;
    for (; sp + 3 * SG < splits; sp += 4 * SG) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(slab + (long long)sp * total + col);
      const f32x4 b = *reinterpret_cast<const f32x4*>(slab + (long long)(sp + SG) * total + col);
      const f32x4 c = *reinterpret_cast<const f32x4*>(slab + (long long)(sp + 2 * SG) * total + col);
      const f32x4 d = *reinterpret_cast<const f32x4*>(slab + (long long)(sp + 3 * SG) * total + col);
      acc += a;
      acc += b;
      acc += c;
      acc += d;
    }
    for (; sp < splits; sp += SG) acc += *reinterpret_cast<const f32x4*>(slab + (long long)sp * total + col);
  }
  part[rg][qd] = acc;
  __syncthreads();
  if (rg == 0 && col < total) {
    f32x4 t = part[0][qd];
#pragma unroll
    for (int gg = 1; gg < SG; ++gg) t += part[gg][qd];
    const int k = (int)(col / RSC);
    const long long n = col - (long long)k * RSC;  // (r*S + s)*C + c, c % 4 == 0
    const int c = (int)(n % C), rs = (int)(n / C), r = rs / S, s = rs - r * S;
    if (r < Rd && s < Sd) {
      float* o = grad + (((long long)k * Cd + c) * Rd + r) * Sd + s;
      const int st = Rd * Sd;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < Cd) o[j * st] = t[j];
    }
  }
}

__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ grad, int splits, int K, int C, int R, int S,
                    int Cd, int Rd, int Sd) {
  wgrad_reduce_block(slab, grad, blockIdx.x, splits, K, C, R, S, Cd, Rd, Sd);
}

// The same reduction for a whole backward pass's weight gradients in ONE launch
// (ops/conv_igemm.WgradBatch): every conv left its split partials in a slab of its own, and
// at the end of the backward one grid covers all of them -- instead of one small, tail-bound
// launch per conv (53 launches, ~9 us each on ResNet-50: profiles/r5a_rn_steady.txt).  The
// entries ride in the kernel arguments by value (graph-capturable, no table upload); a
// workgroup finds its entry by its block index (prefix blk0).  Same per-block association
// as wgrad_reduce_kernel: bitwise the same gradients.
constexpr int WB_MAX = 48;
struct WBEntry {
  const float* slab;
  float* grad;
  int splits, K, C, R, S, Cd, Rd, Sd;
  long long blk0;  // first block of this entry
};
struct WBList {
  int n;
  WBEntry e[WB_MAX];
};

__global__ void __launch_bounds__(256) wgrad_reduce_batch_kernel(WBList L) {
  const long long b = blockIdx.x;
  int lo = 0, hi = L.n - 1;  // the entry holding block b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.e[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const WBEntry& E = L.e[lo];
  wgrad_reduce_block(E.slab, E.grad, b - E.blk0, E.splits, E.K, E.C, E.R, E.S, E.Cd, E.Rd, E.Sd);
}

// weight gradients on conv_wgrad_glds_kernel: DPA_WGRAD_GLDS = 1 the 1x1 convs, 2 (default)
// every MODE_GEN conv, 0 none (the register-staged kernel); wgrad_config sets it at run time.
// 2 (3x3 included, with 8-wave workgroups): network wgrad 2600 vs 2668 us (1x1 only) vs 2760
// (4 waves): profiles/r5d_wgrad_ab.txt
static Knob k_wgrad_glds{"DPA_WGRAD_GLDS", 2, knob_nonneg};
int64_t wgrad_config(int64_t glds) { return k_wgrad_glds.set(glds); }
// waves per workgroup of conv_wgrad_glds_kernel: 8 (default) or 4 (DPA_WGRAD_WAVES;
// wgrad_waves_config).  8: network wgrad 2668 vs 2760 us
static Knob k_wgrad_waves{"DPA_WGRAD_WAVES", 8, [](long long v, long long keep) { return v == 4 || v == 8 ? v : keep; }};
int64_t wgrad_waves_config(int64_t w) { return k_wgrad_waves.set(w); }

// wgrad tile shapes: BM | Cout, BN | C (a column tile stays inside one filter tap)
static int wtile(int64_t v) { return v % 128 == 0 ? 128 : 64; }

// In-launch split-K reduction (conv_wgrad_glds_kernel FIX) for convs of at most
// DPA_WGRAD_FIXUP_MAXSP splits (default 0: off; wgrad_fixup_config sets it).  Measured
// slower on ResNet-50 at every bound -- 13.77 ms off, 14.02 at 8 splits, 14.74 at 32, 17.69
// for every conv (profiles/r6v_wgrad_fixup_ab.txt): the partial tiles' write-through stores
// and each tile's serial last-arriver sum cost more than the separate, fully parallel launch.  Tickets: one
// zeroed device array per device, re-armed by every tile's last arriver; allocated outside
// any capture (a first use inside one takes the reduce launch instead).
static Knob k_fix_maxsp{"DPA_WGRAD_FIXUP_MAXSP", 0, knob_nonneg};
int64_t wgrad_fixup_config(int64_t maxsp) { return k_fix_maxsp.set(maxsp); }
constexpr int kFixTickets = 4096;
static unsigned* fix_tickets(long long tiles) {
  static unsigned* per_dev[64] = {};
  if (tiles > kFixTickets) return nullptr;
  int dev = 0;
  DPA_CHECK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return nullptr;
  if (per_dev[dev] == nullptr) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    DPA_CHECK_HIP(hipStreamIsCapturing(cur_stream(), &st));
    if (st != hipStreamCaptureStatusNone) return nullptr;
    unsigned* p = nullptr;
    DPA_CHECK_HIP(hipMalloc(&p, kFixTickets * sizeof(unsigned)));
    DPA_CHECK_HIP(hipMemset(p, 0, kFixTickets * sizeof(unsigned)));
    DPA_CHECK_HIP(hipDeviceSynchronize());
    per_dev[dev] = p;
  }
  return per_dev[dev];
}

int64_t wgrad_splits(int64_t M, int64_t K, int64_t C, int64_t R, int64_t S) {
  // ~2 workgroups per CU, each at least 16 K-steps of 64 pixels, and the fp32
  // partials at most ~48 MB (written and re-read once: ~12 us at HBM rate)
  const int64_t tiles = (K / wtile(K)) * (R * S * C / wtile(C));
  // ResNet-50 sweeps: blocks 384 15.01, 512 14.50, 768 14.59, 1024 14.67 ms; pixels per split
  // (round 6 re-sweep, profiles/r6bb_rn_wgrad_minpix.txt) 1024 13.81, 512 13.73, 384 13.74, 256 13.72 ms
  static Knob k_target{"DPA_WGRAD_BLOCKS", 512, knob_any}, k_minpix{"DPA_WGRAD_MINPIX", 512, knob_any};
  const int64_t target = k_target.get(), minpix = k_minpix.get();
  int64_t sp = std::max<int64_t>(1, target / tiles);
  sp = std::min<int64_t>(sp, std::max<int64_t>(1, M / minpix));
  sp = std::min<int64_t>(sp, std::max<int64_t>(1, (12LL << 20) / (K * R * S * C)));
  return sp;
}

// The instantiated variants: conv_wgrad_kernel <BM, BN, MODE>, conv_wgrad_glds_kernel
// <BM, BN, NWM, NWN, FIX>
using WgradVariants = std::tuple<Var<128, 64, MODE_STEM>, Var<64, 64, MODE_STEM>, Var<128, 128, MODE_GEN>,
                                 Var<128, 64, MODE_GEN>, Var<64, 128, MODE_GEN>, Var<64, 64, MODE_GEN>>;
using WgradGldsVariants =
    std::tuple<Var<128, 128, 2, 4, 1>, Var<128, 64, 4, 2, 1>, Var<64, 128, 2, 4, 1>, Var<64, 64, 2, 4, 1>,
               Var<128, 128, 2, 4, 0>, Var<128, 64, 4, 2, 0>, Var<64, 128, 2, 4, 0>, Var<64, 64, 2, 4, 0>,
               Var<128, 128, 2, 2, 0>, Var<128, 64, 2, 2, 0>, Var<64, 128, 2, 2, 0>, Var<64, 64, 2, 2, 0>>;

std::vector<std::vector<int64_t>> wgrad_variants(bool glds) {
  return glds ? variant_list(WgradGldsVariants{}) : variant_list(WgradVariants{});
}

// dy: [N, K, OH, OW] channels_last; x: [N, C, H, W] channels_last; grad: fp32 [K, C, R, S]
// contiguous (written, not accumulated); slab: fp32 >= splits * K * R*S*C.
// mode MODE_STEM: x = the stem_pack image [N, 4, H, W], grad [K, 3, 7, 7] (stride 2, pad 3).
std::vector<int64_t> conv_wgrad(at::Tensor dy, at::Tensor x, at::Tensor grad, int64_t stride, int64_t pad,
                                at::Tensor slab, int64_t mode, bool reduce) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && grad.is_cuda() && slab.is_cuda(), "conv_wgrad: device tensors");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf),
              "conv_wgrad: bf16 / f16 activations");
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast) && x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv_wgrad: channels_last dy / x");
  TORCH_CHECK(grad.scalar_type() == at::kFloat && grad.is_contiguous() && grad.dim() == 4, "conv_wgrad: fp32 grad");
  const bool stem = mode == MODE_STEM;
  TORCH_CHECK(mode == MODE_GEN || stem, "conv_wgrad: mode");
  launch_log().clear();
  const char* dn = dtype_name(x);
  Geom g = geom(x, grad, (int)stride, (int)pad);
  int Cd = g.C, Rd = g.R, Sd = g.S;  // gradient dims (the stem's padded K space drops to these)
  if (stem) {
    TORCH_CHECK(x.size(1) == 4 && grad.size(1) == 3 && g.R == 7 && g.S == 7 && stride == 2 && pad == 3 &&
                    g.K % 64 == 0, "conv_wgrad: stem needs the stem_pack image and a [K, 3, 7, 7] gradient");
    g.C = 4;
    Cd = 3;
  } else {
    TORCH_CHECK(grad.size(1) == g.C && supported(g.C, g.K), "conv_wgrad: needs C % 64 == 0 and Cout % 64 == 0");
  }
  TORCH_CHECK(dy.size(0) == g.N && dy.size(1) == g.K && dy.size(2) == g.OH && dy.size(3) == g.OW, "conv_wgrad: dy");
  TORCH_CHECK(g.M < (1LL << 31), "conv_wgrad: too many pixels");
  const int SR = stem ? 8 : g.R, SS = stem ? 8 : g.S;  // slab column space [SR][SS][C]
  const int64_t sp = wgrad_splits(g.M, g.K, g.C, SR, SS);
  const int64_t RSC = (int64_t)SR * SS * g.C;
  TORCH_CHECK(slab.scalar_type() == at::kFloat && slab.numel() >= sp * g.K * RSC, "conv_wgrad: slab too small");
  const long long pps = ((g.M + sp - 1) / sp + 63) / 64 * 64;
  const int BM = wtile(g.K), BN = wtile(g.C);
  const long long blocks = sp * (g.K / BM) * (RSC / BN);
  // in-launch split-K reduction: 8-wave LDS-DMA kernels, reduced gradients wanted
  // 1x1 (mode 1) or every MODE_GEN conv (mode 2, default): on 3x3 it measured ~5 % slower
  const long long mglds = k_wgrad_glds.get();
  const bool glds = !stem && ((g.R == 1 && g.S == 1 && mglds >= 1) || mglds == 2);
  const bool w8 = glds && k_wgrad_waves.get() == 8;
  unsigned* tk = nullptr;
  const bool fixed = reduce && w8 && sp <= k_fix_maxsp.get() && (tk = fix_tickets((g.K / BM) * (RSC / BN))) != nullptr;
  // the tile configuration: 8 waves as 2 x 4 (4 x 2 on the 128 x 64 tile), 4 waves as 2 x 2
  const int NWM = w8 && BM == 128 && BN == 64 ? 4 : 2, NWN = w8 ? 8 / NWM : 2;
  auto launch = [&](auto tag) {
    using T = decltype(tag);
    const T* dp = reinterpret_cast<const T*>(dy.data_ptr());
    const T* xp = reinterpret_cast<const T*>(x.data_ptr());
    float* sl = slab.data_ptr<float>();
    const dim3 gr((unsigned)blocks);
    if (glds)
      return for_variant(WgradGldsVariants{}, [&](auto v) {
        using V = decltype(v);
        if (!V::is({BM, BN, NWM, NWN, fixed})) return false;
        note_launch<V>("wgrad_glds", dn);
        hipLaunchKernelGGL((conv_wgrad_glds_kernel<T, V::v[0], V::v[1], V::v[2], V::v[3], V::v[4] != 0>), gr,
                           dim3(64 * NWM * NWN), 0, cur_stream(), dp, xp, sl, g, (int)sp, pps, grad.data_ptr<float>(), tk);
        return true;
      });
    return for_variant(WgradVariants{}, [&](auto v) {
      using V = decltype(v);
      if (!V::is({BM, BN, stem ? MODE_STEM : MODE_GEN})) return false;
      note_launch<V>("wgrad", dn);
      hipLaunchKernelGGL((conv_wgrad_kernel<T, V::v[0], V::v[1], V::v[2]>), gr, dim3(THR), 0, cur_stream(), dp, xp, sl,
                         g, (int)sp, pps);
      return true;
    });
  };
  const bool found = x.scalar_type() == at::kBFloat16 ? launch(__hip_bfloat16{}) : launch(__half{});
  TORCH_CHECK(found, "conv_wgrad: no kernel variant for tile ", BM, " x ", BN);
  DPA_CHECK_LAUNCH();
  // reduce = false: the slab stays for wgrad_reduce_batch (the geometry below is its entry)
  std::vector<int64_t> geo{sp, g.K, g.C, SR, SS, Cd, Rd, Sd};
  if (!reduce || fixed) return geo;
  const long long total = (long long)g.K * RSC;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 4 * WR_QC - 1) / (4 * WR_QC))), dim3(256), 0,
                     cur_stream(),
                     slab.data_ptr<float>(), grad.data_ptr<float>(), (int)sp, g.K, g.C, SR, SS, Cd, Rd, Sd);
  DPA_CHECK_LAUNCH();
  return geo;
}

// One launch reducing every (slab, grad) pair of a backward pass (conv_wgrad with reduce =
// false; geo = the geometry it returned), WB_MAX entries per launch.
void wgrad_reduce_batch(std::vector<at::Tensor> slabs, std::vector<at::Tensor> grads,
                        std::vector<std::vector<int64_t>> geos) {
  TORCH_CHECK(slabs.size() == grads.size() && slabs.size() == geos.size(), "wgrad_reduce_batch: one geometry per pair");
  for (size_t s0 = 0; s0 < slabs.size(); s0 += WB_MAX) {
    WBList L{};
    long long blk = 0;
    const size_t e = std::min(slabs.size(), s0 + (size_t)WB_MAX);
    for (size_t i = s0; i < e; ++i) {
      const auto& q = geos[i];
      TORCH_CHECK(q.size() == 8, "wgrad_reduce_batch: geometry {splits, K, C, R, S, Cd, Rd, Sd}");
      const long long total = q[1] * q[3] * q[4] * q[2];
      TORCH_CHECK(slabs[i].is_cuda() && slabs[i].scalar_type() == at::kFloat && slabs[i].numel() >= q[0] * total,
                  "wgrad_reduce_batch: slab");
      TORCH_CHECK(grads[i].is_cuda() && grads[i].scalar_type() == at::kFloat && grads[i].is_contiguous() &&
                      grads[i].numel() == q[1] * q[5] * q[6] * q[7], "wgrad_reduce_batch: fp32 OIHW grad");
      WBEntry& E = L.e[i - s0];
      E.slab = slabs[i].data_ptr<float>();
      E.grad = grads[i].data_ptr<float>();
      E.splits = (int)q[0]; E.K = (int)q[1]; E.C = (int)q[2]; E.R = (int)q[3]; E.S = (int)q[4];
      E.Cd = (int)q[5]; E.Rd = (int)q[6]; E.Sd = (int)q[7];
      E.blk0 = blk;
      blk += (total + 4 * WR_QC - 1) / (4 * WR_QC);
    }
    L.n = (int)(e - s0);
    if (blk == 0) continue;
    hipLaunchKernelGGL(wgrad_reduce_batch_kernel, dim3((unsigned)blk), dim3(256), 0, cur_stream(), L);
    DPA_CHECK_LAUNCH();
  }
}

}  // namespace igemm
}  // namespace dpa
