// Fused "conv block" kernels for the ConvNet hot path:
//     Conv2d(CIN->COUT, 5x5, stride 1, pad 2) -> BatchNorm2d -> ReLU -> MaxPool2d(2,2)
// (the reference model: origin_main.py:12-23, ddp_main.py:16-27).
//
// Forward (train):  [conv_fwd: implicit-GEMM MFMA + bias + per-workgroup BN partial sums -> fslab]
//                   -> (SyncBN: one all-reduce of fslab, host side)
//                   -> [bn_relu_pool: reduce fslab, running-stat update,
//                       normalise, ReLU, 2x2 max-pool, argmax index]
// Backward:         [bwd_reduce: pool/ReLU routing + per-channel partial sum(dy), sum(dy*xhat) -> bslab]
//                   -> (SyncBN: one all-reduce of bslab)
//                   -> [bwd_elemt: BN input-grad at full resolution]
//                   -> [conv_wgrad: MFMA per image chunk -> wslab]
//                   -> [grad_reduce: wslab -> dW, db ; bslab -> dgamma, dbeta]
//                   -> [conv_fwd<DGRAD>: input grad = conv of dy with flipped W^T]
//
// Design notes (MI355X):
//  * Everything here is latency-bound (per-step GEMMs are 20-160 MFLOP): few
//    launches, one LDS round trip per operand, >= 64 workgroups per launch.
//  * No float atomics and no zero-fill launches: every cross-workgroup sum is
//    a per-workgroup partial row ("slab") reduced by its consumer kernel.
//    (Contended atomics — every workgroup adding into the same few hundred
//    addresses — serialise at the memory side; the first version of this file
//    spent 32 us per wgrad on them.)  Deterministic as a bonus.
//  * im2col never touches HBM: the input image (with halo) sits in LDS in
//    HWC order so that 8 K-consecutive elements (8 input channels of one tap)
//    are one 16-B ds_read; conv1 (CIN=1) gathers its 25 taps element-wise.
//  * wgrad keeps 5 kw-shifted copies of the input in LDS so that the B operand
//    (8 consecutive output columns of one tap) is again one aligned 16-B read.
//  * BN statistics are sums around a per-channel shift (the running mean,
//    identical on every rank) to avoid E[x^2]-E[x]^2 cancellation; partial
//    sums + counts make SyncBN ONE all-reduce with no device->host mask sync
//    (cf. torch/nn/modules/_functions.py:74-101).
//
// This header: the BatchNorm side (all the classifier head needs).  conv5x5.h: the forward / data-gradient
// kernel.  conv5x5_wgrad.h: the weight gradient and the slab column sums.  convblock.hip: the per-layer op's kernels.
#pragma once
#include "common.h"
#include "comm/xsite.h"

namespace dpa {
namespace cb {

constexpr int NTHR = 256;

// The head's packed fc weights (conv5x5.h pack_fc writes them, convnet_head.hip head_row_kernel
// PK reads them): [FCP_LANES][NM][8] elements, NM = fcp_nm(N) the class count the head's
// register tiles are sized for.
constexpr int FCP_K = 32 * 49, FCP_LANES = 256, FCP_IT = (FCP_K + FCP_LANES - 1) / FCP_LANES;
static_assert(FCP_IT == 7, "a head lane's features of one class fit one 16-B granule of 8");
__host__ __device__ constexpr int fcp_nm(int N) { return N > 10 ? 16 : 10; }
__host__ __device__ constexpr int fcp_len(int NM) { return FCP_LANES * NM * 8; }

// Final statistics buffer written by bn_relu_pool (read by the backward):
// [0,C) sum(y-shift) | [C,2C) sum((y-shift)^2) | [2C] count | [2C+1,3C+1) shift
__host__ __device__ constexpr int stats_len(int C) { return 3 * C + 1; }
// forward partial-sum row per conv workgroup: [sum(C) | sumsq(C) | count]
__host__ __device__ constexpr int fslab_row(int C) { return 2 * C + 1; }

// The big LDS tiles of a launch that hosts several roles (conv5x5_body / conv5x5_wgrad_body DYN)
extern __shared__ __attribute__((aligned(16))) unsigned char dpa_dyn_lds[];

// Workgroups per image of the FUSED conv2 forward (convnet_fused.hip conv2_fwd; the per-layer
// op keeps SH<1>::SPLIT, conv5x5.h), per storage type.  Here because its consumer, the head's BN2
// finalize (convnet_head.hip), sizes its one load batch by the slab's B * split rows.
// 4 for every type: with row windows (conv5x5_body WR) a quarter's 9 input rows are ONE staging
// iteration per lane where a half's 10 need two, and each wave runs one m-tile instead of two;
// bf16 step 0.0426 -> 0.0409 ms (profiles/conv2_rowwin_ab.txt; with every split staging the
// whole image, 4 was 0.6 us slower: r6m_split_ab.txt).
// Experiment builds: -DDPA_FWD2_SPLIT=2|4 (bf16 / fp16), -DDPA_FWD2_SPLIT_F32=...
#ifndef DPA_FWD2_SPLIT
#define DPA_FWD2_SPLIT 4
#endif
#ifndef DPA_FWD2_SPLIT_F32
#define DPA_FWD2_SPLIT_F32 4
#endif
template <typename T>
constexpr int kFwd2SplitT = sizeof(T) == 4 ? DPA_FWD2_SPLIT_F32 : DPA_FWD2_SPLIT;

template <typename F>  // f(T{}) for the activation storage dtype (host side)
static void with_t(DT dt, F&& f) {
  switch (dt) {
    case DT::F32: f(float{}); break;
    case DT::BF16: f(__hip_bfloat16{}); break;
    case DT::F16: f(__half{}); break;
  }
}

// ---------------------------------------------------------------------------
// Staging helpers.  Every global->LDS staging loop is split into "issue every
// load into registers" then "convert + scatter into LDS", with compile-time
// trip counts so all of a thread's loads are in flight together: one L2
// round trip per staging phase instead of one per loop iteration (the loop
// form cost 20+ us per kernel in the first profile).
// ---------------------------------------------------------------------------
// f32 array of N elements (N % 4 == 0, 16-B aligned) -> sink(e, v) per element
template <int N, typename Sink>
__device__ __forceinline__ void stage_f32(const float* __restrict__ src, Sink&& sink) {
  static_assert(N % 4 == 0, "N must be a multiple of 4");
  constexpr int N4 = N / 4;
  constexpr int IT = (N4 + NTHR - 1) / NTHR;
  f32x4 v[IT];
  const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * NTHR;
    if (e < N4) v[i] = s4[e];
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * NTHR;
    if (e < N4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sink(4 * e + j, v[i][j]);
    }
  }
}

// [C][H][W] image of T (W even) -> sink(c, h, w, v_w, v_w+1) per element pair
template <typename T> struct Pair2 { typedef uint32_t type; };
template <> struct Pair2<float> { typedef uint64_t type; };
template <typename T, int C, int H, int W, typename Sink>
__device__ __forceinline__ void stage_chw(const T* __restrict__ src, Sink&& sink) {
  static_assert(W % 2 == 0, "W must be even");
  typedef typename Pair2<T>::type P;
  constexpr int NP = C * H * W / 2;
  constexpr int IT = (NP + NTHR - 1) / NTHR;
  P v[IT];
  const P* s2 = reinterpret_cast<const P*>(src);
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * NTHR;
    if (e < NP) v[i] = s2[e];
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * NTHR;
    if (e < NP) {
      const int pe = 2 * e;
      const int c = pe / (H * W), rem = pe % (H * W);
      T a, b;
      __builtin_memcpy(&a, &v[i], sizeof(T));
      __builtin_memcpy(&b, reinterpret_cast<const char*>(&v[i]) + sizeof(T), sizeof(T));
      sink(c, rem / W, rem % W, a, b);
    }
  }
}

// ---------------------------------------------------------------------------
// BatchNorm finalize, shared by bn_relu_pool and the fused prologues of the
// next layer's kernel (ops/convnet_fused.py).  train: reduce the conv's
// per-workgroup partial sums (nrows x (2C+1), L2-resident), publish the final
// sums to fstats and update running stats on the leader workgroup; eval: use
// the running stats.  Leaves per-channel y*sc + sh coefficients in LDS.
// ---------------------------------------------------------------------------
struct BNParams {
  const float* fslab;
  int nrows;
  float* fstats;
  const float* gamma;
  const float* beta;
  float* rmean;
  float* rvar;
  int64_t* nbt;
  float momentum;
  float eps;
  int train;
  xgmi::XSite xs;  // active: SyncBN sums exchanged in here (comm/xsite.h), fslab holds local rows
};

// Sum of src[r * RL + j] over rows r = g, g + G, ...: up to RSUM_U rows per
// lane are loaded in ONE batch (all loads in flight before the first add), so
// a slab of up to RSUM_U * G rows costs one L2 round trip instead of one per
// 4 rows (the partial-sum slabs are 64-256 rows: this was 3-5 serial trips).
// U: the batch size, a template parameter (RSUM_U unless the caller knows its slab is taller:
// the adds stay in row order g, g + G, ..., so the sum does not depend on U).
constexpr int RSUM_U = 24;
template <int U = RSUM_U, typename F>
__device__ __forceinline__ float strided_rowsum(const float* __restrict__ src, int rows, int RL, int j, int g, int G,
                                                F&& after_issue) {
  // The first batch is peeled out of the loop (at a loop header hipcc waits vmcnt(0) for the
  // previous iteration's loads, which on entry also waited for every load the kernel had
  // issued before), and the loads are unconditional (clamped row, masked by a multiply: a
  // conditional load was branched around and its add waited right behind it) -- so the whole
  // batch is issued behind the kernel's earlier loads instead of a round trip after them.
  float acc = 0.f;
  auto batch = [&](int base, bool first) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int rr = base + u * G;
      v[u] = src[(size_t)min(rr, rows - 1) * RL + j] * (rr < rows ? 1.f : 0.f);
    }
    if (first) after_issue();  // e.g. an atomic whose round trip then overlaps these loads
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u];
  };
  batch(g, true);
  for (int base = g + U * G; base < rows; base += U * G) batch(base, false);
  return acc;
}
__device__ __forceinline__ float strided_rowsum(const float* __restrict__ src, int rows, int RL, int j, int g, int G) {
  return strided_rowsum(src, rows, RL, j, g, G, [] {});
}

// part: >= NTHR floats of LDS; ends with __syncthreads().  Every caller runs NTHR-thread
// workgroups: the constant, not blockDim.x -- on gfx950 blockDim is a load from the hidden
// kernel arguments, and the s_waitcnt vmcnt(0) before its use waited for every load the
// kernel had issued so far (a whole memory round trip ahead of the slab loads, head .s).
// U: rows per lane of the slab reduction's one load batch (strided_rowsum).
template <int C, int U = RSUM_U>
__device__ __forceinline__ void bn_finalize(const BNParams& bp, float* sc_s, float* beta_s, float* mean_s,
                                            float* istd_s, float* part, int bid) {
  const int tid = threadIdx.x, nthr = NTHR;
  const bool leader = bid == 0;  // writes fstats / running stats (and pushes the SyncBN row)
  if (bp.train) {
    constexpr int RL = 2 * C + 1;
    const int G = nthr / RL;
    const int j = tid % RL, g = tid / RL;
    // per-channel parameters first: their loads overlap the slab reduction's
    float gam = 0.f, bet = 0.f, shf = 0.f, rm = 0.f, rv = 0.f;
    if (tid < C) {
      gam = bp.gamma[tid];
      bet = bp.beta[tid];
      shf = bp.fstats[2 * C + 1 + tid];
      if (leader) {
        rm = bp.rmean[tid];
        rv = bp.rvar[tid];
      }
    }
    const int64_t nb0 = leader ? bp.nbt[0] : 0;
    const bool xon = bp.xs.active();
    unsigned long long tk = 0;
    // the SyncBN ticket is taken right after the slab loads are issued: its round trip overlaps
    // theirs (taken before them, its returned value's wait held the loads back)
    auto ticket = [&] {
      if (xon && tid == 0) tk = xgmi::xsite_ticket(bp.xs, bid);
    };
    if (g < G) {
      part[tid] = strided_rowsum<U>(bp.fslab, bp.nrows, RL, j, g, G, ticket);
    } else {
      ticket();
      part[tid] = 0.f;
    }
    DPA_STAMP(11);
    __syncthreads();
    DPA_STAMP(12);
    if (tid < RL) {
      float t = 0.f;
      for (int gg = 0; gg < G; ++gg) t += part[gg * RL + tid];
      part[tid] = t;  // only this thread reads slot tid (its gg = 0 term) before the write
    }
    __syncthreads();
    if (xon) xgmi::xsite_exchange(bp.xs, part, RL, tk, bid);  // local -> global sums (SyncBN)
    if (tid < C) {
      const float n = part[2 * C];
      const float m1 = part[tid] / n;
      const float mean = shf + m1;
      const float var = fmaxf(part[C + tid] / n - m1 * m1, 0.f);
      const float istd = rsqrtf(var + bp.eps);
      const float s = gam * istd;
      sc_s[tid] = s;
      beta_s[tid] = bet;
      mean_s[tid] = mean;
      istd_s[tid] = istd;
      if (leader) {
        bp.fstats[tid] = part[tid];
        bp.fstats[C + tid] = part[C + tid];
        if (tid == 0) bp.fstats[2 * C] = n;
        const int64_t nb = nb0 + 1;
        const float mom = bp.momentum >= 0.f ? bp.momentum : 1.f / (float)nb;
        bp.rmean[tid] = (1.f - mom) * rm + mom * mean;
        bp.rvar[tid] = (1.f - mom) * rv + mom * var * (n / fmaxf(n - 1.f, 1.f));
      }
    }
    __syncthreads();
    if (leader && tid == 0) bp.nbt[0] = nb0 + 1;
  } else {
    if (tid < C) {
      const float istd = rsqrtf(bp.rvar[tid] + bp.eps);
      const float s = bp.gamma[tid] * istd;
      sc_s[tid] = s;
      beta_s[tid] = bp.beta[tid];
      mean_s[tid] = bp.rmean[tid];
      istd_s[tid] = istd;
    }
    __syncthreads();
  }
}

// BN -> ReLU -> 2x2 max (first max wins, ATen's scan order) of one window given
// as two row pairs; also returns xhat = (y - mean) * invstd at the argmax.
// z = (y - mean) * (gamma * invstd) + beta: near the ReLU threshold this form
// keeps the rounding error at the scale of beta instead of gamma*mean*invstd.
template <typename T>
__device__ __forceinline__ void bn_relu_max4x(const typename Pair2<T>::type top, const typename Pair2<T>::type bot,
                                              float sc, float beta, float mean, float istd, float& best, int& bi,
                                              float& xh) {
  T v[4];
  __builtin_memcpy(&v[0], &top, 2 * sizeof(T));
  __builtin_memcpy(&v[2], &bot, 2 * sizeof(T));
  best = -1.f;
  bi = 0;
  float yb = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float yv = Cvt<T>::to_f(v[k]);
    const float z = fmaxf(rnd_t<T>((yv - mean) * sc + beta), 0.f);
    if (z > best) { best = z; bi = k; yb = yv; }
  }
  xh = (yb - mean) * istd;
}

// Pooled-index byte of the fused path: bits 0-1 argmax in the 2x2 window
// (dy * 2 + dx), bit 2 set when the ReLU passed the value (pooled output > 0).
constexpr int IDX_POS = 3, IDX_RELU = 4;

// Input of a conv that starts with the previous block's BN -> ReLU -> MaxPool.
template <typename T>
struct PoolIn {
  const T* y;          // previous conv output (pre-BN) [B][CIN][2H][2W]
  BNParams bn;         // its BatchNorm
  T* p_out;            // pooled output written for the backward (or null)
  uint8_t* idx_out;    // argmax index | relu bit, written for the backward
  T* xh_out;           // normalised value at the argmax (BN backward sums)
};

// ---------------------------------------------------------------------------
// Backward through [BN -> ReLU -> MaxPool2d(2,2)] fused into the staging of the
// next backward kernel: the conv-output gradient is produced on the fly as
//   dy = gi * (g - k1 - xhat * k2),  g = pooled grad at the window's argmax if
//   the ReLU passed it, else 0;  k1 = S1/n, k2 = S2/n, gi = gamma * invstd,
// with S1 = sum g, S2 = sum g * xhat over the (global) batch.
// ---------------------------------------------------------------------------
template <typename T>
struct BwdIn {
  const T* dp;            // pooled grad [B][C][H/2][W/2]
  const uint8_t* idx;     // argmax | relu bit
  const T* y;             // pre-BN conv output [B][C][H][W]
  const float* fstats;    // forward statistics (stats_len(C))
  const float* gsum;      // rows x [S1(C) | S2(C)], all-reduced under SyncBN
  int grows;
  const float* lsum;      // this rank's rows (dgamma / dbeta); may alias gsum
  int lrows;
  const float* gamma;
  float eps;
  float* dgamma;          // written by workgroup 0 when non-null
  float* dbeta;
  xgmi::XSite xs;         // active: gsum holds local rows, exchanged in here (comm/xsite.h)
  GradChk chk;            // producer-side non-finite check (common.h; not with xs active):
  int chk_coef = 0;       //   1: workgroup 0's dgamma / dbeta
  int chk_rows = 0;       //   1: the weight-gradient workgroups' partial rows (|v| <= chk_row_bound)
  float chk_row_bound = 0.f;
};

// Column sums of rows x RL floats (row-major) -> out[0..RL) in LDS, using the
// whole (NTHR-thread) workgroup; part: >= NTHR floats of LDS.  Ends with a barrier.
// (NTHR, not blockDim.x: see bn_finalize)
__device__ __forceinline__ void colsum_rows(const float* __restrict__ src, int rows, int RL, float* part,
                                            float* out) {
  const int tid = threadIdx.x, nthr = NTHR;
  const int G = nthr / RL;
  const int j = tid % RL, g = tid / RL;
  part[tid] = g < G ? strided_rowsum(src, rows, RL, j, g, G) : 0.f;
  __syncthreads();
  float t = 0.f;
  if (tid < RL)
    for (int gg = 0; gg < G; ++gg) t += part[gg * RL + tid];
  __syncthreads();
  if (tid < RL) out[tid] = t;
  __syncthreads();
}

// coef (LDS, 5C floats): [k1 | k2 | gi | mean | invstd]; part: >= blockDim.x
// floats of LDS, sums: >= 2C floats of LDS.  Workgroup `leader` also writes
// dgamma / dbeta from the local rows.  Ends with a barrier.
// `part` is scratch of this function alone: its last use is the leader's second colsum_rows, which
// ends with a barrier.  cb::conv5x5_body's 2-way data-gradient epilogue reuses the same floats for
// its statistics partials after its compute barrier (conv5x5.h LS_IN_PART), so a caller must not
// keep anything in `part` past that barrier.
template <int C, typename T>
__device__ __forceinline__ void bn_bwd_coef(const BwdIn<T>& bi, float* coef, float* part, float* sums, int bid) {
  const int tid = threadIdx.x;
  const bool leader = bid == 0;
  float n = 0.f, f0 = 0.f, f1 = 0.f, shf = 0.f, gam = 0.f;
  if (tid < C) {  // issued before the reduction: latencies overlap
    n = bi.fstats[2 * C];
    f0 = bi.fstats[tid];
    f1 = bi.fstats[C + tid];
    shf = bi.fstats[2 * C + 1 + tid];
    gam = bi.gamma[tid];
  }
  const bool xon = bi.xs.active();
  unsigned long long tk = 0;
  if (xon && tid == 0) tk = xgmi::xsite_ticket(bi.xs, bid);  // latency hides behind the slab loads
  const bool cchk = leader && bi.dgamma != nullptr && bi.chk_coef && !xon;  // producer-side check (xon: above)
  colsum_rows(bi.gsum, bi.grows, 2 * C, part, sums);
  if (xon) {
    // dgamma / dbeta are this rank's (DDP averages them); the coefficients use the global sums
    if (leader && bi.dgamma != nullptr && tid < C) {
      bi.dgamma[tid] = sums[C + tid];
      bi.dbeta[tid] = sums[tid];
      if (bi.chk_coef) bi.chk.flag(GradChk::bad(sums[C + tid], bi.chk.bound) || GradChk::bad(sums[tid], bi.chk.bound));
    }
    xgmi::xsite_exchange(bi.xs, sums, 2 * C, tk, bid);
  }
  if (tid < C) {
    const float m1 = f0 / n;
    const float mean = shf + m1;
    const float istd = rsqrtf(fmaxf(f1 / n - m1 * m1, 0.f) + bi.eps);
    coef[tid] = sums[tid] / n;
    coef[C + tid] = sums[C + tid] / n;
    coef[2 * C + tid] = gam * istd;
    coef[3 * C + tid] = mean;
    coef[4 * C + tid] = istd;
    if (leader && bi.dgamma != nullptr && bi.lsum == bi.gsum && !xon) {
      bi.dgamma[tid] = sums[C + tid];
      bi.dbeta[tid] = sums[tid];
    }
  }
  __syncthreads();
  if (leader && bi.dgamma != nullptr && bi.lsum != bi.gsum && !xon) {
    colsum_rows(bi.lsum, bi.lrows, 2 * C, part, sums);
    if (tid < C) {
      bi.dgamma[tid] = sums[C + tid];
      bi.dbeta[tid] = sums[tid];
    }
  }
  if (cchk && tid < C)  // the values just written
    bi.chk.flag(GradChk::bad(sums[C + tid], bi.chk.bound) || GradChk::bad(sums[tid], bi.chk.bound));
}

// Produce dy[c][h][w] of image b for every 2x2 window.  Two phases so that the
// loads can be issued before the coefficient reduction (their latencies
// overlap): load(bi, b) ... bn_bwd_coef(...) ... emit(coef, sink) with
// sink(c, h, w, v00, v01, v10, v11), (h, w) = the window's top-left pixel.
// ROWS (even): the conv-output rows [r0, r0 + ROWS) of one image (pooled rows
// [r0/2, r0/2 + ROWS/2), clipped at the image); the sink gets chunk-relative rows.
// CL: the channels [c0, c0 + CL) of the image's C; the sink gets the channel relative to c0.
template <typename T, int C, int H, int W, int NT_, int ROWS = H, int CL = C>
struct BnBwdStage {
  typedef typename Pair2<T>::type P;
  static_assert(ROWS % 2 == 0 && ROWS <= H, "BN-backward staging works on whole 2x2 pooling windows");
  static constexpr int HO = H / 2, WO = W / 2, PP = HO * WO;
  static constexpr int CHO = ROWS / 2, CPP = CHO * WO, NWIN = CL * CPP;  // windows of one chunk
  static constexpr int IT = (NWIN + NT_ - 1) / NT_;
  P top[IT], bot[IT];
  T g[IT];
  uint8_t ix[IT];
  int ho0 = 0, cb0 = 0;

  __device__ __forceinline__ void load(const BwdIn<T>& bi, int b, int r0 = 0, int c0 = 0) {
    ho0 = r0 / 2;
    cb0 = c0;
    const T* yb = bi.y + ((size_t)b * C + c0) * H * W;
    const T* dpb = bi.dp + ((size_t)b * C + c0) * PP;
    const uint8_t* ib = bi.idx + ((size_t)b * C + c0) * PP;
    // unconditional loads (clamped window; emit() skips the out-of-range ones): guarded
    // loads were branched around and waited for group by group (conv2_bwd / wgrad1 .s,
    // scripts/asm_loads.py)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = min((int)threadIdx.x + i * NT_, NWIN - 1);
      const int c = e / CPP, pix = e % CPP, ho = min(ho0 + pix / WO, HO - 1), wo = pix % WO;
      const P* src = reinterpret_cast<const P*>(yb + ((size_t)c * H + 2 * ho) * W + 2 * wo);
      top[i] = src[0];
      bot[i] = src[W / 2];
      const int ew = c * PP + ho * WO + wo;
      g[i] = dpb[ew];
      ix[i] = ib[ew];
    }
  }

  template <typename Sink>
  __device__ __forceinline__ void emit(const float* coef, Sink&& sink) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = threadIdx.x + i * NT_;
      const int c = e / CPP, pix = e % CPP, hl = pix / WO, wo = pix % WO;
      if (e < NWIN && ho0 + hl < HO) {
        const int ho = hl;  // chunk-relative pooled row
        const int cg = cb0 + c;
        const float k1 = coef[cg], k2 = coef[C + cg], gi = coef[2 * C + cg], mean = coef[3 * C + cg],
                    istd = coef[4 * C + cg];
        T v[4];
        __builtin_memcpy(&v[0], &top[i], 2 * sizeof(T));
        __builtin_memcpy(&v[2], &bot[i], 2 * sizeof(T));
        const int k = ix[i] & IDX_POS;
        const float gg = (ix[i] & IDX_RELU) ? Cvt<T>::to_f(g[i]) : 0.f;
        T o[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const float xh = (Cvt<T>::to_f(v[qq]) - mean) * istd;
          o[qq] = Cvt<T>::from_f(gi * ((qq == k ? gg : 0.f) - k1 - xh * k2));
        }
        sink(c, 2 * ho, 2 * wo, o[0], o[1], o[2], o[3]);
      }
    }
  }
};

// As BnBwdStage (whole images), but a lane owns 8 CHANNELS of one 2x2 window
// (lanes along the windows: each load instruction still reads consecutive pairs of
// one row) and the sink receives the window's 4 pixels as 8-channel vectors: the
// data-grad kernel writes them as 16-B LDS stores into its [pixel][channel] image.
// ROWS (even), r0 (even): as BnBwdStage -- the conv-output rows [r0, r0 + ROWS) of the image,
// clipped at its end; the sink gets chunk-relative rows.
template <typename T, int C, int H, int W, int NT_, int ROWS = H>
struct BnBwdStage8 {
  typedef typename Pair2<T>::type P;
  static_assert(C % 8 == 0 && sizeof(T) == 2, "8-channel staging: 16-bit types, C % 8 == 0");
  static_assert(ROWS % 2 == 0 && ROWS <= H, "BN-backward staging works on whole 2x2 pooling windows");
  static constexpr int HO = H / 2, WO = W / 2, PP = HO * WO;
  static constexpr int CPP = ROWS / 2 * WO;  // windows of one chunk, per channel
  static constexpr int NO = C / 8, NWIN = NO * CPP;
  static constexpr int IT = (NWIN + NT_ - 1) / NT_;
  P top[IT][8], bot[IT][8];
  T g[IT][8];
  uint8_t ix[IT][8];
  int ho0 = 0;

  __device__ __forceinline__ void load(const BwdIn<T>& bi, int b, int r0 = 0) {
    ho0 = r0 / 2;
    const T* yb = bi.y + (size_t)b * C * H * W;
    const T* dpb = bi.dp + (size_t)b * C * PP;
    const uint8_t* ib = bi.idx + (size_t)b * C * PP;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = min((int)threadIdx.x + i * NT_, NWIN - 1);  // clamped: unconditional loads
      const int o = e / CPP, pl = e % CPP, wo = pl % WO;
      int ho = pl / WO;
      if constexpr (ROWS < H) ho = min(ho0 + ho, HO - 1);  // clamped too (emit() skips the row)
      const int pix = ho * WO + wo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = 8 * o + j;
        const P* src = reinterpret_cast<const P*>(yb + ((size_t)c * H + 2 * ho) * W + 2 * wo);
        top[i][j] = src[0];
        bot[i][j] = src[W / 2];
        g[i][j] = dpb[c * PP + pix];
        ix[i][j] = ib[c * PP + pix];
      }
    }
  }

  // sink(h, w, c0, q00, q01, q10, q11): the 4 pixels of window (h, w) (top-left, h relative
  // to r0), channels c0 .. c0+7, each packed as uint4
  template <typename Sink>
  __device__ __forceinline__ void emit(const float* coef, Sink&& sink) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = (int)threadIdx.x + i * NT_;
      const int o = e / CPP, pl = e % CPP, ho = pl / WO, wo = pl % WO;
      if (e < NWIN && (ROWS == H || ho0 + ho < HO)) {
        unsigned q[4][4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = 8 * o + j;
          const float k1 = coef[c], k2 = coef[C + c], gi = coef[2 * C + c], mean = coef[3 * C + c],
                      istd = coef[4 * C + c];
          T v[4];
          __builtin_memcpy(&v[0], &top[i][j], 2 * sizeof(T));
          __builtin_memcpy(&v[2], &bot[i][j], 2 * sizeof(T));
          const int k = ix[i][j] & IDX_POS;
          const float gg = (ix[i][j] & IDX_RELU) ? Cvt<T>::to_f(g[i][j]) : 0.f;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const float xh = (Cvt<T>::to_f(v[qq]) - mean) * istd;
            const T o_ = Cvt<T>::from_f(gi * ((qq == k ? gg : 0.f) - k1 - xh * k2));
            const unsigned bits = __builtin_bit_cast(unsigned short, o_);
            if (j & 1) q[qq][j >> 1] |= bits << 16; else q[qq][j >> 1] = bits;
          }
        }
        sink(2 * ho, 2 * wo, 8 * o, make_uint4(q[0][0], q[0][1], q[0][2], q[0][3]),
             make_uint4(q[1][0], q[1][1], q[1][2], q[1][3]), make_uint4(q[2][0], q[2][1], q[2][2], q[2][3]),
             make_uint4(q[3][0], q[3][1], q[3][2], q[3][3]));
      }
    }
  }
};

}  // namespace cb
}  // namespace dpa
