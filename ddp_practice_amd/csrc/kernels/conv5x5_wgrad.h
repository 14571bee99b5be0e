// Weight gradient of the 5x5 conv and the column sums of its slabs (overview: convblock_bn.h).
#pragma once
#include "convblock_bn.h"

namespace dpa {
namespace cb {

// ---------------------------------------------------------------------------
// Weight/bias gradient partials of the 5x5 conv.  One workgroup per
// (image, row-chunk); writes wslab[blk][COUT*N + COUT] (dW partial | db partial).
// (NSL > 0, below: one workgroup per (image, output slice) and one slab row per image.)
// GEMM: rows = COUT, cols = (ci, kh, kw) natural order, K = pixels of the chunk
// with the row padded to WP = ceil8(W) (dy is zero in the pad columns).
// LDS: dy[COUT][ROWS][WP] and 5 kw-shifted copies xs[kw][CIN][ROWS+4][WP] of
// the zero-padded input so both operands are aligned 16-B LDS reads.
// When there are fewer (m,n) tile pairs than waves, waves split K instead
// and combine through LDS.
// ---------------------------------------------------------------------------
// PRO 2: dy is produced on the fly from the pooled grad of the next block
// (bin: backward through MaxPool -> ReLU -> BN); needs ROWS == H.
// NSL > 0: output slices instead of row chunks.  One workgroup per (image b, 16-channel
// output tile mt, input-channel slice j of NSL) keeps the whole image as its K range
// (ROWS == H, PRO 2) and writes the 16 x (N / NSL) block [mt*16 .. +16][j*CIN/NSL .. ) of
// slab row b, so an image yields ONE row [COUT*N + COUT] (blk = (b * COUT/16 + mt) * NSL + j;
// the j == 0 workgroup writes its tile's 16 bias partials).  It stages only the dy of its
// 16 output channels and the CIN/NSL input channels of its slice; in the natural
// [co][ci][kh][kw] order a slice by input channel is one contiguous run per output channel.
// Dynamic-LDS bytes of conv5x5_wgrad_body<..., DYN = true> (its dy rows, shifted input
// copies, padded input and staged partial row; the small arrays stay static).
// The LDS pitches are padded by 16 B so the MFMA operand reads spread over the banks:
//  * dy rows (A operand: 16 lanes = 16 output channels) DYS apart;
//  * input copies (B operand) XCS apart per (kw, ci); with CIN >= 16 the GEMM columns
//    run ci-fastest (column n = tap*CIN + ci), so the 16 lanes of a fragment read 16
//    channels of one tap: 16 distinct 4-bank windows.  (CIN = 1: 16 taps, <= 2-way.)
template <typename T, int CIN, int COUT, int H, int W, int ROWS, int NSL = 0>
struct WgradLds {
  static constexpr int WP = ceil_to(W, 8), XR = ROWS + 4, N = CIN * 25;
  static constexpr int WX = WP + 4;  // padded input row (2 halo columns each side, room for the kw shift)
  static constexpr int DYS = ROWS * WP + 8, XCS = XR * WP + 8;
  // DIRECT, whole image per workgroup: the 5 shifted copies are written straight from
  // registers (no padded staging image, no LDS->LDS copy pass); CIF: ci-fastest column order
  static constexpr bool DIRECT = ROWS == H, CIF = CIN >= 16;
  static constexpr int CL = NSL > 0 ? 16 : COUT;          // output channels of one workgroup
  static constexpr int CIS = NSL > 0 ? CIN / NSL : CIN;   // input channels of one workgroup
  static constexpr int NS = CIS * 25;                     // its GEMM columns
  static constexpr size_t DYL = sizeof(T) * (size_t)CL * DYS;
  static constexpr size_t XS = sizeof(T) * (size_t)5 * CIS * XCS;
  static constexpr size_t XPAD = sizeof(T) * (size_t)(DIRECT ? 8 : CIN * XR * WX);
  static constexpr size_t BASE = DYL + XS + XPAD;
  // the partial row in natural order, staged for whole-chunk stores where LDS allows
  static constexpr bool STAGE = CIF && BASE + sizeof(float) * (size_t)CL * NS <= 144 * 1024;
  static constexpr size_t o_xs = (DYL + 15) / 16 * 16, o_xpad = (o_xs + XS + 15) / 16 * 16,
                          o_wt = (o_xpad + XPAD + 15) / 16 * 16;
  static constexpr size_t bytes = o_wt + sizeof(float) * (STAGE ? (size_t)CL * NS : 4);
};

template <typename T, int CIN, int COUT, int H, int W, int ROWS, int PRO = 0, bool CHK = false, bool DYN = false,
          int NSL = 0>
__device__ __forceinline__ void
conv5x5_wgrad_body(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ wslab, int nsplit,
                   const BwdIn<T>& bin, const int bid) {
  static_assert(PRO == 0 || (PRO == 2 && ROWS % 2 == 0), "PRO 2 works on whole 2x2 pooling windows");
  using WL = WgradLds<T, CIN, COUT, H, W, ROWS, NSL>;  // the sizes, shared with the dynamic-LDS launchers
  constexpr int WP = WL::WP, XR = WL::XR, WX = WL::WX, N = WL::N, DYS = WL::DYS, XCS = WL::XCS;
  constexpr int CL = WL::CL, CIS = WL::CIS, NS = WL::NS;
  constexpr bool DIRECT = WL::DIRECT, CIF = WL::CIF, STAGE = WL::STAGE;
  static_assert((ROWS * WP) % 32 == 0, "ROWS*WP must be a multiple of 32");
  constexpr int KSTEPS = ROWS * WP / 32;
  constexpr bool SL = NSL > 0;  // output slices (one slab row per image), see WgradLds
  static_assert(!SL || (PRO == 2 && ROWS == H && CIN >= 16 && CIN % NSL == 0 && COUT % 16 == 0 && !CHK),
                "output slices: whole image, dy produced on the fly, ci-fastest columns");
  static_assert(!SL || NS % 4 == 0, "a slice leaves as whole 16-B chunks");
  static_assert(!SL || STAGE, "output slices leave through the staged tile");
  constexpr int NTL = (NS + 15) / 16, MTL = CL / 16, PAIRS = MTL * NTL, NW = NTHR / 64;
  constexpr int KSPLIT = PAIRS >= NW ? 1 : NW / PAIRS;  // waves per pair
  constexpr int ROWLEN = COUT * N + COUT;
  typedef MM<T> mm;
  __shared__ f32x4 kred[KSPLIT > 1 ? NW : 1][64];
  T* dyl;
  T* xs;
  T* xpad;
  float* wtile;
  if constexpr (DYN) {
    dyl = reinterpret_cast<T*>(dpa_dyn_lds);
    xs = reinterpret_cast<T*>(dpa_dyn_lds + WL::o_xs);
    xpad = reinterpret_cast<T*>(dpa_dyn_lds + WL::o_xpad);
    wtile = reinterpret_cast<float*>(dpa_dyn_lds + WL::o_wt);
  } else {
    __shared__ __attribute__((aligned(16))) T dyl_s[CL * DYS];
    __shared__ __attribute__((aligned(16))) T xs_s[5 * CIS * XCS];
    __shared__ __attribute__((aligned(16))) T xpad_s[DIRECT ? 8 : CIN * XR * WX];
    __shared__ __attribute__((aligned(16))) float wtile_s[STAGE ? CL * NS : 4];
    dyl = dyl_s;
    xs = xs_s;
    xpad = xpad_s;
    wtile = wtile_s;
  }

  const int tid = threadIdx.x;
  const int b = bid / nsplit, sp = bid % nsplit;
  DPA_STAMP(0);
  // producer-side check of this workgroup's partial row (BwdIn::chk_row_slot0, common.h)
  const bool rchk = CHK && bin.chk_rows;  // (compiled only where a launch can ask for it)
  // output slices: nsplit = (COUT / 16) * NSL workgroups per image, sp = (mt0, sl)
  const int r0 = SL ? 0 : sp * ROWS;
  const int mt0 = SL ? sp / (SL ? NSL : 1) : 0, sl = SL ? sp % (SL ? NSL : 1) : 0;
  const T* xb = x + ((size_t)b * CIN + sl * CIS) * H * W;
  // input rows r0-2 .. r0+ROWS+1 -> xpad interior; all loads issued before the
  // first LDS store (one memory round trip, not one per loop iteration)
  auto stage_xpad = [&]() {
    if constexpr (!DIRECT) {
      constexpr int XN = CIN * XR * W, XIT = (XN + NTHR - 1) / NTHR;
      T xv[XIT];
#pragma unroll
      for (int i = 0; i < XIT; ++i) {
        const int e = threadIdx.x + i * NTHR;
        const int ci = e / (XR * W), rem = e % (XR * W);
        const int rr = rem / W, cc = rem % W;
        const int ih = r0 + rr - 2;
        const bool ok = e < XN && ih >= 0 && ih < H;
        xv[i] = xb[ok ? (ci * H + ih) * W + cc : 0];
      }
#pragma unroll
      for (int i = 0; i < XIT; ++i) {
        const int e = threadIdx.x + i * NTHR;
        const int ci = e / (XR * W), rem = e % (XR * W);
        const int rr = rem / W, cc = rem % W;
        const int ih = r0 + rr - 2;
        if (e < XN && ih >= 0 && ih < H) xpad[(ci * XR + rr) * WX + cc + 2] = xv[i];
      }
    }
  };
  const T* dyb = dy + (size_t)b * COUT * H * W;
  const T zero = Cvt<T>::from_f(0.f);

  // dy chunk -> dyl[co][rr][0..WP) (pad columns zero)
  for (int e = tid; e < CL * ROWS * (WP - W); e += NTHR) {
    const int cr = e / (WP - W), cc = W + e % (WP - W);
    dyl[(cr / ROWS) * DYS + (cr % ROWS) * WP + cc] = zero;
  }
  if (r0 + ROWS > H) {  // rows past the image (last chunk): zero
    for (int e = tid; e < CL * ROWS * WP; e += NTHR)
      if (r0 + (e / WP) % ROWS >= H) dyl[(e / (ROWS * WP)) * DYS + e % (ROWS * WP)] = zero;
  }
  // xs[kw][ci][rr][c] = x[ci][r0 + rr - 2][c + kw - 2] (zero outside the image)
  auto scatter5 = [&](int ci, int rr, int w, T v) {
#pragma unroll
    for (int kw = 0; kw < 5; ++kw) {
      const int c = w + 2 - kw;
      if (c >= 0 && c < WP) xs[(kw * CIS + ci) * XCS + rr * WP + c] = v;
    }
  };
  if constexpr (DIRECT) {
    constexpr int NZ = 5 * CIS * XCS * (int)sizeof(T) / 16;
    static_assert((5 * CIS * XCS * sizeof(T)) % 16 == 0, "xs must be a whole number of 16-B chunks");
    uint4* z = reinterpret_cast<uint4*>(xs);
    for (int e = tid; e < NZ; e += NTHR) z[e] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    // input rows r0-2 .. r0+ROWS+1 -> xpad[ci][XR][WX], columns shifted by 2 (zero halo)
    for (int e = tid; e < CIN * XR * WX; e += NTHR) {
      const int cc = e % WX, rr = (e / WX) % XR;
      const int ih = r0 + rr - 2;
      if (cc < 2 || cc >= W + 2 || ih < 0 || ih >= H) xpad[e] = zero;
    }
  }
  if constexpr (PRO == 2) {
    __shared__ float coef[5 * COUT], sums[2 * COUT];
    __shared__ float part[NTHR];
    BnBwdStage<T, COUT, H, W, NTHR, ROWS, CL> st;
    st.load(bin, b, r0, mt0 * 16);
    if constexpr (DIRECT) {
      __syncthreads();  // xs zero-fill before the scatter
      stage_chw<T, CIS, H, W>(xb, [&](int ci, int h, int ww, T a, T bb) {
        scatter5(ci, h + 2, ww, a);
        scatter5(ci, h + 2, ww + 1, bb);
      });
    } else {  // input rows r0-2 .. r0+ROWS+1 -> xpad (kw copies after the barrier below)
      stage_xpad();
    }
    bn_bwd_coef<COUT, T>(bin, coef, part, sums, bid);
    DPA_STAMP(3);
    st.emit(coef, [&](int co, int h, int ww, T v00, T v01, T v10, T v11) {
      dyl[co * DYS + h * WP + ww] = v00;
      dyl[co * DYS + h * WP + ww + 1] = v01;
      dyl[co * DYS + (h + 1) * WP + ww] = v10;
      dyl[co * DYS + (h + 1) * WP + ww + 1] = v11;
    });
  } else if constexpr (DIRECT) {  // both operands are full [C][H][W] images
    stage_chw<T, COUT, H, W>(dyb, [&](int co, int h, int ww, T a, T bb) {
      dyl[co * DYS + h * WP + ww] = a;
      dyl[co * DYS + h * WP + ww + 1] = bb;
    });
    __syncthreads();  // xs zero-fill before the scatter
    stage_chw<T, CIN, H, W>(xb, [&](int ci, int h, int ww, T a, T bb) {
      scatter5(ci, h + 2, ww, a);
      scatter5(ci, h + 2, ww + 1, bb);
    });
  } else {
    for (int e = tid; e < COUT * ROWS * W; e += NTHR) {
      const int co = e / (ROWS * W), rem = e % (ROWS * W);
      const int rr = rem / W, cc = rem % W;
      if (r0 + rr < H) dyl[co * DYS + rr * WP + cc] = dyb[(co * H + r0 + rr) * W + cc];
    }
    stage_xpad();
  }
  DPA_STAMP(4);
  __syncthreads();
  if constexpr (!DIRECT) {
    // 5 kw-shifted copies, LDS -> LDS: xs[kw][ci][rr][c] = xpad[ci][rr][c + kw]
    for (int e = tid; e < 5 * CIN * XR * (WP / 8); e += NTHR) {
      const int c8 = e % (WP / 8);
      const int rowid = e / (WP / 8);  // (kw, ci, rr)
      const int kw = rowid / (CIN * XR), cr = rowid % (CIN * XR);
      const T* srcp = &xpad[cr * WX + 8 * c8 + kw];
      T* dstp = &xs[(kw * CIN + cr / XR) * XCS + (cr % XR) * WP + 8 * c8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dstp[j] = srcp[j];
    }
    __syncthreads();
  }

  float* row_out = wslab + (size_t)(SL ? b : bid) * ROWLEN;
  DPA_STAMP(5);
  const int lane = tid & 63, wv = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  // bias grad partial: per output channel sum of dy over this chunk.  TPC lanes
  // per channel, each summing 16-B groups (fixed order), then a TPC-lane
  // butterfly: one pass for all channels (a wave-wide reduction per channel
  // cost ~2 us here)
  {
    constexpr int TPC = NTHR / CL;
    static_assert(NTHR % CL == 0 && TPC <= 64 && (TPC & (TPC - 1)) == 0, "bias-sum lane groups");
    constexpr int E = ROWS * WP;
    static_assert(E % 8 == 0, "dy rows are whole 16-B groups");
    const int co = tid / TPC, sub = tid % TPC;
    float a = 0.f;
    for (int i = sub * 8; i < E; i += TPC * 8) {
      const typename mm::frag v = mm::ld(&dyl[co * DYS + i]);
      const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int j = 0; j < 8; ++j) a += Cvt<T>::to_f(e[j]);
    }
    a = group_sum<TPC>(a);  // VALU lane moves (every lane active here)
    if (sub == 0 && sl == 0) {
      row_out[COUT * N + mt0 * 16 + co] = a;
      // the bias column is summed by the AMP step like the weight columns: same row bound
      if (rchk) bin.chk.flag(GradChk::bad(a, bin.chk_row_bound));
    }
  }
  DPA_STAMP(6);
  const int ks = KSPLIT > 1 ? wv % KSPLIT : 0;
  const int pstart = KSPLIT > 1 ? wv / KSPLIT : wv;
  const int pstep = KSPLIT > 1 ? NW / KSPLIT : NW;
  for (int pr = pstart; pr < PAIRS; pr += pstep) {
    const int mt = pr / NTL, nt = pr % NTL;
    int n = nt * 16 + r;
    n = n < NS ? n : 0;
    const int ci = CIF ? n % CIS : n / 25, tap = CIF ? n / CIS : n % 25;
    const int kh = tap / 5, kw = tap % 5;
    const T* brow = &xs[(kw * CIS + ci) * XCS + kh * WP];
    const T* arow = &dyl[(mt * 16 + r) * DYS];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = ks; s < KSTEPS; s += KSPLIT) {
      const int P = 32 * s + 8 * q;  // pixel index within the chunk
      const int row = P / WP, col0 = P % WP;
      const typename mm::frag a = mm::ld(arow + P);
      const typename mm::frag bf = mm::ld(brow + row * WP + col0);
      acc = mm::mma(a, bf, acc);
    }
    if constexpr (KSPLIT > 1) {
      kred[wv][lane] = acc;
      __syncthreads();
      if (ks != 0) continue;
      for (int k2 = 1; k2 < KSPLIT; ++k2) acc += kred[wv + k2][lane];
    }
    // D[row = 4q+i][col = r]: dW[co = mt*16+4q+i][ci][kh][kw] (natural order in the row)
    const int col = nt * 16 + r;
    if (col < NS) {
      const int nat = CIF ? (col % CIS) * 25 + col / CIS : col;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (STAGE) wtile[(mt * 16 + 4 * q + i) * NS + nat] = acc[i];
        else row_out[(mt * 16 + 4 * q + i) * N + nat] = acc[i];
        if (rchk) bin.chk.flag(GradChk::bad(acc[i], bin.chk_row_bound));
      }
    }
  }
  if constexpr (STAGE) {
    // ci-fastest columns land 25 floats apart in the natural row: 64-lane stores to ~40
    // lines each.  Staged through LDS instead, the row leaves as whole 16-B chunks
    // (consecutive lanes, consecutive addresses).
    static_assert((COUT * N) % 4 == 0 && ROWLEN % 4 == 0, "wgrad rows: whole 16-B chunks");
    __syncthreads();
    if constexpr (SL) {  // 16 runs of NS floats: [mt0*16 + rr][sl*CIS ..][kh][kw]
      for (int e = tid; e < CL * NS / 4; e += NTHR) {
        const int rr = e / (NS / 4), c4 = e % (NS / 4);
        *reinterpret_cast<f32x4*>(&row_out[(mt0 * 16 + rr) * N + sl * NS + 4 * c4]) =
            *reinterpret_cast<const f32x4*>(&wtile[rr * NS + 4 * c4]);
      }
    } else {
      for (int e = tid; e < COUT * N / 4; e += NTHR)
        *reinterpret_cast<f32x4*>(&row_out[4 * e]) = *reinterpret_cast<const f32x4*>(&wtile[4 * e]);
    }
  }
  DPA_STAMP(7);
}

template <typename T, int CIN, int COUT, int H, int W, int ROWS, int PRO = 0>
__global__ void __launch_bounds__(NTHR)
conv5x5_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ wslab,
                     int nsplit, BwdIn<T> bin = BwdIn<T>{}) {
  conv5x5_wgrad_body<T, CIN, COUT, H, W, ROWS, PRO>(x, dy, wslab, nsplit, bin, (int)blockIdx.x);
}

// ---------------------------------------------------------------------------
// Column sums of up to two slabs in one launch:
//   out1[i] = sum_r slab1[r*n1 + i]  (i < n1),  out2[j] = sum_r slab2[r*n2 + j]  (j < n2)
// A workgroup owns 16 columns; its 16 row-groups each sum every 16th row
// (independent loads in flight), then combine through LDS.
// ---------------------------------------------------------------------------
constexpr int SR_COLS = 16, SR_GROUPS = NTHR / SR_COLS;
__device__ __forceinline__ void slab_reduce_body(const float* __restrict__ slab1, int rows1, int n1,
                                                 float* __restrict__ out1, const float* __restrict__ slab2, int rows2,
                                                 int n2, float* __restrict__ out2, int bid,
                                                 GradChk chk = GradChk{}) {
  __shared__ float part[SR_GROUPS][SR_COLS + 1];
  const int nb1 = (n1 + SR_COLS - 1) / SR_COLS;
  const bool first = bid < nb1;
  const float* slab = first ? slab1 : slab2;
  const int rows = first ? rows1 : rows2;
  const int n = first ? n1 : n2;
  float* out = first ? out1 : out2;
  const int c0 = (first ? bid : bid - nb1) * SR_COLS;
  const int col = c0 + (threadIdx.x % SR_COLS), g = threadIdx.x / SR_COLS;
  part[g][threadIdx.x % SR_COLS] = slab_colsum<SR_GROUPS>(slab, rows, n, col, g);
  __syncthreads();
  if (threadIdx.x < SR_COLS && c0 + (int)threadIdx.x < n) {
    float t = 0.f;
#pragma unroll
    for (int gg = 0; gg < SR_GROUPS; ++gg) t += part[gg][threadIdx.x];
    out[c0 + threadIdx.x] = t;
    if (chk.word != nullptr) chk.flag(GradChk::bad(t, chk.bound));  // (producer-side check, common.h)
  }
}
// As slab_reduce_body for ONE slab, with K chunks of SR_COLS columns per workgroup: a
// quarter of the workgroups at K = 4, each lane with K independent columns in flight.
// Per column the association is slab_colsum's (SR_GROUPS row groups, rows g, g + G, ... in
// that order, partials added in group order): bitwise the same sums.  A lane loads
// ceil(rows / G) rows where that is <= 2 (the conv2 slab's one row per image at B <= 32)
// instead of slab_colsum's fixed batch of 16 clamped loads.
template <int K, int U>
__device__ __forceinline__ void slab_colsum_chunks(const float* __restrict__ slab, int rows, int n, int c0, int cl,
                                                   int g, float* v) {
  constexpr int G = SR_GROUPS;
  float x[K][U];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int cc = min(c0 + j * SR_COLS + cl, n - 1);
#pragma unroll
    for (int u = 0; u < U; ++u) x[j][u] = slab[(size_t)min(g + u * G, rows - 1) * n + cc];
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int cc = min(c0 + j * SR_COLS + cl, n - 1);
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) a += (g + u * G < rows) ? x[j][u] : 0.f;
    for (int r = g + U * G; r < rows; r += G) a += slab[(size_t)r * n + cc];
    v[j] = a;
  }
}
template <int K>
__device__ __forceinline__ void slab_reduce_chunks_body(const float* __restrict__ slab, int rows, int n,
                                                        float* __restrict__ out, int bid, GradChk chk = GradChk{}) {
  __shared__ float part[SR_GROUPS][K * SR_COLS + 1];
  static_assert(K * SR_COLS <= NTHR, "one lane per column in the final sum");
  if (rows <= 0 || n <= 0) return;
  const int c0 = bid * K * SR_COLS;
  const int cl = threadIdx.x % SR_COLS, g = threadIdx.x / SR_COLS;
  float v[K];
  if (rows <= 2 * SR_GROUPS) slab_colsum_chunks<K, 2>(slab, rows, n, c0, cl, g, v);
  else slab_colsum_chunks<K, 16>(slab, rows, n, c0, cl, g, v);
#pragma unroll
  for (int j = 0; j < K; ++j) part[g][j * SR_COLS + cl] = v[j];
  __syncthreads();
  if (threadIdx.x < K * SR_COLS && c0 + (int)threadIdx.x < n) {
    float t = 0.f;
#pragma unroll
    for (int gg = 0; gg < SR_GROUPS; ++gg) t += part[gg][threadIdx.x];
    out[c0 + threadIdx.x] = t;
    if (chk.word != nullptr) chk.flag(GradChk::bad(t, chk.bound));  // (producer-side check, common.h)
  }
}


}  // namespace cb
}  // namespace dpa
