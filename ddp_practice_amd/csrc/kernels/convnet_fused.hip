// Whole-ConvNet fused kernels (ops/convnet_fused.py).  Layer boundaries are
// fused where the data dependence allows it; every BatchNorm reduction is
// produced as per-workgroup partial sums in the epilogue of the kernel that
// computes its operand and reduced in the prologue of the kernel that needs
// the result, so no launch exists only to reduce or to apply a BatchNorm:
//
//   forward   gather | conv1 (+BN1 sums) | [BN1-ReLU-pool1 -> conv2 (+BN2 sums)]
//             | [BN2-ReLU-pool2 -> fc] -> logits                          (3 launches)
//   backward  [fc bwd -> dp2 (+BN2 sums: complete per channel)]
//             | {[BN2/ReLU2/pool2 bwd -> conv2 dgrad -> dp1 (+BN1 partial sums)],
//                [BN2/ReLU2/pool2 bwd -> conv2 wgrad]}: two roles of one launch (conv2_bwd)
//             | [BN1/ReLU1/pool1 bwd -> conv1 wgrad]
//             | weight-grad sums                                        (4 launches)
//   with an optimizer that sums the conv1 slab in its own launch (a slab sink): the conv1
//   launch also sums the conv2 slab (conv1_wgrad_slab2) and no sum launch follows (3).
//
// (reference model: /root/reference/origin_main.py:9-31.)  With SyncBN the
// partial sums are all-reduced between the launches (host side).  Everything
// is deterministic (no float atomics).
#include <type_traits>

#include "conv5x5.h"
#include "conv5x5_wgrad.h"
#include "comm/xgmi.h"

namespace dpa {
namespace cnf {

using cb::BNParams;
using cb::bn_finalize;
using cb::bn_relu_max4x;
using cb::BwdEpi;
using cb::BwdIn;
using cb::IDX_POS;
using cb::IDX_RELU;
using cb::Pair2;
using cb::PoolIn;
using cb::with_t;

constexpr int HF = 256;        // head forward: one workgroup per image
constexpr int NTHR_HB = 256;   // head backward: one workgroup per BN2 channel

// ---------------------------------------------------------------------------
// [BN2 finalize -> BN -> ReLU -> 2x2 max-pool -> flatten -> Linear] for one
// image per workgroup (B workgroups: the whole chip works on the head instead
// of B/16 tiles).  The fc is a 1 x K x N GEMV per image: every thread owns K/HF
// pooled features, multiplies them against the fc rows and the N partial dot
// products are reduced across the workgroup.  The y2 loads are issued before
// the BN statistics reduction so the two latencies overlap.
// ---------------------------------------------------------------------------
template <typename T, int C, int H, int W, int NMAX>
__global__ void __launch_bounds__(HF)
head_fwd_kernel(const T* __restrict__ y, BNParams bn, const float* __restrict__ wfc, const float* __restrict__ bfc,
                T* __restrict__ logits, T* __restrict__ p_out, uint8_t* __restrict__ idx_out, T* __restrict__ xh_out,
                int N) {
  constexpr int HO = H / 2, WO = W / 2, PP = HO * WO, K = C * PP;
  constexpr int IT = (K + HF - 1) / HF;
  typedef typename Pair2<T>::type P;
  __shared__ float sc_s[C], beta_s[C], mean_s[C], istd_s[C];
  __shared__ float part[HF];
  __shared__ float red[HF / 64][NMAX];
  const int tid = threadIdx.x, b = blockIdx.x;
  const T* yb = y + (size_t)b * C * H * W;
  P top[IT], bot[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int k = tid + i * HF;
    if (k < K) {
      const int c = k / PP, pix = k % PP, ho = pix / WO, wo = pix % WO;
      const P* src = reinterpret_cast<const P*>(yb + ((size_t)c * H + 2 * ho) * W + 2 * wo);
      top[i] = src[0];
      bot[i] = src[W / 2];
    }
  }
  bn_finalize<C>(bn, sc_s, beta_s, mean_s, istd_s, part, b);
  float pf[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int k = tid + i * HF;
    pf[i] = 0.f;
    if (k < K) {
      const int c = k / PP;
      float best, xh;
      int bi;
      bn_relu_max4x<T>(top[i], bot[i], sc_s[c], beta_s[c], mean_s[c], istd_s[c], best, bi, xh);
      const T pv = Cvt<T>::from_f(best);
      pf[i] = Cvt<T>::to_f(pv);
      if (p_out != nullptr) {
        p_out[(size_t)b * K + k] = pv;
        idx_out[(size_t)b * K + k] = (uint8_t)(bi | (best > 0.f ? IDX_RELU : 0));
        xh_out[(size_t)b * K + k] = Cvt<T>::from_f(xh);
      }
    }
  }
  const int lane = tid & 63, wv = tid >> 6;
  // fc rows in chunks of NC outputs: every load of a chunk is issued before
  // its first FMA (rows past N are clamped to N-1 and discarded)
  constexpr int NC = 8;
  for (int n0 = 0; n0 < N; n0 += NC) {  // uniform
    float wr[NC][IT];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int n = min(n0 + j, N - 1);
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int k = min(tid + i * HF, K - 1);
        wr[j][i] = wfc[(size_t)n * K + k];
      }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < IT; ++i) a += pf[i] * wr[j][i];  // pf = 0 past K
      a = wave_sum(a);
      if (lane == 0 && n0 + j < N) red[wv][n0 + j] = a;
    }
  }
  __syncthreads();
  if (tid < N) {
    float t = bfc[tid];
#pragma unroll
    for (int i = 0; i < HF / 64; ++i) t += red[i][tid];
    logits[(size_t)b * N + tid] = Cvt<T>::from_f(t);
  }
}

// ---------------------------------------------------------------------------
// fc backward + the BN2 backward sums, one workgroup per BN2 channel c (its
// PP = 7*7 pooled features; the sums are complete, no partial rows):
//   dp2[b, cPP + j]   = sum_n dlogits[b, n] W[n, cPP + j]          (stored in T)
//   dW_fc[n, cPP + j] = sum_b dlogits[b, n] p2[b, cPP + j]
//   S1[c] = sum g, S2[c] = sum g * xhat, g = dp2 where the ReLU passed it
// dynamic LDS: dlogits [B][N] + W columns [N][PP] + p2 slice [B][PP] (f32).
// ---------------------------------------------------------------------------
template <typename T, int C, int H, int W>
__global__ void __launch_bounds__(NTHR_HB)
head_bwd_kernel(const T* __restrict__ dlogits, const float* __restrict__ wfc, const T* __restrict__ p2,
                const uint8_t* __restrict__ idx2, const T* __restrict__ xh2, int B, int N, float* __restrict__ dwfc,
                float* __restrict__ dbfc, float* __restrict__ dgamma, float* __restrict__ dbeta,
                float* __restrict__ bsum, T* __restrict__ dp2) {
  constexpr int HO = H / 2, WO = W / 2, PP = HO * WO, K = C * PP;
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  __shared__ float red[2][NTHR_HB / 64];
  float* dl = hsm;               // [B][N]
  float* wc = dl + B * N;        // [N][PP]
  float* pc = wc + N * PP;       // [B][PP]
  const int tid = threadIdx.x, c = blockIdx.x, f0 = c * PP;
  for (int e = tid; e < B * N; e += NTHR_HB) dl[e] = Cvt<T>::to_f(dlogits[e]);
  for (int e = tid; e < N * PP; e += NTHR_HB) wc[e] = wfc[(size_t)(e / PP) * K + f0 + e % PP];
  for (int e = tid; e < B * PP; e += NTHR_HB) pc[e] = Cvt<T>::to_f(p2[(size_t)(e / PP) * K + f0 + e % PP]);
  __syncthreads();
  // pooled-map grad + BN2 sums
  float s1 = 0.f, s2 = 0.f;
  for (int e = tid; e < B * PP; e += NTHR_HB) {
    const int b = e / PP, j = e % PP;
    const size_t o = (size_t)b * K + f0 + j;
    const uint8_t ix = idx2[o];
    const float xh = Cvt<T>::to_f(xh2[o]);
    float a = 0.f;
    for (int nn = 0; nn < N; ++nn) a += dl[b * N + nn] * wc[nn * PP + j];
    const T gt = Cvt<T>::from_f(a);
    dp2[o] = gt;
    if (ix & IDX_RELU) {
      const float g = Cvt<T>::to_f(gt);
      s1 += g;
      s2 += g * xh;
    }
  }
  // fc weight grad for this channel's columns, fc bias grad on workgroup 0
  for (int e = tid; e < N * PP; e += NTHR_HB) {
    const int nn = e / PP, j = e % PP;
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dl[b * N + nn] * pc[b * PP + j];
    dwfc[(size_t)nn * K + f0 + j] = a;
  }
  if (c == 0) {
    for (int nn = tid; nn < N; nn += NTHR_HB) {
      float a = 0.f;
      for (int b = 0; b < B; ++b) a += dl[b * N + nn];
      dbfc[nn] = a;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int lane = tid & 63, wv = tid >> 6;
  if (lane == 0) { red[0][wv] = s1; red[1][wv] = s2; }
  __syncthreads();
  if (tid == 0) {
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int i = 0; i < NTHR_HB / 64; ++i) { t1 += red[0][i]; t2 += red[1][i]; }
    dbeta[c] = t1;
    dgamma[c] = t2;
    bsum[c] = t1;
    bsum[C + c] = t2;
  }
}

// ===========================================================================
// Host side
// ===========================================================================
static BNParams bn_params(c10::optional<at::Tensor> fslab, at::Tensor fstats, at::Tensor gamma, at::Tensor beta,
                          at::Tensor rmean, at::Tensor rvar, at::Tensor nbt, double momentum, double eps, bool train,
                          int C) {
  TORCH_CHECK(!train || fslab.has_value(), "train mode needs the forward slab");
  BNParams bp;
  bp.fslab = fslab.has_value() ? fslab->data_ptr<float>() : nullptr;
  bp.nrows = fslab.has_value() ? (int)(fslab->numel() / cb::fslab_row(C)) : 0;
  bp.fstats = fstats.data_ptr<float>();
  bp.gamma = gamma.data_ptr<float>();
  bp.beta = beta.data_ptr<float>();
  bp.rmean = rmean.data_ptr<float>();
  bp.rvar = rvar.data_ptr<float>();
  bp.nbt = nbt.data_ptr<int64_t>();
  bp.momentum = (float)momentum;
  bp.eps = (float)eps;
  bp.train = (int)train;
  return bp;
}

template <typename T>
static BwdIn<T> bwd_in(at::Tensor dp, at::Tensor idx, at::Tensor y, at::Tensor fstats, at::Tensor gsum,
                       c10::optional<at::Tensor> lsum, at::Tensor gamma, double eps, int C,
                       c10::optional<at::Tensor> dgamma, c10::optional<at::Tensor> dbeta) {
  TORCH_CHECK(gsum.numel() % (2 * C) == 0, "BN backward sums: rows of 2C floats expected");
  TORCH_CHECK(dp.scalar_type() == y.scalar_type() && idx.scalar_type() == at::kByte);
  TORCH_CHECK(fstats.numel() == cb::stats_len(C) && gamma.numel() == C);
  BwdIn<T> bi;
  bi.dp = dptr<T>(dp);
  bi.idx = idx.data_ptr<uint8_t>();
  bi.y = dptr<T>(y);
  bi.fstats = fstats.data_ptr<float>();
  bi.gsum = gsum.data_ptr<float>();
  bi.grows = (int)(gsum.numel() / (2 * C));
  at::Tensor ls = lsum.has_value() ? *lsum : gsum;
  TORCH_CHECK(ls.numel() % (2 * C) == 0);
  bi.lsum = ls.data_ptr<float>();
  bi.lrows = (int)(ls.numel() / (2 * C));
  bi.gamma = gamma.data_ptr<float>();
  bi.eps = (float)eps;
  bi.dgamma = dgamma.has_value() ? dgamma->data_ptr<float>() : nullptr;
  bi.dbeta = dbeta.has_value() ? dbeta->data_ptr<float>() : nullptr;
  return bi;
}

// xc (SyncBN over the xGMI engine, training only): the consumer kernel
// exchanges the BN sums itself (comm/xsite.h); the slab arguments then hold
// this rank's partial sums and no all-reduce runs between the launches.
typedef std::shared_ptr<xgmi::XgmiComm> XcPtr;
static xgmi::XSite site_of(const XcPtr& xc, int s) { return xc ? xc->site(s) : xgmi::XSite{}; }

// Workgroups per image of the conv2 forward: cb::kFwd2SplitT<T> (convblock_bn.h; the knobs
// DPA_FWD2_SPLIT / DPA_FWD2_SPLIT_F32).  fp32, whose 16x16x4 MFMA chain per output tile is 4x
// as long, runs 4 workgroups per image (fp32 step 0.0640 -> 0.0617 ms, profiles/r6m_split_ab.txt).
// The consumers take the slab's row count from its size (nrows).
int64_t fwd2_split(bool fp32) { return fp32 ? cb::kFwd2SplitT<float> : cb::kFwd2SplitT<__half>; }

// Row windows (cb::conv5x5_body WR): each workgroup of the fused conv2 kernels stages the
// input rows its own output pixels read, not the whole image.  The kernels' compile-time
// row bound follows from the split count; conv2_row_window re-derives what the launch's
// nsplit needs and refuses a launch whose splits would not fit the bound.
template <int NSPLIT, bool EVEN>
constexpr int conv2_wr() {
  constexpr int need = cb::conv5x5_win_rows(14, 14, NSPLIT, EVEN);
  static_assert(need > 0, "conv2: more workgroups per image than 16-pixel tiles");
  return need < 14 ? need : 14;
}
static void conv2_row_window(int wr, int nsplit, bool even, const char* what) {
  const int need = cb::conv5x5_win_rows(14, 14, nsplit, even);
  TORCH_CHECK(need > 0 && (wr >= 14 || need <= wr), what, ": a split in ", nsplit, " stages up to ", need,
              " rows, the kernel's window holds ", wr);
}
template <typename T>
constexpr int kFwd2WR = conv2_wr<cb::kFwd2SplitT<T>, false>();

// [BN1 -> ReLU -> pool1] -> conv2 (+ BN2 partial sums when training).
void conv2_fwd(at::Tensor y1, c10::optional<at::Tensor> fslab1, at::Tensor fstats1, at::Tensor g1, at::Tensor b1,
               at::Tensor rm1, at::Tensor rv1, at::Tensor nbt1, double momentum, double eps, bool train, at::Tensor w2,
               at::Tensor bias2, at::Tensor y2, c10::optional<at::Tensor> fslab2, at::Tensor fstats2, at::Tensor rm2,
               c10::optional<at::Tensor> p1_out, c10::optional<at::Tensor> idx1_out,
               c10::optional<at::Tensor> xh1_out, at::Tensor wpk, XcPtr xc) {
  DPA_CHECK_INPUT(y1); DPA_CHECK_INPUT(w2); DPA_CHECK_INPUT(y2); DPA_CHECK_INPUT(wpk);
  TORCH_CHECK(wpk.numel() == cb::W2F_LEN && wpk.scalar_type() == y1.scalar_type(), "packed conv2 weights");
  const int B = (int)y1.size(0);
  TORCH_CHECK(y1.size(1) == 16 && y1.size(2) == 28 && y1.size(3) == 28 && w2.size(0) == 32 && w2.size(1) == 16,
              "fused conv2 expects the ConvNet shapes");
  TORCH_CHECK(y2.scalar_type() == y1.scalar_type());
  TORCH_CHECK(p1_out.has_value() == idx1_out.has_value() && p1_out.has_value() == xh1_out.has_value());
  if (p1_out.has_value())
    TORCH_CHECK(p1_out->numel() == (int64_t)B * 16 * 196 && idx1_out->numel() == p1_out->numel() &&
                xh1_out->numel() == p1_out->numel());
  const int ns = fwd2_split(y1.scalar_type() == at::kFloat);  // workgroups per image
  if (train) TORCH_CHECK(fslab2.has_value() && fslab2->numel() == (int64_t)B * ns * cb::fslab_row(32));
  if (B == 0) return;
  BNParams bp = bn_params(fslab1, fstats1, g1, b1, rm1, rv1, nbt1, momentum, eps, train, 16);
  if (train) {
    bp.xs = site_of(xc, xgmi::kSiteFwd1);
    xgmi::set_site_grid(bp.xs, B * ns, "conv2_fwd");  // the grid (ns workgroups per image)
  }
  hipStream_t stream = cur_stream();
  with_t(dt_of(y1), [&](auto tag) {
    typedef decltype(tag) T;
    PoolIn<T> pin{dptr<T>(y1), bp, p1_out.has_value() ? dptr<T>(*p1_out) : nullptr,
                  idx1_out.has_value() ? idx1_out->data_ptr<uint8_t>() : nullptr,
                  xh1_out.has_value() ? dptr<T>(*xh1_out) : nullptr};
    constexpr int WR = kFwd2WR<T>;
    conv2_row_window(WR, ns, false, "conv2_fwd");
    if (train)
      hipLaunchKernelGGL((cb::conv5x5_kernel<T, 16, 32, 14, 14, 0, 1, 0, 1, WR>), dim3(B * ns), dim3(cb::NTHR), 0,
                         stream, nullptr, nullptr, bias2.data_ptr<float>(), dptr<T>(y2), fslab2->data_ptr<float>(),
                         fstats2.data_ptr<float>(), rm2.data_ptr<float>(), ns, pin, BwdIn<T>{}, BwdEpi<T>{},
                         dptr<T>(wpk), cb::WPack<T>{});
    else
      hipLaunchKernelGGL((cb::conv5x5_kernel<T, 16, 32, 14, 14, 1, 1, 0, 1, WR>), dim3(B * ns), dim3(cb::NTHR), 0,
                         stream, nullptr, nullptr, bias2.data_ptr<float>(), dptr<T>(y2), nullptr, nullptr, nullptr,
                         ns, pin, BwdIn<T>{}, BwdEpi<T>{}, dptr<T>(wpk), cb::WPack<T>{});
  });
  DPA_CHECK_LAUNCH();
}

// [BN2 -> ReLU -> pool2] -> flatten -> fc.
void head_fwd(at::Tensor y2, c10::optional<at::Tensor> fslab2, at::Tensor fstats2, at::Tensor g2, at::Tensor b2,
              at::Tensor rm2, at::Tensor rv2, at::Tensor nbt2, double momentum, double eps, bool train, at::Tensor wfc,
              at::Tensor bfc, at::Tensor logits, c10::optional<at::Tensor> p2_out, c10::optional<at::Tensor> idx2_out,
              c10::optional<at::Tensor> xh2_out, XcPtr xc) {
  DPA_CHECK_INPUT(y2); DPA_CHECK_INPUT(wfc); DPA_CHECK_INPUT(logits);
  const int B = (int)y2.size(0), N = (int)wfc.size(0);
  TORCH_CHECK(y2.size(1) == 32 && y2.size(2) == 14 && y2.size(3) == 14 && wfc.size(1) == 32 * 49,
              "fused head expects the ConvNet shapes");
  TORCH_CHECK(N >= 1 && N <= 64, "fused head supports up to 64 classes");
  TORCH_CHECK(logits.numel() == (int64_t)B * N && logits.scalar_type() == y2.scalar_type());
  TORCH_CHECK(p2_out.has_value() == idx2_out.has_value() && p2_out.has_value() == xh2_out.has_value());
  if (p2_out.has_value())
    TORCH_CHECK(p2_out->numel() == (int64_t)B * 1568 && idx2_out->numel() == p2_out->numel() &&
                xh2_out->numel() == p2_out->numel());
  if (B == 0) return;
  BNParams bp = bn_params(fslab2, fstats2, g2, b2, rm2, rv2, nbt2, momentum, eps, train, 32);
  if (train) {
    bp.xs = site_of(xc, xgmi::kSiteFwd2);
    xgmi::set_site_grid(bp.xs, B, "head_fwd");  // one workgroup per image
    bp.xs.nblk = 0;                             // (the kernel reads the grid)
  }
  hipStream_t stream = cur_stream();
  with_t(dt_of(y2), [&](auto tag) {
    typedef decltype(tag) T;
    T* po = p2_out.has_value() ? dptr<T>(*p2_out) : nullptr;
    uint8_t* io = idx2_out.has_value() ? idx2_out->data_ptr<uint8_t>() : nullptr;
    T* xo = xh2_out.has_value() ? dptr<T>(*xh2_out) : nullptr;
    auto go = [&](auto nmax) {
      hipLaunchKernelGGL((head_fwd_kernel<T, 32, 14, 14, decltype(nmax)::value>), dim3(B), dim3(HF), 0, stream,
                         dptr<T>(y2), bp, wfc.data_ptr<float>(), bfc.data_ptr<float>(), dptr<T>(logits), po, io, xo,
                         N);
    };
    if (N <= 16) go(std::integral_constant<int, 16>{});
    else go(std::integral_constant<int, 64>{});
  });
  DPA_CHECK_LAUNCH();
}

size_t head_bwd_lds(int64_t B, int64_t N) { return sizeof(float) * (size_t)(B * N + N * 49 + B * 49); }

// fc backward + BN2 backward sums (local, complete per channel).
void head_bwd(at::Tensor dlogits, at::Tensor wfc, at::Tensor p2, at::Tensor idx2, at::Tensor xh2, at::Tensor dwfc,
              at::Tensor dbfc, at::Tensor dgamma2, at::Tensor dbeta2, at::Tensor bsum2, at::Tensor dp2) {
  DPA_CHECK_INPUT(dlogits); DPA_CHECK_INPUT(p2); DPA_CHECK_INPUT(dp2);
  const int B = (int)p2.size(0), N = (int)wfc.size(0);
  TORCH_CHECK(p2.numel() == (int64_t)B * 1568 && dp2.numel() == p2.numel() && xh2.numel() == p2.numel());
  TORCH_CHECK(dlogits.numel() == (int64_t)B * N);
  TORCH_CHECK(dlogits.scalar_type() == p2.scalar_type() && dp2.scalar_type() == p2.scalar_type());
  TORCH_CHECK(bsum2.numel() == 64 && dwfc.numel() == wfc.numel() && dbfc.numel() == N);
  const size_t lds = head_bwd_lds(B, N);
  TORCH_CHECK(lds <= 64 * 1024, "fused head backward: batch too large for LDS (B*N)");
  if (B == 0) return;
  with_t(dt_of(p2), [&](auto tag) {
    typedef decltype(tag) T;
    hipLaunchKernelGGL((head_bwd_kernel<T, 32, 14, 14>), dim3(32), dim3(NTHR_HB), lds, cur_stream(),
                       dptr<T>(dlogits), wfc.data_ptr<float>(), dptr<T>(p2), idx2.data_ptr<uint8_t>(), dptr<T>(xh2), B,
                       N, dwfc.data_ptr<float>(), dbfc.data_ptr<float>(), dgamma2.data_ptr<float>(),
                       dbeta2.data_ptr<float>(), bsum2.data_ptr<float>(), dptr<T>(dp2));
  });
  DPA_CHECK_LAUNCH();
}

static void check_conv1_pack(const at::Tensor& x, const at::Tensor& w1, const at::Tensor& b1, const at::Tensor& y1,
                             const at::Tensor& w2, const at::Tensor& wpk_f, const at::Tensor& wpk_d) {
  const int64_t B = x.size(0);
  TORCH_CHECK(x.size(1) == 1 && x.size(2) == 28 && x.size(3) == 28 && w1.numel() == 16 * 25 && b1.numel() == 16,
              "fused conv1 expects the ConvNet shapes");
  TORCH_CHECK(w2.numel() == 32 * 16 * 25 && w2.scalar_type() == at::kFloat && w1.scalar_type() == at::kFloat);
  TORCH_CHECK(y1.numel() == (int64_t)B * 16 * 784 && y1.scalar_type() == x.scalar_type());
  TORCH_CHECK(wpk_f.numel() == cb::W2F_LEN && wpk_d.numel() == cb::W2D_LEN &&
              wpk_f.scalar_type() == x.scalar_type() && wpk_d.scalar_type() == x.scalar_type());
}

// The head's fc pack (cb::pack_fc) hosted by a conv1 launch: fills pk and returns the launch's
// extra workgroups, cb::fcp_nm(N); 0 without a buffer (the grid and the kernel's path are then
// what they were).  bf16 / fp16 only: the fp32 head reads the master weights as they are.
template <typename T>
static int fc_pack_args(cb::WPack<T>& pk, const c10::optional<at::Tensor>& wfc, const c10::optional<at::Tensor>& wfc_pk,
                        at::ScalarType st) {
  if (!wfc_pk.has_value()) return 0;
  TORCH_CHECK(wfc.has_value(), "fc pack: wfc and wfc_pk go together");
  DPA_CHECK_INPUT(*wfc); DPA_CHECK_INPUT(*wfc_pk);
  TORCH_CHECK(st != at::kFloat, "fc pack: bf16 / fp16 only");
  TORCH_CHECK(wfc->scalar_type() == at::kFloat && wfc->dim() == 2 && wfc->size(1) == cb::FCP_K && wfc->size(0) >= 1 &&
              wfc->size(0) <= 16, "fc pack: fp32 fc.weight [N <= 16][1568]");
  const int N = (int)wfc->size(0), NM = cb::fcp_nm(N);
  TORCH_CHECK(wfc_pk->scalar_type() == st && wfc_pk->numel() == cb::fcp_len(NM), "fc pack: wfc_pk holds [256][", NM,
              "][8] elements of the compute dtype");
  pk.wfc = wfc->data_ptr<float>();
  pk.fcp = dptr<T>(*wfc_pk);
  pk.N = N;
  pk.NM = NM;
  return NM;
}

// Layer-1 conv (+BN1 sums when training) whose launch also packs the layer-2 weights: B * SPLIT conv
// workgroups, then cb::W2P_WGS pack workgroups (cb::pack_w2), which write no fslab1 row; with
// wfc_pk, cb::fcp_nm(N) more that pack the head's fc weights (cb::pack_fc).
void conv1_fwd_pack(at::Tensor x, at::Tensor w1, at::Tensor b1, at::Tensor y1, c10::optional<at::Tensor> fslab1,
                    c10::optional<at::Tensor> fstats1, c10::optional<at::Tensor> shift1, at::Tensor w2,
                    at::Tensor wpk_f, at::Tensor wpk_d, c10::optional<at::Tensor> wfc,
                    c10::optional<at::Tensor> wfc_pk) {
  DPA_CHECK_INPUT(x); DPA_CHECK_INPUT(w1); DPA_CHECK_INPUT(b1); DPA_CHECK_INPUT(y1); DPA_CHECK_INPUT(w2);
  DPA_CHECK_INPUT(wpk_f); DPA_CHECK_INPUT(wpk_d);
  const int B = (int)x.size(0);
  typedef cb::SH<0> S;
  check_conv1_pack(x, w1, b1, y1, w2, wpk_f, wpk_d);
  const bool st = fslab1.has_value();
  if (st)
    TORCH_CHECK(fslab1->numel() == (int64_t)B * S::SPLIT * cb::fslab_row(16) && fstats1->numel() == cb::stats_len(16) &&
                shift1->numel() == 16);
  if (B == 0) return;
  with_t(dt_of(x), [&](auto tag) {
    typedef decltype(tag) T;
    cb::WPack<T> pk{w2.data_ptr<float>(), dptr<T>(wpk_f), dptr<T>(wpk_d)};
    const int nfcp = fc_pack_args<T>(pk, wfc, wfc_pk, x.scalar_type());
    cb::GatherIn gin;  // no gather: just the conv workgroup count (the pack role starts behind it)
    gin.nimg = B;
    if (st)
      hipLaunchKernelGGL((cb::conv5x5_kernel<T, 1, 16, 28, 28, 0, 0, 0, 2>), dim3(B * S::SPLIT + cb::W2P_WGS + nfcp),
                         dim3(cb::NTHR), 0, cur_stream(), dptr<T>(x), w1.data_ptr<float>(), b1.data_ptr<float>(),
                         dptr<T>(y1), fslab1->data_ptr<float>(), fstats1->data_ptr<float>(),
                         shift1->data_ptr<float>(), S::SPLIT, PoolIn<T>{}, BwdIn<T>{}, BwdEpi<T>{}, nullptr, pk, gin);
    else
      hipLaunchKernelGGL((cb::conv5x5_kernel<T, 1, 16, 28, 28, 1, 0, 0, 2>), dim3(B * S::SPLIT + cb::W2P_WGS + nfcp),
                         dim3(cb::NTHR), 0, cur_stream(), dptr<T>(x), w1.data_ptr<float>(), b1.data_ptr<float>(),
                         dptr<T>(y1), nullptr, nullptr, nullptr, S::SPLIT, PoolIn<T>{}, BwdIn<T>{}, BwdEpi<T>{},
                         nullptr, pk, gin);
  });
  DPA_CHECK_LAUNCH();
}

// conv1_fwd_pack with the batch gather fused in (training; cb::GatherIn): x and lab_out
// are the loader's batch buffers, filled by this launch from the HBM-resident dataset
// at the device step counter, which the launch then advances (data.hip protocol).
void conv1_fwd_pack_gather(at::Tensor x, at::Tensor w1, at::Tensor b1, at::Tensor y1, at::Tensor fslab1,
                           at::Tensor fstats1, at::Tensor shift1, at::Tensor w2, at::Tensor wpk_f, at::Tensor wpk_d,
                           at::Tensor imgs, at::Tensor labels, at::Tensor order, at::Tensor ctr, at::Tensor lab_out,
                           double scale, double shift, c10::optional<at::Tensor> wfc,
                           c10::optional<at::Tensor> wfc_pk) {
  DPA_CHECK_INPUT(x); DPA_CHECK_INPUT(w1); DPA_CHECK_INPUT(b1); DPA_CHECK_INPUT(y1); DPA_CHECK_INPUT(w2);
  DPA_CHECK_INPUT(wpk_f); DPA_CHECK_INPUT(wpk_d); DPA_CHECK_INPUT(imgs); DPA_CHECK_INPUT(labels);
  DPA_CHECK_INPUT(order); DPA_CHECK_INPUT(ctr); DPA_CHECK_INPUT(lab_out);
  const int B = (int)x.size(0);
  typedef cb::SH<0> S;
  TORCH_CHECK(imgs.scalar_type() == at::kByte && imgs.dim() == 3 && imgs.size(1) == 28 && imgs.size(2) == 28,
              "gather: uint8 [N][28][28] dataset");
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.numel() == imgs.size(0));
  TORCH_CHECK(order.scalar_type() == at::kLong && ctr.scalar_type() == at::kInt && ctr.numel() >= 2);
  TORCH_CHECK(lab_out.scalar_type() == at::kLong && lab_out.numel() == B);
  check_conv1_pack(x, w1, b1, y1, w2, wpk_f, wpk_d);
  TORCH_CHECK(fslab1.numel() == (int64_t)B * S::SPLIT * cb::fslab_row(16) && fstats1.numel() == cb::stats_len(16) &&
              shift1.numel() == 16);
  if (B == 0) return;
  cb::GatherIn gin;
  gin.imgs = imgs.data_ptr<uint8_t>();
  gin.labels = labels.data_ptr<int64_t>();
  gin.order = order.data_ptr<int64_t>();
  gin.order_len = order.numel();
  gin.ctr = ctr.data_ptr<int>();
  gin.lab_out = lab_out.data_ptr<int64_t>();
  gin.scale = (float)scale;
  gin.shift = (float)shift;
  gin.nimg = (int)B;
  with_t(dt_of(x), [&](auto tag) {
    typedef decltype(tag) T;
    cb::WPack<T> pk{w2.data_ptr<float>(), dptr<T>(wpk_f), dptr<T>(wpk_d)};
    const int nfcp = fc_pack_args<T>(pk, wfc, wfc_pk, x.scalar_type());
    hipLaunchKernelGGL((cb::conv5x5_kernel<T, 1, 16, 28, 28, 0, 3, 0, 2>), dim3(B * S::SPLIT + cb::W2P_WGS + nfcp),
                       dim3(cb::NTHR), 0, cur_stream(), dptr<T>(x), w1.data_ptr<float>(), b1.data_ptr<float>(),
                       dptr<T>(y1), fslab1.data_ptr<float>(), fstats1.data_ptr<float>(), shift1.data_ptr<float>(),
                       S::SPLIT, PoolIn<T>{}, BwdIn<T>{}, BwdEpi<T>{}, nullptr, pk, gin);
  });
  DPA_CHECK_LAUNCH();
}

// Workgroups per image of the conv2 data gradient, chosen per launch.
// fp32: 4 everywhere; its 16x16x4 MFMA chains are 4x as long (profiles/r6bf_fp32_dgrad_split_ab.txt).
// bf16 / fp16: 4 when the launch exchanges nothing in-kernel (xc null: one rank, or SyncBN
// all-reduced between the launches), 2 when its site is active.  A quarter image per workgroup
// runs one m-tile per wave (MFMA loop 2.0 -> 1.2 us, profiles/conv2_rowwin_ab.txt; the step:
// profiles/dgrad_rows_ab.txt), but the merged backward launch then has 128 + 128 + 7 = 263
// workgroups at batch 32, more than sites_resident() accepts at 2 per CU (co_resident keeps one
// in reserve: 256), and two ranks sharing a card would not fit it together -- so a site launch
// keeps the 2-way grid, LDS and occupancy it always had, and set_site_grid / site_grid_fits /
// sites_resident speak of that grid (kDgradSiteSplitT).
// The two kinds of launch still agree bit for bit: bslab1 has one row per image QUARTER
// (cb::BwdEpi), 4 B rows built by the same operations at either split, so the consumer of the
// rows (the conv1 weight gradient's bn_bwd_coef) cannot tell which launch wrote them.
// The staging pass is one iteration per lane at 2 and at 4 (5 pooled rows x 7 x 4 channel
// groups = 140 windows of 256 lanes): the window shortens no chain there, it removes loads.
// The kernels take the split as a template constant S; `split` arguments: 0 = the rule above,
// 2 / 4 force it (4 on an active site is refused).  DPA_DGRAD2_SPLIT=2 in the environment makes
// the rule answer 2 for bf16 / fp16 as well (A/B runs); it is read once per process, at the first
// launch, so a process runs one setting.  fp32 has no knob any more: the epilogue's shapes follow
// from the split (conv5x5_body ES, 2 or 4), and 4 is its only instantiation.
template <typename T>
constexpr int kDgradSiteSplitT = std::is_same<T, float>::value ? 4 : 2;  // the split of a site launch
static int dgrad_split(bool fp32, bool site, int64_t split, const char* what) {
  TORCH_CHECK(split == 0 || split == 2 || split == 4, what, ": split is 0 (by rule), 2 or 4");
  if (fp32) {
    TORCH_CHECK(split != 2, what, ": the fp32 data gradient runs 4 workgroups per image");
    return 4;
  }
  TORCH_CHECK(!(site && split == 4), what, ": a launch with an in-kernel exchange site runs 2 workgroups per image");
  if (split != 0) return (int)split;
  if (site) return 2;
  static const bool env2 = [] {
    const char* e = std::getenv("DPA_DGRAD2_SPLIT");
    return e != nullptr && std::atoi(e) == 2;
  }();
  return env2 ? 2 : 4;
}
// runs f(std::integral_constant<int, S>) for the launch's split (fp32 instantiates 4 alone)
template <typename T, typename F>
static void with_dgrad_split(int ds, F&& f) {
  if constexpr (std::is_same<T, float>::value) {
    f(std::integral_constant<int, 4>{});
  } else {
    if (ds == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 4>{});
  }
}
template <int S>
constexpr int kDgrad2WR = conv2_wr<S, true>();  // whole 2x2 windows: even rows
// the data-gradient role's kernel body, one spelling for every launch that hosts it
template <typename T, bool DYN, int S>
__device__ __forceinline__ void conv2_dgrad_role(const T* __restrict__ wpk_d, T* __restrict__ dp1,
                                                 const BwdIn<T>& bi_d, const BwdEpi<T>& ep, int bid) {
  cb::conv5x5_body<T, 32, 16, 14, 14, 2, 2, 1, 1, DYN, kDgrad2WR<S>, S>(nullptr, nullptr, nullptr, dp1, nullptr,
                                                                        nullptr, nullptr, S, PoolIn<T>{}, bi_d, ep,
                                                                        wpk_d, cb::WPack<T>{}, bid);
}
// rows of bslab1: one per image quarter, whatever the dtype and the split
int64_t dgrad2_rows(int64_t B, bool fp32) {
  (void)fp32;
  return B * cb::EPI_QUARTERS;
}
// workgroups of the data-gradient role in a launch with (site) or without an active exchange site
int64_t dgrad2_wgs(int64_t B, bool fp32, bool site) { return B * dgrad_split(fp32, site, 0, "dgrad2_wgs"); }

// [pool2/ReLU2/BN2 backward] -> conv2 data grad -> dp1 (+ BN1 partial sums rows).
void conv2_dgrad(at::Tensor wpk_d, at::Tensor y2, at::Tensor dp2, at::Tensor idx2, at::Tensor fstats2,
                 at::Tensor gsum2, at::Tensor g2, double eps2, at::Tensor dp1, at::Tensor idx1, at::Tensor xh1,
                 at::Tensor bslab1, XcPtr xc, int64_t split) {
  DPA_CHECK_INPUT(y2); DPA_CHECK_INPUT(dp1); DPA_CHECK_INPUT(wpk_d);
  TORCH_CHECK(wpk_d.numel() == cb::W2D_LEN && wpk_d.scalar_type() == y2.scalar_type(),
              "packed conv2 data-grad weights");
  const int B = (int)y2.size(0);
  TORCH_CHECK(y2.size(1) == 32 && y2.size(2) == 14 && dp2.numel() == (int64_t)B * 32 * 49);
  TORCH_CHECK(dp1.numel() == (int64_t)B * 16 * 196 && idx1.numel() == dp1.numel() && xh1.numel() == dp1.numel());
  TORCH_CHECK(bslab1.numel() == dgrad2_rows(B, y2.scalar_type() == at::kFloat) * 32, "BN1 partial-sum slab size");
  const int ds = dgrad_split(y2.scalar_type() == at::kFloat, (bool)xc, split, "conv2_dgrad");
  if (B == 0) return;
  with_t(dt_of(y2), [&](auto tag) {
    typedef decltype(tag) T;
    BwdIn<T> bi = bwd_in<T>(dp2, idx2, y2, fstats2, gsum2, c10::nullopt, g2, eps2, 32, c10::nullopt, c10::nullopt);
    bi.xs = site_of(xc, xgmi::kSiteBwd2Dgrad);
    xgmi::set_site_grid(bi.xs, B * ds, "conv2_dgrad");
    BwdEpi<T> ep{idx1.data_ptr<uint8_t>(), dptr<T>(xh1), bslab1.data_ptr<float>()};
    with_dgrad_split<T>(ds, [&](auto sc) {
      constexpr int S = decltype(sc)::value;
      conv2_row_window(kDgrad2WR<S>, S, true, "conv2_dgrad");
      hipLaunchKernelGGL((cb::conv5x5_kernel<T, 32, 16, 14, 14, 2, 2, 1, 1, kDgrad2WR<S>, S>), dim3(B * S),
                         dim3(cb::NTHR), 0, cur_stream(), nullptr, nullptr, nullptr, dptr<T>(dp1), nullptr, nullptr,
                         nullptr, S, PoolIn<T>{}, bi, ep, dptr<T>(wpk_d), cb::WPack<T>{});
    });
  });
  DPA_CHECK_LAUNCH();
}

// The backward through [BN2 -> ReLU2 -> pool2] feeds two independent products of
// layer 2: the data grad (-> dp1 + BN1 partial sums, 2 or 4 workgroups per
// image: dgrad_split) and the weight-grad partials.  One launch hosts both roles -- workgroups
// [0, ndg) the data grad, [ndg, grid) the weight grad -- so they overlap on the chip
// instead of running back to back (each alone fills only 64 / 128 of the 256 CUs at
// B = 32) and one kernel boundary disappears.
//
// The weight-grad role is decomposed by OUTPUT SLICE: a workgroup is (image, 16-channel
// output tile, input-channel slice of WG2_NSL) with the whole image as its K range
// (cb::conv5x5_wgrad_body NSL), 2 * WG2_NSL workgroups per image, and an image yields ONE
// slab row: wslab2 is [B][12832] fp32.
#ifndef DPA_WG2_NSL
#define DPA_WG2_NSL 2
#endif
constexpr int WG2_NSL = DPA_WG2_NSL;
static_assert(WG2_NSL == 1 || WG2_NSL == 2, "conv2 weight gradient: 1 or 2 input-channel slices");
constexpr int WG1_ROWS_ = 4;
constexpr int WG2_PER_IMG = 2 * WG2_NSL;
int64_t wgrad_bn_rows(int64_t layer, int64_t B);
// workgroups of the conv2 weight-gradient role (its grid share, site grid and residency)
static int64_t wgrad2_wgs(int64_t B) { return B * WG2_PER_IMG; }

// the conv2 weight-gradient role of one workgroup (bid within the role)
template <typename T, bool DYN>
__device__ __forceinline__ void conv2_wgrad_role(const T* __restrict__ p1, float* __restrict__ wslab2,
                                                 const BwdIn<T>& bi_w, int bid) {
  cb::conv5x5_wgrad_body<T, 16, 32, 14, 14, 14, 2, false, DYN, WG2_NSL>(p1, nullptr, wslab2, WG2_PER_IMG, bi_w, bid);
}
template <typename T>
constexpr size_t conv2_wgrad_lds() {
  return cb::WgradLds<T, 16, 32, 14, 14, 14, WG2_NSL>::bytes;
}
template <typename T>
__global__ void __launch_bounds__(cb::NTHR)
conv2_wgrad_kernel(const T* __restrict__ p1, float* __restrict__ wslab2, BwdIn<T> bi_w) {
  conv2_wgrad_role<T, false>(p1, wslab2, bi_w, (int)blockIdx.x);
}
// fc weight / bias gradient of the per-image head (csrc/kernels/convnet_head.hip): the head's
// one reduction over the batch, computed by extra workgroups of the conv2 backward launch
// (which needs none of it) instead of on the head's critical path:
//   dW[n][k] = sum_b dls[b][n] * p2[b][k],   db[n] = sum_b dls[b][n]
// dls = d(scale * loss)/dlogits and p2 = the pooled features, both in the storage dtype
// (autocast's operands); fp32 accumulation in batch order.
template <typename T>
struct FcW {
  const T* dls;  // [B][N]
  const T* p2;   // [B][K]
  float* dw;     // [N][K]
  float* db;     // [N]
  int B = 0, N = 0;
  GradChk chk;   // producer-side check (common.h)
};
constexpr int FC_K = 32 * 49;
constexpr int FC_COLS = cb::NTHR;  // columns per workgroup, one per lane
constexpr int FC_BMAX = 64, FC_NMAX = 16;
constexpr int FC_BLOCKS = (FC_K + FC_COLS - 1) / FC_COLS;

template <typename T>
__device__ __forceinline__ void fc_wgrad_body(const FcW<T>& f, int wg) {
  __shared__ __attribute__((aligned(16))) float dl_s[FC_BMAX][FC_NMAX];
  const int tid = threadIdx.x;
  const int col = wg * FC_COLS + tid, cc = min(col, FC_K - 1);
  const int B = f.B, N = f.N;
  const bool chk = f.chk.word != nullptr;  // producer-side check (common.h GradChk)
  // the dls table (B x N, zero-padded to 16 classes) through LDS, broadcast reads below
  for (int e = tid; e < FC_BMAX * FC_NMAX; e += cb::NTHR) {
    const int b = e / FC_NMAX, n = e % FC_NMAX;
    const float v = Cvt<T>::to_f(f.dls[min(b, B - 1) * N + min(n, N - 1)]);
    dl_s[b][n] = (b < B && n < N) ? v : 0.f;
  }
  float acc[FC_NMAX];
#pragma unroll
  for (int n = 0; n < FC_NMAX; ++n) acc[n] = 0.f;
  __syncthreads();
  for (int b0 = 0; b0 < B; b0 += 32) {  // 32 rows in flight per batch (one batch at B <= 32)
    float pv[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const int b = b0 + u;
      pv[u] = Cvt<T>::to_f(f.p2[(size_t)min(b, B - 1) * FC_K + cc]) * (b < B ? 1.f : 0.f);
    }
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const f32x4* row = reinterpret_cast<const f32x4*>(dl_s[min(b0 + u, FC_BMAX - 1)]);
#pragma unroll
      for (int q = 0; q < FC_NMAX / 4; ++q) {
        const f32x4 d = row[q];
        acc[4 * q + 0] += d[0] * pv[u];
        acc[4 * q + 1] += d[1] * pv[u];
        acc[4 * q + 2] += d[2] * pv[u];
        acc[4 * q + 3] += d[3] * pv[u];
      }
    }
  }
  bool bad = false;
  if (col < FC_K) {
#pragma unroll
    for (int n = 0; n < FC_NMAX; ++n)
      if (n < N) {
        f.dw[(size_t)n * FC_K + col] = acc[n];
        bad |= GradChk::bad(acc[n], f.chk.bound);
      }
  }
  if (wg == 0 && tid < N) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dl_s[b][tid];
    f.db[tid] = a;
    bad |= GradChk::bad(a, f.chk.bound);
  }
  if (chk) f.chk.flag(bad);
}

template <typename T>
__global__ void __launch_bounds__(cb::NTHR) fc_wgrad_kernel(FcW<T> f) { fc_wgrad_body<T>(f, (int)blockIdx.x); }

template <typename T, int S>
__global__ void __launch_bounds__(cb::NTHR)
conv2_bwd_kernel(const T* __restrict__ wpk_d, T* __restrict__ dp1, BwdIn<T> bi_d, BwdEpi<T> ep,
                 const T* __restrict__ p1, float* __restrict__ wslab2, BwdIn<T> bi_w, int ndg, int nwg, FcW<T> fw) {
  const int bid = (int)blockIdx.x;
  if (bid < ndg)
    conv2_dgrad_role<T, false, S>(wpk_d, dp1, bi_d, ep, bid);
  else if (bid < ndg + nwg)
    conv2_wgrad_role<T, false>(p1, wslab2, bi_w, bid - ndg);
  else
    fc_wgrad_body<T>(fw, bid - ndg - nwg);
}

// fp32: the same three roles in ONE launch, with the big tiles of both conv roles in
// dynamic LDS (cb::conv5x5_body / conv5x5_wgrad_body DYN): each workgroup runs one role,
// so the launch needs the largest role's tiles (~114 KB) instead of the 173 KB sum of
// the static arrays, which does not fit a CU's 160 KB -- the reason fp32 ran the data
// gradient and the weight gradient as two launches, one after the other, each on at
// most half the CUs (profiles/r6g_cn_steady_fp32.txt: 16.7 + 15.2 us).
template <typename T, int S>
__global__ void __launch_bounds__(cb::NTHR)
conv2_bwd_dyn_kernel(const T* __restrict__ wpk_d, T* __restrict__ dp1, BwdIn<T> bi_d, BwdEpi<T> ep,
                     const T* __restrict__ p1, float* __restrict__ wslab2, BwdIn<T> bi_w, int ndg, int nwg,
                     FcW<T> fw) {
  const int bid = (int)blockIdx.x;
  if (bid < ndg)
    conv2_dgrad_role<T, true, S>(wpk_d, dp1, bi_d, ep, bid);
  else if (bid < ndg + nwg)
    conv2_wgrad_role<T, true>(p1, wslab2, bi_w, bid - ndg);
  else
    fc_wgrad_body<T>(fw, bid - ndg - nwg);
}

template <typename T>
constexpr size_t conv2_bwd_dyn_bytes() {
  return std::max(cb::conv5x5_dyn_bytes<T, 32, 16, 14, 14>(), conv2_wgrad_lds<T>());
}

// DPA_FP32_MERGED_BWD=0: the two fp32 launches below (A/B runs)
static bool fp32_merged_bwd() {
  static const bool on = [] {
    const char* e = std::getenv("DPA_FP32_MERGED_BWD");
    if (e != nullptr && std::atoi(e) == 0) return false;
    const size_t b = conv2_bwd_dyn_bytes<float>();
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<float, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)b) == hipSuccess;
  }();
  return on;
}

// bf16 / fp16: the merged launch with the conv tiles in dynamic LDS too -- the largest
// role's bytes per workgroup instead of the static arrays' sum: step 0.04859 -> 0.04823 ms
// over 5 same-box pairs (7 of 8 pairs faster; forced step unchanged,
// profiles/r6au_lp_dyn_bwd_ab.txt).  DPA_LP_DYN_BWD=0: the static-LDS kernel (A/B runs)
static bool lp_dyn_bwd() {
  static const bool on = [] {
    const char* e = std::getenv("DPA_LP_DYN_BWD");
    if (e != nullptr && std::atoi(e) == 0) return false;
    bool ok = true;
    for (const void* k : {reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<__hip_bfloat16, 2>),
                          reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<__hip_bfloat16, 4>),
                          reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<__half, 2>),
                          reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<__half, 4>)})
      ok = ok && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)std::max(conv2_bwd_dyn_bytes<__hip_bfloat16>(),
                                                   conv2_bwd_dyn_bytes<__half>())) == hipSuccess;
    return ok;
  }();
  return on;
}
template <typename T>  // whether the conv2 backward of T is the one dynamic-LDS launch
static bool conv2_bwd_dyn() { return std::is_same<T, float>::value ? fp32_merged_bwd() : lp_dyn_bwd(); }

// fp32 without the merged launch: the conv2 weight-gradient role and the fc weight gradient
// in one launch (the data-gradient role's static LDS does not fit beside the weight gradient's)
template <typename T>
__global__ void __launch_bounds__(cb::NTHR)
conv2_wgrad_fc_kernel(const T* __restrict__ p1, float* __restrict__ wslab2, BwdIn<T> bi_w, int nwg, FcW<T> fw) {
  const int bid = (int)blockIdx.x;
  if (bid < nwg)
    conv2_wgrad_role<T, false>(p1, wslab2, bi_w, bid);
  else
    fc_wgrad_body<T>(fw, bid - nwg);
}

template <typename T>
static FcW<T> fc_args(const c10::optional<at::Tensor>& dls, const c10::optional<at::Tensor>& p2,
                      const c10::optional<at::Tensor>& dw, const c10::optional<at::Tensor>& db, int B, at::ScalarType st) {
  FcW<T> f{};
  if (!dls.has_value()) return f;
  TORCH_CHECK(p2.has_value() && dw.has_value() && db.has_value(), "fc weight gradient: dls, p2, dw, db go together");
  DPA_CHECK_INPUT(*dls); DPA_CHECK_INPUT(*p2); DPA_CHECK_INPUT(*dw); DPA_CHECK_INPUT(*db);
  const int N = (int)(dls->numel() / std::max(B, 1));
  TORCH_CHECK(dls->numel() == (int64_t)B * N && N >= 1 && N <= FC_NMAX && B <= FC_BMAX, "fc weight gradient: dls [B][N <= 16]");
  TORCH_CHECK(dls->scalar_type() == st && p2->scalar_type() == st && p2->numel() == (int64_t)B * FC_K);
  TORCH_CHECK(dw->scalar_type() == at::kFloat && dw->numel() == (int64_t)N * FC_K && db->scalar_type() == at::kFloat &&
              db->numel() == N, "fc weight gradient: fp32 dw [N][1568], db [N]");
  f.dls = dptr<T>(*dls);
  f.p2 = dptr<T>(*p2);
  f.dw = dw->data_ptr<float>();
  f.db = db->data_ptr<float>();
  f.B = B;
  f.N = N;
  return f;
}

// fc weight / bias gradient as its own launch (fp32 / split-backward paths)
void fc_wgrad(at::Tensor dls, at::Tensor p2, at::Tensor dw, at::Tensor db) {
  const int B = (int)(p2.numel() / FC_K);
  if (B == 0) return;
  with_t(dt_of(p2), [&](auto tag) {
    typedef decltype(tag) T;
    FcW<T> f = fc_args<T>(dls, p2, dw, db, B, p2.scalar_type());
    hipLaunchKernelGGL(fc_wgrad_kernel<T>, dim3(FC_BLOCKS), dim3(cb::NTHR), 0, cur_stream(), f);
  });
  DPA_CHECK_LAUNCH();
}

// The producer-side gradient check's words (optim/sgd.py prechecked AMP step; common.h
// GradChk): int32[2], [0] cleared by the head launch and set by any producer lane that
// writes a bad value, [1] the step's scale (recorded by the head launch).
static GradChk grad_chk_of(const c10::optional<at::Tensor>& chk, const XcPtr& xc) {
  GradChk g;
  if (!chk.has_value()) return g;
  DPA_CHECK_INPUT(*chk);
  TORCH_CHECK(chk->scalar_type() == at::kInt && chk->numel() == 2, "gradient check: int32[2] words");
  g.word = chk->data_ptr<int>();
  g.bound = 3.402823466e38f / (float)(xc ? xc->world() : 1);
  return g;
}

// [pool2/ReLU2/BN2 backward] -> {conv2 data grad -> dp1 (+BN1 partial sums), conv2 weight-grad partials}
// (+ with fc_*: the fc weight / bias gradient of the per-image head in extra workgroups).
// gsum2: rows of BN2 backward sums ([S1 | S2] per row, summed here); lsum2: this rank's rows
// when gsum2 was all-reduced; dg2 / dbe2: BN2's dgamma / dbeta, written from this rank's sums.
void conv2_bwd(at::Tensor wpk_d, at::Tensor y2, at::Tensor dp2, at::Tensor idx2, at::Tensor fstats2,
               at::Tensor gsum2, at::Tensor g2, double eps2, at::Tensor dp1, at::Tensor idx1, at::Tensor xh1,
               at::Tensor bslab1, at::Tensor p1, at::Tensor wslab2, XcPtr xc, c10::optional<at::Tensor> lsum2,
               c10::optional<at::Tensor> dg2, c10::optional<at::Tensor> dbe2, c10::optional<at::Tensor> fc_dls,
               c10::optional<at::Tensor> fc_p2, c10::optional<at::Tensor> fc_dw, c10::optional<at::Tensor> fc_db,
               c10::optional<at::Tensor> chk, int64_t split) {
  DPA_CHECK_INPUT(y2); DPA_CHECK_INPUT(dp1); DPA_CHECK_INPUT(wpk_d); DPA_CHECK_INPUT(p1); DPA_CHECK_INPUT(wslab2);
  TORCH_CHECK(wpk_d.numel() == cb::W2D_LEN && wpk_d.scalar_type() == y2.scalar_type(),
              "packed conv2 data-grad weights");
  const int B = (int)y2.size(0);
  TORCH_CHECK(y2.size(1) == 32 && y2.size(2) == 14 && dp2.numel() == (int64_t)B * 32 * 49);
  TORCH_CHECK(dp1.numel() == (int64_t)B * 16 * 196 && idx1.numel() == dp1.numel() && xh1.numel() == dp1.numel());
  TORCH_CHECK(p1.numel() == dp1.numel() && p1.scalar_type() == y2.scalar_type());
  TORCH_CHECK(bslab1.numel() == dgrad2_rows(B, y2.scalar_type() == at::kFloat) * 32, "BN1 partial-sum slab size");
  TORCH_CHECK(dg2.has_value() == dbe2.has_value(), "conv2_bwd: dg2 and dbe2 go together");
  if (dg2.has_value()) TORCH_CHECK(dg2->numel() == 32 && dbe2->numel() == 32 && dg2->scalar_type() == at::kFloat);
  if (xc) TORCH_CHECK(!lsum2.has_value(), "fused SyncBN exchange: gsum2 must be this rank's rows (no lsum2)");
  const int ds = dgrad_split(y2.scalar_type() == at::kFloat, (bool)xc, split, "conv2_bwd");
  const int ndg = B * ds, nwg = (int)wgrad2_wgs(B);
  TORCH_CHECK(wslab2.numel() == wgrad_bn_rows(2, B) * (32 * 400 + 32), "wgrad slab size");
  if (B == 0) return;
  with_t(dt_of(y2), [&](auto tag) {
    typedef decltype(tag) T;
    BwdIn<T> bd = bwd_in<T>(dp2, idx2, y2, fstats2, gsum2, lsum2, g2, eps2, 32, dg2, dbe2);
    BwdIn<T> bw = bd;
    bw.dgamma = bw.dbeta = nullptr;  // one writer: the data-gradient role's workgroup 0
    bd.xs = site_of(xc, xgmi::kSiteBwd2Dgrad);
    bw.xs = site_of(xc, xgmi::kSiteBwd2Wgrad);
    xgmi::set_site_grid(bd.xs, ndg, "conv2_bwd data gradient");  // each role's workgroups take
    xgmi::set_site_grid(bw.xs, nwg, "conv2_bwd weight gradient");  // tickets on their own site
    BwdEpi<T> ep{idx1.data_ptr<uint8_t>(), dptr<T>(xh1), bslab1.data_ptr<float>()};
    FcW<T> fw = fc_args<T>(fc_dls, fc_p2, fc_dw, fc_db, B, y2.scalar_type());
    const int nfc = fc_dls.has_value() ? FC_BLOCKS : 0;
    if (chk.has_value()) {  // every gradient this launch finishes: BN2's, the fc layer's
      TORCH_CHECK(nfc > 0 && dg2.has_value(), "gradient check: the launch with the fc role and BN2's gradients");
      bd.chk = fw.chk = grad_chk_of(chk, xc);
      bd.chk_coef = 1;
    }
    with_dgrad_split<T>(ds, [&](auto sc) {
      constexpr int S = decltype(sc)::value;
      conv2_row_window(kDgrad2WR<S>, S, true, "conv2_bwd data gradient");
      if (conv2_bwd_dyn<T>()) {  // one launch, the roles' tiles in dynamic LDS (the largest role's bytes)
        hipLaunchKernelGGL((conv2_bwd_dyn_kernel<T, S>), dim3(ndg + nwg + nfc), dim3(cb::NTHR),
                           conv2_bwd_dyn_bytes<T>(), cur_stream(), dptr<T>(wpk_d), dptr<T>(dp1), bd, ep, dptr<T>(p1),
                           wslab2.data_ptr<float>(), bw, ndg, nwg, fw);
      } else if constexpr (std::is_same<T, float>::value) {
        // fp32 static tiles: the two roles' LDS (173 KB) exceed one CU's 160 KB -> separate launches
        // (the fc weight gradient: extra workgroups of the weight-gradient launch; its site's
        // tickets are the nwg conv workgroups', set above)
        bd.xs.nblk = 0;  // the data-gradient launch is its site's whole grid (ndg: checked above)
        hipLaunchKernelGGL((cb::conv5x5_kernel<T, 32, 16, 14, 14, 2, 2, 1, 1, kDgrad2WR<S>, S>), dim3(ndg),
                           dim3(cb::NTHR), 0, cur_stream(), nullptr, nullptr, nullptr, dptr<T>(dp1), nullptr, nullptr,
                           nullptr, S, PoolIn<T>{}, bd, ep, dptr<T>(wpk_d), cb::WPack<T>{});
        hipLaunchKernelGGL(conv2_wgrad_fc_kernel<T>, dim3(nwg + nfc), dim3(cb::NTHR), 0, cur_stream(), dptr<T>(p1),
                           wslab2.data_ptr<float>(), bw, nwg, fw);
      } else {
        hipLaunchKernelGGL((conv2_bwd_kernel<T, S>), dim3(ndg + nwg + nfc), dim3(cb::NTHR), 0, cur_stream(),
                           dptr<T>(wpk_d), dptr<T>(dp1), bd, ep, dptr<T>(p1), wslab2.data_ptr<float>(), bw, ndg, nwg,
                           fw);
      }
    });
  });
  DPA_CHECK_LAUNCH();
}

// [pool/ReLU/BN backward of the block whose conv is (CIN->COUT, HxW)] -> weight-grad partials.
// layer 2: x = p1 [B,16,14,14], (y, dp, idx) = layer-2 tensors; layer 1: x = images, layer-1 tensors.
// Layer 1: weight-gradient row chunks (BN backward applied on the fly per chunk): more,
// shorter workgroups than one image each (B = 32 -> 32 workgroups for 256 CUs), one slab
// row per chunk.  Layer 2: output slices of whole images (conv2_wgrad_role above), one
// slab row per image.  wgrad_bn_rows: the ROWS of a layer's slab (what its consumers sum).
constexpr int WG1_ROWS = WG1_ROWS_;  // layer 1 (28 rows): 7 chunks per image
int64_t wgrad_bn_rows(int64_t layer, int64_t B) {
  TORCH_CHECK(layer == 1 || layer == 2);
  return B * (layer == 1 ? (28 + WG1_ROWS - 1) / WG1_ROWS : 1);
}

void conv_wgrad_bn(at::Tensor x, at::Tensor y, at::Tensor dp, at::Tensor idx, at::Tensor fstats, at::Tensor gsum,
                   c10::optional<at::Tensor> lsum, at::Tensor gamma, double eps, c10::optional<at::Tensor> dgamma,
                   c10::optional<at::Tensor> dbeta, at::Tensor wslab, XcPtr xc) {
  DPA_CHECK_INPUT(x); DPA_CHECK_INPUT(y);
  const int B = (int)y.size(0);
  const int cin = (int)x.size(1), cout = (int)y.size(1), H = (int)y.size(2);
  TORCH_CHECK(x.scalar_type() == y.scalar_type());
  if (B == 0) return;
  with_t(dt_of(y), [&](auto tag) {
    typedef decltype(tag) T;
    BwdIn<T> bi = bwd_in<T>(dp, idx, y, fstats, gsum, lsum, gamma, eps, cout, dgamma, dbeta);
    if (xc) {
      TORCH_CHECK(!lsum.has_value(), "fused SyncBN exchange: gsum must be this rank's rows (no lsum)");
      bi.xs = site_of(xc, cout == 32 ? xgmi::kSiteBwd2Wgrad : xgmi::kSiteBwd1);
    }
    if (cin == 16 && cout == 32 && H == 14) {
      TORCH_CHECK(wslab.numel() == wgrad_bn_rows(2, B) * (32 * 400 + 32), "wgrad slab size");
      hipLaunchKernelGGL(conv2_wgrad_kernel<T>, dim3((int)wgrad2_wgs(B)), dim3(cb::NTHR), 0, cur_stream(),
                         dptr<T>(x), wslab.data_ptr<float>(), bi);
    } else if (cin == 1 && cout == 16 && H == 28) {
      constexpr int ns = (28 + WG1_ROWS - 1) / WG1_ROWS;
      TORCH_CHECK(wslab.numel() == (int64_t)B * ns * (16 * 25 + 16), "wgrad slab size");
      hipLaunchKernelGGL((cb::conv5x5_wgrad_kernel<T, 1, 16, 28, 28, WG1_ROWS, 2>), dim3(B * ns), dim3(cb::NTHR),
                         0, cur_stream(), dptr<T>(x), nullptr, wslab.data_ptr<float>(), ns, bi);
    } else {
      TORCH_CHECK(false, "fused wgrad: shape not instantiated");
    }
  });
  DPA_CHECK_LAUNCH();
}

// BN1 bwd -> conv1 weight-grad partial rows (wslab1) AND, in extra workgroups, the
// column sums of the conv2 weight-grad slab into [dW2 | db2] (independent work that
// fills the CUs the 224 conv1 workgroups leave idle).  The conv1 slab's own column
// sums are left to the consumer: the fused AMP-SGD launch (optim.hip SlabSrc) or a
// slab_reduce launch.  A reduction workgroup owns SLAB2_K chunks of 16 columns (the conv2
// slab has one row per image: few rows per lane, so more columns per lane instead).
constexpr int SLAB2_K = 4;
template <typename T>
__global__ void __launch_bounds__(cb::NTHR)
wgrad1_slab2_kernel(const T* __restrict__ x, float* __restrict__ wslab1, BwdIn<T> bi, int nwg1,
                    const float* __restrict__ wslab2, int rows2, int n2, float* __restrict__ out2, GradChk rc) {
  constexpr int ns = (28 + WG1_ROWS_ - 1) / WG1_ROWS_;
  if ((int)blockIdx.x < nwg1)
    cb::conv5x5_wgrad_body<T, 1, 16, 28, 28, WG1_ROWS_, 2, true>(x, nullptr, wslab1, ns, bi, (int)blockIdx.x);
  else
    cb::slab_reduce_chunks_body<SLAB2_K>(wslab2, rows2, n2, out2, (int)blockIdx.x - nwg1, rc);
}

void conv1_wgrad_slab2(at::Tensor x, at::Tensor y1, at::Tensor dp1, at::Tensor idx1, at::Tensor fstats1,
                       at::Tensor gsum, c10::optional<at::Tensor> lsum, at::Tensor g1, double eps1, at::Tensor dg1,
                       at::Tensor dbe1, at::Tensor wslab1, at::Tensor wslab2, at::Tensor out2, XcPtr xc,
                       c10::optional<at::Tensor> chk) {
  DPA_CHECK_INPUT(x); DPA_CHECK_INPUT(y1); DPA_CHECK_INPUT(wslab1); DPA_CHECK_INPUT(wslab2); DPA_CHECK_INPUT(out2);
  const int B = (int)y1.size(0);
  TORCH_CHECK(x.size(1) == 1 && y1.size(1) == 16 && y1.size(2) == 28 && x.scalar_type() == y1.scalar_type());
  const int nwg1 = (int)wgrad_bn_rows(1, B);
  constexpr int N1 = 16 * 25 + 16, N2 = 32 * 400 + 32;
  const int rows2 = (int)wgrad_bn_rows(2, B);
  TORCH_CHECK(wslab1.numel() == (int64_t)nwg1 * N1, "conv1_wgrad_slab2: conv1 slab size");
  TORCH_CHECK(wslab2.numel() == (int64_t)rows2 * N2 && out2.numel() == N2, "conv1_wgrad_slab2: conv2 slab sizes");
  if (B == 0) return;
  const int nred = (N2 + SLAB2_K * cb::SR_COLS - 1) / (SLAB2_K * cb::SR_COLS);
  with_t(dt_of(y1), [&](auto tag) {
    typedef decltype(tag) T;
    BwdIn<T> bi = bwd_in<T>(dp1, idx1, y1, fstats1, gsum, lsum, g1, eps1, 16, dg1, dbe1);
    if (xc) {
      TORCH_CHECK(!lsum.has_value(), "fused SyncBN exchange: gsum must be this rank's rows (no lsum)");
      bi.xs = site_of(xc, xgmi::kSiteBwd1);
      xgmi::set_site_grid(bi.xs, nwg1, "conv1_wgrad_slab2");  // the reduction workgroups take no tickets
    }
    GradChk rc;
    if (chk.has_value()) {  // BN1's gradients, conv1's partial rows, conv2's column sums
      rc = bi.chk = grad_chk_of(chk, xc);
      bi.chk_coef = 1;
      bi.chk_rows = 1;
      bi.chk_row_bound = rc.bound / (float)nwg1;
    }
    hipLaunchKernelGGL(wgrad1_slab2_kernel<T>, dim3(nwg1 + nred), dim3(cb::NTHR), 0, cur_stream(), dptr<T>(x),
                       wslab1.data_ptr<float>(), bi, nwg1, wslab2.data_ptr<float>(), rows2, N2,
                       out2.data_ptr<float>(), rc);
  });
  DPA_CHECK_LAUNCH();
}

// Whether every launch that exchanges SyncBN sums in-kernel (comm/xsite.h: all
// of its workgroups poll the peers' rows) is co-resident at batch B; if not,
// ops/convnet_fused.py all-reduces between the launches instead.
bool sites_resident(int64_t B, at::ScalarType st) {
  // every site launch must also fit its site's epoch words (comm/xgmi.h set_site_grid):
  // the conv1 weight gradient's 7 B workgroups pass kEpochWords at B >= 74
  bool ok = xgmi::site_grid_fits(wgrad_bn_rows(1, B)) && xgmi::site_grid_fits(wgrad2_wgs(B)) &&
            xgmi::site_grid_fits(dgrad2_wgs(B, st == at::kFloat, true)) &&
            xgmi::site_grid_fits(fwd2_split(st == at::kFloat) * B);
  auto chk = [&](const void* k, int64_t grid) { ok = ok && co_resident(k, (int)grid, cb::NTHR, 0); };
  with_t(dt_of(at::empty({0}, at::TensorOptions().dtype(st))), [&](auto tag) {
    typedef decltype(tag) T;
    chk(reinterpret_cast<const void*>(&cb::conv5x5_kernel<T, 16, 32, 14, 14, 0, 1, 0, 1, kFwd2WR<T>>),
        B * fwd2_split(std::is_same<T, float>::value));
    ok = ok && co_resident(reinterpret_cast<const void*>(&head_fwd_kernel<T, 32, 14, 14, 16>), (int)B, HF, 0) &&
         co_resident(reinterpret_cast<const void*>(&head_fwd_kernel<T, 32, 14, 14, 64>), (int)B, HF, 0);
    constexpr int S = kDgradSiteSplitT<T>;  // what a site launch runs (dgrad_split)
    chk(reinterpret_cast<const void*>(&cb::conv5x5_kernel<T, 32, 16, 14, 14, 2, 2, 1, 1, kDgrad2WR<S>, S>), B * S);
    if (conv2_bwd_dyn<T>())
      ok = ok && co_resident(reinterpret_cast<const void*>(&conv2_bwd_dyn_kernel<T, S>),
                             (int)(B * S + wgrad2_wgs(B) + FC_BLOCKS), cb::NTHR, conv2_bwd_dyn_bytes<T>());
    else if constexpr (!std::is_same<T, float>::value)
      chk(reinterpret_cast<const void*>(&conv2_bwd_kernel<T, S>), B * S + wgrad2_wgs(B) + FC_BLOCKS);
    chk(reinterpret_cast<const void*>(&conv2_wgrad_kernel<T>), wgrad2_wgs(B));
    chk(reinterpret_cast<const void*>(&cb::conv5x5_wgrad_kernel<T, 1, 16, 28, 28, WG1_ROWS, 2>),
        wgrad_bn_rows(1, B));
    chk(reinterpret_cast<const void*>(&wgrad1_slab2_kernel<T>), wgrad_bn_rows(1, B));
  });
  return ok;
}

}  // namespace cnf

void register_convnet_fused(pybind11::module& m) {
  namespace py = pybind11;
  auto s = m.def_submodule("convnet", "whole-ConvNet fused kernels");
  s.def("conv2_fwd", &cnf::conv2_fwd);
  s.def("head_fwd", &cnf::head_fwd);
  s.def("head_bwd", &cnf::head_bwd);
  s.def("head_bwd_lds", &cnf::head_bwd_lds);
  s.def("dgrad2_rows", &cnf::dgrad2_rows, py::arg("B"), py::arg("fp32") = false);
  s.def("dgrad2_wgs", &cnf::dgrad2_wgs, py::arg("B"), py::arg("fp32") = false, py::arg("site") = false);
  // wfc, wfc_pk (trailing, optional): the launch also packs the head's fc weights (cb::pack_fc)
  s.def("conv1_fwd_pack", &cnf::conv1_fwd_pack, py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("y1"),
        py::arg("fslab1"), py::arg("fstats1"), py::arg("shift1"), py::arg("w2"), py::arg("wpk_f"), py::arg("wpk_d"),
        py::arg("wfc") = py::none(), py::arg("wfc_pk") = py::none());
  s.def("conv1_fwd_pack_gather", &cnf::conv1_fwd_pack_gather, py::arg("x"), py::arg("w1"), py::arg("b1"),
        py::arg("y1"), py::arg("fslab1"), py::arg("fstats1"), py::arg("shift1"), py::arg("w2"), py::arg("wpk_f"),
        py::arg("wpk_d"), py::arg("imgs"), py::arg("labels"), py::arg("order"), py::arg("ctr"), py::arg("lab_out"),
        py::arg("scale"), py::arg("shift"), py::arg("wfc") = py::none(), py::arg("wfc_pk") = py::none());
  s.attr("FCP_LANES") = cb::FCP_LANES;
#ifdef DPA_TIMING
  s.def("read_stamps", []() {
    auto out = at::empty({DPA_MAX_STAMP_BLOCKS, DPA_NSTAMPS}, at::TensorOptions().dtype(at::kLong));
    DPA_CHECK_HIP(hipDeviceSynchronize());
    DPA_CHECK_HIP(hipMemcpyFromSymbol(out.data_ptr(), HIP_SYMBOL(dpa_stamps), sizeof(unsigned long long) *
                                      DPA_MAX_STAMP_BLOCKS * DPA_NSTAMPS));
    return out;
  });
  s.def("clear_stamps", []() {
    DPA_CHECK_HIP(hipDeviceSynchronize());
    std::vector<unsigned long long> z(DPA_MAX_STAMP_BLOCKS * DPA_NSTAMPS, 0ull);
    DPA_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dpa_stamps), z.data(), z.size() * sizeof(unsigned long long)));
  });
#endif
  s.attr("W2F_LEN") = cb::W2F_LEN;
  s.attr("W2D_LEN") = cb::W2D_LEN;
  // split (trailing, optional): data-gradient workgroups per image, 0 = by rule (cnf::dgrad_split)
  s.def("conv2_dgrad", &cnf::conv2_dgrad, py::arg("wpk_d"), py::arg("y2"), py::arg("dp2"), py::arg("idx2"),
        py::arg("fstats2"), py::arg("gsum2"), py::arg("g2"), py::arg("eps2"), py::arg("dp1"), py::arg("idx1"),
        py::arg("xh1"), py::arg("bslab1"), py::arg("xc"), py::arg("split") = 0);
  s.def("conv2_bwd", &cnf::conv2_bwd, py::arg("wpk_d"), py::arg("y2"), py::arg("dp2"), py::arg("idx2"),
        py::arg("fstats2"), py::arg("gsum2"), py::arg("g2"), py::arg("eps2"), py::arg("dp1"), py::arg("idx1"),
        py::arg("xh1"), py::arg("bslab1"), py::arg("p1"), py::arg("wslab2"), py::arg("xc"), py::arg("lsum2"),
        py::arg("dg2"), py::arg("dbe2"), py::arg("fc_dls"), py::arg("fc_p2"), py::arg("fc_dw"), py::arg("fc_db"),
        py::arg("chk"), py::arg("split") = 0);
  s.def("fc_wgrad", &cnf::fc_wgrad);
  s.def("conv_wgrad_bn", &cnf::conv_wgrad_bn);
  s.def("wgrad_bn_rows", &cnf::wgrad_bn_rows);
  s.def("sites_resident", &cnf::sites_resident);
  s.def("fwd2_split", &cnf::fwd2_split, py::arg("fp32"));
  s.def("conv1_wgrad_slab2", &cnf::conv1_wgrad_slab2);
}

}  // namespace dpa
