// Squeeze-and-excitation (Hu et al. 2018) fused with a bottleneck's residual add and ReLU, for
// NHWC bf16 / fp16 activations u, identity [N][HW][C] and fp32 master parameters W1 [Cr][C],
// b1 [Cr], W2 [C][Cr], b2 [C] read in-kernel (no pack launch, no WeightPack entry):
//   p = mean_hw u;  h = relu(p W1^T + b1);  s = sigmoid(h W2^T + b2);  y = relu(u * s + identity)
// and its backward (ops/se.py, models/resnet.py se_resnet50 / se_resnext50_32x4d).  C a multiple
// of 64 in [64, 2048], Cr a multiple of 4 in [4, 128], any N, H, W >= 1.  Everything between the
// activation reads and the activation writes is fp32; every sum has an order fixed by (C, Cr, HW, N)
// alone, never by the grid, and there are no atomics: the same inputs give the same bits.
//
// Common to the four activation kernels
//   * Channel blocks of CB = 64: a pixel's 64 channels are 128 contiguous bytes = eight 16-B
//     granules, one per lane (8 channels per lane), so a 256-thread workgroup has 32 pixel rows of
//     8 lanes and a wave reads 8 whole pixels (1 KB) per load instruction.  Each lane keeps UNR = 4
//     pixel rows in flight (all loads of a round issued before the first use).  128-channel blocks
//     (256-B runs, half the workgroups) were NOT built or measured.
//   * The two reductions (squeeze, excite_bwd_sums) give a workgroup one image x one channel block
//     and ALL its pixels: grid (C / 64, N).  HW is not split across workgroups, so there are no
//     partials to sum; at the models' shapes (batch 128) that is 512 .. 4096 workgroups.  A pixel
//     split for small N x large HW was not built: it needs a fourth forward launch or a finisher.
//   * The two elementwise kernels (excite, excite_bwd) give a workgroup one image x one channel
//     block x PIX = 256 consecutive pixels (two rounds of 4 rows per lane): grid (N * ranges, C / 64).
//     The per-workgroup prologue (below) is amortised over 32 KB of activations per tensor.
//     PIX = 128 / 512 were not measured.
//
// 1 squeeze            pool_kernel<T, false>: p[n][c] = (sum over pixels) / HW
//   registers  8 fp32 sums + 4 x 16-B loads per lane; a lane adds its pixels pr, pr+32, ... in order
//   LDS        32 x 64 fp32 row sums (8,192 B) + 4 x 64 (1,024 B): a two-level tree, rows 8q..8q+7
//              summed in order by wave q, then the four waves in order
// 2 fc1                gate_gemm_kernel<false>: h = relu(p W1^T + b1) on v_mfma_f32_16x16x4_f32
//   work split 256 threads own one 16-image x 16-hidden tile: grid (ceil(N/16), ceil(Cr/16)); rows
//              past N and columns past Cr are staged as zeros.  K = C runs in chunks of KC = 256
//              through LDS (a chunk is min(256, C): 64, 128 or 256); wave w takes the w-th quarter
//              of every chunk (4 .. 16 MFMAs per chunk), the four waves' tiles are summed in order.
//   LDS        A and B chunks 2 x 16 x 260 fp32 (33,280 B, row stride 260: a wave's 64 operand
//              reads hit 32 banks twice) + 4 x 256 fp32 wave tiles (4,096 B)
//   registers  one f32x4 accumulator.  fp32 MFMA because the masters are fp32 and p is fp32; the
//              bf16 rate buys nothing at 2 * N * C * Cr <= 67 MFLOP.  KC = 512 was not measured.
// 3 excite             excite_kernel<T>: y = relu(u * s + identity)
//   prologue   h[n][:] to LDS; lane (c = t >> 2, part = t & 3) sums W2[c][j] h[j] over j = 4 * (part
//              + 4 i) .. + 3 with 16-B loads (Cr a multiple of 16) or j = part + 4 i (otherwise), a DPP
//              sum over the 4 lanes, the sigmoid, s to LDS; pixel range 0 stores s[n][block] for the
//              backward.  There is no fc2 launch and the forward never reads s from memory.
//   LDS        128 + 64 fp32 (768 B).  registers: 8 gates + 2 x 4 x 16-B loads per lane.
// 4 excite_bwd_sums    pool_kernel<T, true>: ds = sum over pixels of g [y > 0] u, epilogue
//              dz2 = ds * s * (1 - s).  squeeze's split, LDS and tree; 3 x 4 loads in flight.
// 5 gate_bwd           gate_gemm_kernel<true>: dz1 = (dz2 W2) * [h > 0]: fc1's mirror (batch is M, hidden
//              is N, C is K); W2 [C][Cr] is staged transposed into the same [hidden][k] LDS chunk.
// 6 gate_wgrad         gate_wgrad_kernel: dW2[c][j] = sum_n dz2[n][c] h[n][j], dW1[j][c] = sum_n
//              dz1[n][j] p[n][c], db2, db1 on fp32 MFMA with the batch as K
//   work split grid (C / 64, ceil(Cr/16)) over OUTPUT tiles only: wave w owns channels 16 w .. + 15
//              of the block x 16 hidden units and both products (dW1 as its transpose, stored
//              transposed), so no cross-workgroup reduction exists.  K = N padded to a multiple of 4
//              with zeros, walked in index order.  db2 is the hidden-tile-0 workgroups' extra MFMA
//              against a ones operand, db1 the channel-block-0 wave-0's.
//   LDS        none: every operand element is read once, straight from memory, 64 B per 16 lanes.
//   registers  4 f32x4 accumulators.
// 7 excite_bwd         excite_bwd_kernel<T>: du = g [y > 0] s + dp / HW, d_identity = g [y > 0]
//   prologue   dz1[n][:] to LDS; lane (c = t & 63, part = t >> 6) sums dz1[j] W1[j][c] over the
//              part-th quarter of j (coalesced 256-B rows), four quarters summed in order, / HW.
//   LDS        128 + 4 x 64 + 64 fp32 (1,792 B).  registers: 8 gates + 8 dp + 2 x 4 loads per lane.
//
// Resources (scripts/resource_usage.py, gfx950, bf16 / fp16 where they differ): VGPRs, AGPRs, LDS
// bytes, waves per SIMD; scratch is 0 everywhere (no spills).
//   squeeze 47 / 40, 0, 9,216, 8    fc1, gate_bwd 26, 4, 37,376, 4    excite 42 / 40, 0, 768, 8
//   excite_bwd_sums 76 / 72, 0, 9,216, 6 / 7    gate_wgrad 16, 16, 0, 8    excite_bwd 55, 0, 1,792, 8
// Measured (profiles/se_bench.txt, MI355X, batch 128, bf16, hipGraph replay): the three forward
// launches together move the activation bytes at 5.06 / 4.54 / 3.78 / 1.86 TB/s at 256 x 56^2 /
// 512 x 28^2 / 1024 x 14^2 / 2048 x 7^2, the four backward launches at 3.79 / 3.26 / 2.87 / 1.37 TB/s
// (the BN kernels: 5.5-6 TB/s); 5.2-6.6x / 2.2-2.4x (7^2) faster than the torch composition.  The
// tile sizes above are the first ones built: no other CB, PIX, UNR or KC was measured, and the
// per-kernel split of those times was not measured.  At 7^2 a workgroup's prologue reads as
// many bytes of W2 / W1 (32 KB, from L2) as activation bytes per tensor (6 KB): the next lever there.
#include "common.h"

#include <map>
#include <mutex>
#include <string>

namespace dpa {
namespace se {

constexpr int CB = 64;     // channels per workgroup of the activation kernels
constexpr int ROWS = 32;   // pixel rows of a 256-thread workgroup (8 lanes each)
constexpr int UNR = 4;     // pixel rows a lane keeps in flight
constexpr int PIX = 256;   // pixels per workgroup of the elementwise kernels
constexpr int KC = 256;    // K chunk of the gate GEMMs
constexpr int KS = KC + 4; // LDS row stride of a chunk, floats
constexpr int MAXCR = 128;

template <typename T> __device__ __forceinline__ float up(unsigned short v);
template <> __device__ __forceinline__ float up<__hip_bfloat16>(unsigned short v) {
  return __builtin_bit_cast(float, (unsigned)v << 16);
}
template <> __device__ __forceinline__ float up<__half>(unsigned short v) {
  return (float)__builtin_bit_cast(_Float16, v);
}
template <typename T> __device__ __forceinline__ unsigned short down(float x) {
  return __builtin_bit_cast(unsigned short, MM<T>::cv(x));
}
__device__ __forceinline__ float relu(float v) { return v < 0.f ? 0.f : v; }  // NaN stays NaN

// ---- 1, 4: per-image channel sums -------------------------------------------------------------
// BWD = false: out[n][c] = (sum_p a[n][p][c]) / HW
// BWD = true : out[n][c] = (sum_p a[n][p][c] * [y[n][p][c] > 0] * u[n][p][c]) * s (1 - s)   (a = g)
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void pool_kernel(const T* __restrict__ a, const T* __restrict__ y,
                                                   const T* __restrict__ u, const float* __restrict__ s,
                                                   float* __restrict__ out, int HW, int C) {
  __shared__ float rows[ROWS][CB];
  __shared__ float part[4][CB];
  const int t = threadIdx.x, g8 = t & 7, pr = t >> 3;
  const int n = blockIdx.y, c0 = blockIdx.x * CB;
  const size_t base = (size_t)n * HW * C + c0 + 8 * g8;
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  float acc[8] = {};
  for (int p = pr; p < HW; p += ROWS * UNR) {
    u16x8 va[UNR], vy[UNR], vu[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int pp = p + ROWS * j;
      const bool ok = pp < HW;
      const size_t off = base + (size_t)(ok ? pp : p) * C;  // (p itself is in range)
      va[j] = *reinterpret_cast<const u16x8*>(a + off);
      if constexpr (BWD) {
        vy[j] = *reinterpret_cast<const u16x8*>(y + off);
        vu[j] = *reinterpret_cast<const u16x8*>(u + off);
        if (!ok) vu[j] = z;
      }
      if (!ok) va[j] = z;  // a zero term: + 0 (forward) or 0 * 0 (backward)
    }
#pragma unroll
    for (int j = 0; j < UNR; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if constexpr (BWD) {
          const float gm = up<T>(vy[j][i]) > 0.f ? up<T>(va[j][i]) : 0.f;
          acc[i] = __builtin_fmaf(gm, up<T>(vu[j][i]), acc[i]);
        } else {
          acc[i] += up<T>(va[j][i]);
        }
      }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) rows[pr][8 * g8 + i] = acc[i];
  __syncthreads();
  {
    const int c = t & 63, q = t >> 6;
    float v = rows[8 * q][c];
#pragma unroll
    for (int r = 1; r < 8; ++r) v += rows[8 * q + r][c];
    part[q][c] = v;
  }
  __syncthreads();
  if (t < CB) {
    const float v = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    const size_t o = (size_t)n * C + c0 + t;
    if (BWD) {
      const float sv = s[o];
      out[o] = v * (sv * (1.f - sv));
    } else {
      out[o] = v / (float)HW;
    }
  }
}

// ---- 2, 5: the gate GEMMs, batch x hidden over C -----------------------------------------------
// BWD = false: out[n][j] = relu(sum_c A[n][c] * B[j][c] + aux[j])        A = p,   B = W1, aux = b1
// BWD = true : out[n][j] = (sum_c A[n][c] * B[c][j]) * [aux[n][j] > 0]   A = dz2, B = W2, aux = h
template <bool BWD>
__global__ __launch_bounds__(256) void gate_gemm_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                        const float* __restrict__ aux, float* __restrict__ out,
                                                        int N, int C, int Cr) {
  __shared__ __attribute__((aligned(16))) float As[16 * KS];
  __shared__ __attribute__((aligned(16))) float Bs[16 * KS];
  __shared__ float red[4][256];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc = z4;
  for (int k0 = 0; k0 < C; k0 += KC) {
    const int kc = min(KC, C - k0), kq = kc >> 2;  // kc: 64, 128 or 256
    __syncthreads();
    for (int i = t; i < 16 * kq; i += 256) {
      const int r = i / kq, c4 = i - r * kq;
      f32x4 va = z4, vb = z4;
      if (m0 + r < N) va = *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + r) * C + k0 + 4 * c4);
      if (!BWD && j0 + r < Cr) vb = *reinterpret_cast<const f32x4*>(B + (size_t)(j0 + r) * C + k0 + 4 * c4);
      *reinterpret_cast<f32x4*>(As + r * KS + 4 * c4) = va;
      if (!BWD) *reinterpret_cast<f32x4*>(Bs + r * KS + 4 * c4) = vb;
    }
    if (BWD)
      for (int i = t; i < 16 * kc; i += 256) {
        const int jj = i & 15, kk = i >> 4;
        Bs[jj * KS + kk] = j0 + jj < Cr ? B[(size_t)(k0 + kk) * Cr + j0 + jj] : 0.f;
      }
    __syncthreads();
    const int kb = wv * kq;
    for (int kk = kb; kk < kb + kq; kk += 4)
      acc = mfma_f32_16x16x4(As[li * KS + kk + q], Bs[li * KS + kk + q], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wv][(4 * q + r) * 16 + li] = acc[r];
  __syncthreads();
  const int n = m0 + (t >> 4), j = j0 + (t & 15);
  if (n < N && j < Cr) {
    const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    const size_t o = (size_t)n * Cr + j;
    out[o] = BWD ? (aux[o] > 0.f ? v : 0.f) : relu(v + aux[j]);
  }
}

// ---- 3: gate and residual -----------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void excite_kernel(const T* __restrict__ u, const T* __restrict__ idn,
                                                     const float* __restrict__ h, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ s_out,
                                                     T* __restrict__ y, int HW, int C, int Cr, int ranges) {
  __shared__ __attribute__((aligned(16))) float hs[MAXCR];
  __shared__ float ss[CB];
  const int t = threadIdx.x;
  const int n = blockIdx.x / ranges, rg = blockIdx.x - n * ranges, c0 = blockIdx.y * CB;
  if (t < Cr) hs[t] = h[(size_t)n * Cr + t];
  __syncthreads();
  {
    const int c = t >> 2, pt = t & 3;
    const float* wr = w2 + (size_t)(c0 + c) * Cr;
    float a = 0.f;
    if ((Cr & 15) == 0) {
      for (int j = 4 * pt; j < Cr; j += 16) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wr + j);
        const f32x4 hv = *reinterpret_cast<const f32x4*>(hs + j);
#pragma unroll
        for (int i = 0; i < 4; ++i) a = __builtin_fmaf(w[i], hv[i], a);
      }
    } else {
      for (int j = pt; j < Cr; j += 4) a = __builtin_fmaf(wr[j], hs[j], a);
    }
    a = group_sum<4>(a);
    if (pt == 0) {
      const float sv = 1.f / (1.f + expf(-(a + b2[c0 + c])));
      ss[c] = sv;
      if (rg == 0) s_out[(size_t)n * C + c0 + c] = sv;
    }
  }
  __syncthreads();
  const int g8 = t & 7, pr = t >> 3;
  float sc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) sc[i] = ss[8 * g8 + i];
  const int p1 = min(HW, (rg + 1) * PIX);
  const size_t base = (size_t)n * HW * C + c0 + 8 * g8;
  for (int p = rg * PIX + pr; p < p1; p += ROWS * UNR) {
    u16x8 vu[UNR], vi[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int pp = p + ROWS * j;
      const size_t off = base + (size_t)(pp < p1 ? pp : p) * C;
      vu[j] = *reinterpret_cast<const u16x8*>(u + off);
      vi[j] = *reinterpret_cast<const u16x8*>(idn + off);
    }
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int pp = p + ROWS * j;
      if (pp >= p1) break;
      u16x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = down<T>(relu(__builtin_fmaf(up<T>(vu[j][i]), sc[i], up<T>(vi[j][i]))));
      *reinterpret_cast<u16x8*>(y + base + (size_t)pp * C) = o;
    }
  }
}

// ---- 6: parameter gradients ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_wgrad_kernel(const float* __restrict__ dz2, const float* __restrict__ dz1,
                                                         const float* __restrict__ p, const float* __restrict__ h,
                                                         float* __restrict__ dw1, float* __restrict__ db1,
                                                         float* __restrict__ dw2, float* __restrict__ db2, int N,
                                                         int C, int Cr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, q = lane >> 4;
  const int c = blockIdx.x * CB + 16 * wv + li;  // this lane's channel as an A row (always < C)
  const int j0 = blockIdx.y * 16, j = j0 + li;   // this lane's hidden unit as a B column
  const bool jok = j < Cr;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 a2 = z4, a1 = z4, ab2 = z4, ab1 = z4;
  for (int k0 = 0; k0 < N; k0 += 4) {
    const int n = k0 + q;
    const bool ok = n < N;
    const float x2 = ok ? dz2[(size_t)n * C + c] : 0.f;         // A[c][n] of dW2
    const float xp = ok ? p[(size_t)n * C + c] : 0.f;           // A[c][n] of dW1^T
    const float yh = ok && jok ? h[(size_t)n * Cr + j] : 0.f;    // B[n][j] of dW2
    const float y1 = ok && jok ? dz1[(size_t)n * Cr + j] : 0.f;  // B[n][j] of dW1^T
    a2 = mfma_f32_16x16x4(x2, yh, a2);
    a1 = mfma_f32_16x16x4(xp, y1, a1);
    ab2 = mfma_f32_16x16x4(x2, 1.f, ab2);  // every column: sum_n dz2[n][c]
    ab1 = mfma_f32_16x16x4(1.f, y1, ab1);  // every row:    sum_n dz1[n][j]
  }
  // D[row = 4 q + r][col = li]: row = channel of the wave's 16, col = hidden unit
  const int cb = blockIdx.x * CB + 16 * wv + 4 * q;
  if (jok) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dw2[(size_t)(cb + r) * Cr + j] = a2[r];
      dw1[(size_t)j * C + cb + r] = a1[r];
    }
  }
  if (blockIdx.y == 0 && li == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) db2[cb + r] = ab2[r];
  }
  if (blockIdx.x == 0 && wv == 0 && q == 0 && jok) db1[j] = ab1[0];
}

// ---- 7: input gradients ----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void excite_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                                                         const float* __restrict__ s, const float* __restrict__ dz1,
                                                         const float* __restrict__ w1, T* __restrict__ du,
                                                         T* __restrict__ did, int HW, int C, int Cr, int ranges) {
  __shared__ float zs[MAXCR];
  __shared__ float part[4][CB];
  __shared__ float dps[CB];
  const int t = threadIdx.x;
  const int n = blockIdx.x / ranges, rg = blockIdx.x - n * ranges, c0 = blockIdx.y * CB;
  if (t < Cr) zs[t] = dz1[(size_t)n * Cr + t];
  __syncthreads();
  {
    const int c = t & 63, pt = t >> 6, per = Cr >> 2;
    float a = 0.f;
    for (int j = pt * per; j < (pt + 1) * per; ++j) a = __builtin_fmaf(zs[j], w1[(size_t)j * C + c0 + c], a);
    part[pt][c] = a;
  }
  __syncthreads();
  if (t < CB) dps[t] = (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]) / (float)HW;
  __syncthreads();
  const int g8 = t & 7, pr = t >> 3;
  float sc[8], dp[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = s[(size_t)n * C + c0 + 8 * g8 + i];
    dp[i] = dps[8 * g8 + i];
  }
  const int p1 = min(HW, (rg + 1) * PIX);
  const size_t base = (size_t)n * HW * C + c0 + 8 * g8;
  for (int p = rg * PIX + pr; p < p1; p += ROWS * UNR) {
    u16x8 vg[UNR], vy[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int pp = p + ROWS * j;
      const size_t off = base + (size_t)(pp < p1 ? pp : p) * C;
      vg[j] = *reinterpret_cast<const u16x8*>(g + off);
      vy[j] = *reinterpret_cast<const u16x8*>(y + off);
    }
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int pp = p + ROWS * j;
      if (pp >= p1) break;
      u16x8 ou, oi;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool on = up<T>(vy[j][i]) > 0.f;
        oi[i] = on ? vg[j][i] : (unsigned short)0;
        ou[i] = down<T>(__builtin_fmaf(on ? up<T>(vg[j][i]) : 0.f, sc[i], dp[i]));
      }
      *reinterpret_cast<u16x8*>(du + base + (size_t)pp * C) = ou;
      *reinterpret_cast<u16x8*>(did + base + (size_t)pp * C) = oi;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------
static bool supported(int64_t C, int64_t Cr) {
  return C % 64 == 0 && C >= 64 && C <= 2048 && Cr % 4 == 0 && Cr >= 4 && Cr <= MAXCR;
}

// Which kernels ran since clear_launches(): family -> (C, Cr), dtype, calls.  Host bookkeeping
// only; forward and backward come from different threads (autograd's).
struct Rec {
  int C = 0, Cr = 0;
  const char* dtype = "";
  int calls = 0;
};
static std::mutex g_mu;
static std::map<std::string, Rec> g_log;
static void note(const char* family, int C, int Cr, const at::Tensor& t) {
  std::lock_guard<std::mutex> lk(g_mu);
  Rec& r = g_log[family];
  r.C = C;
  r.Cr = Cr;
  r.dtype = t.scalar_type() == at::kBFloat16 ? "bf16" : "f16";
  ++r.calls;
}
static std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> last_launch() {
  std::map<std::string, std::tuple<std::vector<int64_t>, std::string, int64_t>> out;
  std::lock_guard<std::mutex> lk(g_mu);
  for (const auto& kv : g_log)
    out[kv.first] = std::make_tuple(std::vector<int64_t>{kv.second.C, kv.second.Cr}, std::string(kv.second.dtype),
                                    (int64_t)kv.second.calls);
  return out;
}
static void clear_launches() {
  std::lock_guard<std::mutex> lk(g_mu);
  g_log.clear();
}

struct Dims {
  int N, HW, C, Cr;
};
static void check_act(const at::Tensor& t, const at::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4, "se: ", name, ": a 4-d HIP tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf, "se: ", name, ": bf16 or fp16");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), "se: ", name, ": channels_last");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "se: ", name, ": 16-byte aligned");
  TORCH_CHECK(t.sizes() == like.sizes() && t.scalar_type() == like.scalar_type() && t.device() == like.device(),
              "se: ", name, ": shape, dtype and device of u");
}
static void check_f32(const at::Tensor& t, const at::Tensor& u, int64_t numel, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == u.device() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.numel() == numel && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "se: ", name, ": fp32 contiguous, ", numel, " elements, on u's device");
}
// u: [N, C, H, W]; w1: [Cr, C] or [Cr, C, 1, 1]
static Dims dims(const at::Tensor& u, const at::Tensor& w1) {
  check_act(u, u, "u");
  TORCH_CHECK(w1.dim() >= 2, "se: fc1 weight [Cr, C]");
  const int64_t C = u.size(1), Cr = w1.size(0);
  TORCH_CHECK(supported(C, Cr), "se: unsupported C / Cr ", C, " / ", Cr);
  const int64_t N = u.size(0), HW = u.size(2) * u.size(3);
  TORCH_CHECK(N >= 1 && HW >= 1, "se: empty input");
  TORCH_CHECK(u.numel() < (1ll << 31), "se: activation of 2^31 elements or more");
  const int64_t ranges = (HW + PIX - 1) / PIX;
  TORCH_CHECK(N * ranges < (1ll << 31) && N <= 65535, "se: batch too large for the grid");
  return Dims{(int)N, (int)HW, (int)C, (int)Cr};
}

#define SE_DISPATCH(t, ...)                                                    \
  do {                                                                         \
    if ((t).scalar_type() == at::kBFloat16) { typedef __hip_bfloat16 T; __VA_ARGS__; } \
    else { typedef __half T; __VA_ARGS__; }                                    \
  } while (0)

// y = relu(u * sigmoid(fc2(relu(fc1(mean u)))) + identity); p [N, C], h [N, Cr], s [N, C] are kept
// for the backward.  Three launches.
static void fwd(const at::Tensor& u, const at::Tensor& identity, const at::Tensor& w1, const at::Tensor& b1,
                const at::Tensor& w2, const at::Tensor& b2, at::Tensor& p, at::Tensor& h, at::Tensor& s,
                at::Tensor& y) {
  const Dims d = dims(u, w1);
  check_act(identity, u, "identity");
  check_act(y, u, "y");
  const int64_t NC = (int64_t)d.N * d.C, NR = (int64_t)d.N * d.Cr, CC = (int64_t)d.C * d.Cr;
  check_f32(w1, u, CC, "fc1 weight");
  check_f32(b1, u, d.Cr, "fc1 bias");
  check_f32(w2, u, CC, "fc2 weight");
  check_f32(b2, u, d.C, "fc2 bias");
  check_f32(p, u, NC, "p");
  check_f32(h, u, NR, "h");
  check_f32(s, u, NC, "s");
  hipStream_t st = cur_stream();
  const dim3 pool_grid(d.C / CB, d.N), gemm_grid((d.N + 15) / 16, (d.Cr + 15) / 16);
  const int ranges = (d.HW + PIX - 1) / PIX;
  const dim3 elem_grid((unsigned)(d.N * ranges), d.C / CB);
  note("squeeze", d.C, d.Cr, u);
  SE_DISPATCH(u, hipLaunchKernelGGL((pool_kernel<T, false>), pool_grid, dim3(256), 0, st, dptr<const T>(u),
                                    (const T*)nullptr, (const T*)nullptr, (const float*)nullptr, dptr<float>(p),
                                    d.HW, d.C));
  DPA_CHECK_LAUNCH();
  note("fc1", d.C, d.Cr, u);
  hipLaunchKernelGGL(gate_gemm_kernel<false>, gemm_grid, dim3(256), 0, st, dptr<const float>(p),
                     dptr<const float>(w1), dptr<const float>(b1), dptr<float>(h), d.N, d.C, d.Cr);
  DPA_CHECK_LAUNCH();
  note("excite", d.C, d.Cr, u);
  SE_DISPATCH(u, hipLaunchKernelGGL((excite_kernel<T>), elem_grid, dim3(256), 0, st, dptr<const T>(u),
                                    dptr<const T>(identity), dptr<const float>(h), dptr<const float>(w2),
                                    dptr<const float>(b2), dptr<float>(s), dptr<T>(y), d.HW, d.C, d.Cr, ranges));
  DPA_CHECK_LAUNCH();
}

// Four launches: dz2 [N, C] and dz1 [N, Cr] are workspaces the caller allocates.
static void bwd(const at::Tensor& g, const at::Tensor& y, const at::Tensor& u, const at::Tensor& s,
                const at::Tensor& p, const at::Tensor& h, const at::Tensor& w1, const at::Tensor& w2,
                at::Tensor& dz2, at::Tensor& dz1, at::Tensor& dw1, at::Tensor& db1, at::Tensor& dw2,
                at::Tensor& db2, at::Tensor& du, at::Tensor& did) {
  const Dims d = dims(u, w1);
  check_act(g, u, "g");
  check_act(y, u, "y");
  check_act(du, u, "du");
  check_act(did, u, "d_identity");
  const int64_t NC = (int64_t)d.N * d.C, NR = (int64_t)d.N * d.Cr, CC = (int64_t)d.C * d.Cr;
  check_f32(s, u, NC, "s");
  check_f32(p, u, NC, "p");
  check_f32(h, u, NR, "h");
  check_f32(w1, u, CC, "fc1 weight");
  check_f32(w2, u, CC, "fc2 weight");
  check_f32(dz2, u, NC, "dz2");
  check_f32(dz1, u, NR, "dz1");
  check_f32(dw1, u, CC, "fc1 weight gradient");
  check_f32(db1, u, d.Cr, "fc1 bias gradient");
  check_f32(dw2, u, CC, "fc2 weight gradient");
  check_f32(db2, u, d.C, "fc2 bias gradient");
  hipStream_t st = cur_stream();
  const dim3 pool_grid(d.C / CB, d.N), gemm_grid((d.N + 15) / 16, (d.Cr + 15) / 16);
  const dim3 wgrad_grid(d.C / CB, (d.Cr + 15) / 16);
  const int ranges = (d.HW + PIX - 1) / PIX;
  const dim3 elem_grid((unsigned)(d.N * ranges), d.C / CB);
  note("excite_bwd_sums", d.C, d.Cr, u);
  SE_DISPATCH(u, hipLaunchKernelGGL((pool_kernel<T, true>), pool_grid, dim3(256), 0, st, dptr<const T>(g),
                                    dptr<const T>(y), dptr<const T>(u), dptr<const float>(s), dptr<float>(dz2),
                                    d.HW, d.C));
  DPA_CHECK_LAUNCH();
  note("gate_bwd", d.C, d.Cr, u);
  hipLaunchKernelGGL(gate_gemm_kernel<true>, gemm_grid, dim3(256), 0, st, dptr<const float>(dz2),
                     dptr<const float>(w2), dptr<const float>(h), dptr<float>(dz1), d.N, d.C, d.Cr);
  DPA_CHECK_LAUNCH();
  note("gate_wgrad", d.C, d.Cr, u);
  hipLaunchKernelGGL(gate_wgrad_kernel, wgrad_grid, dim3(256), 0, st, dptr<const float>(dz2),
                     dptr<const float>(dz1), dptr<const float>(p), dptr<const float>(h), dptr<float>(dw1),
                     dptr<float>(db1), dptr<float>(dw2), dptr<float>(db2), d.N, d.C, d.Cr);
  DPA_CHECK_LAUNCH();
  note("excite_bwd", d.C, d.Cr, u);
  SE_DISPATCH(u, hipLaunchKernelGGL((excite_bwd_kernel<T>), elem_grid, dim3(256), 0, st, dptr<const T>(g),
                                    dptr<const T>(y), dptr<const float>(s), dptr<const float>(dz1),
                                    dptr<const float>(w1), dptr<T>(du), dptr<T>(did), d.HW, d.C, d.Cr, ranges));
  DPA_CHECK_LAUNCH();
}

}  // namespace se

void register_se(pybind11::module& m) {
  auto s = m.def_submodule("se", "squeeze-and-excitation with the residual add and ReLU (NHWC, fp32 MFMA gate)");
  s.def("supported", &se::supported);
  s.def("fwd", &se::fwd, pybind11::arg("u"), pybind11::arg("identity"), pybind11::arg("w1"), pybind11::arg("b1"),
        pybind11::arg("w2"), pybind11::arg("b2"), pybind11::arg("p"), pybind11::arg("h"), pybind11::arg("s"),
        pybind11::arg("y"));
  s.def("bwd", &se::bwd, pybind11::arg("g"), pybind11::arg("y"), pybind11::arg("u"), pybind11::arg("s"),
        pybind11::arg("p"), pybind11::arg("h"), pybind11::arg("w1"), pybind11::arg("w2"), pybind11::arg("dz2"),
        pybind11::arg("dz1"), pybind11::arg("dw1"), pybind11::arg("db1"), pybind11::arg("dw2"), pybind11::arg("db2"),
        pybind11::arg("du"), pybind11::arg("did"));
  s.def("last_launch", &se::last_launch);
  s.def("clear_launches", &se::clear_launches);
  s.attr("PIXELS") = se::PIX;
}

}  // namespace dpa
