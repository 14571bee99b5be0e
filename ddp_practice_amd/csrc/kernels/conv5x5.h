// 5x5 convolution of the ConvNet blocks, forward and data gradient (overview: convblock_bn.h).
#pragma once
#include "convblock_bn.h"

namespace dpa {
namespace cb {

template <int I> struct SH;
template <> struct SH<0> { static constexpr int CIN = 1, COUT = 16, H = 28, W = 28, SPLIT = 4, WROWS = 28; };
template <> struct SH<1> { static constexpr int CIN = 16, COUT = 32, H = 14, W = 14, SPLIT = 2, WROWS = 14; };

// Row-window staging of conv5x5_body (its WR parameter): the most input rows any of the nsplit
// workgroups of an H x W image stages.  Workgroup sp computes the output pixels of m-tiles
// [MT*sp/nsplit, MT*(sp+1)/nsplit) and reads their rows plus the two halo rows each side,
// clipped to the image; `even`: rounded out to whole 2x2 pooling windows (PRO 2).
// 0: some split is empty (nsplit > MT).
__host__ __device__ constexpr int conv5x5_win_rows(int H, int W, int nsplit, bool even) {
  const int HW = H * W, MT = (HW + 15) / 16;
  int mx = 0;
  for (int sp = 0; sp < nsplit; ++sp) {
    const int p0 = 16 * (MT * sp / nsplit), p1e = 16 * (MT * (sp + 1) / nsplit), p1 = p1e < HW ? p1e : HW;
    if (p1 <= p0) return 0;
    int lo = p0 / W - 2, hi = (p1 - 1) / W + 2;
    lo = lo < 0 ? 0 : lo;
    hi = hi > H - 1 ? H - 1 : hi;
    if (even) {
      lo &= ~1;
      hi |= 1;
    }
    mx = hi - lo + 1 > mx ? hi - lo + 1 : mx;
  }
  return mx;
}

// Epilogue of the data-grad kernel that produces a pooled grad: BN partial sums of the block
// below, [S1 | S2] per channel, one slab row per QUARTER of an image, whatever the launch's split.
// Quarter k of an image is the m-tiles [MT*k/4, MT*(k+1)/4) (at most 4), the range of workgroup k
// of a 4-way split; a workgroup of a 2-way split covers exactly two of them and writes both rows.
// Within a quarter the m-tile mt has slot mt - quarter start.  A slot's partial is what one wave
// produces for that one m-tile (the lane's 4 pixels added in order from zero, then xor16_sum /
// xor32_sum); the row is the slots' partials added in slot order from 0.f.  Either split builds
// every row by exactly these operations, so the slab's 4 * B rows are the same bit for bit.
constexpr int EPI_QUARTERS = 4;
template <typename T>
struct BwdEpi {
  const uint8_t* idx;  // that block's pooled index (relu bit)
  const T* xh;         // that block's xhat at the argmax
  float* bslab;        // [EPI_QUARTERS * B] rows, row 4 b + k = [S1(COUT) | S2(COUT)] of quarter k of image b
};

// ---------------------------------------------------------------------------
// Pre-packed low-precision weights of the 16->32 conv (ConvNet layer 2), in
// exactly the LDS tile layout conv5x5_kernel uses (rows padded to KPW, K
// padding zeroed): the forward tile [32][424] (k = tap*16 + ci) and the
// data-grad tile [16][808] (k = (24-tap)*32 + co, the flipped transpose).
// The layer-1 forward launch writes them as a side job: W2P_WGS workgroups of
// their own appended behind its conv workgroups (conv5x5_kernel WPK 2; the conv
// workgroups leave most of the chip idle anyway), so the layer-2 kernels stage
// their weight tile with straight 16-B copies instead of 12,800 converted,
// scattered element stores per workgroup (the VALU-heaviest part of their
// staging), and the conv workgroups do not carry the pack's memory round trips
// ahead of their own.
// ---------------------------------------------------------------------------
constexpr int W2F_ROWS = 32, W2F_PITCH = 424;   // ceil_to(25*16, 32) + 8
constexpr int W2D_ROWS = 16, W2D_PITCH = 808;   // ceil_to(25*32, 32) + 8
constexpr int W2F_LEN = W2F_ROWS * W2F_PITCH, W2D_LEN = W2D_ROWS * W2D_PITCH;
// the pack workgroups of a launch and the elements per lane: fixed, whatever the batch
constexpr int W2P_WGS = 26, W2P_IT = 4;
static_assert(W2P_WGS * W2P_IT * NTHR >= W2F_LEN + W2D_LEN, "the pack workgroups cover both packs");
// The fc weights of the one-launch head (convnet_head.hip head_row_kernel PK), packed by the
// same launch in fcp_nm(N) further workgroups behind the W2P_WGS: [FCP_LANES][NM][8] of T,
// entry [lane][n][i] = T(wfc[n][lane + 256 i]), zero where n >= N, lane + 256 i >= FCP_K or
// i = 7 -- a head lane's class row is one 16-B granule, already in the compute dtype, instead
// of 7 scalar f32 loads and 7 roundings that every one of the head's workgroups repeated.
// NM: the class count the head's register tiles are sized for (what head_step selects).
// (the layout constants: convblock_bn.h FCP_*, shared with the head)
template <typename T>
struct WPack {
  const float* w2 = nullptr;  // [32][16][5][5] f32 master weights
  T* fwd = nullptr;           // [W2F_LEN]
  T* dgrad = nullptr;         // [W2D_LEN]
  const float* wfc = nullptr; // [N][FCP_K] f32 master fc weights (with fcp)
  T* fcp = nullptr;           // [fcp_len(NM)] or null: no fc pack workgroups in the launch
  int N = 0, NM = 0;          // classes; fcp_nm(N) = the launch's fc pack workgroups
};
// Pack workgroup wg of W2P_WGS: element (wg * W2P_IT + i) * NTHR + lane of
// [fwd | dgrad].  Compile-time trip counts and no blockDim / gridDim (hidden-argument loads
// with a wait of their own); every w2 load is issued (clamped, unconditional: the padding
// columns and the lanes past the end read a valid element they do not use) before the first
// conversion or store, so the role is one memory round trip.
template <typename T>
__device__ __forceinline__ void pack_w2(const WPack<T>& pk, const int wg) {
  constexpr int TOTAL = W2F_LEN + W2D_LEN;
  const int tid = threadIdx.x;
  DPA_STAMP(0);
  float v[W2P_IT];
  bool pad[W2P_IT];
#pragma unroll
  for (int i = 0; i < W2P_IT; ++i) {
    const int e = min((wg * W2P_IT + i) * NTHR + tid, TOTAL - 1);
    int src;
    if (e < W2F_LEN) {
      const int co = e / W2F_PITCH, k = e % W2F_PITCH, kk = min(k, 399);
      pad[i] = k >= 400;
      src = (co * 16 + (kk & 15)) * 25 + (kk >> 4);
    } else {
      const int e2 = e - W2F_LEN;
      const int ci = e2 / W2D_PITCH, k = e2 % W2D_PITCH, kk = min(k, 799);
      pad[i] = k >= 800;
      src = ((kk & 31) * 16 + ci) * 25 + (24 - (kk >> 5));
    }
    v[i] = pk.w2[src];  // src < 32 * 16 * 25
  }
#pragma unroll
  for (int i = 0; i < W2P_IT; ++i) {
    const int e = (wg * W2P_IT + i) * NTHR + tid;
    const T o = Cvt<T>::from_f(pad[i] ? 0.f : v[i]);
    if (e < W2F_LEN)
      pk.fwd[e] = o;
    else if (e < TOTAL)
      pk.dgrad[e - W2F_LEN] = o;
  }
  DPA_STAMP(7);
}

// fc pack workgroup n of pk.NM: class n for every head lane.  The same discipline as pack_w2:
// compile-time trip counts, no blockDim / gridDim, the 7 loads of the class row (coalesced
// across the lanes; clamped and unconditional) issued before the first conversion, one 16-B
// store per lane.  The padding (n >= N, features >= FCP_K, element 7) is written every step.
template <typename T>
__device__ __forceinline__ void pack_fc(const WPack<T>& pk, const int n) {
  static_assert(FCP_LANES == NTHR, "one lane of a pack workgroup per head lane");
  if constexpr (sizeof(T) == 2) {
    const int tid = threadIdx.x;
    DPA_STAMP(0);
    const float* row = pk.wfc + (size_t)min(n, pk.N - 1) * FCP_K;
    float v[FCP_IT];
#pragma unroll
    for (int i = 0; i < FCP_IT; ++i) v[i] = row[min(tid + FCP_LANES * i, FCP_K - 1)];
    u16x8 o;
#pragma unroll
    for (int i = 0; i < FCP_IT; ++i) {
      const bool pad = n >= pk.N || tid + FCP_LANES * i >= FCP_K;
      const T t = Cvt<T>::from_f(pad ? 0.f : v[i]);
      unsigned short bits;
      __builtin_memcpy(&bits, &t, 2);
      o[i] = bits;
    }
    o[7] = 0;
    *reinterpret_cast<u16x8*>(pk.fcp + ((size_t)tid * pk.NM + n) * 8) = o;
    DPA_STAMP(7);
  }
}

// Batch gather fused into the first conv (PRO 3): the input image is read from
// the uint8 dataset resident in HBM through the epoch's sample order at the
// device step counter, converted (ToTensor: x * scale + shift, data/loader.py)
// and staged; split 0 of each image also writes it (and its label) to the
// batch buffers the rest of the step reads.  The launch's last-arriving conv
// workgroup advances the step counter (data.hip gather_kernel's protocol); a
// workgroup arrives as its last act, after its partial-sum row is stored, so no
// wave waits for the atomic's return ahead of the compute barrier.
// Only counter -> order[pos] -> pixels depend on each other: the counter load is
// the workgroup's first memory instruction, bias / shift / weights are issued
// behind it, and the LDS zeroing and the weight scatter run under the order load.
struct GatherIn {
  const uint8_t* imgs = nullptr;   // [N][npix]
  const int64_t* labels = nullptr; // [N]
  const int64_t* order = nullptr;  // epoch order
  long long order_len = 0;
  int* ctr = nullptr;              // [0] step, [1] arrivals (self-resetting)
  int64_t* lab_out = nullptr;      // [B]
  float scale = 1.f, shift = 0.f;
  int nimg = 0;                    // B (the launch has nimg * nsplit conv workgroups; not gridDim,
                                   // a hidden-argument load with its own wait on gfx950).  Set by
                                   // every WPK 2 launch: the workgroups from nimg * nsplit on pack
};

// ---------------------------------------------------------------------------
// Implicit-GEMM 5x5 convolution, one (image, m-range) per workgroup.
//   MODE 0: forward + bias + BN partial sums        (train)
//   MODE 1: forward + bias                          (eval)
//   MODE 2: data-grad: input = dy (CIN = COUT_orig), output = dx,
//           W_eff[co][ci][kh][kw] = W[ci][co][4-kh][4-kw], no bias
// GEMM view: rows = output pixels of one image, cols = output channels,
// K = 25*CIN ordered (kh, kw, ci) with ci fastest.
// ---------------------------------------------------------------------------
//   PRO 0: the input image is read from x;
//   PRO 3: (CIN 1) the input image is gathered from the dataset (gin, above) and
//          written to x by split 0;
//   PRO 1: the input is produced in the staging pass from the previous block's
//          pre-BN output (pin: BN finalize -> normalise -> ReLU -> 2x2 max-pool),
//          which also writes the pooled map + argmax|relu index + xhat at the
//          argmax for the backward (split 0);
//   PRO 2: (MODE 2) the input dy is produced from the pooled grad of the next
//          block (bin: backward through MaxPool -> ReLU -> BN, see BwdIn).
//   EPI 1: (MODE 2) the output is a pooled grad: also write the BN partial sums [S1 | S2] of
//          the block below, one row per image quarter this workgroup covers (epi, BwdEpi).
//          ES: the launch's nsplit at compile time, 2 or 4 (the epilogue's register and LDS
//          shapes follow from the quarters per workgroup).
//   WPK 0: stage the weight tile from the f32 master weights w;
//   WPK 1: w is ignored, the tile is copied from the pre-packed wpk (pack_w2);
//   WPK 2: (CIN 1, PRO 0 / 3) as 0 with every load of the prologue issued before the first
//          wait, and this launch also writes the layer-2 packs (pk) in W2P_WGS workgroups
//          appended behind the gin.nimg * nsplit conv workgroups (conv5x5_kernel).
// bid: this workgroup's index among the launch's workgroups of this role (blockIdx.x
// for a launch of its own; conv5x5_kernel / dgrad_wgrad_kernel below).
// DYN: the two big LDS tiles (image, weights) are carved from the launch's dynamic LDS
// instead of being static arrays, so a launch hosting several roles (convnet_fused.hip
// conv2_bwd_dyn_kernel) needs the LARGEST role's tiles, not their sum (conv5x5_dyn_bytes).
template <typename T, int CIN, int H, int W>
__host__ __device__ constexpr size_t conv5x5_img_bytes() {
  return ((sizeof(T) * (size_t)(H + 4) * (W + 4) * CIN) + 15) / 16 * 16;
}
template <typename T, int CIN, int COUT, int H, int W>
__host__ __device__ constexpr size_t conv5x5_dyn_bytes() {
  return conv5x5_img_bytes<T, CIN, H, W>() + sizeof(T) * (size_t)COUT * (ceil_to(25 * CIN, 32) + 8);
}

// WR: row-window staging (PRO 1 / 2).  A workgroup reads only the input rows of its own output
// pixels plus two halo rows each side; with WR < H it stages just those (clipped to the image,
// PRO 2: rounded out to whole 2x2 windows) instead of the whole image, and zeroes just the
// halo it reads.  WR is the compile-time bound on that row count (conv5x5_win_rows of the
// launch's nsplit: the launcher checks it); the per-lane trip counts of the staging pass and
// its register arrays follow from it.  WR = H: every workgroup stages the whole image.
template <typename T, int CIN, int COUT, int H, int W, int MODE, int PRO = 0, int EPI = 0, int WPK = 0,
          bool DYN = false, int WR = H, int ES = 0>
__device__ __forceinline__ void
conv5x5_body(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
             T* __restrict__ y, float* __restrict__ fslab, float* __restrict__ fstats,
             const float* __restrict__ shift, int nsplit, const PoolIn<T>& pin, const BwdIn<T>& bin,
             const BwdEpi<T>& epi, const T* __restrict__ wpk, const WPack<T>& pk, const int bid,
             const GatherIn& gin = GatherIn{}) {
  static_assert(CIN == 1 || CIN % 8 == 0, "CIN must be 1 or a multiple of 8");
  static_assert(COUT % 16 == 0, "COUT must be a multiple of 16");
  static_assert((H * W) % 4 == 0, "H*W must be a multiple of 4");
  static_assert(PRO != 2 || MODE == 2, "PRO 2 is a data-grad prologue");
  static_assert(PRO != 3 || (CIN == 1 && MODE != 2), "PRO 3 gathers single-channel input images");
  static_assert(EPI == 0 || MODE == 2, "EPI 1 is a data-grad epilogue");
  static_assert(EPI == 0 ? ES == 0 : (ES == 2 || ES == 4), "EPI 1: a 2-way or a 4-way split, known at compile time");
  constexpr int NCH = CIN >= 8 ? CIN / 8 : 1;              // 16-B groups per pixel
  constexpr int HP = H + 4, WPD = W + 4;
  constexpr int K = 25 * CIN;
  constexpr int KP = ceil_to(K, 32);
  constexpr int KS = KP / 32;
  constexpr int KPW = KP + 8;  // LDS row pitch of the weight tile (breaks bank aliasing)
  constexpr int NT = COUT / 16;
  constexpr int HW = H * W;
  constexpr int MT = (HW + 15) / 16;
  typedef MM<T> mm;

  T* img;
  T* wl;
  if constexpr (DYN) {
    img = reinterpret_cast<T*>(dpa_dyn_lds);
    wl = reinterpret_cast<T*>(dpa_dyn_lds + conv5x5_img_bytes<T, CIN, H, W>());
  } else {
    __shared__ __attribute__((aligned(16))) T img_s[HP * WPD * CIN];
    __shared__ __attribute__((aligned(16))) T wl_s[COUT * KPW];
    img = img_s;
    wl = wl_s;
  }
  // img is [padded pixel][CIN] with the 8-channel (16-B) groups of each pixel
  // XOR-swizzled by the pixel index: an A-fragment read takes 16 consecutive
  // pixels x one 16-B group; with a 32/64-B pixel pitch those 16 addresses would
  // share 8/4 bank groups (2/4-way conflicts), swizzled they hit 16 distinct ones
  // (conv2 dgrad: SQ_LDS_BANK_CONFLICT -54 %)
  constexpr int PPB = NCH <= 16 ? 16 / NCH : 1;            // pixels per 256-B bank row
  auto imo = [](int px, int c) -> int {
    if constexpr (NCH <= 1) {
      return px * CIN + c;
    } else {
      return px * CIN + ((((c >> 3) ^ ((px / PPB) & (NCH - 1)))) << 3) + (c & 7);
    }
  };
  // EPI 1: NQ quarters per workgroup, each with up to NTHR / 64 slots (BwdEpi)
  constexpr int NQ = EPI == 1 ? EPI_QUARTERS / ES : 1;
  static_assert(EPI == 0 || (MT + EPI_QUARTERS - 1) / EPI_QUARTERS <= NTHR / 64,
                "EPI 1: a quarter has at most one m-tile per wave");
  // the per-(quarter, wave / slot) partials of the statistics epilogue.  PRO 2's reduction scratch
  // (part: bn_bwd_coef) is dead from the compute barrier on, so the two-quarter epilogue keeps its
  // partials there and a 2-way data-gradient workgroup's static LDS does not grow with them
  // (it shrinks by the 512 B of lstat_s).  The assert below covers the size; the LIFETIME is a
  // rule of this body: nothing may read or write `part` after the compute barrier (its last use
  // is inside bn_bwd_coef, see the note there), and lstat is first written after the MFMA loop.
  // Instantiations that use neither array declare it with one float, which the compiler drops
  // (their LDS sizes are the parent's: profiles/dgrad_rows_ab.txt, resources)
  constexpr int LSN = NQ * (NTHR / 64) * 2 * COUT;
  constexpr bool LS_IN_PART = PRO == 2 && NQ > 1;
  static_assert(!LS_IN_PART || LSN <= NTHR, "EPI 1: the partials fit the reduction scratch");
  __shared__ float part_s[PRO == 2 ? NTHR : 1];
  __shared__ float lstat_s[LS_IN_PART ? 1 : LSN];
  float* const lstat = LS_IN_PART ? part_s : lstat_s;

  const int tid = threadIdx.x;
  const int b = bid / nsplit;
  DPA_STAMP(0);
  // C1: the fused step's first conv (WPK 2).  Its prologue issues every global load before the
  // first wait; with the gather (PRO 3) the step counter's load goes first: counter -> order ->
  // pixels is the workgroup's one dependent chain (GatherIn)
  constexpr bool C1 = WPK == 2;
  static_assert(!C1 || (CIN == 1 && MODE != 2 && EPI == 0 && (PRO == 0 || PRO == 3)), "WPK 2: the first conv");
  static_assert(PRO != 3 || C1, "the gather prologue belongs to the fused step's first conv");
  int step = 0, step_v = 0;
  // (a relaxed atomic load: the previous launch's atomic store is visible at this launch's start;
  //  a volatile load is waited for right where it is issued)
  if constexpr (PRO == 3) step_v = __hip_atomic_load(gin.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int sp = bid % nsplit;
  const T* xb = x + (size_t)b * CIN * HW;
  const int mt0 = (MT * sp) / nsplit, mt1 = (MT * (sp + 1)) / nsplit;
  // this workgroup's output pixels [p_lo, p_hi); the input rows [r_lo, r_lo + SR) it stages (the
  // rows it needs; past them up to the bound SR, clipped at the image's end) and the padded
  // LDS rows [z_lo, z_lo + z_n) its MFMA loop reads (wave-uniform)
  constexpr bool WIN = WR < H;
  static_assert(!WIN || PRO == 1 || PRO == 2, "row windows: the BN prologues' staging passes");
  static_assert(WR >= 1 && (PRO != 2 || WR % 2 == 0 || !WIN), "PRO 2 stages whole 2x2 windows");
  constexpr int SR = WIN ? WR : H;
  const int p_lo = mt0 * 16, p_hi = min(mt1 * 16, HW);
  int r_lo = 0, r_n = H, z_lo = 0, z_n = HP;
  if constexpr (WIN) {
    const int oh_lo = p_lo / W, oh_hi = (p_hi - 1) / W;
    r_lo = max(oh_lo - 2, 0);
    int r_hi = min(oh_hi + 2, H - 1);
    if constexpr (PRO == 2) {
      r_lo &= ~1;
      r_hi |= 1;
    }
    r_n = r_hi - r_lo + 1;  // <= WR (host-checked)
    z_lo = oh_lo;
    z_n = oh_hi + 5 - oh_lo;
  }
  // epilogue operands of this lane's channels (co = nt*16 + lane%16), loaded up front
  float pre_bias[NT], pre_shift[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = nt * 16 + (tid & 15);
    pre_bias[nt] = (MODE == 2) ? 0.f : bias[co];
    pre_shift[nt] = (MODE == 0) ? shift[co] : 0.f;
  }

  // --- stage weights (batched float4 reads in natural [co][ci][kh][kw] order,
  //     scattered LDS writes to wl[co][(kh*5+kw)*CIN + ci])
  const T zero = Cvt<T>::from_f(0.f);
  // WPK 1: the pre-packed tile goes global -> LDS directly (global_load_lds_dwordx4: no
  // VGPRs, so it can be issued with the prologue's first loads without register pressure);
  // with a BN prologue it is issued before the statistics reduction, whose loads and barrier
  // then cover its latency (the barrier's vmcnt(0) retires it; the tile is read only after
  // the compute barrier).  LDS destination = wave-uniform base + lane x 16 B: wl is a
  // contiguous run of 16-B chunks, chunk c at byte 16c.
  constexpr int WN16 = WPK == 1 ? COUT * KPW * (int)sizeof(T) / 16 : 1;
  constexpr int WIT = (WN16 + NTHR - 1) / NTHR;
  auto load_wpk = [&]() {
    if constexpr (WPK == 1) {
      static_assert((COUT * KPW * sizeof(T)) % 16 == 0, "packed weight tile must be whole 16-B chunks");
      static_assert(COUT * KPW == (MODE == 2 ? W2D_LEN : W2F_LEN), "pre-packed weights exist for layer 2 only");
      typedef __attribute__((address_space(3))) void* lds_ptr_t;
      const uint4* src = reinterpret_cast<const uint4*>(wpk);
      uint4* dstl = reinterpret_cast<uint4*>(wl);
      const int wv0 = (tid >> 6) * 64, ln = tid & 63;
#pragma unroll
      for (int i = 0; i < WIT; ++i) {
        const int c0 = i * NTHR + wv0;  // this wave's first chunk (wave-uniform)
        if (c0 + ln < WN16)             // lanes past the tile are masked off: they write nothing
          __builtin_amdgcn_global_load_lds(src + c0 + ln, (lds_ptr_t)(dstl + c0), 16, 0, 0);
      }
    }
  };
  if constexpr (WPK == 1) {
    if constexpr (PRO == 0 || PRO == 3) load_wpk();
  } else if constexpr (!C1) {
    if constexpr (KP > K) {
      for (int e = tid; e < COUT * (KP - K); e += NTHR) wl[(e / (KP - K)) * KPW + K + e % (KP - K)] = zero;
    }
    // natural W index e = (o * WIN + i) * 25 + tap, WIN = in-channels of W
    // (= CIN here, = COUT for the data-grad where W is [CIN][COUT][5][5])
    constexpr int KO = 25 * (MODE == 2 ? COUT : CIN);
    stage_f32<COUT * K>(w, [&](int e, float v) {
      const int o = e / KO, rem = e % KO;      // o: out-ch of W
      const int i = rem / 25, tap = rem % 25;  // i: in-ch of W
      if (MODE == 2)  // W_eff[co=i][ci=o][tap'] with tap' = 24 - tap
        wl[i * KPW + (24 - tap) * CIN + o] = Cvt<T>::from_f(v);
      else
        wl[o * KPW + tap * CIN + i] = Cvt<T>::from_f(v);
    });
  }
  DPA_STAMP(1);
  // --- stage the zero-padded image in HWC order: zero the halo pixels
  //     (whole 16-B groups when a pixel is, else element by element)
  if constexpr (C1) {
    // (the first conv zeroes its halo under its loads: fill_lds below)
  } else if constexpr ((CIN * sizeof(T)) % 16 == 0) {
    constexpr int G = CIN * (int)sizeof(T) / 16;  // 16-B groups per pixel
    uint4* img4 = reinterpret_cast<uint4*>(img);
    if constexpr (WIN) {  // the halo pixels of the padded rows this workgroup reads
      uint4* row4 = img4 + z_lo * WPD * G;
      for (int e = tid; e < z_n * WPD * G; e += NTHR) {
        const int px = e / G, hp = z_lo + px / WPD, wp = px % WPD;
        if (hp < 2 || hp >= H + 2 || wp < 2 || wp >= W + 2) row4[e] = make_uint4(0u, 0u, 0u, 0u);
      }
    } else {
      for (int e = tid; e < HP * WPD * G; e += NTHR) {
        const int px = e / G, hp = px / WPD, wp = px % WPD;
        if (hp < 2 || hp >= H + 2 || wp < 2 || wp >= W + 2) img4[e] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
  } else {
    static_assert(!WIN, "row windows: whole 16-B channel groups per pixel");
    for (int e = tid; e < HP * WPD * CIN; e += NTHR) {
      const int hp = e / (WPD * CIN), rem = e % (WPD * CIN);
      const int wp = rem / CIN;
      if (hp < 2 || hp >= H + 2 || wp < 2 || wp >= W + 2) img[e] = zero;
    }
  }
  // EPI: this workgroup's output range of the pooled index / xhat of the block below
  constexpr int EPIX = EPI ? MT * 16 : 1;
  __shared__ uint8_t eidx[EPI ? COUT * EPIX : 1];
  __shared__ T exh[EPI ? COUT * EPIX : 1];
  // (the loads: issued after the BN prologue's barrier; the LDS stores: after
  //  the emit, so the round trip overlaps it)
  const int ep0 = mt0 * 16, enp = min(mt1 * 16, HW) - ep0;
  constexpr int EIT = EPI ? (COUT * EPIX + NTHR - 1) / NTHR : 1;
  uint8_t ei[EIT];
  T ex[EIT];
  auto load_epi = [&]() {
    if constexpr (EPI == 1) {
#pragma unroll
      for (int i = 0; i < EIT; ++i) {
        const int e = tid + i * NTHR;
        const int ec = e < COUT * enp ? e : 0;  // clamped: the loads stay unconditional
        const int co = ec / enp, pp = ec % enp;
        const size_t o = ((size_t)b * COUT + co) * HW + ep0 + pp;
        ei[i] = epi.idx[o];
        ex[i] = epi.xh[o];
      }
    }
  };
  auto store_epi = [&]() {
    if constexpr (EPI == 1) {
#pragma unroll
      for (int i = 0; i < EIT; ++i) {
        const int e = tid + i * NTHR;
        if (e < COUT * enp) {
          const int co = e / enp, pp = e % enp;
          eidx[co * EPIX + pp] = ei[i];
          exh[co * EPIX + pp] = ex[i];
        }
      }
    }
  };
  if constexpr (PRO != 2) {
    load_epi();
    store_epi();
  }
  DPA_STAMP(2);
  // PRO 1: this lane's pooled map / index / xhat outputs (for the backward) are stored AFTER
  // the compute barrier: __syncthreads() waits vmcnt(0), so issued before it they held the
  // whole workgroup until they retired; issued after it they overlap the MFMA loop (step
  // -0.4 us; the same deferral of conv1's gather stores measured no gain,
  // profiles/r4p_deferred_stores_ab.txt)
  constexpr int DQ = PRO != 1 ? 1
                     : (CIN % 8 == 0 && sizeof(T) == 2) ? 8 * ((CIN / 8 * SR * W + NTHR - 1) / NTHR)
                                                          : (CIN * SR * W + NTHR - 1) / NTHR;
  int dq_e[DQ];  // pooled-output element of entry d, -1: none
  T dq_p[DQ], dq_x[DQ];
  uint8_t dq_i[DQ];
#pragma unroll
  for (int d = 0; d < DQ; ++d) dq_e[d] = -1;
  if constexpr (C1) {
    // the weights as one float4 per lane (clamped: the load stays unconditional), issued
    // behind the bias / shift loads (and the counter's) with no wait in between
    constexpr int WN4 = COUT * K / 4;
    static_assert((COUT * K) % 4 == 0 && WN4 <= NTHR, "one float4 of the weights per lane");
    const f32x4 w4 = reinterpret_cast<const f32x4*>(w)[min(tid, WN4 - 1)];
    // the LDS work that needs no global data (K padding of the weight tile, the halo), then the
    // weight scatter to wl[co][tap]: run while the input's loads are in flight
    auto fill_lds = [&]() {
      for (int e = tid; e < COUT * (KP - K); e += NTHR) wl[(e / (KP - K)) * KPW + K + e % (KP - K)] = zero;
      for (int e = tid; e < HP * WPD; e += NTHR) {
        const int hp = e / WPD, wp = e % WPD;
        if (hp < 2 || hp >= H + 2 || wp < 2 || wp >= W + 2) img[e] = zero;
      }
      if (tid < WN4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * tid + j;
          wl[(e / 25) * KPW + e % 25] = Cvt<T>::from_f(w4[j]);
        }
      }
    };
    if constexpr (PRO == 0) {
      typedef typename Pair2<T>::type P;
      static_assert(W % 2 == 0, "pixel pairs stay inside a row");
      constexpr int NP = HW / 2, XIT = (NP + NTHR - 1) / NTHR;
      const P* s2 = reinterpret_cast<const P*>(xb);
      P xv[XIT];
#pragma unroll
      for (int i = 0; i < XIT; ++i) xv[i] = s2[min(tid + i * NTHR, NP - 1)];
      fill_lds();
      DPA_STAMP(3);
#pragma unroll
      for (int i = 0; i < XIT; ++i) {
        const int e = tid + i * NTHR;
        if (e < NP) {
          const int h = (2 * e) / W, ww = (2 * e) % W;
          T a, bb;
          __builtin_memcpy(&a, &xv[i], sizeof(T));
          __builtin_memcpy(&bb, reinterpret_cast<const char*>(&xv[i]) + sizeof(T), sizeof(T));
          img[imo((h + 2) * WPD + (ww + 2), 0)] = a;
          img[imo((h + 2) * WPD + (ww + 3), 0)] = bb;
        }
      }
    } else {
      // step counter -> sample -> 4 uint8 pixels per lane load
      static_assert(HW % 4 == 0 && W % 4 == 0, "4-pixel groups stay inside a row");
      constexpr int G4 = HW / 4, GIT = (G4 + NTHR - 1) / NTHR;
      step = __builtin_amdgcn_readfirstlane(step_v);  // waits for the counter alone: it was issued first
      DPA_STAMP(8);
      long long pos = (long long)step * gin.nimg + b;
      pos = pos < gin.order_len ? pos : gin.order_len - 1;  // never taken with a correct host-side batch count
      const int64_t src_v = gin.order[pos];
      fill_lds();
      DPA_STAMP(3);
      // wave-uniform: the sample's base addresses stay scalar
      const uint32_t src_lo = __builtin_amdgcn_readfirstlane((uint32_t)src_v);
      const uint32_t src_hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)src_v >> 32));
      const int64_t src = (int64_t)(((uint64_t)src_hi << 32) | src_lo);
      DPA_STAMP(9);
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(gin.imgs + src * HW);
      uint32_t v4[GIT];
#pragma unroll
      for (int i = 0; i < GIT; ++i) v4[i] = s4[min(tid + i * NTHR, G4 - 1)];  // clamped: unconditional
      const int64_t lab_v = gin.labels[src];  // every lane (one address): no branch around the load
      T px[GIT][4];
#pragma unroll
      for (int i = 0; i < GIT; ++i) {
        const int g = tid + i * NTHR;
        const int h = (4 * g) / W, ww = (4 * g) % W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          px[i][k] = Cvt<T>::from_f((float)((v4[i] >> (8 * k)) & 0xffu) * gin.scale + gin.shift);
          if (g < G4) img[imo((h + 2) * WPD + (ww + k + 2), 0)] = px[i][k];
        }
      }
      // taken by every wave, here, right behind the pixels: left pending on the waves that do not
      // store it, the load would be waited for with vmcnt(0) wherever its registers are reused --
      // after the compute barrier and after the MFMA loop, behind this wave's own stores
      const uint32_t lab_lo = __builtin_amdgcn_readfirstlane((uint32_t)lab_v);
      const uint32_t lab_hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)lab_v >> 32));
      const int64_t lab = (int64_t)(((uint64_t)lab_hi << 32) | lab_lo);
      DPA_STAMP(10);
      if (sp == 0) {  // the batch buffers (conv1's weight gradient, the loss and the user read them)
        T* xo = const_cast<T*>(xb);
#pragma unroll
        for (int i = 0; i < GIT; ++i) {
          const int g = tid + i * NTHR;
          if (g < G4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) xo[4 * g + k] = px[i][k];
          }
        }
        if (tid == 0) gin.lab_out[b] = lab;
      }
    }
  } else if constexpr (PRO == 0) {
    stage_chw<T, CIN, H, W>(xb, [&](int ci, int h, int ww, T a, T bb) {
      img[imo((h + 2) * WPD + (ww + 2), ci)] = a;
      img[imo((h + 2) * WPD + (ww + 3), ci)] = bb;
    });
  } else if constexpr (PRO == 1) {
    __shared__ float sc_s[CIN], beta_s[CIN], mean_s[CIN], istd_s[CIN];
    __shared__ float part[NTHR];
    typedef typename Pair2<T>::type P;
    // the staged pooled pixels (= this conv's input) are the rows [r_lo, r_lo + r_n) of every
    // channel; RP: their compile-time bound per channel (the whole image without a window)
    constexpr int RP = SR * W;
    const T* yb = pin.y + (size_t)b * CIN * 4 * HW;
    // The pooled map / index / xhat outputs (for the backward) are written by all nsplit
    // workgroups of the image: each the pooled pixels of its own output pixel range
    // [p_lo, p_hi), every channel.  That range lies inside its window and the ranges
    // partition the image, so every element is written exactly once for any nsplit.
    const bool wr = pin.p_out != nullptr;
    if constexpr (CIN % 8 == 0 && sizeof(T) == 2) {
      // a lane owns 8 channels of one pooled pixel (lanes along the pixels: every load
      // instruction reads consecutive pairs of one row): ONE 16-B LDS write of the 8
      // pooled values instead of eight 2-B writes to the same bank group
      constexpr int NO = CIN / 8, NPI = NO * RP, IT8 = (NPI + NTHR - 1) / NTHR;
      P top[IT8][8], bot[IT8][8];
      auto ld8 = [&](int i, int o, int ho, int wo) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const P* src = reinterpret_cast<const P*>(yb + ((size_t)(8 * o + j) * 2 * H + 2 * ho) * 2 * W + 2 * wo);
          top[i][j] = src[0];
          bot[i][j] = src[W];  // next input row (2W elements = W pairs)
        }
      };
#pragma unroll
      for (int i = 0; i < IT8; ++i) {  // issued before the statistics reduction: the latencies overlap
        const int e8 = tid + i * NTHR;
        if constexpr (WIN) {
          // unconditional (clamped item and row, skipped by the pass below): guarded loads
          // are branched around and waited for group by group (BnBwdStage::load)
          const int ec = min(e8, NPI - 1);
          ld8(i, ec / RP, min(r_lo + (ec % RP) / W, H - 1), ec % W);
        } else if (e8 < NPI) {
          ld8(i, e8 / RP, (e8 % RP) / W, e8 % W);
        }
      }
      load_wpk();
      bn_finalize<CIN>(pin.bn, sc_s, beta_s, mean_s, istd_s, part, bid);
      DPA_STAMP(3);
#pragma unroll
      for (int i = 0; i < IT8; ++i) {
        const int e8 = tid + i * NTHR;
        const int o = e8 / RP, hl = (e8 % RP) / W, ho = r_lo + hl, wo = e8 % W;
        if (e8 < NPI && (!WIN || hl < r_n)) {
          const int pix = ho * W + wo;
          const bool own = wr && pix >= p_lo && pix < p_hi;
          unsigned pk[4];  // the 8 pooled values packed in registers (no local array in memory)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ci = 8 * o + j;
            float best, xh;
            int bi;
            bn_relu_max4x<T>(top[i][j], bot[i][j], sc_s[ci], beta_s[ci], mean_s[ci], istd_s[ci], best, bi, xh);
            const T pvj = Cvt<T>::from_f(best);
            const unsigned bits = __builtin_bit_cast(unsigned short, pvj);
            if (j & 1) pk[j >> 1] |= bits << 16; else pk[j >> 1] = bits;
            const int e = ci * HW + pix;  // (ci, pix) index of the pooled outputs
            const int d = i * 8 + j;
            dq_e[d] = own ? e : -1;
            dq_p[d] = pvj;
            dq_i[d] = (uint8_t)(bi | (best > 0.f ? IDX_RELU : 0));
            dq_x[d] = Cvt<T>::from_f(xh);
          }
          // imo keeps each 8-channel group of a pixel contiguous (the swizzle moves groups)
          *reinterpret_cast<uint4*>(&img[imo((ho + 2) * WPD + (wo + 2), 8 * o)]) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
      }
    } else {
      constexpr int NPS = CIN * RP, IT = (NPS + NTHR - 1) / NTHR;  // a lane owns one pooled pixel of one channel
      P top[IT], bot[IT];
      auto ld1 = [&](int i, int ci, int ho, int wo) {
        const P* src = reinterpret_cast<const P*>(yb + ((size_t)ci * 2 * H + 2 * ho) * 2 * W + 2 * wo);
        top[i] = src[0];
        bot[i] = src[W];  // next input row (2W elements = W pairs)
      };
#pragma unroll
      for (int i = 0; i < IT; ++i) {  // issued before the statistics reduction: the latencies overlap
        const int e = tid + i * NTHR;
        if constexpr (WIN) {  // unconditional, clamped (see the 8-channel branch)
          const int ec = min(e, NPS - 1);
          ld1(i, ec / RP, min(r_lo + (ec % RP) / W, H - 1), ec % W);
        } else if (e < NPS) {
          ld1(i, e / RP, (e % RP) / W, e % W);
        }
      }
      load_wpk();
      bn_finalize<CIN>(pin.bn, sc_s, beta_s, mean_s, istd_s, part, bid);
      DPA_STAMP(3);
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int e = tid + i * NTHR;
        const int ci = e / RP, hl = (e % RP) / W, ho = r_lo + hl, wo = e % W;
        if (e < NPS && (!WIN || hl < r_n)) {
          const int pix = ho * W + wo;
          float best, xh;
          int bi;
          bn_relu_max4x<T>(top[i], bot[i], sc_s[ci], beta_s[ci], mean_s[ci], istd_s[ci], best, bi, xh);
          const T pv = Cvt<T>::from_f(best);
          img[imo((ho + 2) * WPD + (wo + 2), ci)] = pv;
          dq_e[i] = wr && pix >= p_lo && pix < p_hi ? ci * HW + pix : -1;
          dq_p[i] = pv;
          dq_i[i] = (uint8_t)(bi | (best > 0.f ? IDX_RELU : 0));
          dq_x[i] = Cvt<T>::from_f(xh);
        }
      }
    }
  } else {
    __shared__ float coef[5 * CIN], sums[2 * CIN];
    float* const part = part_s;
    // the stages produce the windows of rows [r_lo, r_lo + SR) (h: relative to r_lo); this
    // workgroup's are the first r_n (even) of them
    if constexpr (CIN % 8 == 0 && sizeof(T) == 2) {
      BnBwdStage8<T, CIN, H, W, NTHR, SR> st;
      st.load(bin, b, r_lo);
      DPA_STAMP(8);
      load_wpk();
      bn_bwd_coef<CIN, T>(bin, coef, part, sums, bid);
      load_epi();
      DPA_STAMP(3);
      st.emit(coef, [&](int h, int ww, int c0, uint4 q00, uint4 q01, uint4 q10, uint4 q11) {
        if (WIN && h >= r_n) return;
        const int hp = r_lo + h + 2;
        *reinterpret_cast<uint4*>(&img[imo(hp * WPD + (ww + 2), c0)]) = q00;
        *reinterpret_cast<uint4*>(&img[imo(hp * WPD + (ww + 3), c0)]) = q01;
        *reinterpret_cast<uint4*>(&img[imo((hp + 1) * WPD + (ww + 2), c0)]) = q10;
        *reinterpret_cast<uint4*>(&img[imo((hp + 1) * WPD + (ww + 3), c0)]) = q11;
      });
    } else {
      BnBwdStage<T, CIN, H, W, NTHR, SR> st;
      st.load(bin, b, r_lo);
      DPA_STAMP(8);
      load_wpk();
      bn_bwd_coef<CIN, T>(bin, coef, part, sums, bid);
      load_epi();
      DPA_STAMP(3);
      st.emit(coef, [&](int c, int h, int ww, T v00, T v01, T v10, T v11) {
        if (WIN && h >= r_n) return;
        const int hp = r_lo + h + 2;
        img[imo(hp * WPD + (ww + 2), c)] = v00;
        img[imo(hp * WPD + (ww + 3), c)] = v01;
        img[imo((hp + 1) * WPD + (ww + 2), c)] = v10;
        img[imo((hp + 1) * WPD + (ww + 3), c)] = v11;
      });
    }
    store_epi();
  }
  DPA_STAMP(4);
  __syncthreads();
  DPA_STAMP(5);
  if constexpr (PRO == 1) {  // the deferred pooled outputs (see dq_e)
    constexpr int NPO = CIN * HW;
#pragma unroll
    for (int d = 0; d < DQ; ++d)
      if (dq_e[d] >= 0) {
        const size_t o = (size_t)b * NPO + dq_e[d];
        pin.p_out[o] = dq_p[d];
        pin.idx_out[o] = dq_i[d];
        pin.xh_out[o] = dq_x[d];
      }
  }

  const int lane = tid & 63, wv = tid >> 6;
  const int r = lane & 15, q = lane >> 4;

  // statistics accumulators: one pair per quarter with EPI 1 (sq: the slot of the m-tile this
  // wave met in the quarter, -1: none -- a wave meets at most one, its m-tiles lie NTHR / 64 apart)
  float s1[NQ][NT], s2[NQ][NT];
  int sq[NQ];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    sq[k] = -1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) s1[k][nt] = s2[k][nt] = 0.f;
  }
  // EPI 1, two quarters: this workgroup's second quarter starts at m-tile qmid
  const int qmid = NQ == 2 ? (MT * (2 * sp + 1)) / EPI_QUARTERS : mt1;

  for (int mt = mt0 + wv; mt < mt1; mt += NTHR / 64) {
    const int m = mt * 16 + r;
    const int mm_ = m < HW ? m : HW - 1;
    const int oh = mm_ / W, ow = mm_ % W;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      typename mm::frag a;
      if constexpr (CIN == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int tap = 32 * s + 8 * q + j;
          float v = 0.f;
          if (tap < 25) v = Cvt<T>::to_f(img[(oh + tap / 5) * WPD + ow + tap % 5]);
          a[j] = mm::cv(v);
        }
      } else {
        const int kb = 32 * s + 8 * q;
        int tap = kb / CIN;
        const int ci0 = kb % CIN;
        tap = tap < 25 ? tap : 24;  // K padding: weights are zero there
        a = mm::ld(&img[imo((oh + tap / 5) * WPD + ow + tap % 5, ci0)]);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const typename mm::frag bf = mm::ld(&wl[(nt * 16 + r) * KPW + 32 * s + 8 * q]);
        acc[nt] = mm::mma(a, bf, acc[nt]);
      }
    }
    // --- epilogue: D[row = 4q+i][col = r] -> pixel mt*16+4q+i, channel nt*16+r
    const int pix0 = mt * 16 + 4 * q;
    // EPI 1: this m-tile's sums start at zero (e1, e2) and become its quarter's accumulators
    float e1[NT], e2[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) e1[nt] = e2[nt] = 0.f;
    if (pix0 < HW) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int co = nt * 16 + r;
        const float bs = pre_bias[nt];
        T* dst = y + ((size_t)b * COUT + co) * HW + pix0;
        const float sh = pre_shift[nt];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = acc[nt][i] + bs;
          dst[i] = Cvt<T>::from_f(v);
          if (MODE == 0) {
            const float d = rnd_t<T>(v) - sh;
            s1[0][nt] += d;
            s2[0][nt] += d * d;
          }
          if (EPI == 1) {
            const int le = co * EPIX + pix0 - mt0 * 16 + i;
            const float g = (eidx[le] & IDX_RELU) ? rnd_t<T>(v) : 0.f;
            e1[nt] += g;
            e2[nt] += g * Cvt<T>::to_f(exh[le]);
          }
        }
      }
    }
    if constexpr (EPI == 1) {  // (selects, wave-uniform: no indexed registers)
      const bool second = mt >= qmid;
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const bool mine = second == (k == 1);
        sq[k] = mine ? mt - (k == 1 ? qmid : mt0) : sq[k];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          s1[k][nt] = mine ? e1[nt] : s1[k][nt];
          s2[k][nt] = mine ? e2[nt] : s2[k][nt];
        }
      }
    }
  }
  DPA_STAMP(6);
  if constexpr (MODE == 0 || EPI == 1) {
    // partial (k, j) of the workgroup: MODE 0 (k = 0) wave j's; EPI 1 slot j's of its quarter k.
    // Every lane sum first, the masked stores behind them: the quarters' permlane chains are
    // independent and overlap (with the stores in between, each quarter's chain waited for the one
    // before it behind an exec change)
    float a1[NQ][NT], a2[NQ][NT];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        // lanes r, r+16, r+32, r+48 (VALU permlane swaps, no LDS round trip; every lane active)
        a1[k][nt] = xor32_sum(xor16_sum(s1[k][nt]));
        a2[k][nt] = xor32_sum(xor16_sum(s2[k][nt]));
      }
    }
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
      const int j = EPI == 1 ? sq[k] : wv;
      if (q == 0 && j >= 0) {  // summed below in a fixed order (deterministic)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          lstat[(k * (NTHR / 64) + j) * 2 * COUT + nt * 16 + r] = a1[k][nt];
          lstat[(k * (NTHR / 64) + j) * 2 * COUT + COUT + nt * 16 + r] = a2[k][nt];
        }
      }
    }
    __syncthreads();
    if constexpr (EPI == 1) {
      // row 4 b + (this workgroup's first quarter + k): the quarter's slots in slot order from
      // 0.f; a slot past the quarter's m-tiles was written by no wave: whatever its floats hold
      // is loaded (all slots in one batch, one wait) and dropped, and it contributes the 0.f a
      // wave without an m-tile would have stored
      if (tid < NQ * 2 * COUT) {
        const int k = tid / (2 * COUT), c = tid % (2 * COUT);
        const int nsl = k == 0 ? qmid - mt0 : mt1 - qmid;
        float v[NTHR / 64];
#pragma unroll
        for (int j = 0; j < NTHR / 64; ++j) v[j] = lstat[(k * (NTHR / 64) + j) * 2 * COUT + c];
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < NTHR / 64; ++j) t += j < nsl ? v[j] : 0.f;
        epi.bslab[((size_t)b * EPI_QUARTERS + sp * NQ + k) * 2 * COUT + c] = t;
      }
    }
    if constexpr (MODE == 0) {
      float* row = fslab + (size_t)bid * fslab_row(COUT);
      if (tid < 2 * COUT) {
        float t = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NTHR / 64; ++w2) t += lstat[w2 * 2 * COUT + tid];
        row[tid] = t;
      }
      if (tid == 0) {
        const int p0 = mt0 * 16, p1 = min(mt1 * 16, HW);
        row[2 * COUT] = (float)(p1 - p0);
      }
      if (bid == 0 && tid < COUT) fstats[2 * COUT + 1 + tid] = shift[tid];
    }
  }
  if constexpr (PRO == 3) {
    // arrive, as this workgroup's last act (nothing here needs the atomic's return but the
    // completing workgroup); the last of the launch's nimg * nsplit conv workgroups advances
    // the step counter: every one of them has read it by then (relaxed: the next launch reads
    // it after this one completes)
    if (tid == 0) {
      const int arrived = __hip_atomic_fetch_add(&gin.ctr[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (arrived == gin.nimg * nsplit - 1) {
        __hip_atomic_store(&gin.ctr[1], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&gin.ctr[0], step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  DPA_STAMP(7);
}

template <typename T, int CIN, int COUT, int H, int W, int MODE, int PRO = 0, int EPI = 0, int WPK = 0, int WR = H,
          int ES = 0>
__global__ void __launch_bounds__(NTHR)
conv5x5_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
               T* __restrict__ y, float* __restrict__ fslab, float* __restrict__ fstats,
               const float* __restrict__ shift, int nsplit, PoolIn<T> pin = PoolIn<T>{},
               BwdIn<T> bin = BwdIn<T>{}, BwdEpi<T> epi = BwdEpi<T>{}, const T* __restrict__ wpk = nullptr,
               WPack<T> pk = WPack<T>{}, GatherIn gin = GatherIn{}) {
  if constexpr (WPK == 2) {  // the workgroups behind the conv role's pack the layer-2 weights
    const int nconv = gin.nimg * nsplit;
    if ((int)blockIdx.x >= nconv) {
      const int pw = (int)blockIdx.x - nconv;
      if (pw < W2P_WGS)
        pack_w2<T>(pk, pw);
      else  // the head's fc weights (launched only with pk.fcp: pk.NM workgroups)
        pack_fc<T>(pk, pw - W2P_WGS);
      return;
    }
  }
  conv5x5_body<T, CIN, COUT, H, W, MODE, PRO, EPI, WPK, false, WR, ES>(x, w, bias, y, fslab, fstats, shift, nsplit,
                                                                       pin, bin, epi, wpk, pk, (int)blockIdx.x, gin);
}

}  // namespace cb
}  // namespace dpa
