// Granule helpers shared by the depthwise kernels (conv_dw.hip: 3x3, conv_dw5.hip: 5x5): the
// channel block, the LDS pixel stride, 16-B granule loads / stores and the zero-filled halo tile.
#pragma once

#include "common.h"

namespace dpa {
namespace dwconv {

constexpr int CB = 64;  // channels per workgroup
constexpr int NG = 8;   // granules (8 channels, 16 B) per channel block
constexpr int PS = 72;  // LDS pixel stride, elements

typedef unsigned short lds_t;  // LDS arrays are raw 16-bit words
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// ---- granules ----------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void unpack(u32x4 v, float (&f)[8]);
template <> __device__ __forceinline__ void unpack<__hip_bfloat16>(u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __builtin_bit_cast(float, v[i] << 16);
    f[2 * i + 1] = __builtin_bit_cast(float, v[i] & 0xffff0000u);
  }
}
template <> __device__ __forceinline__ void unpack<__half>(u32x4 v, float (&f)[8]) {
  const f16x8 h = __builtin_bit_cast(f16x8, v);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
}
template <typename T> __device__ __forceinline__ void ld_gran(const lds_t* p, float (&f)[8]) {
  unpack<T>(*reinterpret_cast<const u32x4*>(p), f);
}
// eight fp32 values -> one rounding each -> one 16-B store
template <typename T> __device__ __forceinline__ void st_gran(T* p, const float (&f)[8]) {
  typedef typename MM<T>::elem E;
  u16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const E e = MM<T>::cv(f[i]);
    v[i] = __builtin_bit_cast(unsigned short, e);
  }
  *reinterpret_cast<u16x8*>(p) = v;
}

// RH x RW pixels x ng granules of image n from (h0, w0) of an [N][H][W][C] tensor; zeros
// outside [0, H) x [0, W) and in the masked granules.
template <typename T, int RH, int RW>
__device__ __forceinline__ void stage_tile(lds_t* lds, const T* __restrict__ src, int n, int H, int W, int C, int c0,
                                           int ng, int h0, int w0) {
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int i = threadIdx.x; i < RH * RW * NG; i += 256) {
    const int p = i >> 3, g = i & 7;
    const int h = h0 + p / RW, x = w0 + p % RW;
    u16x8 v = z;
    if (g < ng && (unsigned)h < (unsigned)H && (unsigned)x < (unsigned)W)
      v = *reinterpret_cast<const u16x8*>(src + (((size_t)n * H + h) * W + x) * C + c0 + 8 * g);
    *reinterpret_cast<u16x8*>(lds + p * PS + 8 * g) = v;
  }
}

// bf16 / fp16 only: the callers' check_act has refused everything else
#define DWCONV_DISPATCH(t, ...)                                                \
  do {                                                                         \
    if ((t).scalar_type() == at::kBFloat16) { typedef __hip_bfloat16 T; __VA_ARGS__; } \
    else { typedef __half T; __VA_ARGS__; }                                    \
  } while (0)

}  // namespace dwconv
}  // namespace dpa
