// The two per-value rules of the challenge format (reference inference.py:168-181), shared by quantize.hip and the quantising
// epilogue of conv_ws.hip's outconv_pair_gather_kernel: both kernels must produce the same byte from the same float.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define QZ_RUN 256        // cells per workgroup of quantize_waypoints_kernel

// uint8 np.round(sigmoid(x) * 255): accurate expf, IEEE division, round-half-to-even; NaN -> 0
__device__ __forceinline__ uint32_t quant_prob(float x) {
  const float p = 255.f * (1.f / (1.f + expf(-x)));
  return p == p ? (uint32_t)(int)rintf(p) : 0u;
}
// int8 np.clip(np.round(x), -128, 127) as its byte; NaN -> 0
__device__ __forceinline__ uint32_t quant_flow(float x) {
  const float r = fminf(fmaxf(rintf(x), -128.f), 127.f);
  return x == x ? (uint32_t)(int)r & 0xffu : 0u;
}
