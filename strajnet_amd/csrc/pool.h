// A pool of N packed scenes resident on the device, expanded B at a time by an index vector that lives on the device too (the format:
// strajnet_amd/data.py, PoolLayout / reference_gather).  The kernel bodies live here so that a host program can compile them, as with
// unpack.h: beyond plain C++ they use threadIdx / blockIdx, __shared__, __syncthreads, __shfl_up, __popc and uint4.
//
//   gather_bits_kernel     pool [N][n / 32] words in pack_bits' order            -> dst[b] = unpack_bits of scene idx[b]
//   gather_sparse_kernel   mask [N][n / 32], offs [N][nblk + 1], val_base int64 [N + 1], vals [n_vals]
//                                                                                -> dst[b] = unpack_sparse of scene idx[b]
//   gather_raw_kernel      pool [N][n] elements of KIND (rawcast.h)              -> dst[b][i] = scale * cast(pool[idx[b]][i])
//
// All three: one short-lived workgroup of UP_NT threads per (output scene b, block of UP_BLOCK elements), UP_PASSES passes, a thread
// stores one 16-byte vector per pass, no grid-stride loop.  The scene index is one uniform load per workgroup, clamped to [0, N - 1]: no
// value of idx[b] makes a kernel read outside the pool.  Unlike unpack_bits_kernel the bits kernel addresses per scene: n is a multiple
// of 32, not of UP_BLOCK, so a scene's last block is partial and the next scene starts inside a block of the batch.
#pragma once
#include "unpack_block.h"
#include "rawcast.h"

__device__ __forceinline__ uint32_t pool_scene(const int* __restrict__ idx, uint32_t b, int N) {
  const int s = idx[b];
  return (uint32_t)(s < 0 ? 0 : (s > N - 1 ? N - 1 : s));               // N >= 1 (the launcher refuses N < 1)
}

// grid = B * nblk
__global__ __launch_bounds__(UP_NT) void gather_bits_kernel(const uint32_t* __restrict__ pool, const int* __restrict__ idx, int N,
                                                            uint4* __restrict__ dst, uint32_t n_words, uint32_t nblk) {
  const uint32_t tid = threadIdx.x;
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  const uint32_t* __restrict__ src = pool + (size_t)pool_scene(idx, b, N) * n_words;
  const uint32_t w0 = blk * (UP_BLOCK / 32);                            // the block's first word within its scene
  uint4* __restrict__ out = dst + ((size_t)b * n_words + w0) * 8;       // 8 vectors per word
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint32_t q = (uint32_t)p * UP_NT + tid;                       // vector of 4 elements within the block
    const uint32_t w = w0 + (q >> 3);
    if (w < n_words) {
      const uint32_t m = src[w] >> ((q & 7u) * 4u);
      uint4 v;
      v.x = UP_BIT(m, 0); v.y = UP_BIT(m, 1); v.z = UP_BIT(m, 2); v.w = UP_BIT(m, 3);
      out[q] = v;                                                       // inside scene b of dst because w < n_words
    }
  }
}

// grid = B * nblk.  val_base is 64-bit and so is every index into vals; a garbage val_base / offs wraps or not, the clamp of
// up_sparse_block holds it inside vals either way.
__global__ __launch_bounds__(UP_NT) void gather_sparse_kernel(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ offs,
                                                              const long long* __restrict__ val_base, const uint32_t* __restrict__ vals,
                                                              uint64_t n_vals, const int* __restrict__ idx, int N, uint4* __restrict__ dst,
                                                              uint32_t n_words, uint32_t nblk) {
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  const uint32_t s = pool_scene(idx, b, N);
  const uint32_t w0 = blk * (UP_BLOCK / 32);
  const uint64_t first = (uint64_t)val_base[s] + offs[(size_t)s * (nblk + 1) + blk];
  up_sparse_block<uint64_t>(mask + (size_t)s * n_words, vals, first, n_vals, dst + ((size_t)b * n_words + w0) * 8, n_words, w0);
}

// grid = B * nblk, nblk = ceil(n / UP_BLOCK); any n.  dst is 16-byte aligned as a whole, so scene b's row is where (b * n) % 4 == 0: there
// a thread stores its 4 elements as one vector, except the row's last n % 4 elements; elsewhere element by element.
template <int KIND>
__global__ __launch_bounds__(UP_NT) void gather_raw_kernel(const void* __restrict__ pool, const int* __restrict__ idx, int N,
                                                           float* __restrict__ dst, uint32_t n, uint32_t nblk, float scale) {
  const uint32_t tid = threadIdx.x;
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  const long long s0 = (long long)pool_scene(idx, b, N) * n;            // the scene's first element in the pool
  float* __restrict__ out = dst + (size_t)b * n;
  const bool aligned = (((size_t)b * n) & 3u) == 0;
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint64_t i = (uint64_t)blk * UP_BLOCK + ((uint32_t)p * UP_NT + tid) * 4u;      // first of the thread's 4 elements; n < 2^32
    if (i + 4 <= n && aligned) {
      float f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = raw_to_f32<KIND>(pool, s0 + (long long)i + j) * scale;
      uint4 v;
      __builtin_memcpy(&v, f, 16);
      *reinterpret_cast<uint4*>(out + i) = v;
    } else {
      for (uint64_t j = i; j < i + 4 && j < n; ++j) out[j] = raw_to_f32<KIND>(pool, s0 + (long long)j) * scale;
    }
  }
}
