// Expansion of the packed record features (the format: strajnet_amd/data.py, pack_bits / pack_sparse / unpack_reference) into the float32
// tensors the model takes.  The kernel bodies live here so that a host program can compile them too, with a workgroup as threads plus a
// barrier: everything they use beyond plain C++ is threadIdx / blockIdx, __shared__, __syncthreads, __shfl_up, __popc and uint4.
//
//   unpack_bits_kernel     one workgroup per UP_BLOCK elements: bit i & 7 of byte i >> 3 (= bit i & 31 of little-endian word i >> 5)
//                          -> 1.0f / 0.0f
//   unpack_sparse_kernel   one workgroup per (scene, block of UP_BLOCK elements): element i of the scene is
//                          vals[val_base[scene] + offs[scene][block] + popcount(mask bits of the block below i)] where its mask bit is set,
//                          +0.0f elsewhere (the block itself: up_sparse_block in unpack_block.h, shared with pool.h)
//
// Both: UP_NT threads, UP_PASSES passes, a thread stores one 16-byte vector per pass (a wave: 1 KB contiguous); short-lived workgroups,
// no grid-stride loop.  Sizes are multiples of 32 elements, so a vector of 4 elements and a mask word are inside or outside as a whole.
#pragma once
#include "unpack_block.h"

__global__ __launch_bounds__(UP_NT) void unpack_bits_kernel(const uint32_t* __restrict__ bits, uint4* __restrict__ dst, uint32_t n_words) {
  const uint32_t tid = threadIdx.x;
  const uint32_t w0 = (uint32_t)blockIdx.x * (UP_BLOCK / 32);          // the block's first word; blockIdx.x < 2^19
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint32_t q = (uint32_t)p * UP_NT + tid;                       // vector of 4 elements within the block
    const uint32_t w = w0 + (q >> 3);
    if (w < n_words) {
      const uint32_t m = bits[w] >> ((q & 7u) * 4u);
      uint4 v;
      v.x = UP_BIT(m, 0); v.y = UP_BIT(m, 1); v.z = UP_BIT(m, 2); v.w = UP_BIT(m, 3);
      dst[(size_t)blockIdx.x * (UP_BLOCK / 4) + q] = v;                 // < n_total / 4 because w < n_words
    }
  }
}

// mask [B][n_words], offs [B][nblk + 1], val_base [B + 1], vals [n_vals], dst [B][n_words * 32]; grid = B * nblk.
// A malformed stream cannot read outside `vals`: see up_sparse_block.
__global__ __launch_bounds__(UP_NT) void unpack_sparse_kernel(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ offs,
                                                              const uint32_t* __restrict__ val_base, const uint32_t* __restrict__ vals,
                                                              uint32_t n_vals, uint4* __restrict__ dst, uint32_t n_words, uint32_t nblk) {
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  const uint32_t w0 = blk * (UP_BLOCK / 32);                            // the block's first word within its scene
  const uint32_t first = val_base[b] + offs[(size_t)b * (nblk + 1) + blk];
  up_sparse_block<uint32_t>(mask + (size_t)b * n_words, vals, first, n_vals, dst + ((size_t)b * n_words + w0) * 8, n_words, w0);   // 8 vectors per word
}
