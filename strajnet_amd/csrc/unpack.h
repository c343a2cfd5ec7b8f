// Expansion of the packed record features (the format: strajnet_amd/data.py, pack_bits / pack_sparse / unpack_reference) into the float32
// tensors the model takes.  The kernel bodies live here so that a host program can compile them too, with a workgroup as threads plus a
// barrier: everything they use beyond plain C++ is threadIdx / blockIdx, __shared__, __syncthreads, __shfl_up, __popc and uint4.
//
//   unpack_bits_kernel     one workgroup per UP_BLOCK elements: bit i & 7 of byte i >> 3 (= bit i & 31 of little-endian word i >> 5)
//                          -> 1.0f / 0.0f
//   unpack_sparse_kernel   one workgroup per (scene, block of UP_BLOCK elements): element i of the scene is
//                          vals[val_base[scene] + offs[scene][block] + popcount(mask bits of the block below i)] where its mask bit is set,
//                          +0.0f elsewhere
//
// Both: UP_NT threads, UP_PASSES passes, a thread stores one 16-byte vector per pass (a wave: 1 KB contiguous); short-lived workgroups,
// no grid-stride loop.  Sizes are multiples of 32 elements, so a vector of 4 elements and a mask word are inside or outside as a whole.
#pragma once
#include <stdint.h>

#define UP_BLOCK 8192                       // elements per block = data.SPARSE_BLOCK
#define UP_NT 256                           // threads per workgroup: one mask word of the block each
#define UP_PASSES (UP_BLOCK / (4 * UP_NT))  // 8
#define UP_ONE 0x3f800000u                  // 1.0f

static_assert(UP_BLOCK == 32 * UP_NT, "a thread owns one mask word of its block");

// the 4 elements of nibble `nib` (0..7) of a mask word as float32 bit patterns 1.0f / 0.0f
#define UP_BIT(m, k) ((((m) >> (k)) & 1u) ? UP_ONE : 0u)

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
// A malformed stream cannot read outside `vals`: every gather index is clamped to n_vals - 1, and with n_vals == 0 nothing is gathered.
__global__ __launch_bounds__(UP_NT) void unpack_sparse_kernel(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ offs,
                                                              const uint32_t* __restrict__ val_base, const uint32_t* __restrict__ vals,
                                                              uint32_t n_vals, uint4* __restrict__ dst, uint32_t n_words, uint32_t nblk) {
  __shared__ uint32_t mw[UP_NT];            // the block's mask words
  __shared__ uint32_t pre[UP_NT];           // present elements of the block in front of each word
  __shared__ uint32_t wsum[UP_NT / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  const uint32_t w0 = blk * (UP_BLOCK / 32);                            // the block's first word within its scene
  const uint32_t wi = w0 + tid;
  const uint32_t m = (wi < n_words && n_vals) ? mask[(size_t)b * n_words + wi] : 0u;
  const uint32_t c = (uint32_t)__popc(m);
  uint32_t inc = c;                                                     // inclusive scan over the wave, then over the 4 waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
    if (lane >= (uint32_t)o) inc += y;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t ex = inc - c;
#pragma unroll
  for (uint32_t k = 0; k < UP_NT / 64; ++k)
    if (k < wv) ex += wsum[k];
  mw[tid] = m;
  pre[tid] = ex;
  __syncthreads();
  const uint32_t first = val_base[b] + offs[(size_t)b * (nblk + 1) + blk];
  const uint32_t last = n_vals ? n_vals - 1u : 0u;
  uint4* out = dst + ((size_t)b * n_words + w0) * 8;                    // 8 vectors per word
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint32_t q = (uint32_t)p * UP_NT + tid;
    const uint32_t w = q >> 3, sh = (q & 7u) * 4u;
    if (w0 + w < n_words) {
      const uint32_t mm = mw[w];
      uint32_t idx = first + pre[w] + (uint32_t)__popc(mm & ((1u << sh) - 1u));
      const uint32_t nib = mm >> sh;
      uint32_t e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = 0u;
        if ((nib >> j) & 1u) { e[j] = vals[idx < last ? idx : last]; ++idx; }
      }
      uint4 v;
      v.x = e[0]; v.y = e[1]; v.z = e[2]; v.w = e[3];
      out[q] = v;
    }
  }
}
