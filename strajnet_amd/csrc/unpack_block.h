// What the expanding kernels of unpack.h and pool.h share: the block geometry, the bit -> float32 macro and one block of a sparse plane.
// Plain enough for a host program to compile: threadIdx, __shared__, __syncthreads, __shfl_up, __popc and uint4 are all it uses.
#pragma once
#include <stdint.h>

#define UP_BLOCK 8192                       // elements per block = data.SPARSE_BLOCK
#define UP_NT 256                           // threads per workgroup: one mask word of the block each
#define UP_PASSES (UP_BLOCK / (4 * UP_NT))  // 8
#define UP_ONE 0x3f800000u                  // 1.0f

static_assert(UP_BLOCK == 32 * UP_NT, "a thread owns one mask word of its block");

// the 4 elements of nibble `nib` (0..7) of a mask word as float32 bit patterns 1.0f / 0.0f
#define UP_BIT(m, k) ((((m) >> (k)) & 1u) ? UP_ONE : 0u)

// One block of a sparse plane, shared by unpack_sparse_kernel and gather_sparse_kernel (pool.h): mask_s the scene's mask [n_words], w0 the
// block's first word within the scene, first = the index in `vals` of the block's first present word, out the block's first vector.
// I is the index type: uint32_t for a batch, uint64_t for a pool (its value words can pass 2^32).  Every gather index is clamped to
// n_vals - 1, and with n_vals == 0 nothing is gathered: whatever mask and `first` hold, the reads stay inside `vals`.
template <typename I>
__device__ __forceinline__ void up_sparse_block(const uint32_t* __restrict__ mask_s, const uint32_t* __restrict__ vals, I first, I n_vals,
                                                uint4* __restrict__ out, uint32_t n_words, uint32_t w0) {
  __shared__ uint32_t mw[UP_NT];            // the block's mask words
  __shared__ uint32_t pre[UP_NT];           // present elements of the block in front of each word
  __shared__ uint32_t wsum[UP_NT / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t wi = w0 + tid;
  const uint32_t m = (wi < n_words && n_vals) ? mask_s[wi] : 0u;
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
  const I last = n_vals ? n_vals - 1u : 0u;
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint32_t q = (uint32_t)p * UP_NT + tid;
    const uint32_t w = q >> 3, sh = (q & 7u) * 4u;
    if (w0 + w < n_words) {
      const uint32_t mm = mw[w];
      I idx = first + pre[w] + (uint32_t)__popc(mm & ((1u << sh) - 1u));
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
