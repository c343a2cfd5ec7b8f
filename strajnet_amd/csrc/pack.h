// Raw record bytes packed on the device into the slots of a resident pool: the inverse of unpack.h / pool.h (the format and the semantics:
// strajnet_amd/data.py, pack_bits / pack_sparse / PoolLayout.replace_reference).  The kernel bodies live here so that a host program can
// compile them, as with unpack.h and pool.h: beyond plain C++ they use threadIdx / blockIdx, __shared__, __syncthreads, __shfl_up,
// __ballot, __popc / __popcll and uint4.
//
// The source is the record's own bytes for B scenes, [B][T][H][W][C] elements; decoded element i of a scene (i < n = T Ho Wo C) is source
// element (t, y0 + y, x0 + x, c) as in stj_decode_raw, uncropped T = H = C = 1, W = n.  A decoded row is R = Wo C contiguous source elements.
//
//   pack_bits_kernel       bool bytes -> pool_words[slot][n / 32] in pack_bits' order; a thread owns one word (32 source bytes, as two
//                          16-byte loads where the word lies in one row and its address is 16-byte aligned)
//   pack_count_kernel      float32 words -> offs_stage[b][blk] = present words (32-bit pattern != 0) of the block
//   pool_admit_kernel      offs_stage[b][0 .. nblk]: counts -> exclusive prefix, the total at [nblk]; ok[b] (&)= slot in [0, N) and
//                          total <= val_base[s + 1] - val_base[s]
//   pack_commit_kernel     float32 words -> the slot's mask words, its offs row and vals[val_base[s] + offs_stage[b][blk] + rank]
//   put_raw_kernel         rows of bytes -> pool[slot]
//
// pack_bits / pack_count / pack_commit: one short-lived workgroup of UP_NT threads per (scene b, block of UP_BLOCK decoded elements), no
// grid-stride loop, no atomics.  In the two sparse kernels a wave owns UP_BLOCK / 4 consecutive elements and takes them 64 at a time: one
// coalesced word load per lane, __ballot(word != 0) is two mask words, and popcount(ballot & lanes below) ranks the present words in
// element order.  A scene with ok[b] == 0 or a slot outside [0, N) is skipped whole, never clamped.
#pragma once
#include "unpack_block.h"

#define PK_WAVES (UP_NT / 64)                       // 4
#define PK_ITERS (UP_BLOCK / UP_NT)                 // 32 ballots of 64 elements per wave
#define PK_RAW_BLOCK (UP_BLOCK * 4)                 // bytes per workgroup of put_raw_kernel: UP_PASSES passes of one 16-byte vector per thread

// the source geometry of one launch; R >= 1 and Ho >= 1 wherever a kernel is launched (n > 0)
struct pk_geom {
  uint64_t S;      // source elements per scene = T H W C
  uint64_t WC;     // source elements per source row = W C
  uint64_t off0;   // (y0 W + x0) C
  uint32_t R;      // Wo C
  uint32_t Ho, H;
};

// where decoded element i of a scene lies in the scene's source: j within its decoded row, y the row within its frame, row = the source
// offset of the row's first element
struct pk_pos {
  uint64_t row;
  uint32_t j, y;
};

__device__ __forceinline__ pk_pos pk_locate(const pk_geom& g, uint32_t i) {
  const uint32_t r = i / g.R, t = r / g.Ho;
  pk_pos p;
  p.j = i - r * g.R;
  p.y = r - t * g.Ho;
  p.row = ((uint64_t)t * g.H + p.y) * g.WC + g.off0;
  return p;
}

// k elements on (any k; a row may be shorter than k)
__device__ __forceinline__ void pk_advance(const pk_geom& g, pk_pos& p, uint32_t k) {
  p.j += k;
  while (p.j >= g.R) {
    p.j -= g.R;
    p.row += g.WC;
    if (++p.y == g.Ho) { p.y = 0; p.row += (uint64_t)(g.H - g.Ho) * g.WC; }
  }
}

// 64 elements on where a row holds at least 64 (so at most one row ends), written as selects: no branch stands between a wave's loads.
// on == false leaves p where it is.
__device__ __forceinline__ void pk_step64(const pk_geom& g, pk_pos& p, bool on) {
  const uint32_t j = p.j + 64u;
  const bool wrap = on && j >= g.R, top = wrap && p.y + 1u == g.Ho;
  p.j = wrap ? j - g.R : (on ? j : p.j);
  p.y = top ? 0u : (wrap ? p.y + 1u : p.y);
  p.row += (wrap ? g.WC : 0u) + (top ? (uint64_t)(g.H - g.Ho) * g.WC : 0u);
}

__device__ __forceinline__ bool pk_slot(const int* __restrict__ ok, const int* __restrict__ slots, uint32_t b, int N, uint32_t* s) {
  const int v = slots[b];
  *s = (uint32_t)v;
  return ok[b] != 0 && v >= 0 && v < N;
}

// bit k of the result = byte k of d is non-zero (k = 0..3)
__device__ __forceinline__ uint32_t pk_nibble(uint32_t d) {
  const uint32_t hi = ((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u) >> 7;      // bit 8 k = byte k non-zero
  return ((hi * 0x00204081u) >> 21) & 15u;                                               // bits 0 / 8 / 16 / 24 -> 21 .. 24, no carries
}

// grid = B * nblk
__global__ __launch_bounds__(UP_NT) void pack_bits_kernel(const uint8_t* __restrict__ src, const int* __restrict__ ok, const int* __restrict__ slots,
                                                          int N, uint32_t* __restrict__ pool, pk_geom g, uint32_t n_words, uint32_t nblk) {
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  uint32_t s;
  if (!pk_slot(ok, slots, b, N, &s)) return;
  const uint32_t wi = blk * (UP_BLOCK / 32) + threadIdx.x;
  if (wi >= n_words) return;
  const uint8_t* __restrict__ sc = src + (size_t)b * g.S;
  pk_pos p = pk_locate(g, wi * 32u);
  uint32_t m = 0;
  const uint8_t* at = sc + p.row + p.j;
  if (p.j + 32u <= g.R && ((uintptr_t)at & 15u) == 0) {
    const uint4 lo = *reinterpret_cast<const uint4*>(at), hi = *reinterpret_cast<const uint4*>(at + 16);
    m = pk_nibble(lo.x) | pk_nibble(lo.y) << 4 | pk_nibble(lo.z) << 8 | pk_nibble(lo.w) << 12 | pk_nibble(hi.x) << 16 | pk_nibble(hi.y) << 20 |
        pk_nibble(hi.z) << 24 | pk_nibble(hi.w) << 28;
  } else {
    for (uint32_t k = 0; k < 32; ++k) {
      m |= (sc[p.row + p.j] != 0 ? 1u : 0u) << k;
      pk_advance(g, p, 1);
    }
  }
  pool[(size_t)s * n_words + wi] = m;                                   // s < N, wi < n_words
}

// A wave's pass over its UP_BLOCK / 4 elements: w[it] = the word of element base + 64 it + lane (0 beyond the scene), -> the wave's present
// words.  `base` is the wave's first element within the scene.
__device__ __forceinline__ uint32_t pk_wave_load(const uint32_t* __restrict__ sc, const pk_geom& g, uint32_t base, uint32_t n, uint32_t lane,
                                                 uint32_t (&w)[PK_ITERS]) {
  uint32_t cnt = 0;
  if (base >= n) {                                                      // uniform over the wave: nothing of the scene here
#pragma unroll
    for (int it = 0; it < PK_ITERS; ++it) w[it] = 0u;
    return 0;
  }
  const uint32_t i0 = base + lane;
  pk_pos p = pk_locate(g, i0 < n ? i0 : base);                          // a lane beyond the scene stays on an element of it
  if (g.R >= 64u) {                                                     // uniform.  Every load is issued before the first word is looked at:
#pragma unroll
    for (int it = 0; it < PK_ITERS; ++it) {                             // a lane that has left the scene re-reads its last element
      w[it] = sc[p.row + p.j];
      pk_step64(g, p, i0 + 64u * (uint32_t)it + 64u < n);
    }
#pragma unroll
    for (int it = 0; it < PK_ITERS; ++it) w[it] = i0 + 64u * (uint32_t)it < n ? w[it] : 0u;
  } else {                                                              // short rows: one load at a time
#pragma unroll
    for (int it = 0; it < PK_ITERS; ++it) {
      const uint32_t i = i0 + 64u * (uint32_t)it;
      w[it] = i < n ? sc[p.row + p.j] : 0u;
      if (i + 64u < n) pk_advance(g, p, 64);
    }
  }
#pragma unroll
  for (int it = 0; it < PK_ITERS; ++it) cnt += (uint32_t)__popcll(__ballot(w[it] != 0u));
  return cnt;
}

// grid = B * nblk; offs_stage [B][nblk + 1]
__global__ __launch_bounds__(UP_NT) void pack_count_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ offs_stage, pk_geom g, uint32_t n,
                                                           uint32_t nblk) {
  __shared__ uint32_t wsum[PK_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  uint32_t w[PK_ITERS];
  const uint32_t cnt = pk_wave_load(src + (size_t)b * g.S, g, blk * UP_BLOCK + wv * (UP_BLOCK / PK_WAVES), n, lane, w);
  if (lane == 0) wsum[wv] = cnt;
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < PK_WAVES; ++k) c += wsum[k];
    offs_stage[(size_t)b * (nblk + 1) + blk] = c;
  }
}

// grid = B, one workgroup per scene; any nblk >= 0.  offs_stage == NULL: no sparse key, the range check of the slot alone.
__global__ __launch_bounds__(UP_NT) void pool_admit_kernel(uint32_t* __restrict__ offs_stage, uint32_t nblk, const long long* __restrict__ val_base,
                                                           const int* __restrict__ slots, int N, int* __restrict__ ok, int first) {
  __shared__ uint32_t wsum[PK_WAVES];
  __shared__ uint32_t carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t b = blockIdx.x;
  uint32_t total = 0;
  bool over = false;                                                    // the total passed 2^32: no slot holds that
  if (offs_stage) {
    uint32_t* __restrict__ row = offs_stage + (size_t)b * (nblk + 1);
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < nblk; k0 += UP_NT) {                     // nblk is 64 - 128 at the real geometry: one round
      const uint32_t k = k0 + tid;
      const uint32_t c = k < nblk ? row[k] : 0u;
      uint32_t inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= (uint32_t)o) inc += y;
      }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      uint32_t ex = carry_s + inc - c;
#pragma unroll
      for (uint32_t q = 0; q < PK_WAVES; ++q)
        if (q < wv) ex += wsum[q];
      if (k < nblk) row[k] = ex;
      __syncthreads();                                                  // everyone has read carry_s and wsum
      if (tid == UP_NT - 1) {
        if (ex + c < carry_s) over = true;                              // (a count is at most UP_BLOCK: only the running total can wrap)
        carry_s = ex + c;
      }
      __syncthreads();
    }
    total = carry_s;
    if (tid == 0) row[nblk] = total;
  }
  if (tid == UP_NT - 1) {                                               // the thread that knows `over`
    const int s = slots[b];
    int v = (s >= 0 && s < N) ? 1 : 0;
    if (!first) v &= ok[b] != 0 ? 1 : 0;
    if (v && offs_stage) {
      const long long lo = val_base[s], hi = val_base[s + 1];
      if (over || hi < lo || (unsigned long long)(hi - lo) < (unsigned long long)total) v = 0;
    }
    ok[b] = v;
  }
}

// grid = B * nblk.  Index arithmetic into vals is 64-bit; every store into vals is below both n_vals and the slot's end and not below
// its start, whatever offs_stage and val_base hold.
__global__ __launch_bounds__(UP_NT) void pack_commit_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ offs_stage,
                                                            const int* __restrict__ ok, const int* __restrict__ slots, int N,
                                                            uint32_t* __restrict__ mask_pool, uint32_t* __restrict__ offs_pool,
                                                            const long long* __restrict__ val_base, uint32_t* __restrict__ vals, uint64_t n_vals,
                                                            pk_geom g, uint32_t n, uint32_t nblk) {
  __shared__ uint32_t wsum[PK_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  uint32_t s;
  if (!pk_slot(ok, slots, b, N, &s)) return;                            // uniform over the workgroup
  const uint32_t n_words = n / 32u;
  const uint32_t base = blk * UP_BLOCK + wv * (UP_BLOCK / PK_WAVES);
  uint32_t w[PK_ITERS];
  const uint32_t cnt = pk_wave_load(src + (size_t)b * g.S, g, base, n, lane, w);
  if (lane == 0) wsum[wv] = cnt;
  __syncthreads();
  const uint32_t* __restrict__ srow = offs_stage + (size_t)b * (nblk + 1);
  const long long lo = val_base[s], hi = val_base[s + 1];
  const uint64_t end = (lo < 0 || hi < lo) ? 0u : ((uint64_t)hi < n_vals ? (uint64_t)hi : n_vals);      // stores stay in [lo, end)
  uint64_t at = (uint64_t)lo + srow[blk];
#pragma unroll
  for (uint32_t k = 0; k < PK_WAVES; ++k)
    if (k < wv) at += wsum[k];
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t mine = 0;                                                    // lane `it` keeps ballot `it`: two mask words
#pragma unroll
  for (int it = 0; it < PK_ITERS; ++it) {
    const uint64_t bal = __ballot(w[it] != 0u);
    if (w[it] != 0u) {
      const uint64_t q = at + (uint32_t)__popcll(bal & below);
      if (q >= (uint64_t)lo && q < end) vals[q] = w[it];
    }
    at += (uint32_t)__popcll(bal);
    if (lane == (uint32_t)it) mine = bal;
  }
  if (lane < PK_ITERS) {
    const uint32_t wi = base / 32u + 2u * lane;
    uint32_t* __restrict__ mrow = mask_pool + (size_t)s * n_words;
    if (wi < n_words) mrow[wi] = (uint32_t)mine;
    if (wi + 1u < n_words) mrow[wi + 1u] = (uint32_t)(mine >> 32);
  }
  if (tid == 0) {
    uint32_t* __restrict__ orow = offs_pool + (size_t)s * (nblk + 1);
    orow[blk] = srow[blk];
    if (blk == nblk - 1) orow[nblk] = srow[nblk];
  }
}

// grid = B * nblk, nblk = ceil(row_bytes / PK_RAW_BLOCK); src [B][row_bytes], pool [N][row_bytes].  A 16-byte piece goes as one vector
// where it is whole and both addresses are 16-byte aligned, byte by byte elsewhere.
__global__ __launch_bounds__(UP_NT) void put_raw_kernel(const uint8_t* __restrict__ src, const int* __restrict__ ok, const int* __restrict__ slots, int N,
                                                        uint8_t* __restrict__ pool, uint64_t row_bytes, uint32_t nblk) {
  const uint32_t b = (uint32_t)blockIdx.x / nblk, blk = (uint32_t)blockIdx.x % nblk;
  uint32_t s;
  if (!pk_slot(ok, slots, b, N, &s)) return;
  const uint8_t* __restrict__ from = src + (size_t)b * row_bytes;
  uint8_t* __restrict__ to = pool + (size_t)s * row_bytes;
#pragma unroll
  for (int p = 0; p < UP_PASSES; ++p) {
    const uint64_t o = (uint64_t)blk * PK_RAW_BLOCK + ((uint32_t)p * UP_NT + threadIdx.x) * 16u;
    if (o + 16u <= row_bytes && (((uintptr_t)(from + o) | (uintptr_t)(to + o)) & 15u) == 0) {
      *reinterpret_cast<uint4*>(to + o) = *reinterpret_cast<const uint4*>(from + o);
    } else {
      for (uint64_t q = o; q < o + 16u && q < row_bytes; ++q) to[q] = from[q];
    }
  }
}
