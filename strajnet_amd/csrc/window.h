// A shuffle window over a resident pool: the draw of a batch from the live slots and the refill of consumed slots from records that are
// already packed (the semantics: strajnet_amd/data.py, ShuffleWindow.reference / PoolLayout.replace_packed_reference).  The rules live in
// plain functions (WIN_FN) that a host program compiles as they stand; the kernels below them, compiled for the device only, hand each
// thread its share of those functions and add nothing but a barrier.
//
//   pool_draw_kernel          perm int32 [N], u uint32 [B] -> B steps of a Fisher-Yates shuffle over perm[tail : tail + n_live) (circular),
//                             idx[i] = the slot drawn at step i.  One workgroup, one lane: the steps depend on each other and B is a few dozen.
//   pool_admit_packed_kernel  offs_src [B][nblk + 1] (scene-relative, as pack_sparse writes them), src_base int64 [B + 1]: check_sparse and the
//                             capacity rule -> ok[b].  One workgroup per scene, launched once per sparse key.
//   pool_put_vals_kernel      vals_src[src_base[b] ..) -> vals[val_base[slots[b]] ..): a workgroup per (scene, piece of WIN_PIECE words).
//
// 256-thread short-lived workgroups, no grid-stride loop, no allocation, no atomics.  Every access to perm is taken mod N and a value read
// from it is clamped to [0, N - 1] before it becomes an index; every store of put_vals lies inside [val_base[s], min(val_base[s + 1], n_vals)).
// A scene with ok[b] == 0 or a slot outside [0, N) is skipped, never clamped.
#pragma once
#include <stdint.h>

#define WIN_NT 256                          // threads per workgroup
#define WIN_BLOCK 8192                      // elements per block of a sparse plane's offs = data.SPARSE_BLOCK
#define WIN_PIECE 8192                      // value words per workgroup of pool_put_vals_kernel
#define WIN_PASSES (WIN_PIECE / (4 * WIN_NT))    // 8 passes of one 16-byte vector per thread

#if defined(__HIPCC__) || defined(__HIP__)
#define WIN_FN __host__ __device__ __forceinline__
#else
#define WIN_FN static inline
#endif

// ---------------------------------------------------------------------------------------------------------------------------- draw
// B steps of the partial Fisher-Yates shuffle; the caller guarantees N >= 1, 0 <= tail < N, 0 <= B <= n_live.  j = (u[i] * m) >> 32 is in
// [0, m): the multiply-shift, biased by at most m / 2^32.  n_live may exceed N (garbage): the positions are taken mod N all the same.
WIN_FN void win_draw(int* perm, int N, int tail, int n_live, const uint32_t* u, int* idx, int B) {
  for (int i = 0; i < B; ++i) {
    const uint64_t m = (uint64_t)(uint32_t)(n_live - i);
    const uint64_t j = ((uint64_t)u[i] * m) >> 32;
    const uint64_t at = (uint64_t)(uint32_t)tail + (uint64_t)(uint32_t)i;
    const uint32_t p = (uint32_t)(at % (uint32_t)N), q = (uint32_t)((at + j) % (uint32_t)N);
    const int a = perm[p], b = perm[q];
    perm[p] = b;
    perm[q] = a;
    idx[i] = b < 0 ? 0 : (b > N - 1 ? N - 1 : b);
  }
}

// --------------------------------------------------------------------------------------------------------------------------- admit
// Block k (k < nblk) of a scene's offs row: it starts at 0, does not decrease, and holds no more present words than the block has elements.
WIN_FN bool win_block_ok(const uint32_t* row, uint32_t k, uint32_t nblk, uint64_t n) {
  const uint32_t lo = row[k], hi = row[k + 1];
  const uint64_t first = (uint64_t)k * WIN_BLOCK;
  const uint64_t cap = first >= n ? 0u : (n - first < WIN_BLOCK ? n - first : (uint64_t)WIN_BLOCK);
  (void)nblk;
  return hi >= lo && (uint64_t)(hi - lo) <= cap && (k != 0 || lo == 0u);
}

// What one thread decides once every block has been looked at.  rows_ok: all blocks passed win_block_ok; row: the scene's offs row.
WIN_FN int win_admit_decide(int first, int prev, int s, int N, bool rows_ok, const uint32_t* row, uint32_t nblk, const long long* src_base, uint32_t b,
                            const long long* val_base) {
  int v = (s >= 0 && s < N) ? 1 : 0;
  if (!first) v &= prev != 0 ? 1 : 0;
  if (!rows_ok || row[0] != 0u) return 0;
  const uint64_t total = row[nblk];
  const long long slo = src_base[b], shi = src_base[b + 1];
  if (shi < slo || (uint64_t)shi - (uint64_t)slo != total) return 0;
  if (v) {
    const long long lo = val_base[s], hi = val_base[s + 1];
    if (hi < lo || (uint64_t)hi - (uint64_t)lo < total) v = 0;
  }
  return v;
}

// -------------------------------------------------------------------------------------------------------------------------- put vals
struct win_span {
  uint64_t src, dst;      // first word of the piece in vals_src / in vals
  uint32_t cnt;           // words of the piece, 1 .. WIN_PIECE
};

// The piece `piece` of scene b going to slot s (0 <= s < N): false when there is nothing of it.  The copied words are the scene's first
// min(total, room) with room = min(val_base[s + 1], n_vals) - val_base[s]: the destination range is clipped, never moved.
WIN_FN bool win_put_span(const long long* src_base, const long long* val_base, uint64_t n_vals, uint32_t b, uint32_t s, uint64_t piece, win_span* sp) {
  const long long slo = src_base[b], shi = src_base[b + 1];
  const long long lo = val_base[s], hi = val_base[s + 1];
  if (slo < 0 || shi < slo || lo < 0 || hi < lo) return false;
  const uint64_t end = (uint64_t)hi < n_vals ? (uint64_t)hi : n_vals;
  if ((uint64_t)lo >= end) return false;
  const uint64_t total = (uint64_t)shi - (uint64_t)slo, room = end - (uint64_t)lo;
  const uint64_t all = total < room ? total : room;
  const uint64_t o = piece * (uint64_t)WIN_PIECE;
  if (o >= all) return false;
  sp->src = (uint64_t)slo + o;
  sp->dst = (uint64_t)lo + o;
  sp->cnt = (uint32_t)(all - o < WIN_PIECE ? all - o : (uint64_t)WIN_PIECE);
  return true;
}

// Thread tid's share of a piece: 16-byte vectors where both addresses are 16-byte aligned (a piece starts a multiple of WIN_PIECE words
// into its scene, so all pieces of a scene take the same path), words elsewhere, one word per thread and pass.
WIN_FN void win_put_thread(const uint32_t* vals_src, uint32_t* vals, const win_span& sp, uint32_t tid) {
  const uint32_t* from = vals_src + sp.src;
  uint32_t* to = vals + sp.dst;
  if ((((uintptr_t)from | (uintptr_t)to) & 15u) == 0) {
    for (uint32_t p = 0; p < WIN_PASSES; ++p) {
      const uint32_t w = (p * WIN_NT + tid) * 4u;
      if (w + 4u <= sp.cnt) {
        uint32_t v[4];
        __builtin_memcpy(v, __builtin_assume_aligned(from + w, 16), 16);
        __builtin_memcpy(__builtin_assume_aligned(to + w, 16), v, 16);
      } else {
        for (uint32_t k = w; k < w + 4u && k < sp.cnt; ++k) to[k] = from[k];
      }
    }
  } else {
    for (uint32_t p = 0; p < WIN_PIECE / WIN_NT; ++p) {
      const uint32_t w = p * WIN_NT + tid;
      if (w < sp.cnt) to[w] = from[w];
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------------- kernels
#if defined(__HIPCC__) || defined(__HIP__)
__global__ __launch_bounds__(WIN_NT) void pool_draw_kernel(int* __restrict__ perm, int N, int tail, int n_live, const uint32_t* __restrict__ u,
                                                           int* __restrict__ idx, int B) {
  if (blockIdx.x == 0 && threadIdx.x == 0) win_draw(perm, N, tail, n_live, u, idx, B);
}

// grid = B, one workgroup per scene; any nblk >= 0 (the blocks 256 at a time)
__global__ __launch_bounds__(WIN_NT) void pool_admit_packed_kernel(const uint32_t* __restrict__ offs_src, uint32_t nblk, uint64_t n,
                                                                   const long long* __restrict__ src_base, const long long* __restrict__ val_base,
                                                                   const int* __restrict__ slots, int N, int* __restrict__ ok, int first) {
  __shared__ int bad_s;
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const uint32_t* __restrict__ row = offs_src + (size_t)b * (nblk + 1);
  if (tid == 0) bad_s = 0;
  __syncthreads();
  bool bad = false;
  for (uint32_t k = tid; k < nblk; k += WIN_NT) bad |= !win_block_ok(row, k, nblk, n);
  if (bad) bad_s = 1;                                                   // every writer stores the same value
  __syncthreads();
  if (tid == 0) ok[b] = win_admit_decide(first, first ? 0 : ok[b], slots[b], N, bad_s == 0, row, nblk, src_base, b, val_base);
}

// grid = (ceil(n_vals / WIN_PIECE), B): the launcher knows no bound on a scene's words but n_vals; a workgroup beyond its scene's words
// leaves after four loads.
__global__ __launch_bounds__(WIN_NT) void pool_put_vals_kernel(const uint32_t* __restrict__ vals_src, const long long* __restrict__ src_base,
                                                               const int* __restrict__ ok, const int* __restrict__ slots, int N,
                                                               const long long* __restrict__ val_base, uint32_t* __restrict__ vals, uint64_t n_vals) {
  const uint32_t b = blockIdx.y;
  const int s = slots[b];
  if (ok[b] == 0 || s < 0 || s >= N) return;                            // uniform over the workgroup
  win_span sp;
  if (!win_put_span(src_base, val_base, n_vals, b, (uint32_t)s, blockIdx.x, &sp)) return;
  win_put_thread(vals_src, vals, sp, threadIdx.x);
}
#endif
