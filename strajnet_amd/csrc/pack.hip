// Raw record bytes packed on the device into the slots of a resident pool: the writing twin of pool.hip.  The record's own bytes of B scenes
// are centre-cropped and bit-packed (stj_pack_bits) or stream-compacted (stj_pack_sparse_count -> stj_pool_admit -> stj_pack_sparse_commit)
// into slot slots[b] of the pool's arrays; rows of the raw keys are copied (stj_pool_put_raw).  A scene lands with every key or with none:
// ok[b] is settled by the admits before any commit runs.  Semantics: PoolLayout.replace_reference in strajnet_amd/data.py; kernels: pack.h.
#include "common.h"
#include "pack.h"

// The checks the packing entry points share.  *n = T Ho Wo C; *grid = B * ceil(n / UP_BLOCK), 0 = nothing to launch.
static int pack_shape(const char* who, int B, int N, int T, int H, int W, int C, int y0, int x0, int Ho, int Wo, pk_geom* g, long long* n,
                      unsigned* grid) {
  *grid = 0;
  *n = 0;
  if (B < 0 || N < 0 || T < 0 || H < 0 || W < 0 || C < 0 || y0 < 0 || x0 < 0 || Ho < 0 || Wo < 0) {
    stj_set_error("%s: negative size (B %d, N %d, source [%d][%d][%d][%d], crop %d %d %d %d)", who, B, N, T, H, W, C, y0, x0, Ho, Wo);
    return STJ_EINVAL;
  }
  if ((long long)y0 + Ho > H || (long long)x0 + Wo > W) {
    stj_set_error("%s: the crop %d %d %d %d leaves the source [%d][%d][%d][%d]", who, y0, x0, Ho, Wo, T, H, W, C);
    return STJ_EINVAL;
  }
  const __int128 nn = (__int128)T * Ho * Wo * C, S = (__int128)T * H * W * C;
  if (nn % 32 || nn >= ((__int128)1 << 32) || S >= ((__int128)1 << 56)) {
    stj_set_error("%s: a multiple of 32 and fewer than 2^32 elements per scene only (source [%d][%d][%d][%d], crop %d %d %d %d)", who, T, H, W,
                  C, y0, x0, Ho, Wo);
    return STJ_EUNSUPPORTED;
  }
  *n = (long long)nn;
  if (B == 0 || nn == 0) return STJ_OK;
  const long long gr = (long long)B * ((*n + UP_BLOCK - 1) / UP_BLOCK);
  if (gr > 0x7fffffffll) { stj_set_error("%s: %lld workgroups are beyond the launch limit (B %d, n %lld)", who, gr, B, *n); return STJ_EUNSUPPORTED; }
  g->S = (uint64_t)S;
  g->WC = (uint64_t)W * (uint64_t)C;
  g->off0 = ((uint64_t)y0 * (uint64_t)W + (uint64_t)x0) * (uint64_t)C;
  g->R = (uint32_t)((long long)Wo * C);                                 // <= n < 2^32
  g->Ho = (uint32_t)Ho;
  g->H = (uint32_t)H;
  *grid = (unsigned)gr;
  return STJ_OK;
}

extern "C" int stj_pack_bits(const uint8_t* src, const int* ok, const int* slots, int N, uint32_t* pool_words, int B, int T, int H, int W, int C,
                             int y0, int x0, int Ho, int Wo, hipStream_t stream) {
  pk_geom g;
  long long n;
  unsigned grid;
  const int rc = pack_shape("stj_pack_bits", B, N, T, H, W, C, y0, x0, Ho, Wo, &g, &n, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!src || !ok || !slots || !pool_words) { stj_set_error("stj_pack_bits: src / ok / slots / pool_words is NULL"); return STJ_EINVAL; }
  if (((uintptr_t)ok | (uintptr_t)slots | (uintptr_t)pool_words) & 3) {
    stj_set_error("stj_pack_bits: 4-byte aligned ok / slots / pool_words only");
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(pack_bits_kernel, dim3(grid), dim3(UP_NT), 0, stream, src, ok, slots, N, pool_words, g, (uint32_t)(n / 32), grid / (unsigned)B);
  return stj_check_launch("stj_pack_bits");
}

extern "C" int stj_pack_sparse_count(const float* src, uint32_t* offs_stage, int B, int T, int H, int W, int C, int y0, int x0, int Ho, int Wo,
                                     hipStream_t stream) {
  pk_geom g;
  long long n;
  unsigned grid;
  const int rc = pack_shape("stj_pack_sparse_count", B, 0, T, H, W, C, y0, x0, Ho, Wo, &g, &n, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!src || !offs_stage) { stj_set_error("stj_pack_sparse_count: src / offs_stage is NULL"); return STJ_EINVAL; }
  if (((uintptr_t)src | (uintptr_t)offs_stage) & 3) { stj_set_error("stj_pack_sparse_count: 4-byte aligned src / offs_stage only"); return STJ_EUNSUPPORTED; }
  hipLaunchKernelGGL(pack_count_kernel, dim3(grid), dim3(UP_NT), 0, stream, reinterpret_cast<const uint32_t*>(src), offs_stage, g, (uint32_t)n,
                     grid / (unsigned)B);
  return stj_check_launch("stj_pack_sparse_count");
}

extern "C" int stj_pool_admit(uint32_t* offs_stage, int nblk, const long long* val_base, const int* slots, int N, int* ok, int B, int first,
                              hipStream_t stream) {
  if (B < 0 || N < 0 || nblk < 0) { stj_set_error("stj_pool_admit: negative size (B %d, N %d, nblk %d)", B, N, nblk); return STJ_EINVAL; }
  if (B == 0) return STJ_OK;
  if (!slots || !ok || (offs_stage && !val_base)) { stj_set_error("stj_pool_admit: slots / ok / val_base is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)offs_stage | (uintptr_t)slots | (uintptr_t)ok) & 3) || ((uintptr_t)val_base & 7)) {
    stj_set_error("stj_pool_admit: 4-byte aligned offs_stage / slots / ok, 8-byte aligned val_base only");
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(pool_admit_kernel, dim3((unsigned)B), dim3(UP_NT), 0, stream, offs_stage, (uint32_t)nblk, val_base, slots, N, ok, first);
  return stj_check_launch("stj_pool_admit");
}

extern "C" int stj_pack_sparse_commit(const float* src, const uint32_t* offs_stage, const int* ok, const int* slots, int N, uint32_t* mask_pool,
                                      uint32_t* offs_pool, const long long* val_base, float* vals, long long n_vals, int B, int T, int H, int W,
                                      int C, int y0, int x0, int Ho, int Wo, hipStream_t stream) {
  if (n_vals < 0) { stj_set_error("stj_pack_sparse_commit: negative n_vals %lld", n_vals); return STJ_EINVAL; }
  pk_geom g;
  long long n;
  unsigned grid;
  const int rc = pack_shape("stj_pack_sparse_commit", B, N, T, H, W, C, y0, x0, Ho, Wo, &g, &n, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!src || !offs_stage || !ok || !slots || !mask_pool || !offs_pool || !val_base || (n_vals > 0 && !vals)) {
    stj_set_error("stj_pack_sparse_commit: a stream is NULL (n_vals %lld)", n_vals);
    return STJ_EINVAL;
  }
  if ((((uintptr_t)src | (uintptr_t)offs_stage | (uintptr_t)ok | (uintptr_t)slots | (uintptr_t)mask_pool | (uintptr_t)offs_pool | (uintptr_t)vals) & 3) ||
      ((uintptr_t)val_base & 7)) {
    stj_set_error("stj_pack_sparse_commit: 4-byte aligned streams / ok / slots, 8-byte aligned val_base only");
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(pack_commit_kernel, dim3(grid), dim3(UP_NT), 0, stream, reinterpret_cast<const uint32_t*>(src), offs_stage, ok, slots, N,
                     mask_pool, offs_pool, val_base, reinterpret_cast<uint32_t*>(vals), (uint64_t)n_vals, g, (uint32_t)n, grid / (unsigned)B);
  return stj_check_launch("stj_pack_sparse_commit");
}

extern "C" int stj_pool_put_raw(const void* src, int itemsize, const int* ok, const int* slots, int N, void* pool, int B, long long n,
                                hipStream_t stream) {
  if (itemsize != 1 && itemsize != 4 && itemsize != 8) { stj_set_error("stj_pool_put_raw: itemsize %d (1, 4 or 8 only)", itemsize); return STJ_EINVAL; }
  if (B < 0 || N < 0 || n < 0) { stj_set_error("stj_pool_put_raw: negative size (B %d, N %d, n %lld)", B, N, n); return STJ_EINVAL; }
  if (n >= (1ll << 32)) { stj_set_error("stj_pool_put_raw: fewer than 2^32 elements per scene only (n %lld)", n); return STJ_EUNSUPPORTED; }
  if (B == 0 || n == 0) return STJ_OK;
  if (!src || !ok || !slots || !pool) { stj_set_error("stj_pool_put_raw: src / ok / slots / pool is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)ok | (uintptr_t)slots) & 3) || (((uintptr_t)src | (uintptr_t)pool) & (uintptr_t)(itemsize - 1))) {
    stj_set_error("stj_pool_put_raw: 4-byte aligned ok / slots, src and pool aligned to the element size only");
    return STJ_EUNSUPPORTED;
  }
  const long long bytes = n * itemsize, nblk = (bytes + PK_RAW_BLOCK - 1) / PK_RAW_BLOCK, gr = (long long)B * nblk;
  if (gr > 0x7fffffffll) { stj_set_error("stj_pool_put_raw: %lld workgroups are beyond the launch limit (B %d, n %lld)", gr, B, n); return STJ_EUNSUPPORTED; }
  hipLaunchKernelGGL(put_raw_kernel, dim3((unsigned)gr), dim3(UP_NT), 0, stream, static_cast<const uint8_t*>(src), ok, slots, N,
                     static_cast<uint8_t*>(pool), (uint64_t)bytes, (uint32_t)nblk);
  return stj_check_launch("stj_pool_put_raw");
}
