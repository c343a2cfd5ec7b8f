// Batches gathered from a pool of packed scenes that stays in HBM: the resident twin of unpack.hip.  Scene b of the output is pool scene
// clamp(idx[b], 0, N - 1), idx an int32 array on the device; the result is what stj_unpack_bits / stj_unpack_sparse / stj_decode_raw give
// for that scene.  The format is stated by PoolLayout.reference_gather in strajnet_amd/data.py; the kernels: pool.h.
#include "common.h"
#include "pool.h"

// the checks the three entry points share; *grid = B * ceil(n / UP_BLOCK), 0 = nothing to launch
static int pool_shape(const char* who, const void* idx, int N, const void* dst, int B, long long n, bool words, unsigned* grid) {
  *grid = 0;
  if (B < 0 || n < 0) { stj_set_error("%s: negative size (B %d, n %lld)", who, B, n); return STJ_EINVAL; }
  if ((words && n % 32) || n >= (1ll << 32)) {
    stj_set_error("%s: %sfewer than 2^32 elements per scene only (n %lld)", who, words ? "a multiple of 32 and " : "", n);
    return STJ_EUNSUPPORTED;
  }
  if (B == 0) return STJ_OK;
  if (N < 1) { stj_set_error("%s: an empty pool (N %d) with B %d", who, N, B); return STJ_EUNSUPPORTED; }
  if (n == 0) return STJ_OK;
  if (!idx || !dst) { stj_set_error("%s: idx / dst is NULL", who); return STJ_EINVAL; }
  if (((uintptr_t)idx & 3) || ((uintptr_t)dst & 15)) {
    stj_set_error("%s: 4-byte aligned idx, 16-byte aligned dst only", who);
    return STJ_EUNSUPPORTED;
  }
  const long long g = (long long)B * ((n + UP_BLOCK - 1) / UP_BLOCK);
  if (g > 0x7fffffffll) { stj_set_error("%s: %lld workgroups are beyond the launch limit (B %d, n %lld)", who, g, B, n); return STJ_EUNSUPPORTED; }
  *grid = (unsigned)g;
  return STJ_OK;
}

extern "C" int stj_gather_bits(const uint32_t* pool, const int* idx, int N, float* dst, int B, long long n, hipStream_t stream) {
  unsigned grid;
  const int rc = pool_shape("stj_gather_bits", idx, N, dst, B, n, true, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!pool || ((uintptr_t)pool & 3)) { stj_set_error("stj_gather_bits: a 4-byte aligned pool only"); return pool ? STJ_EUNSUPPORTED : STJ_EINVAL; }
  hipLaunchKernelGGL(gather_bits_kernel, dim3(grid), dim3(UP_NT), 0, stream, pool, idx, N, reinterpret_cast<uint4*>(dst), (uint32_t)(n / 32),
                     grid / (unsigned)B);
  return stj_check_launch("stj_gather_bits");
}

extern "C" int stj_gather_sparse(const uint32_t* mask, const uint32_t* offs, const long long* val_base, const float* vals, long long n_vals,
                                 const int* idx, int N, float* dst, int B, long long n, hipStream_t stream) {
  if (n_vals < 0) { stj_set_error("stj_gather_sparse: negative n_vals %lld", n_vals); return STJ_EINVAL; }
  unsigned grid;
  const int rc = pool_shape("stj_gather_sparse", idx, N, dst, B, n, true, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!mask || !offs || !val_base || (n_vals > 0 && !vals)) { stj_set_error("stj_gather_sparse: a stream is NULL (n_vals %lld)", n_vals); return STJ_EINVAL; }
  if ((((uintptr_t)mask | (uintptr_t)offs | (uintptr_t)vals) & 3) || ((uintptr_t)val_base & 7)) {
    stj_set_error("stj_gather_sparse: 4-byte aligned mask / offs / vals, 8-byte aligned val_base only");
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(gather_sparse_kernel, dim3(grid), dim3(UP_NT), 0, stream, mask, offs, val_base, reinterpret_cast<const uint32_t*>(vals),
                     (uint64_t)n_vals, idx, N, reinterpret_cast<uint4*>(dst), (uint32_t)(n / 32), grid / (unsigned)B);
  return stj_check_launch("stj_gather_sparse");
}

extern "C" int stj_gather_raw(const void* pool, int kind, const int* idx, int N, float* dst, int B, long long n, float scale, hipStream_t stream) {
  if (kind < 0 || kind > 3) { stj_set_error("stj_gather_raw: bad kind %d", kind); return STJ_EINVAL; }
  unsigned grid;
  const int rc = pool_shape("stj_gather_raw", idx, N, dst, B, n, false, &grid);
  if (rc != STJ_OK || !grid) return rc;
  if (!pool) { stj_set_error("stj_gather_raw: pool is NULL"); return STJ_EINVAL; }
  if ((uintptr_t)pool & (kind == 3 ? 7 : kind == 2 ? 3 : 0)) { stj_set_error("stj_gather_raw: a pool aligned to its element size only (kind %d)", kind); return STJ_EUNSUPPORTED; }
  const uint32_t nblk = grid / (unsigned)B;
  if (kind == 0) hipLaunchKernelGGL(gather_raw_kernel<0>, dim3(grid), dim3(UP_NT), 0, stream, pool, idx, N, dst, (uint32_t)n, nblk, scale);
  else if (kind == 1) hipLaunchKernelGGL(gather_raw_kernel<1>, dim3(grid), dim3(UP_NT), 0, stream, pool, idx, N, dst, (uint32_t)n, nblk, scale);
  else if (kind == 2) hipLaunchKernelGGL(gather_raw_kernel<2>, dim3(grid), dim3(UP_NT), 0, stream, pool, idx, N, dst, (uint32_t)n, nblk, scale);
  else hipLaunchKernelGGL(gather_raw_kernel<3>, dim3(grid), dim3(UP_NT), 0, stream, pool, idx, N, dst, (uint32_t)n, nblk, scale);
  return stj_check_launch("stj_gather_raw");
}
