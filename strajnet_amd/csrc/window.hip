// The shuffle window over a resident pool: a batch drawn from the live slots on the device (stj_pool_draw) and consumed slots refilled from
// records that are already packed -- check_sparse and the capacity rule (stj_pool_admit_packed), then the value words (stj_pool_put_vals);
// the fixed-length rows (bits words, mask and offs rows, raw rows) go through stj_pool_put_raw of pack.hip.  Semantics:
// ShuffleWindow.reference / PoolLayout.replace_packed_reference in strajnet_amd/data.py; kernels and their rules: window.h.
#include "common.h"
#include "window.h"

extern "C" int stj_pool_draw(int* perm, int N, int tail, int n_live, const uint32_t* u, int* idx, int B, hipStream_t stream) {
  if (B < 0 || N < 1 || tail < 0 || tail >= N || n_live < B) {
    stj_set_error("stj_pool_draw: B %d of %d live slots, tail %d, N %d", B, n_live, tail, N);
    return STJ_EINVAL;
  }
  if (B == 0) return STJ_OK;
  if (!perm || !u || !idx) { stj_set_error("stj_pool_draw: perm / u / idx is NULL"); return STJ_EINVAL; }
  if (((uintptr_t)perm | (uintptr_t)u | (uintptr_t)idx) & 3) { stj_set_error("stj_pool_draw: 4-byte aligned perm / u / idx only"); return STJ_EUNSUPPORTED; }
  hipLaunchKernelGGL(pool_draw_kernel, dim3(1), dim3(WIN_NT), 0, stream, perm, N, tail, n_live, u, idx, B);
  return stj_check_launch("stj_pool_draw");
}

extern "C" int stj_pool_admit_packed(const uint32_t* offs_src, int nblk, long long n, const long long* src_base, const long long* val_base,
                                     const int* slots, int N, int* ok, int B, int first, hipStream_t stream) {
  if (B < 0 || N < 0 || nblk < 0 || n < 0) {
    stj_set_error("stj_pool_admit_packed: negative size (B %d, N %d, nblk %d, n %lld)", B, N, nblk, n);
    return STJ_EINVAL;
  }
  if (n % 32 || n >= (1ll << 32) || (long long)nblk != (n + WIN_BLOCK - 1) / WIN_BLOCK) {
    stj_set_error("stj_pool_admit_packed: a multiple of 32 and fewer than 2^32 elements per scene in ceil(n / %d) blocks only (n %lld, nblk %d)",
                  WIN_BLOCK, n, nblk);
    return STJ_EUNSUPPORTED;
  }
  if (B == 0) return STJ_OK;
  if (!offs_src || !src_base || !val_base || !slots || !ok) { stj_set_error("stj_pool_admit_packed: offs_src / src_base / val_base / slots / ok is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)offs_src | (uintptr_t)slots | (uintptr_t)ok) & 3) || (((uintptr_t)src_base | (uintptr_t)val_base) & 7)) {
    stj_set_error("stj_pool_admit_packed: 4-byte aligned offs_src / slots / ok, 8-byte aligned src_base / val_base only");
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(pool_admit_packed_kernel, dim3((unsigned)B), dim3(WIN_NT), 0, stream, offs_src, (uint32_t)nblk, (uint64_t)n, src_base, val_base,
                     slots, N, ok, first);
  return stj_check_launch("stj_pool_admit_packed");
}

extern "C" int stj_pool_put_vals(const uint32_t* vals_src, const long long* src_base, const int* ok, const int* slots, int N,
                                 const long long* val_base, uint32_t* vals, long long n_vals, int B, hipStream_t stream) {
  if (B < 0 || N < 0 || n_vals < 0) { stj_set_error("stj_pool_put_vals: negative size (B %d, N %d, n_vals %lld)", B, N, n_vals); return STJ_EINVAL; }
  if (B == 0 || n_vals == 0) return STJ_OK;
  if (!vals_src || !src_base || !ok || !slots || !val_base || !vals) { stj_set_error("stj_pool_put_vals: a stream / src_base / ok / slots / val_base is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)vals_src | (uintptr_t)vals | (uintptr_t)ok | (uintptr_t)slots) & 3) || (((uintptr_t)src_base | (uintptr_t)val_base) & 7)) {
    stj_set_error("stj_pool_put_vals: 4-byte aligned vals_src / vals / ok / slots, 8-byte aligned src_base / val_base only");
    return STJ_EUNSUPPORTED;
  }
  const long long pieces = (n_vals + WIN_PIECE - 1) / WIN_PIECE;
  if (pieces > 0x7fffffffll || B > 65535) {
    stj_set_error("stj_pool_put_vals: %lld x %d workgroups are beyond the launch limit (n_vals %lld)", pieces, B, n_vals);
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(pool_put_vals_kernel, dim3((unsigned)pieces, (unsigned)B), dim3(WIN_NT), 0, stream, vals_src, src_base, ok, slots, N, val_base,
                     vals, (uint64_t)n_vals);
  return stj_check_launch("stj_pool_put_vals");
}
