// Packed record features expanded on the device: the input-side twin of quantize.hip / deflate.hip.  A bool plane crosses PCIe as one
// bit per element, a sparse float32 plane as one bit per element plus its non-zero words; both become exactly the float32 tensors that
// stj_decode_raw makes of the record's own bytes.  The format is stated by unpack_reference in strajnet_amd/data.py; the kernels: unpack.h.
#include "common.h"
#include "unpack.h"

static int up_sizes(const char* who, long long n_total) {
  if (n_total < 0 || n_total % 32 || n_total >= (1ll << 32)) {
    stj_set_error("%s: a multiple of 32 and fewer than 2^32 elements only (%lld)", who, n_total);
    return STJ_EUNSUPPORTED;
  }
  return STJ_OK;
}

extern "C" int stj_unpack_bits(const uint32_t* bits, float* dst, long long n_total, hipStream_t stream) {
  const int rc = up_sizes("stj_unpack_bits", n_total);
  if (rc != STJ_OK) return rc;
  if (n_total == 0) return STJ_OK;
  if (((uintptr_t)bits & 3) || ((uintptr_t)dst & 15)) {
    stj_set_error("stj_unpack_bits: 4-byte aligned bits, 16-byte aligned dst only");
    return STJ_EUNSUPPORTED;
  }
  const uint32_t n_words = (uint32_t)(n_total / 32);
  const unsigned grid = (unsigned)((n_total + UP_BLOCK - 1) / UP_BLOCK);
  hipLaunchKernelGGL(unpack_bits_kernel, dim3(grid), dim3(UP_NT), 0, stream, bits, reinterpret_cast<uint4*>(dst), n_words);
  return stj_check_launch("stj_unpack_bits");
}

extern "C" int stj_unpack_sparse(const uint32_t* mask, const uint32_t* offs, const uint32_t* val_base, const float* vals, long long n_vals,
                                 float* dst, int B, long long n, hipStream_t stream) {
  if (B < 0 || n < 0 || n_vals < 0) { stj_set_error("stj_unpack_sparse: negative size"); return STJ_EINVAL; }
  if (n % 32 || n >= (1ll << 32) || n_vals >= (1ll << 32)) {
    stj_set_error("stj_unpack_sparse: n a multiple of 32, fewer than 2^32 elements only (B %d, n %lld, n_vals %lld)", B, n, n_vals);
    return STJ_EUNSUPPORTED;
  }
  const int rc = up_sizes("stj_unpack_sparse", (long long)B * n);
  if (rc != STJ_OK) return rc;
  if (B == 0 || n == 0) return STJ_OK;
  if ((((uintptr_t)mask | (uintptr_t)offs | (uintptr_t)val_base | (uintptr_t)vals) & 3) || ((uintptr_t)dst & 15)) {
    stj_set_error("stj_unpack_sparse: 4-byte aligned streams, 16-byte aligned dst only");
    return STJ_EUNSUPPORTED;
  }
  if (n_vals > 0 && !vals) { stj_set_error("stj_unpack_sparse: vals is NULL with n_vals %lld", n_vals); return STJ_EINVAL; }
  const uint32_t nblk = (uint32_t)((n + UP_BLOCK - 1) / UP_BLOCK);
  hipLaunchKernelGGL(unpack_sparse_kernel, dim3((unsigned)B * nblk), dim3(UP_NT), 0, stream, mask, offs, val_base,
                     reinterpret_cast<const uint32_t*>(vals), (uint32_t)n_vals, reinterpret_cast<uint4*>(dst), (uint32_t)(n / 32), nblk);
  return stj_check_launch("stj_unpack_sparse");
}
