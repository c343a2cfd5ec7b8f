// The per-byte rules of the device-side zlib streams (deflate.hip; the format: strajnet_amd/submission.py, compress_reference).  Plain
// C++ that compiles for the host as well, so that the token rules can be exercised without a GPU.
#pragma once
#include <stdint.h>

#define DF_SEG 8192                 // bytes of a plane per DEFLATE block = submission.DEFLATE_SEGMENT (4096 .. 16384 build)
#define DF_RUN 32                   // consecutive bytes per thread: its matchable flags are one 32-bit mask
#define DF_NT (DF_SEG / DF_RUN)     // threads per workgroup
#define DF_SLOT (DF_SEG + 16)       // a segment's slot in the workspace: 5 + DF_SEG (the stored form) rounded up to 16
#define DF_ADLER 65521u

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ __forceinline__
#else
#define DF_HD inline
#endif

DF_HD uint32_t df_rev32(uint32_t v) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  return (v >> 16) | (v << 16);
}

// fixed Huffman code of a literal byte, as it enters the LSB-first bit stream (the code's most significant bit first)
DF_HD uint32_t df_literal(uint32_t v, int* nbits) {
  if (v < 144) { *nbits = 8; return df_rev32(0x30u + v) >> 24; }
  *nbits = 9;
  return df_rev32(0x190u + v - 144u) >> 23;
}

// length code 257..285 of a match of length m (3..258): *eb its count of extra bits, *ex their value
DF_HD uint32_t df_len_code(int m, uint32_t* eb, uint32_t* ex) {
  const uint32_t l = (uint32_t)(m - 3);
  *eb = 0; *ex = 0;
  if (m == 258) return 285;
  if (l < 8) return 257 + l;
  *eb = (uint32_t)(31 - __builtin_clz(l)) - 2;            // lengths 11.. come in groups of 4 codes per count of extra bits
  *ex = l & ((1u << *eb) - 1);
  return 261 + 4 * *eb + ((l >> *eb) & 3);
}

// a match of length m (3..258) at distance d (1 or 2): length code 257..285 + its extra bits + the 5-bit distance code d - 1
DF_HD uint32_t df_match(int m, int d, int* nbits) {
  uint32_t eb, ex;
  const uint32_t sym = df_len_code(m, &eb, &ex);
  uint32_t hv; int hn;
  if (sym < 280) { hv = df_rev32(sym - 256) >> 25; hn = 7; }
  else { hv = df_rev32(0xC0u + sym - 280) >> 24; hn = 8; }
  *nbits = hn + (int)eb + 5;
  return hv | (ex << hn) | ((d == 2 ? 16u : 0u) << (hn + eb));
}

// matchable flags of the 32 bytes in w[0..7] (little-endian), `prev` the 4 bytes in front of them: bit e = (byte e == byte e - d)
DF_HD uint32_t df_match_mask(const uint32_t* w, uint32_t prev, int d) {
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t p = k ? w[k - 1] : prev;
    const uint32_t x = w[k] ^ (d == 1 ? (w[k] << 8) | (p >> 24) : (w[k] << 16) | (p >> 16));
#pragma unroll
    for (int e = 0; e < 4; ++e) mask |= (((x >> (8 * e)) & 0xffu) == 0 ? 1u : 0u) << (4 * k + e);
  }
  return mask;
}

// The role of byte `e` of a thread's run: -1 a literal, 0 none (the byte is covered by a match that starts earlier), else the length
// of the match that starts with it.
// nm: the run's NON-matchable flags (bytes past the segment's end count as non-matchable); base: the run's first index in the segment;
// P: index of the last non-matchable byte in front of the run (-1: none); N: index of the first one behind it (DF_SEG: none).
// The stretch of matchable bytes around the byte is [st, en): matches of 258 start every 258 bytes from st while at least 3 bytes are
// left; the last one takes all that is left if that is at least 3, else those bytes are literals.
DF_HD int df_role(uint32_t nm, int e, int base, int P, int N) {
  if ((nm >> e) & 1) return -1;
  const uint32_t lo = nm & ((1u << e) - 1u);
  const uint32_t hi = e == 31 ? 0u : nm >> (e + 1);
  const int st = lo ? base + 32 - __builtin_clz(lo) : P + 1;
  const int en = hi ? base + e + 1 + __builtin_ctz(hi) : N;
  const int o = base + e - st;
  const int rem = (en - st) - (o / 258) * 258;
  if (rem < 3) return -1;
  if (o % 258) return 0;
  return rem < 258 ? rem : 258;
}

// The token that byte `e` contributes in the fixed Huffman code (*nbits = 0: none).
DF_HD uint32_t df_token(uint32_t nm, int e, int base, int P, int N, uint32_t byte, int d, int* nbits) {
  const int r = df_role(nm, e, base, P, N);
  if (r < 0) return df_literal(byte, nbits);
  if (r == 0) { *nbits = 0; return 0; }
  return df_match(r, d, nbits);
}
