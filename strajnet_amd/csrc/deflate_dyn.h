// The per-symbol rules of level 2 of the device-side zlib streams: a dynamic Huffman code per segment (deflate.hip,
// deflate_encode_dyn_kernel; the format: strajnet_amd/submission.py, compress_reference(level=2) and huffman_code_lengths).  Plain C++
// over arrays that the caller owns, so that it compiles for the host as well: the kernel runs the per-symbol functions one symbol per
// thread and the serial ones on one lane; dfd_lengths and dfd_block_header run all of it in order, on the host.
#pragma once
#include "deflate.h"

#define DFD_NLIT 286                // literal/length symbols
#define DFD_NCL 19                  // code-length symbols
#define DFD_NSEQ 288                // code lengths in a header at most: 286 + 2 distance codes
#define DFD_LIT_LIMIT 15
#define DFD_CL_LIMIT 7

// A used symbol's sort key: ascending by (count, symbol).  0: unused.  Counts stay below 2^14 (a segment's tokens + EOB).
DF_HD uint32_t dfd_key(uint32_t count, int s) { return count ? count << 9 | (uint32_t)s : 0u; }

// The place of used symbol s in the sorted order: the number of smaller keys.
DF_HD int dfd_rank(const uint32_t* cnt, int nsym, int s) {
  const uint32_t k = dfd_key(cnt[s], s);
  int r = 0;
  for (int t = 0; t < nsym; ++t) {
    const uint32_t kt = dfd_key(cnt[t], t);
    r += (kt != 0 && kt < k) ? 1 : 0;
  }
  return r;
}

// The two-queue Huffman merge over srt[0 .. n), n >= 2 keys ascending: internal node k = 0 .. n - 2 (creation order) gets weight iw[k];
// lpar[i] / ipar[k]: the internal node that took leaf i / internal node k.  On equal weight a leaf goes before an internal node.
DF_HD void dfd_merge(const uint32_t* srt, int n, uint32_t* iw, uint16_t* lpar, uint16_t* ipar) {
  int li = 0, ii = 0;
  for (int k = 0; k < n - 1; ++k) {
    uint32_t w = 0;
    for (int j = 0; j < 2; ++j) {
      bool leaf = li < n;
      if (leaf && ii < k) leaf = (srt[li] >> 9) <= iw[ii];
      if (leaf) { w += srt[li] >> 9; lpar[li++] = (uint16_t)k; }
      else { w += iw[ii]; ipar[ii++] = (uint16_t)k; }
    }
    iw[k] = w;
  }
}

// Depth of every internal node, the root (n - 2) at 0.
DF_HD void dfd_depths(const uint16_t* ipar, int n, uint16_t* idep) {
  idep[n - 2] = 0;
  for (int k = n - 3; k >= 0; --k) idep[k] = (uint16_t)(idep[ipar[k]] + 1);
}

// Leaf i's depth, counted at `limit` if it lies deeper.
DF_HD int dfd_leaf_len(const uint16_t* lpar, const uint16_t* idep, int i, int limit) {
  const int l = idep[lpar[i]] + 1;
  return l < limit ? l : limit;
}

// The Kraft repair of the histogram cnt[1 .. limit] of lengths: each round takes one code off the limit and splits the deepest shorter
// one, which lowers sum cnt[l] 2^(limit - l) by exactly 1.
DF_HD void dfd_kraft(int* cnt, int limit) {
  int over = -(1 << limit);
  for (int l = 1; l <= limit; ++l) over += cnt[l] << (limit - l);
  for (; over > 0; --over) {
    int l = limit - 1;
    while (l > 0 && cnt[l] == 0) --l;
    if (l == 0) return;                       // (cannot happen: an over-full histogram has a code shorter than the limit)
    cnt[limit] -= 1;
    cnt[l] -= 1;
    cnt[l + 1] += 2;
  }
}

// The length of the symbol at place r of the n sorted ones: the histogram's lengths go, increasing, to the symbols in DESCENDING order.
DF_HD int dfd_len_of_rank(const int* cnt, int limit, int n, int r) {
  int q = n - 1 - r;
  for (int l = 1; l < limit; ++l) {
    if (q < cnt[l]) return l;
    q -= cnt[l];
  }
  return limit;
}

// RFC 1951 3.2.2: the first code of every length.
DF_HD void dfd_next_codes(const int* cnt, int limit, int* nx) {
  int code = 0;
  nx[0] = 0;
  for (int b = 1; b <= limit; ++b) {
    code = (code + (b > 1 ? cnt[b - 1] : 0)) << 1;
    nx[b] = code;
  }
}

// Symbol s's canonical code as it enters the LSB-first bit stream (its most significant bit first).  len[s] > 0.
DF_HD uint32_t dfd_code(const uint8_t* len, const int* nx, int s) {
  const int l = len[s];
  int c = nx[l];
  for (int t = 0; t < s; ++t) c += len[t] == l ? 1 : 0;
  return df_rev32((uint32_t)c) >> (32 - l);
}

// The whole construction in order (the host's path): len[0 .. nsym) and code[0 .. nsym) from cnt[0 .. nsym).  srt, iw, lpar, ipar, idep:
// nsym entries each; lc, nx: limit + 1.  Returns the number of used symbols; a single used symbol gets length 1.
DF_HD int dfd_lengths(const uint32_t* cnt, int nsym, int limit, uint8_t* len, uint16_t* code, uint32_t* srt, uint32_t* iw, uint16_t* lpar,
                      uint16_t* ipar, uint16_t* idep, int* lc, int* nx) {
  int n = 0;
  for (int s = 0; s < nsym; ++s) {
    len[s] = 0; code[s] = 0;
    if (cnt[s]) { srt[dfd_rank(cnt, nsym, s)] = dfd_key(cnt[s], s); ++n; }
  }
  for (int l = 0; l <= limit; ++l) lc[l] = 0;
  if (n >= 2) {
    dfd_merge(srt, n, iw, lpar, ipar);
    dfd_depths(ipar, n, idep);
    for (int i = 0; i < n; ++i) lc[dfd_leaf_len(lpar, idep, i, limit)] += 1;
    dfd_kraft(lc, limit);
  } else if (n == 1) lc[1] = 1;
  dfd_next_codes(lc, limit, nx);
  for (int i = 0; i < n; ++i) len[srt[i] & 511u] = (uint8_t)dfd_len_of_rank(lc, limit, n, i);
  for (int s = 0; s < nsym; ++s)
    if (len[s]) code[s] = (uint16_t)dfd_code(len, nx, s);
  return n;
}

// Number of literal/length codes the header carries: up to the highest used symbol, 257 at least.
DF_HD int dfd_num_lit(const uint8_t* ll) {
  int s = DFD_NLIT - 1;
  while (s > 256 && ll[s] == 0) --s;
  return s + 1;
}

DF_HD int dfd_cl_extra_bits(int s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }

// The order in which the header lists the code-length code: 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15.
DF_HD int dfd_cl_order(int j) {
  if (j < 3) return 16 + j;
  if (j == 3) return 0;
  const int t = j - 4;
  return (t & 1) ? 7 - (t >> 1) : 8 + (t >> 1);
}

// The run-length code of the code lengths: ll[0 .. nl) followed by the d distance lengths (code d - 1: 1, any other: 0), in maximal runs
// of equal values.  rsym / rext [DFD_NSEQ]: the code-length symbols and the values of their extra bits; cc[DFD_NCL]: their counts.
// Returns their number.
DF_HD int dfd_rle(const uint8_t* ll, int nl, int d, uint8_t* rsym, uint8_t* rext, uint32_t* cc) {
  for (int s = 0; s < DFD_NCL; ++s) cc[s] = 0;
  const int total = nl + d;
  int nr = 0, i = 0;
  while (i < total) {
    const int v = i < nl ? ll[i] : (i - nl == d - 1 ? 1 : 0);
    int r = 1;
    while (i + r < total && (i + r < nl ? ll[i + r] : (i + r - nl == d - 1 ? 1 : 0)) == v) ++r;
    i += r;
    if (v == 0) {
      while (r >= 11) { const int t = r < 138 ? r : 138; rsym[nr] = 18; rext[nr++] = (uint8_t)(t - 11); cc[18] += 1; r -= t; }
      if (r >= 3) { rsym[nr] = 17; rext[nr++] = (uint8_t)(r - 3); cc[17] += 1; r = 0; }
    } else {
      rsym[nr] = (uint8_t)v; rext[nr++] = 0; cc[v] += 1; r -= 1;
      while (r >= 3) { const int t = r < 6 ? r : 6; rsym[nr] = 16; rext[nr++] = (uint8_t)(t - 3); cc[16] += 1; r -= t; }
    }
    for (; r > 0; --r) { rsym[nr] = (uint8_t)v; rext[nr++] = 0; cc[v] += 1; }
  }
  return nr;
}

// HCLEN + 4: up to the last non-zero length in dfd_cl_order, 4 at least.
DF_HD int dfd_num_cl(const uint8_t* cl) {
  int j = DFD_NCL - 1;
  while (j > 3 && cl[dfd_cl_order(j)] == 0) --j;
  return j + 1;
}

// Bits of the header, BFINAL up to the last code length.
DF_HD int dfd_header_bits(const uint32_t* cc, const uint8_t* cl) {
  int bits = 17 + 3 * dfd_num_cl(cl);
  for (int s = 0; s < DFD_NCL; ++s) bits += (int)cc[s] * (cl[s] + dfd_cl_extra_bits(s));
  return bits;
}

// The header's tokens in stream order through sink.put(value, bits): BFINAL, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code, the
// run-length coded lengths.
template <class Sink>
DF_HD void dfd_put_header(Sink& sink, int final_, int nl, int d, const uint8_t* cl, const uint16_t* ccode, const uint8_t* rsym,
                          const uint8_t* rext, int nr) {
  const int ncl = dfd_num_cl(cl);
  sink.put((uint32_t)final_ | 4u | (uint32_t)(nl - 257) << 3 | (uint32_t)(d - 1) << 8 | (uint32_t)(ncl - 4) << 13, 17);
  for (int j = 0; j < ncl; ++j) sink.put(cl[dfd_cl_order(j)], 3);
  for (int i = 0; i < nr; ++i) {
    const int s = rsym[i];
    sink.put((uint32_t)ccode[s] | (uint32_t)rext[i] << cl[s], cl[s] + dfd_cl_extra_bits(s));
  }
}
