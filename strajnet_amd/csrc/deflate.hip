// The challenge-format planes (quantize.hip's Q) as zlib streams, on the device: one stream per (scene, waypoint, field) plane, a
// run-length DEFLATE with the fixed Huffman code (the format: strajnet_amd/submission.py, compress_reference; the per-byte rules:
// deflate.h).  The reader of the challenge format only calls zlib.decompress, so any valid stream conforms; these are larger than zlib's
// own and cost no host work.
//
//   deflate_encode_kernel   one workgroup per (plane, segment of DF_SEG bytes): the segment's DEFLATE block(s) into its slot of the
//                           workspace, its byte count and its Adler-32 partials into the segment table
//   deflate_encode_dyn_kernel  level 2: the same workgroup, slot and table entry; the segment's block in the shortest of its stored,
//                           fixed and dynamic-Huffman forms (the code is built per segment; the per-symbol rules: deflate_dyn.h)
//   deflate_offsets_kernel  one workgroup: per plane the scan of its segments' byte counts and its Adler-32, the scan of the planes'
//                           totals -> `offsets`, and every stream's header and trailer
//   deflate_offsets_framed_kernel  the same for stj_compress_waypoints_framed: + room for, and the bytes of, the protobuf header in front
//                           of every stream and waypoint (frame.h), stream starts, lengths and scene starts -> the framed table
//   deflate_pack_kernel     one workgroup per (plane, segment): the slot's bytes to their place in the packed buffer
//
// Workspace: [ segment table, 4 uint32 per segment: bytes, byte sum, weighted byte sum, offset in its stream | slots of DF_SLOT bytes ];
// segments in the order of Q's memory (scene; 8 obs, 8 occ planes of nso segments each, 8 flow planes of nsf).  Streams in the order
// scene, waypoint, (obs, occ, flow).
#include "common.h"
#include "deflate.h"
#include "deflate_dyn.h"
#include "frame.h"

static_assert(DF_SEG >= 4096 && DF_SEG <= 16384 && (DF_SEG & (DF_SEG - 1)) == 0, "DF_SEG: a power of two, 64 KB of static LDS at most");
constexpr int DF_NW = DF_NT / 64;          // waves per workgroup

// A workgroup's segment: where it lies in Q, its length and match distance, the plane's place in the stream order.
struct DfSeg { long long src; int len, d, seg, final_, stream; };
__device__ __forceinline__ DfSeg df_locate(long long g, int HW, int nso, int nsf) {
  const int sps = 16 * nso + 8 * nsf;
  const long long b = g / sps;
  const int j = (int)(g % sps);
  int mp, seg, n;
  DfSeg r;
  if (j < 16 * nso) { mp = j / nso; seg = j % nso; n = HW; r.d = 1; r.src = (long long)mp * HW; r.stream = (mp & 7) * 3 + (mp >> 3); }
  else { const int jj = j - 16 * nso; mp = jj / nsf; seg = jj % nsf; n = 2 * HW; r.d = 2; r.src = 16ll * HW + (long long)mp * 2 * HW; r.stream = mp * 3 + 2; }
  r.src += b * 32 * HW + (long long)seg * DF_SEG;
  r.len = min(DF_SEG, n - seg * DF_SEG);
  r.seg = seg;
  r.final_ = seg * DF_SEG + r.len == n;
  r.stream += (int)b * 24;
  return r;
}

__global__ __launch_bounds__(DF_NT) void deflate_encode_kernel(const uint8_t* __restrict__ Q, uint8_t* __restrict__ slots, uint32_t* __restrict__ table,
                                                               int HW, int nso, int nsf) {
  __shared__ __attribute__((aligned(16))) uint32_t inw[4 + DF_SEG / 4];         // 16 bytes of history, then the segment
  __shared__ __attribute__((aligned(16))) uint32_t bb[DF_SLOT / 4 + 4];         // the segment's output, built by OR into zeroed words
  __shared__ int sc[5][DF_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const DfSeg s = df_locate(blockIdx.x, HW, nso, nsf);
  const int len = s.len, d = s.d;
  const uint4* src4 = reinterpret_cast<const uint4*>(Q + s.src);
  uint4* in4 = reinterpret_cast<uint4*>(inw);
  for (int v = tid; v < len / 16; v += DF_NT) in4[1 + v] = src4[v];
  if (tid == 0) in4[0] = s.seg ? src4[-1] : make_uint4(0, 0, 0, 0);               // history: the same plane's previous segment only
  __syncthreads();

  // this thread's run of 32 bytes (len is a multiple of 16: a run is whole, half, or empty)
  const int base = tid * DF_RUN, cnt = max(0, min(DF_RUN, len - base));
  uint32_t w[8];
  {
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 a = cnt > 0 ? in4[1 + 2 * tid] : z, b = cnt > 16 ? in4[2 + 2 * tid] : z;
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
  uint32_t mask = cnt > 0 ? df_match_mask(w, inw[3 + 8 * tid], d) : 0u;
  mask &= cnt == DF_RUN ? ~0u : (1u << cnt) - 1u;
  if (s.seg == 0 && tid == 0) mask &= ~((1u << d) - 1u);                           // no history in front of the plane
  const uint32_t nm = ~mask;

  // P: the last non-matchable byte in front of this run; N: the first one behind it (workgroup exclusive max-scan / reverse min-scan)
  int P, N;
  {
    int a = nm ? base + 31 - __builtin_clz(nm) : -1, b = nm ? base + __builtin_ctz(nm) : DF_SEG;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ya = __shfl_up(a, o), yb = __shfl_down(b, o);
      if (lane >= o) a = max(a, ya);
      if (lane + o < 64) b = min(b, yb);
    }
    if (lane == 63) sc[0][wv] = a;
    if (lane == 0) sc[1][wv] = b;
    P = __shfl_up(a, 1); N = __shfl_down(b, 1);
    if (lane == 0) P = -1;
    if (lane == 63) N = DF_SEG;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DF_NW; ++k) {
      if (k < wv) P = max(P, sc[0][k]);
      if (k > wv) N = min(N, sc[1][k]);
    }
  }

  // bits of this run's tokens; the Adler-32 partials: sum of bytes, and sum of (len - i) * byte (what the bytes add to the running
  // sum-of-sums by the segment's end), each reduced mod 65521 before 32 bits can overflow (a run: 32 * 255 * 16384 at most)
  int tb = 0;
  uint32_t s1 = 0, s2 = 0;
#pragma unroll
  for (int e = 0; e < DF_RUN; ++e) {
    if (e >= cnt) continue;
    const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
    int nb;
    df_token(nm, e, base, P, N, byte, d, &nb);
    tb += nb;
    s1 += byte;
    s2 += (uint32_t)(len - base - e) * byte;
  }
  s2 %= DF_ADLER;
  int off = tb, total;
  {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(off, o);
      if (lane >= o) off += y;
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (lane == 63) { sc[2][wv] = off; sc[3][wv] = (int)(s1 % DF_ADLER); sc[4][wv] = (int)(s2 % DF_ADLER); }
    __syncthreads();
    off -= tb;
    total = 0;
    uint32_t t1 = 0, t2 = 0;
#pragma unroll
    for (int k = 0; k < DF_NW; ++k) {
      if (k < wv) off += sc[2][k];
      total += sc[2][k];
      t1 += (uint32_t)sc[3][k];
      t2 += (uint32_t)sc[4][k];
    }
    s1 = t1 % DF_ADLER;
    s2 = t2 % DF_ADLER;
  }

  // fixed block: 3 header bits, the tokens, EOB (7 zero bits); a non-final one + the empty stored block 000, pad, 00 00 FF FF
  const int fixed_bits = 3 + total + 7 + (s.final_ ? 0 : 3);
  const int fixed_bytes = (fixed_bits + 7) / 8 + (s.final_ ? 0 : 4);
  const bool stored = fixed_bytes > 5 + len;
  const int out_bytes = stored ? 5 + len : fixed_bytes;
  const int out_vecs = (out_bytes + 15) / 16;                 // <= DF_SLOT / 16
  if (!stored) {
    for (int i = tid; i < out_vecs * 4 + 2; i += DF_NT) bb[i] = 0;
    __syncthreads();
    if (tid == 0) {
      atomicOr(&bb[0], (uint32_t)s.final_ | 2u);
      if (!s.final_) {                                        // FF FF: the last two bytes
        const int p = 8 * (fixed_bytes - 2);
        atomicOr(&bb[p >> 5], 0xffffu << (p & 31));
        if ((p & 31) > 16) atomicOr(&bb[(p >> 5) + 1], 0xffffu >> (32 - (p & 31)));
      }
    }
    int wi = (3 + off) >> 5, fill = (3 + off) & 31;
    unsigned long long acc = 0;
#pragma unroll
    for (int e = 0; e < DF_RUN; ++e) {
      if (e >= cnt) continue;
      const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
      int nb;
      const uint32_t v = df_token(nm, e, base, P, N, byte, d, &nb);
      acc |= (unsigned long long)v << fill;
      fill += nb;
      if (fill >= 32) { atomicOr(&bb[wi], (uint32_t)acc); acc >>= 32; fill -= 32; ++wi; }
    }
    if (fill > 0 && acc) atomicOr(&bb[wi], (uint32_t)acc);
  } else {
    // stored block: BFINAL (BTYPE 00, padding), LEN, ~LEN, the raw bytes -- the segment shifted by 5 bytes
    const uint32_t* x = inw + 4;
    const uint32_t h4 = ((uint32_t)~len >> 8) & 0xffu;
    for (int m = tid; m < out_vecs * 4; m += DF_NT) {
      uint32_t v;
      if (m == 0) v = (uint32_t)s.final_ | ((uint32_t)len & 0xffffu) << 8 | ((uint32_t)~len & 0xffu) << 24;
      else {
        const uint32_t lo = m == 1 ? h4 : m - 2 < len / 4 ? x[m - 2] >> 24 : 0u, hi = m - 1 < len / 4 ? x[m - 1] : 0u;
        v = lo | hi << 8;
      }
      bb[m] = v;
    }
  }
  __syncthreads();
  uint4* slot4 = reinterpret_cast<uint4*>(slots + (long long)blockIdx.x * DF_SLOT);
  const uint4* bb4 = reinterpret_cast<const uint4*>(bb);
  for (int v = tid; v < out_vecs; v += DF_NT) slot4[v] = bb4[v];
  if (tid == 0) {
    uint32_t* t = table + 4ll * blockIdx.x;
    t[0] = (uint32_t)out_bytes; t[1] = s1; t[2] = s2;
  }
}

// ---------------------------------------------------------------------------------------------------- level 2
// The arrays of one code construction, in LDS.
struct DfdWork { uint32_t* srt; uint32_t* iw; uint16_t* lpar; uint16_t* ipar; uint16_t* idep; int* lc; int* nx; int* nused; };

// huffman_code_lengths + the canonical codes over cnt[0 .. NSYM) by the whole workgroup: the rank sort, the leaves' depths, the lengths
// and the codes one symbol per thread; the merge, the internal depths and the Kraft repair on one lane.  cnt is complete and visible on
// entry; len and code are on return.
template <int NSYM, int LIMIT>
__device__ __forceinline__ void dfd_build(const uint32_t* cnt, uint8_t* len, uint16_t* code, const DfdWork& k, int tid) {
  if (tid <= LIMIT) k.lc[tid] = 0;
  if (tid == 0) *k.nused = 0;
  __syncthreads();
  for (int s = tid; s < NSYM; s += DF_NT) {
    len[s] = 0;
    if (cnt[s]) { k.srt[dfd_rank(cnt, NSYM, s)] = dfd_key(cnt[s], s); atomicAdd(k.nused, 1); }
  }
  __syncthreads();
  const int n = *k.nused;
  if (tid == 0 && n >= 2) { dfd_merge(k.srt, n, k.iw, k.lpar, k.ipar); dfd_depths(k.ipar, n, k.idep); }
  __syncthreads();
  if (n >= 2) {
    for (int i = tid; i < n; i += DF_NT) atomicAdd(&k.lc[dfd_leaf_len(k.lpar, k.idep, i, LIMIT)], 1);
  } else if (n == 1 && tid == 0) k.lc[1] = 1;
  __syncthreads();
  if (tid == 0) { dfd_kraft(k.lc, LIMIT); dfd_next_codes(k.lc, LIMIT, k.nx); }
  __syncthreads();
  for (int i = tid; i < n; i += DF_NT) len[k.srt[i] & 511u] = (uint8_t)dfd_len_of_rank(k.lc, LIMIT, n, i);
  __syncthreads();
  for (int s = tid; s < NSYM; s += DF_NT) code[s] = len[s] ? (uint16_t)dfd_code(len, k.nx, s) : (uint16_t)0;
  __syncthreads();
}

// Bits laid end to end from bit `at` of bb: accumulated in a register, a whole word at a time into the zeroed buffer by OR.
struct DfdSink {
  uint32_t* bb; int wi, fill; unsigned long long acc;
  __device__ __forceinline__ DfdSink(uint32_t* b, int at) : bb(b), wi(at >> 5), fill(at & 31), acc(0) {}
  __device__ __forceinline__ void put(uint32_t v, int nb) {                      // nb <= 25
    acc |= (unsigned long long)v << fill;
    fill += nb;
    if (fill >= 32) { atomicOr(&bb[wi], (uint32_t)acc); acc >>= 32; fill -= 32; ++wi; }
  }
  __device__ __forceinline__ void flush() { if (fill > 0 && acc) atomicOr(&bb[wi], (uint32_t)acc); }
};

__global__ __launch_bounds__(DF_NT) void deflate_encode_dyn_kernel(const uint8_t* __restrict__ Q, uint8_t* __restrict__ slots, uint32_t* __restrict__ table,
                                                                   int HW, int nso, int nsf) {
  __shared__ __attribute__((aligned(16))) uint32_t inw[4 + DF_SEG / 4];         // 16 bytes of history, then the segment
  __shared__ __attribute__((aligned(16))) uint32_t bb[DF_SLOT / 4 + 4];         // the segment's output, built by OR into zeroed words
  __shared__ int sc[6][DF_NW];
  __shared__ uint32_t hist[DFD_NSEQ], srt[DFD_NSEQ], iw[DFD_NSEQ], cc[DFD_NCL]; // counts per literal/length and per code-length symbol
  __shared__ uint16_t lpar[DFD_NSEQ], ipar[DFD_NSEQ], idep[DFD_NSEQ], lcode[DFD_NSEQ], ccode[32];
  __shared__ uint8_t ll[DFD_NSEQ], cl[32], rsym[DFD_NSEQ], rext[DFD_NSEQ];
  __shared__ int lc[16], nx[16], meta[3];                                        // meta: used symbols, literal/length codes, RLE symbols
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const DfSeg s = df_locate(blockIdx.x, HW, nso, nsf);
  const int len = s.len, d = s.d;
  const uint4* src4 = reinterpret_cast<const uint4*>(Q + s.src);
  uint4* in4 = reinterpret_cast<uint4*>(inw);
  for (int v = tid; v < len / 16; v += DF_NT) in4[1 + v] = src4[v];
  if (tid == 0) in4[0] = s.seg ? src4[-1] : make_uint4(0, 0, 0, 0);               // history: the same plane's previous segment only
  for (int i = tid; i < DFD_NSEQ; i += DF_NT) hist[i] = i == 256 ? 1u : 0u;       // EOB once
  __syncthreads();

  // this thread's run of 32 bytes, its matchable flags, P and N: as in deflate_encode_kernel
  const int base = tid * DF_RUN, cnt = max(0, min(DF_RUN, len - base));
  uint32_t w[8];
  {
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 a = cnt > 0 ? in4[1 + 2 * tid] : z, b = cnt > 16 ? in4[2 + 2 * tid] : z;
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
  uint32_t mask = cnt > 0 ? df_match_mask(w, inw[3 + 8 * tid], d) : 0u;
  mask &= cnt == DF_RUN ? ~0u : (1u << cnt) - 1u;
  if (s.seg == 0 && tid == 0) mask &= ~((1u << d) - 1u);                           // no history in front of the plane
  const uint32_t nm = ~mask;
  int P, N;
  {
    int a = nm ? base + 31 - __builtin_clz(nm) : -1, b = nm ? base + __builtin_ctz(nm) : DF_SEG;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ya = __shfl_up(a, o), yb = __shfl_down(b, o);
      if (lane >= o) a = max(a, ya);
      if (lane + o < 64) b = min(b, yb);
    }
    if (lane == 63) sc[0][wv] = a;
    if (lane == 0) sc[1][wv] = b;
    P = __shfl_up(a, 1); N = __shfl_down(b, 1);
    if (lane == 0) P = -1;
    if (lane == 63) N = DF_SEG;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DF_NW; ++k) {
      if (k < wv) P = max(P, sc[0][k]);
      if (k > wv) N = min(N, sc[1][k]);
    }
  }

  // first pass over the run: the tokens' symbols into the histogram, their bits in the fixed code, the Adler-32 partials
  int tb = 0;
  uint32_t s1 = 0, s2 = 0;
#pragma unroll
  for (int e = 0; e < DF_RUN; ++e) {
    if (e >= cnt) continue;
    const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
    const int r = df_role(nm, e, base, P, N);
    if (r < 0) { atomicAdd(&hist[byte], 1u); tb += byte < 144 ? 8 : 9; }
    else if (r > 0) {
      uint32_t eb, ex;
      const uint32_t sym = df_len_code(r, &eb, &ex);
      atomicAdd(&hist[sym], 1u);
      tb += (sym < 280 ? 7 : 8) + (int)eb + 5;
    }
    s1 += byte;
    s2 += (uint32_t)(len - base - e) * byte;
  }
  s2 %= DF_ADLER;
  int off = tb, total;
  {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(off, o);
      if (lane >= o) off += y;
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (lane == 63) { sc[2][wv] = off; sc[3][wv] = (int)(s1 % DF_ADLER); sc[4][wv] = (int)(s2 % DF_ADLER); }
    __syncthreads();
    off -= tb;
    total = 0;
    uint32_t t1 = 0, t2 = 0;
#pragma unroll
    for (int k = 0; k < DF_NW; ++k) {
      if (k < wv) off += sc[2][k];
      total += sc[2][k];
      t1 += (uint32_t)sc[3][k];
      t2 += (uint32_t)sc[4][k];
    }
    s1 = t1 % DF_ADLER;
    s2 = t2 % DF_ADLER;
  }

  // the segment's code: literal/length lengths and codes, their run-length code, the code-length code
  const DfdWork wk = {srt, iw, lpar, ipar, idep, lc, nx, &meta[0]};
  dfd_build<DFD_NLIT, DFD_LIT_LIMIT>(hist, ll, lcode, wk, tid);
  if (tid == 0) {
    meta[1] = dfd_num_lit(ll);
    meta[2] = dfd_rle(ll, meta[1], d, rsym, rext, cc);
  }
  __syncthreads();
  dfd_build<DFD_NCL, DFD_CL_LIMIT>(cc, cl, ccode, wk, tid);
  const int nl = meta[1], nr = meta[2];
  const int hbits = dfd_header_bits(cc, cl);

  // second pass: the tokens' bits in the segment's code (a match: + 1 bit of distance)
  int td = 0;
#pragma unroll
  for (int e = 0; e < DF_RUN; ++e) {
    if (e >= cnt) continue;
    const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
    const int r = df_role(nm, e, base, P, N);
    if (r < 0) td += ll[byte];
    else if (r > 0) {
      uint32_t eb, ex;
      const uint32_t sym = df_len_code(r, &eb, &ex);
      td += ll[sym] + (int)eb + 1;
    }
  }
  int offd = td, totald = 0;
  {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(offd, o);
      if (lane >= o) offd += y;
    }
    if (lane == 63) sc[5][wv] = offd;
    __syncthreads();
    offd -= td;
#pragma unroll
    for (int k = 0; k < DF_NW; ++k) {
      if (k < wv) offd += sc[5][k];
      totald += sc[5][k];
    }
  }

  // the three forms from their totals; a non-final fixed or dynamic block + the empty stored block 000, pad, 00 00 FF FF
  const int fixed_bits = 3 + total + 7 + (s.final_ ? 0 : 3);
  const int fixed_bytes = (fixed_bits + 7) / 8 + (s.final_ ? 0 : 4);
  const int dyn_bits = hbits + totald + ll[256] + (s.final_ ? 0 : 3);
  const int dyn_bytes = (dyn_bits + 7) / 8 + (s.final_ ? 0 : 4);
  const bool dyn = dyn_bytes < fixed_bytes;
  const int coded_bytes = dyn ? dyn_bytes : fixed_bytes;
  const bool stored = coded_bytes > 5 + len;
  const int out_bytes = stored ? 5 + len : coded_bytes;
  const int out_vecs = (out_bytes + 15) / 16;                 // <= DF_SLOT / 16
  if (!stored) {
    for (int i = tid; i < out_vecs * 4 + 2; i += DF_NT) bb[i] = 0;
    __syncthreads();
    if (tid == 0 && !s.final_) {                              // FF FF: the last two bytes
      const int p = 8 * (coded_bytes - 2);
      atomicOr(&bb[p >> 5], 0xffffu << (p & 31));
      if ((p & 31) > 16) atomicOr(&bb[(p >> 5) + 1], 0xffffu >> (32 - (p & 31)));
    }
    if (dyn) {
      if (tid == DF_NT - 1) {                                 // the header and EOB: the thread whose run is the first to be short
        DfdSink hs(bb, 0);
        dfd_put_header(hs, s.final_, nl, d, cl, ccode, rsym, rext, nr);
        hs.flush();
        DfdSink es(bb, hbits + totald);
        es.put(lcode[256], ll[256]);
        es.flush();
      }
      DfdSink ts(bb, hbits + offd);
#pragma unroll
      for (int e = 0; e < DF_RUN; ++e) {
        if (e >= cnt) continue;
        const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
        const int r = df_role(nm, e, base, P, N);
        if (r < 0) ts.put(lcode[byte], ll[byte]);
        else if (r > 0) {
          uint32_t eb, ex;
          const uint32_t sym = df_len_code(r, &eb, &ex);
          ts.put((uint32_t)lcode[sym] | ex << ll[sym], ll[sym] + (int)eb + 1);
        }
      }
      ts.flush();
    } else {
      if (tid == 0) atomicOr(&bb[0], (uint32_t)s.final_ | 2u);
      DfdSink ts(bb, 3 + off);
#pragma unroll
      for (int e = 0; e < DF_RUN; ++e) {
        if (e >= cnt) continue;
        const uint32_t byte = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
        int nb;
        const uint32_t v = df_token(nm, e, base, P, N, byte, d, &nb);
        ts.put(v, nb);
      }
      ts.flush();
    }
  } else {
    // stored block: BFINAL (BTYPE 00, padding), LEN, ~LEN, the raw bytes -- the segment shifted by 5 bytes
    const uint32_t* x = inw + 4;
    const uint32_t h4 = ((uint32_t)~len >> 8) & 0xffu;
    for (int m = tid; m < out_vecs * 4; m += DF_NT) {
      uint32_t v;
      if (m == 0) v = (uint32_t)s.final_ | ((uint32_t)len & 0xffffu) << 8 | ((uint32_t)~len & 0xffu) << 24;
      else {
        const uint32_t lo = m == 1 ? h4 : m - 2 < len / 4 ? x[m - 2] >> 24 : 0u, hi = m - 1 < len / 4 ? x[m - 1] : 0u;
        v = lo | hi << 8;
      }
      bb[m] = v;
    }
  }
  __syncthreads();
  uint4* slot4 = reinterpret_cast<uint4*>(slots + (long long)blockIdx.x * DF_SLOT);
  const uint4* bb4 = reinterpret_cast<const uint4*>(bb);
  for (int v = tid; v < out_vecs; v += DF_NT) slot4[v] = bb4[v];
  if (tid == 0) {
    uint32_t* t = table + 4ll * blockIdx.x;
    t[0] = (uint32_t)out_bytes; t[1] = s1; t[2] = s2;
  }
}

// Stream p of the batch: the scan of its segments' byte counts (each segment's offset in the stream into its table entry, behind the two
// header bytes) and its Adler-32 from the segments' partial sums.  Returns the stream's length, header and trailer included.
__device__ __forceinline__ uint32_t df_stream_scan(uint32_t* __restrict__ table, int p, int HW, int nso, int nsf, uint32_t* adler) {
  const int sps = 16 * nso + 8 * nsf;
  const int b = p / 24, k = (p % 24) / 3, f = p % 3;
  const int ns = f < 2 ? nso : nsf, n = f < 2 ? HW : 2 * HW;
  uint32_t* t = table + 4 * ((long long)b * sps + (f < 2 ? (f * 8 + k) * nso : 16 * nso + k * nsf));
  uint32_t A = 1, Bs = 0, acc = 2;
  for (int s = 0; s < ns; ++s) {
    const uint32_t L = (uint32_t)min(DF_SEG, n - s * DF_SEG);
    t[4 * s + 3] = acc;
    acc += t[4 * s];
    Bs = (Bs + L * A + t[4 * s + 2]) % DF_ADLER;          // L * A < 2^14 * 2^16
    A = (A + t[4 * s + 1]) % DF_ADLER;
  }
  *adler = Bs << 16 | A;
  return acc + 4;
}

// One workgroup of 1024: thread <-> stream, in chunks of 1024 streams with a running carry.
__global__ __launch_bounds__(1024) void deflate_offsets_kernel(uint32_t* __restrict__ table, uint8_t* __restrict__ out, uint32_t* __restrict__ offsets,
                                                               int P, int HW, int nso, int nsf) {
  __shared__ uint32_t ws[16];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int p0 = 0; p0 < P; p0 += 1024) {
    const int p = p0 + tid;
    uint32_t total = 0, adler = 1;
    if (p < P) total = df_stream_scan(table, p, HW, nso, nsf, &adler);
    uint32_t inc = total;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o);
      if (lane >= o) inc += y;
    }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint32_t off = carry + inc - total;
    for (int k = 0; k < wv; ++k) off += ws[k];
    if (p < P) {
      offsets[p] = off;
      out[off] = 0x78; out[off + 1] = 0x01;
      uint8_t* tr = out + off + total - 4;
      tr[0] = adler >> 24; tr[1] = adler >> 16; tr[2] = adler >> 8; tr[3] = adler;
    }
    __syncthreads();
    if (tid == 1023) carry = off + total;
    __syncthreads();
  }
  if (tid == 0) offsets[P] = carry;
}

// deflate_offsets_kernel for the framed layout (frame.h): besides each stream's scan, header and trailer, the protobuf header in front of
// every stream and every waypoint.  One workgroup of 1024, thread <-> stream in chunks of DFF_CHUNK = 1008 = 42 scenes, so that a
// waypoint's three streams and a scene's 24 always lie in one chunk (1024 is a multiple of neither); a waypoint's body length is read
// from its three threads' field lengths in LDS, and ONE scan then runs over the extents (the stream's field, + the waypoint's header on
// its first stream).  ftable: [ stream starts P | stream lengths P | scene starts P / 24 + 1 ]; the starts are what deflate_pack_kernel
// takes for `offsets`.
// A thread's header bytes, at most 2 * FRM_MAX_HEADER + 2, gathered in registers and written with two stores that may overlap: a store
// instruction per byte, each to 64 different cache lines per wave, put the chain outside its gate.  Byte addresses, so the
// stores are unaligned ones.
struct DffBytes {
  uint64_t lo = 0, hi = 0;
  uint32_t n = 0;
  __device__ __forceinline__ void put(uint8_t b) {
    if (n < 8) lo |= (uint64_t)b << (8 * n); else hi |= (uint64_t)b << (8 * (n - 8));
    ++n;
  }
  __device__ __forceinline__ void put_varint(uint32_t v) {
    for (; v >= 0x80u; v >>= 7) put((uint8_t)(v | 0x80u));
    put((uint8_t)v);
  }
  __device__ __forceinline__ void store(uint8_t* q) const {             // 4 <= n <= 16
    if (n >= 8) {
      const uint32_t sh = 8 * (n - 8);
      const uint64_t tail = sh == 0 ? lo : sh == 64 ? hi : lo >> sh | hi << (64 - sh);
      __builtin_memcpy(q, &lo, 8);
      __builtin_memcpy(q + n - 8, &tail, 8);
    } else {
      const uint32_t head = (uint32_t)lo, tail = (uint32_t)(lo >> (8 * (n - 4)));
      __builtin_memcpy(q, &head, 4);
      __builtin_memcpy(q + n - 4, &tail, 4);
    }
  }
};
constexpr int DFF_CHUNK = 1008;
static_assert(DFF_CHUNK % 24 == 0 && DFF_CHUNK <= 1024, "whole scenes per chunk");
__global__ __launch_bounds__(1024) void deflate_offsets_framed_kernel(uint32_t* __restrict__ table, uint8_t* __restrict__ out, uint32_t* __restrict__ ftable,
                                                                      int P, int HW, int nso, int nsf, uint32_t tags) {
  __shared__ uint32_t ws[16];
  __shared__ uint32_t fl[1024];
  __shared__ uint32_t carry;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int f = tid % 3;                                   // (= p % 3: a chunk starts with a scene)
  if (tid == 0) carry = 0;
  for (int p0 = 0; p0 < P; p0 += DFF_CHUNK) {
    const int p = p0 + tid;
    const bool live = tid < DFF_CHUNK && p < P;
    uint32_t total = 0, adler = 1, field = 0;
    if (live) { total = df_stream_scan(table, p, HW, nso, nsf, &adler); field = frm_field_len(total); }
    fl[tid] = field;
    __syncthreads();
    uint32_t body = 0, ext = field;
    if (live && f == 0) { body = field + fl[tid + 1] + fl[tid + 2]; ext += 1u + pb_varint_len(body); }      // tid + 2 <= 1007
    uint32_t inc = ext;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o);
      if (lane >= o) inc += y;
    }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint32_t off = carry + inc - ext;
    for (int k = 0; k < wv; ++k) off += ws[k];
    if (live) {
      DffBytes h;
      if (f == 0) {
        if (tid % 24 == 0) ftable[2 * P + p / 24] = off;
        h.put(frm_tag(tags, 0));
        h.put_varint(body);
      }
      h.put(frm_tag(tags, 1 + f));
      h.put_varint(total);
      const uint32_t start = off + h.n;
      ftable[p] = start;
      ftable[P + p] = total;
      h.put(0x78); h.put(0x01);
      h.store(out + off);
      const uint32_t be = __builtin_bswap32(adler);
      __builtin_memcpy(out + start + total - 4, &be, 4);
    }
    __syncthreads();
    if (tid == 1023) carry = off + ext;                    // (ext = 0 here: the chunk's end)
  }
  __syncthreads();
  if (tid == 0) ftable[2 * P + P / 24] = carry;
}

// The slot's bytes to out + offsets[stream] + (offset in the stream): whole aligned 16-byte vectors of the destination are composed from
// the slot's dwords (a funnel shift by the destination's misalignment); the destination's first and last partial vectors go bytewise.
__global__ __launch_bounds__(256) void deflate_pack_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ table,
                                                           const uint32_t* __restrict__ offsets, uint8_t* __restrict__ out, int HW, int nso, int nsf) {
  __shared__ __attribute__((aligned(16))) uint32_t lw[DF_SLOT / 4 + 8];
  const int tid = threadIdx.x;
  const DfSeg s = df_locate(blockIdx.x, HW, nso, nsf);
  const uint32_t* t = table + 4ll * blockIdx.x;
  const int bytes = (int)t[0];
  const unsigned long long dst = (unsigned long long)offsets[s.stream] + t[3];
  const int nv = (bytes + 15) / 16;
  const uint4* slot4 = reinterpret_cast<const uint4*>(slots + (long long)blockIdx.x * DF_SLOT);
  uint4* lw4 = reinterpret_cast<uint4*>(lw);
  for (int v = tid; v <= nv; v += 256) lw4[v] = v < nv ? slot4[v] : make_uint4(0, 0, 0, 0);
  __syncthreads();
  const int a = (int)(dst & 15);
  uint8_t* dsta = out + (dst - a);                       // 16-byte aligned; destination byte 16 c + i is slot byte 16 c + i - a
  const int nch = (a + bytes + 15) / 16;
  const uint8_t* lb = reinterpret_cast<const uint8_t*>(lw);
  for (int c = tid; c < nch; c += 256) {
    const int j0 = 16 * c - a;
    if (j0 >= 0 && j0 + 16 <= bytes) {
      const int jd = j0 >> 2, sh = (j0 & 3) * 8;
      uint32_t v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = sh ? lw[jd + q] >> sh | lw[jd + q + 1] << (32 - sh) : lw[jd + q];
      *reinterpret_cast<uint4*>(dsta + 16 * c) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
      for (int i = 0; i < 16; ++i)
        if (j0 + i >= 0 && j0 + i < bytes) dsta[16 * c + i] = lb[j0 + i];
    }
  }
}

static int df_shape(const char* who, int B, int Tn, int Hh, int Ww, bool framed, long long* nseg, long long* cap, int* nso, int* nsf) {
  if (B <= 0 || Hh <= 0 || Ww <= 0) { stj_set_error("%s: empty problem", who); return STJ_EINVAL; }
  const long long HW = (long long)Hh * Ww;
  if (Tn != 8 || HW % 256 || HW > (1 << 28)) {
    stj_set_error("%s: Tn = 8, H * W a multiple of 256 only (Tn %d, H %d, W %d)", who, Tn, Hh, Ww);
    return STJ_EUNSUPPORTED;
  }
  *nso = (int)((HW + DF_SEG - 1) / DF_SEG);
  *nsf = (int)((2 * HW + DF_SEG - 1) / DF_SEG);
  *nseg = (long long)B * (16 * *nso + 8 * *nsf);
  *cap = (long long)B * (32 * HW + 5ll * (16 * *nso + 8 * *nsf) + 6 * 24);            // n + 5 ceil(n / DF_SEG) + 6 per stream
  if (framed) *cap += (long long)B * FRM_MAX_HEADER * (24 + 8);                          // + a header per stream and per waypoint (frame.h)
  if (*nseg > 0x7fffffffLL || *cap > 0xffffffffLL) {
    stj_set_error("%s: batch too large for 32-bit stream offsets (B %d, H %d, W %d)", who, B, Hh, Ww);
    return STJ_EUNSUPPORTED;
  }
  return STJ_OK;
}
static inline long long df_table_bytes(long long nseg) { return (nseg * 16 + 255) / 256 * 256; }

extern "C" int stj_compress_sizes(int B, int Tn, int H, int W, long long* work_bytes, long long* out_capacity) {
  long long nseg, cap; int nso, nsf;
  const int rc = df_shape("stj_compress_sizes", B, Tn, H, W, false, &nseg, &cap, &nso, &nsf);
  if (rc != STJ_OK) return rc;
  *work_bytes = df_table_bytes(nseg) + nseg * DF_SLOT;
  *out_capacity = (cap + 15) / 16 * 16;
  return STJ_OK;
}

// `framed`: `offsets` is the framed table (stream starts first: what the pack kernel reads), `tags` the four tag bytes.
static int df_launch(const char* who, const uint8_t* Q, void* work, uint8_t* out, uint32_t* offsets, int B, int Tn, int H, int W, int level,
                     bool framed, uint32_t tags, hipStream_t stream) {
  if (level != 1 && level != 2) { stj_set_error("%s: level 1 (fixed Huffman code) or 2 (dynamic per segment), got %d", who, level); return STJ_EINVAL; }
  long long nseg, cap; int nso, nsf;
  const int rc = df_shape(who, B, Tn, H, W, framed, &nseg, &cap, &nso, &nsf);
  if (rc != STJ_OK) return rc;
  if (((uintptr_t)Q | (uintptr_t)work | (uintptr_t)out | (uintptr_t)offsets) & 15) {
    stj_set_error("%s: 16-byte aligned buffers only", who);
    return STJ_EUNSUPPORTED;
  }
  uint32_t* table = reinterpret_cast<uint32_t*>(work);
  uint8_t* slots = reinterpret_cast<uint8_t*>(work) + df_table_bytes(nseg);
  const int HW = H * W;
  if (level == 1) hipLaunchKernelGGL(deflate_encode_kernel, dim3((unsigned)nseg), dim3(DF_NT), 0, stream, Q, slots, table, HW, nso, nsf);
  else hipLaunchKernelGGL(deflate_encode_dyn_kernel, dim3((unsigned)nseg), dim3(DF_NT), 0, stream, Q, slots, table, HW, nso, nsf);
  if (framed) hipLaunchKernelGGL(deflate_offsets_framed_kernel, dim3(1), dim3(1024), 0, stream, table, out, offsets, B * 24, HW, nso, nsf, tags);
  else hipLaunchKernelGGL(deflate_offsets_kernel, dim3(1), dim3(1024), 0, stream, table, out, offsets, B * 24, HW, nso, nsf);
  hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)nseg), dim3(256), 0, stream, (const uint8_t*)slots, (const uint32_t*)table,
                     (const uint32_t*)offsets, out, HW, nso, nsf);
  return stj_check_launch(who);
}

extern "C" int stj_compress_waypoints(const uint8_t* Q, void* work, uint8_t* out, uint32_t* offsets, int B, int Tn, int H, int W, hipStream_t stream) {
  return df_launch("stj_compress_waypoints", Q, work, out, offsets, B, Tn, H, W, 1, false, 0u, stream);
}

extern "C" int stj_compress_waypoints_level(const uint8_t* Q, void* work, uint8_t* out, uint32_t* offsets, int B, int Tn, int H, int W, int level,
                                            hipStream_t stream) {
  return df_launch("stj_compress_waypoints_level", Q, work, out, offsets, B, Tn, H, W, level, false, 0u, stream);
}

extern "C" int stj_compress_framed_sizes(int B, int Tn, int H, int W, long long* work_bytes, long long* out_capacity, long long* table_words) {
  long long nseg, cap; int nso, nsf;
  const int rc = df_shape("stj_compress_framed_sizes", B, Tn, H, W, true, &nseg, &cap, &nso, &nsf);
  if (rc != STJ_OK) return rc;
  *work_bytes = df_table_bytes(nseg) + nseg * DF_SLOT;
  *out_capacity = (cap + 15) / 16 * 16;
  *table_words = 6ll * B * Tn + B + 1;
  return STJ_OK;
}

extern "C" int stj_compress_waypoints_framed(const uint8_t* Q, void* work, uint8_t* out, uint32_t* table, int B, int Tn, int H, int W, int level,
                                             uint32_t tags, hipStream_t stream) {
  return df_launch("stj_compress_waypoints_framed", Q, work, out, table, B, Tn, H, W, level, true, tags, stream);
}
