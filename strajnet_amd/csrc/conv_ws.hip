// Weight-stationary, persistent forward kernel for the folded nearest-2x-upsample 3x3 convolution (bf16).
// (reference op: UpSampling3D(1,2,2) -> Conv2D 3x3 SAME + bias -> ELU, modules.py:746-748,732-735; algebra in conv.hip)
//
// Why: the first kernel (conv.hip) re-staged all 16 effective-tap weight matrices through LDS for every 8x16 pixel
// tile and ran at ~8 % MFMA utilisation (rocprof PMC: 57 % of wave cycles waiting, half of all LDS cycles bank
// conflicts; profiles/r01_b_*).  Here
//   * one wavefront owns one output phase (a,b); its 4 tap matrices Weff[a,b,r,s] (CoutTile x Cin) sit in VGPRs for the
//     whole kernel as MFMA *A* fragments (v_mfma_f32_16x16x32_bf16: D[cout][pixel] += W[cout][k] * X[k][pixel]);
//   * workgroups are persistent (one per CU) and walk over pixel tiles; the only LDS traffic of the main loop is the
//     B fragment (16 pixels x 32 channels = one ds_read_b128 per lane) which feeds NF MFMAs;
//   * the input halo (10 x 18 low-res pixels x Cin) is double buffered: the next tile's global loads are issued before
//     the MFMA loop and written to the other LDS buffer after it;
//   * results (bias + ELU applied) are staged in LDS and leave as full rows of 8-byte segments, coalesced.
// The file has grown beyond that kernel.  It holds, each under its own banner: the wave-specialised forward (with the inference heads'
// epilogue), the transpose-read weight gradient (tr, tr4), the MFMA output heads (forward, pair, gather, backward, reduce) and the
// weight-stationary input gradients (ws, ws2).  The entry points that try them are in conv.hip.  Every kernel here with dynamic LDS
// takes its layout from a ...Geo struct in front of it, and its launcher takes the byte count from the same struct.
#include "common.h"
#include "quantize.h"
#include <stdlib.h>
#include <type_traits>

#ifndef DG_PF
#define DG_PF 3         // fragment groups in flight ahead of their MFMAs, upconv_dgrad_ws2_kernel (2 / 3 / 5: 230 / 227 / 229 us; old order 244)
#endif
#ifndef WS2_PF_K4
#define WS2_PF_K4 6
#endif
#ifndef WS2_PF
#define WS2_PF 6        // ... upconv_fwd_ws2_kernel (2 / 4 / 6: 209 / 199 / 194 us; 7 spills)
#endif
#define WS_TH 8
#define WS_TW 16
#define WS_HW (WS_TW + 2)
#define WS_HH (WS_TH + 2)

// =====================================================================================================
// Wave-specialised forward kernel (round 2).  The first weight-stationary kernel (`upconv_fwd_ws_kernel`: every wave prefetched, ran its MFMAs, applied
// the ELU, committed the next halo and stored; removed in round 6, see upconv_fwd_ws_try_t) measured by rocprof PMC: MFMA busy 22 %, HBM 27 %, one wave
// per SIMD -- the phases of a tile (prefetch issue, MFMA + LDS fragment reads, ELU epilogue, LDS commit of the next halo, barrier,
// coalesced store loop, barrier) add up serially inside each wave because nothing else is resident on the SIMD to overlap them.
// Here a workgroup has EIGHT waves with two roles:
//   * waves 0-3 ("compute"): own one output phase each, tap matrices stationary in VGPRs, do nothing but ds_read fragments ->
//     MFMA -> bias + ELU -> 8-byte writes into a small output stage;
//   * waves 4-7 ("movers"): never touch the matrix pipe: they drain the output stage of the PREVIOUS step to global memory
//     (16-byte coalesced stores), and fetch the next tile's halo (global -> registers at the tile's first step, registers -> LDS at
//     its last one).
// A "step" is two low-res rows of a tile (= 4 output rows); the output stage is double buffered at step granularity (2 x 14 KB
// instead of one 57 KB tile stage), the halo at tile granularity; one workgroup barrier per step.  Both roles run on every SIMD (one
// compute + one mover wave each), so global traffic, LDS staging and the epilogue's VALU work overlap the MFMAs of the other role.
// =====================================================================================================
// HEAD = true (inference, the last level: Cout = 48 = one channel tile): the 3x3 48 -> 2 output head that follows (modules.py:767-770)
// starts in this kernel's epilogue.  out[p][o] = sum_taps sum_c Wh[tap][c][o] y[p + tap][c] = sum_taps z[p + tap][tap, o] with the per-pixel
// projection z[q][tap, o] = sum_c Wh[tap][c][o] y[q][c]: 18 numbers per pixel instead of 48, and no halo -- y never leaves the chip.  The
// ELU outputs a lane holds after the main MFMAs (D layout: channels 16 n + 4 g + r of ITS pixel) ARE an MFMA B operand for pixel = column
// if the head weights (A operand, rows = (tap, o)) are laid out with the same k order -- the contraction order is free -- so z costs 4 more
// MFMAs per 16 pixels and no data movement.  Y is then the z tensor [F, 2 Hi, 2 Wi, STJ_HEAD_CZ = 20] (18 + 2 zero channels: whole 8-byte pieces), which
// stj_outconv_pair_gather sums over the 9 neighbours: 48 + 48 bytes per pixel of traffic instead of 96 + 96.
// LDS layout of upconv_fwd_ws2_kernel (16-bit elements): two halo buffers [HPIX][LDK], then two output-stage buffers.
template <int KS, int NF, bool HEAD>
struct Ws2Geo {
  static constexpr int CIN = KS * 32, CT = NF * 16;
  static constexpr int LDK = CIN + 16;                   // halo pixel stride
  static constexpr int LDO = HEAD ? 40 : CT + 8;         // stage pixel stride
  static constexpr int HPIX = WS_HH * WS_HW;
  static constexpr int SR = 4;                           // low-res rows per step
  static constexpr int OST = 2 * SR * (2 * WS_TW) * LDO; // one output-stage buffer: 2*SR output rows x 32 pixels
  static constexpr int OST_ALLOC = 2 * SR * (2 * WS_TW) * (CT + 8);   // (the z stage of HEAD is smaller than the y stage it replaces and keeps its allocation)
  static constexpr int HALO_BYTES = 2 * HPIX * LDK * 2;  // both halo buffers; the stage buffers follow (the kernel's ost0)
  static constexpr int LDS_BYTES = HALO_BYTES + 2 * OST_ALLOC * 2;
  static_assert(OST <= OST_ALLOC && LDS_BYTES <= 160 * 1024, "the layout fits its allocation and the CU's LDS");
};
template <typename T, int KS, int NF, bool EXACT, bool HEAD = false, int XCT = 0>
__global__ __launch_bounds__(512, 1) void upconv_fwd_ws2_kernel(const T* __restrict__ X, const T* __restrict__ Wf,
                                                             const float* __restrict__ bias, T* __restrict__ Y,
                                                             int F, int Hi, int Wi, int Cout_, int ntiles, int dbg, const float* __restrict__ Wh) {
  static_assert(sizeof(T) == 2, "16-bit operands");
  using G = Ws2Geo<KS, NF, HEAD>;
  constexpr int CIN = G::CIN;
  constexpr bool XMAP = XCT > 1;
  constexpr int LDK = G::LDK;
  constexpr int CT = G::CT;
  constexpr int CTO = HEAD ? STJ_HEAD_CZ : CT;           // channels of a stage pixel / of the result
  constexpr int LDO = G::LDO;
  const int Cout = HEAD ? CT : Cout_;                    // channels of the convolution itself
  const int Cres = HEAD ? STJ_HEAD_CZ : Cout_;           // channels of the tensor the movers write
  static_assert(!HEAD || (NF == 3 && EXACT), "the head epilogue is written for the 48-channel level, whole tiles");
  constexpr int HPIX = G::HPIX;
  constexpr int CPP = CIN / 8;
  constexpr int NCH = (HPIX * CPP + 255) / 256;          // halo chunks per mover thread
  constexpr int SR = G::SR;
  constexpr int OST = G::OST;
  constexpr int STEPS = WS_TH / SR;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* halo0 = reinterpret_cast<T*>(smem_raw);
  T* halo1 = halo0 + HPIX * LDK;
  T* ost0 = halo1 + HPIX * LDK;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool mover = w >= 4;
  const int mt = tid - 256;                              // mover thread index 0..255
  const int g = lane >> 4, ln = lane & 15;
  // Workgroup map: 1-D grid of (walkers x cout groups).  With several cout groups (the 128 -> 96 layer: 3) the groups that walk the SAME
  // tile sequence sit on ONE XCD (workgroup id % 8) and share the halo tiles through that XCD's L2: as a (walker, group) 2-D grid they
  // landed on three XCDs and X was fetched 266 MB per launch for a 67 MB input (profiles/r04_h_roofline_traffic.json, the one-role kernel).
  const int BX = XMAP ? ((int)(blockIdx.x >> 3) / XCT) * 8 + (int)(blockIdx.x & 7) : (int)blockIdx.x;
  const int BY = XMAP ? (int)(blockIdx.x >> 3) % XCT : (int)blockIdx.y;
  const int GX = XMAP ? (int)gridDim.x / XCT : (int)gridDim.x;
  const int n0 = BY * CT;
  const int tiles_x = (Wi + WS_TW - 1) / WS_TW, tiles_y = (Hi + WS_TH - 1) / WS_TH;
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  auto tile_coords = [&](int tile, int& f, int& ty0, int& tx0) {
    const int tx = tile % tiles_x; const int t2 = tile / tiles_x;
    ty0 = (t2 % tiles_y) * WS_TH; f = t2 / tiles_y; tx0 = tx * WS_TW;
  };

  if (!mover) {
    // ------------------------------------------------------------------ compute role
    const int a = w >> 1, b = w & 1;
    s16x8 wf[4][NF][KS];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int pt = a * 8 + b * 4 + t;
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int co = n0 + n * 16 + ln;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if (co < Cout) wf[t][n][ks] = *reinterpret_cast<const s16x8*>(Wf + ((long long)pt * Cout + co) * CIN + ks * 32 + g * 8);
          else wf[t][n][ks] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
    }
    float bv[NF][4];
#pragma unroll
    for (int n = 0; n < NF; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = n0 + n * 16 + g * 4 + r;
        bv[n][r] = co < Cout ? bias[co] : 0.f;
      }
    // head weights Wh f32 [9 taps][48][2] as MFMA A fragments: row t = 2 tap + o (t-fragment tf: t = 16 tf + ln, 18 rows used), k slot j
    // of lane group g = channel 16 (j / 4) + 4 g + j % 4 (k-step 0: channels 0..31) / 32 + 4 g + j, j < 4 (k-step 1: channels 32..47)
    s16x8 hw[2][2];
    if constexpr (HEAD) {
#pragma unroll
      for (int tf = 0; tf < 2; ++tf) {
        const int t = 16 * tf + ln;
        float v0[8], v1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c0 = 16 * (j / 4) + 4 * g + j % 4, c1 = 32 + 4 * g + j;
          v0[j] = t < 18 ? Wh[((t >> 1) * CT + c0) * 2 + (t & 1)] : 0.f;
          v1[j] = (t < 18 && j < 4) ? Wh[((t >> 1) * CT + c1) * 2 + (t & 1)] : 0.f;
        }
        typedef __attribute__((ext_vector_type(4))) uint32_t u4;
        hw[tf][0] = __builtin_bit_cast(s16x8, (u4){pack2<T>(v0[0], v0[1]), pack2<T>(v0[2], v0[3]), pack2<T>(v0[4], v0[5]), pack2<T>(v0[6], v0[7])});
        hw[tf][1] = __builtin_bit_cast(s16x8, (u4){pack2<T>(v1[0], v1[1]), pack2<T>(v1[2], v1[3]), 0u, 0u});
      }
      // the four fragments depend on the lane only: one copy in LDS behind the stage (the launcher sizes the stage for LDO = CT + 8; as 16
      // stationary registers per lane they spilled once the fragment ring was added), read back where the projection runs
      if (w == 0) {
#pragma unroll
        for (int tf = 0; tf < 2; ++tf)
#pragma unroll
          for (int k = 0; k < 2; ++k) *reinterpret_cast<s16x8*>(ost0 + 2 * OST + ((tf * 2 + k) * 64 + lane) * 8) = hw[tf][k];
      }
    }
    __syncthreads();                                     // halo of the first tile committed by the movers
    int q = 0;
    for (int tile = BX; tile < ntiles; tile += GX) {
      const T* halo = ((tile - BX) / GX) & 1 ? halo1 : halo0;
#pragma unroll 1
      for (int st = 0; st < STEPS; ++st, ++q) {
        const int mf = SR * st;
        T* ost = ost0 + (q & 1) * OST;
        // the accumulators start at the bias (the MFMA's C operand: no add in the epilogue)
        f32x4 acc[SR][NF];
#pragma unroll
        for (int m = 0; m < SR; ++m)
#pragma unroll
          for (int n = 0; n < NF; ++n) acc[m][n] = (f32x4){bv[n][0], bv[n][1], bv[n][2], bv[n][3]};
        // a halo row feeds tap row r = 0 of output row j and tap row r = 1 of output row j - 1: SR + 1 fragment reads per (s, ks)
        // serve 2 SR row-taps (the tile-at-a-time kernel reads each twice).  The reads are issued PF groups AHEAD of their MFMAs (ring of
        // PF + 1 fragments): written as read-then-use, the ISA was ds_read, s_waitcnt lgkmcnt(0), 3-6 MFMAs, ds_read, ... -- the LDS
        // latency exposed 30 times per step to a wave that is alone on its SIMD's matrix pipe (230 -> 208 us at F = 64, role ablation in DESIGN 4m).
        // Round 6: the groups in HALO-ROW-MAJOR order (below) with the ring 6 deep: 210 -> 194 us alone in a hot loop (2 deep: 209; the old
        // (s, ks, row) order 4 deep: 214), profiles/r06_z2_ws2_pf.txt.  (The role-ablation bits 1 and 2 of `dbg` went with the old order.)
        // Halo-row-major order: after the 2 KS fragments of halo row hr, output row hr - 1 is COMPLETE (its r = 1 taps were the last it
        // was waiting for), so its epilogue -- 12 ELUs per lane, a quarter-rate v_exp each, the packs, the stage writes (HEAD: + the
        // projection MFMAs) -- is issued THERE, in front of halo row hr + 1's 36 MFMAs, whose matrix-pipe time covers its VALU work.  In
        // the (s, ks, row) order every accumulator finished at the very end of the step and the whole epilogue ran with the matrix pipe idle
        // (role ablation: 44 of the kernel's 218 us).
        s16x8 hwr[2][2];
        if constexpr (HEAD) {
#pragma unroll
          for (int tf = 0; tf < 2; ++tf)
#pragma unroll
            for (int k = 0; k < 2; ++k) hwr[tf][k] = *reinterpret_cast<const s16x8*>(ost0 + 2 * OST + ((tf * 2 + k) * 64 + lane) * 8);
        }
        auto epi = [&](const int m) __attribute__((always_inline)) {
          if constexpr (HEAD) {
            uint32_t pk[NF][2];
#pragma unroll
            for (int n = 0; n < NF; ++n) {
              pk[n][0] = pack2<T>(elu_c(acc[m][n][0]), elu_c(acc[m][n][1]));
              pk[n][1] = pack2<T>(elu_c(acc[m][n][2]), elu_c(acc[m][n][3]));
            }
            typedef __attribute__((ext_vector_type(4))) uint32_t u4;
            const s16x8 y0 = __builtin_bit_cast(s16x8, (u4){pk[0][0], pk[0][1], pk[1][0], pk[1][1]});
            const s16x8 y1 = __builtin_bit_cast(s16x8, (u4){pk[2][0], pk[2][1], 0u, 0u});
            T* zp = ost + ((2 * m + a) * (2 * WS_TW) + 2 * ln + b) * LDO;
#pragma unroll
            for (int tf = 0; tf < 2; ++tf) {
              f32x4 z = (f32x4){0.f, 0.f, 0.f, 0.f};
              z = Mma<T>::mma(hwr[tf][0], y0, z);
              z = Mma<T>::mma(hwr[tf][1], y1, z);
              if (tf == 0 || 16 + 4 * g < STJ_HEAD_CZ) *reinterpret_cast<uint2*>(zp + 16 * tf + 4 * g) = make_uint2(pack2<T>(z[0], z[1]), pack2<T>(z[2], z[3]));
            }
          } else {
#pragma unroll
            for (int n = 0; n < NF; ++n) {
              const uint32_t p0 = pack2<T>(elu_c(acc[m][n][0]), elu_c(acc[m][n][1]));
              const uint32_t p1 = pack2<T>(elu_c(acc[m][n][2]), elu_c(acc[m][n][3]));
              *reinterpret_cast<uint2*>(ost + ((2 * m + a) * (2 * WS_TW) + 2 * ln + b) * LDO + n * 16 + g * 4) = make_uint2(p0, p1);
            }
          }
        };
        {
          constexpr int PF = KS == 4 ? WS2_PF_K4 : WS2_PF, NG = 2 * KS * (SR + 1);
          auto frag = [&](const int gi) -> s16x8 {
            const int hr = gi / (2 * KS), s2 = (gi / KS) & 1, ks = gi % KS;
            return *reinterpret_cast<const s16x8*>(halo + ((mf + hr + a) * WS_HW + ln + b + s2) * LDK + ks * 32 + g * 8);
          };
          s16x8 xr[PF + 1];
#pragma unroll
          for (int i = 0; i < PF; ++i) xr[i] = frag(i);
#pragma unroll
          for (int gi = 0; gi < NG; ++gi) {
            if (gi + PF < NG) xr[(gi + PF) % (PF + 1)] = frag(gi + PF);
            const int hr = gi / (2 * KS), s2 = (gi / KS) & 1, ks = gi % KS;
            const s16x8 xb = xr[gi % (PF + 1)];
            if (hr < SR) {
#pragma unroll
              for (int n = 0; n < NF; ++n) acc[hr][n] = Mma<T>::mma(wf[s2][n][ks], xb, acc[hr][n]);
            }
            if (hr > 0) {
#pragma unroll
              for (int n = 0; n < NF; ++n) acc[hr - 1][n] = Mma<T>::mma(wf[2 + s2][n][ks], xb, acc[hr - 1][n]);
            }
            if (gi % (2 * KS) == 2 * KS - 1 && hr > 0) epi(hr - 1);
          }
        }
        __syncthreads();                                 // step q's stage is complete; the movers drain it during step q + 1
      }
    }
    __syncthreads();                                     // matches the movers' final drain barrier
  } else if constexpr (EXACT) {
    // ------------------------------------------------------------------ mover role, straight-line version (whole tiles, Cout % CT == 0)
    // Same duties as below with every load, LDS write and store unconditional (clamped halo addresses, zeroing at commit through a
    // pinned mask, a thread's surplus chunk repeats its previous one, the tile after the last is the last again): with guarded
    // memory operations the compiler waits on vmcnt(0) before the commit -- i.e. for the drain's STORES, which count in vmcnt on
    // gfx9 -- once per tile, and before every drain on the prefetch issued just above it.
    static_assert(STEPS == 2, "the step sequence below is written out for two steps per tile");
    constexpr int NCHK = HPIX * CPP;
    uint4 pre[NCH];
    int msk = 0;
    int cgeo[NCH];                                        // halo pixel | channel chunk << 16
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = mt + i * 256;
      if (c >= NCHK) c -= 256;                            // surplus chunk of the last round: the thread's previous chunk again
      cgeo[i] = (c / CPP) | ((c % CPP) << 16);
    }
    const int last_tile = ntiles - 1;
    auto prefetch = [&](int tile) {
      tile = tile < last_tile ? tile : last_tile;
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
      const T* Xf = X + (long long)f * Hi * Wi * CIN;
      int m = 0;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int px = cgeo[i] & 0xffff, ch = (cgeo[i] >> 16) * 8;
        const int gy = ty0 + px / WS_HW - 1, gx = tx0 + px % WS_HW - 1;
        const int cy = min(max(gy, 0), Hi - 1), cx = min(max(gx, 0), Wi - 1);
        m |= (cy == gy && cx == gx) ? (1 << i) : 0;
        pre[i] = *reinterpret_cast<const uint4*>(Xf + (cy * Wi + cx) * CIN + ch);
      }
      msk = m;
    };
    auto commit = [&](T* halo) {
      int m = msk;
      asm volatile("" : "+v"(m));                         // keeps the zeroing below the barrier that precedes the commit
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const bool in = (m >> i) & 1;
        const uint4 v = make_uint4(in ? pre[i].x : 0u, in ? pre[i].y : 0u, in ? pre[i].z : 0u, in ? pre[i].w : 0u);
        *reinterpret_cast<uint4*>(halo + (cgeo[i] & 0xffff) * LDK + (cgeo[i] >> 16) * 8) = v;
      }
    };
    constexpr int IE = HEAD ? 4 : 8;                       // elements per drained item: 8-byte pieces of the 40-byte z pixels | 16-byte pieces
    constexpr int SEG = CTO / IE, NIT = 2 * SR * 2 * WS_TW * SEG;
    static_assert(NIT % 256 == 0, "whole rounds of items per step");
    auto drain = [&](const T* ost, int f, int ty0, int tx0, int st) {
      T* Yf = Y + (long long)f * Ho * Wo * Cres + ((long long)(2 * ty0 + 2 * SR * st) * Wo + 2 * tx0) * Cres + (HEAD ? 0 : n0);
#pragma unroll
      for (int i = 0; i < NIT / 256; ++i) {
        const int c = mt + i * 256;
        const int sg = c % SEG, p = c / SEG;
        if constexpr (HEAD)
          *reinterpret_cast<uint2*>(Yf + ((p / (2 * WS_TW)) * Wo + p % (2 * WS_TW)) * Cres + sg * IE) = *reinterpret_cast<const uint2*>(ost + p * LDO + sg * IE);
        else
          *reinterpret_cast<uint4*>(Yf + ((p / (2 * WS_TW)) * Wo + p % (2 * WS_TW)) * Cres + sg * 8) = *reinterpret_cast<const uint4*>(ost + p * LDO + sg * 8);
      }
    };
    int tile = BX;
    prefetch(tile); commit(halo0);
    __syncthreads();
    int lt = 0, f, ty0, tx0, pf, pty, ptx;
    // first tile: no previous stage at its first step
    tile_coords(tile, f, ty0, tx0);
    prefetch(tile + GX);                           // loads fly for the whole tile
    __syncthreads();
    drain(ost0, f, ty0, tx0, 0);
    commit(halo1);
    pf = f; pty = ty0; ptx = tx0; lt = 1;
    __syncthreads();
    for (tile += GX; tile < ntiles; tile += GX, ++lt) {
      tile_coords(tile, f, ty0, tx0);
      prefetch(tile + GX);
      drain(ost0 + OST, pf, pty, ptx, 1);                 // stage of the previous tile's second step (odd q)
      __syncthreads();
      drain(ost0, f, ty0, tx0, 0);
      commit((lt & 1) ? halo0 : halo1);                   // the NEXT tile's buffer
      pf = f; pty = ty0; ptx = tx0;
      __syncthreads();
    }
    drain(ost0 + OST, pf, pty, ptx, 1);
    __syncthreads();
  } else {
    // ------------------------------------------------------------------ mover role
    uint4 pre[NCH];
    auto prefetch = [&](int tile) {
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
      const T* Xf = X + (long long)f * Hi * Wi * CIN;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = mt + i * 256;
        const int px = c / CPP, ch = (c % CPP) * 8;
        const int gy = ty0 + px / WS_HW - 1, gx = tx0 + px % WS_HW - 1;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (c < HPIX * CPP && gy >= 0 && gy < Hi && gx >= 0 && gx < Wi)
          v = *reinterpret_cast<const uint4*>(Xf + ((long long)gy * Wi + gx) * CIN + ch);
        pre[i] = v;
      }
    };
    auto commit = [&](T* halo) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = mt + i * 256;
        if (c < HPIX * CPP) *reinterpret_cast<uint4*>(halo + (c / CPP) * LDK + (c % CPP) * 8) = pre[i];
      }
    };
    constexpr int SEG = CT / 8;
    auto drain = [&](const T* ost, int f, int ty0, int tx0, int st) {
      T* Yf = Y + (long long)f * Ho * Wo * Cout;
      for (int c = mt; c < 2 * SR * 2 * WS_TW * SEG; c += 256) {
        const int sg = c % SEG, p = c / SEG;
        const int hr = p / (2 * WS_TW), hc = p % (2 * WS_TW);
        const int oy = 2 * ty0 + 2 * SR * st + hr, ox = 2 * tx0 + hc, co = n0 + sg * 8;
        if (oy < Ho && ox < Wo && co < Cout)
          *reinterpret_cast<uint4*>(Yf + ((long long)oy * Wo + ox) * Cout + co) = *reinterpret_cast<const uint4*>(ost + p * LDO + sg * 8);
      }
    };
    int tile = BX;
    if (tile < ntiles) { prefetch(tile); commit(halo0); }
    __syncthreads();
    int q = 0, pf = 0, pty = 0, ptx = 0, pst = 0;       // coordinates of the step whose stage is drained next
    bool have = false;
    for (; tile < ntiles; tile += GX) {
      const int nbuf = (((tile - BX) / GX) & 1) ^ 1;
      const int next = tile + GX;
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
#pragma unroll 1
      for (int st = 0; st < STEPS; ++st, ++q) {
        if (st == 0 && next < ntiles && !(dbg & 8)) prefetch(next);    // loads fly for the whole tile
        if (have && !(dbg & 4)) drain(ost0 + ((q - 1) & 1) * OST, pf, pty, ptx, pst);
        if (st == STEPS - 1 && next < ntiles && !(dbg & 8)) commit(nbuf ? halo1 : halo0);
        pf = f; pty = ty0; ptx = tx0; pst = st; have = true;
        __syncthreads();
      }
    }
    if (have) drain(ost0 + ((q - 1) & 1) * OST, pf, pty, ptx, pst);
    __syncthreads();
  }
}

template <typename T, int KS, int NF, bool EXACT>
static bool ws2_launch_t(const void* X, const void* Wf, const float* bias, void* Y, int F, int Hi, int Wi, int Cout, hipStream_t st) {
  constexpr int CT = NF * 16, lds = Ws2Geo<KS, NF, false>::LDS_BYTES;
  if (!stj_reserve_lds<upconv_fwd_ws2_kernel<T, KS, NF, EXACT>>(lds)) return false;
  const int ntiles = ((Wi + WS_TW - 1) / WS_TW) * ((Hi + WS_TH - 1) / WS_TH) * F;
  const int ct = (Cout + CT - 1) / CT;
  int nblk = 256 / ct;
  if (nblk > ntiles) nblk = ntiles;
  if (nblk < 1) nblk = 1;
  const int dbg = 0;      // (role-ablation mask of the kernel; profiling builds only)
  if constexpr (NF == 2) {
    // three cout groups of 32 (the 128 -> 96 layer): 1-D grid, the groups of a walker on one XCD (XCT = 3); walkers a multiple of 8
    int nw = 256 / 3 / 8 * 8;                          // 80 walkers x 3 groups = 240 workgroups
    while (nw > 8 && nw - 8 >= ntiles) nw -= 8;
    // The straight-line movers (EXACT) drain their walker's first tile without asking whether it exists: a walker past the last tile
    // (ntiles no multiple of 8 and below 80) would store one step of stage beyond Y.  Such a shape takes the 2-D grid, whose walkers
    // all have a tile; the guarded movers test every tile.
    if (ct == 3 && ntiles >= 8 && (!EXACT || nw <= ntiles)) {
      if (!stj_reserve_lds<upconv_fwd_ws2_kernel<T, KS, NF, EXACT, false, 3>>(lds)) return false;
      hipLaunchKernelGGL((upconv_fwd_ws2_kernel<T, KS, NF, EXACT, false, 3>), dim3(nw * 3), dim3(512), lds, st, (const T*)X, (const T*)Wf, bias, (T*)Y, F, Hi, Wi, Cout,
                         ntiles, dbg, (const float*)nullptr);
      return true;
    }
  }
  hipLaunchKernelGGL((upconv_fwd_ws2_kernel<T, KS, NF, EXACT>), dim3(nblk, ct), dim3(512), lds, st, (const T*)X, (const T*)Wf, bias, (T*)Y, F, Hi, Wi, Cout, ntiles, dbg,
                     (const float*)nullptr);
  return true;
}
// the 96 -> 48 level with the 48 -> 2 head's channel projection in its epilogue: Z [F, 2 Hi, 2 Wi, STJ_HEAD_CZ] instead of Y (whole tiles only)
template <typename T>
static bool ws2_head_launch(const void* X, const void* Wf, const float* bias, const float* Wh, void* Z, int F, int Hi, int Wi, hipStream_t st) {
  constexpr int KS = 3, NF = 3, CT = NF * 16, lds = Ws2Geo<KS, NF, true>::LDS_BYTES;
  if (!stj_reserve_lds<upconv_fwd_ws2_kernel<T, KS, NF, true, true>>(lds)) return false;
  const int ntiles = (Wi / WS_TW) * (Hi / WS_TH) * F;
  const int nblk = ntiles < 256 ? ntiles : 256;
  hipLaunchKernelGGL((upconv_fwd_ws2_kernel<T, KS, NF, true, true>), dim3(nblk, 1), dim3(512), lds, st, (const T*)X, (const T*)Wf, bias, (T*)Z, F, Hi, Wi, CT, ntiles, 0, Wh);
  return true;
}
bool upconv_fwd_head_try(const void* X, const void* Wf, const float* bias, const float* Wh, void* Z, int F, int Hi, int Wi, int Cin, int Cout, int dtype,
                         hipStream_t st) {
  if (Cin != 96 || Cout != 48 || Hi % WS_TH || Wi % WS_TW) return false;
  bool took = false;
  return stj_with_dtype16(dtype, [&](auto t) { took = ws2_head_launch<typename decltype(t)::type>(X, Wf, bias, Wh, Z, F, Hi, Wi, st); }) && took;
}
template <typename T, int KS, int NF>
static bool ws2_launch(const void* X, const void* Wf, const float* bias, void* Y, int F, int Hi, int Wi, int Cout, hipStream_t st) {
  if (Hi % WS_TH == 0 && Wi % WS_TW == 0 && Cout % (NF * 16) == 0)      // whole tiles: straight-line movers (ragged ones: the guarded form)
    return ws2_launch_t<T, KS, NF, true>(X, Wf, bias, Y, F, Hi, Wi, Cout, st);
  return ws2_launch_t<T, KS, NF, false>(X, Wf, bias, Y, F, Hi, Wi, Cout, st);
}

// returns true when the weight-stationary kernel handles this shape (bf16 / fp16, Cin in {96,128}, Cout multiple of 8)
template <typename T>
static bool upconv_fwd_ws_try_t(const void* X, const void* Wf, const float* bias, void* Y, int F, int Hi, int Wi, int Cin, int Cout, int act,
                       hipStream_t st) {
  if (Cout % 8 || act != ACT_ELU) return false;
  // Cin = 96 and, since round 6, Cin = 128: the wave-specialised kernel (compute + mover waves).  In round 2 the 128 -> 96 layer measured
  // 139 (wave-specialised) vs 142 us (one role, eight waves that each prefetch, compute, commit and store) and kept the one-role kernel;
  // with the halo-row-major fragment order and the 6-deep ring the wave-specialised form runs it in 126-132 us against 147-153
  // (profiles/r06_z6_ws2_for_128.txt; ring 4 / 8 / 10 deep: 135 / 128 / 127), inference +0.5-1.2 % in alternating same-box runs
  // (profiles/r06_z7_ws2_for_128_step.txt).  The one-role kernel is gone with it; what was tried on it in round 6 and bought nothing:
  // every halo row read once (40 instead of 64 fragment reads per tile: 147 / 141 vs 144 / 147 us), the row-major order with a 2-8 deep
  // ring (153-158 vs 156): its waves waited in their prefetch / commit / store phases, not on fragments (profiles/r06_y_*, r06_z5_*).
  if (Cin == 96) return ws2_launch<T, 3, 3>(X, Wf, bias, Y, F, Hi, Wi, Cout, st);
  if (Cin == 128) return ws2_launch<T, 4, 2>(X, Wf, bias, Y, F, Hi, Wi, Cout, st);
  return false;
}
bool upconv_fwd_ws_try(const void* X, const void* Wf, const float* bias, void* Y, int F, int Hi, int Wi, int Cin, int Cout, int act,
                       int dtype, hipStream_t st) {
  bool took = false;
  return stj_with_dtype16(dtype, [&](auto t) { took = upconv_fwd_ws_try_t<typename decltype(t)::type>(X, Wf, bias, Y, F, Hi, Wi, Cin, Cout, act, st); }) && took;
}

// =====================================================================================================
// Weight gradient, v2 (bf16): output-stationary, both operands read with ds_read_b64_tr_b16.
//   dWeff[a,b,r,s][co][ci] = sum_{f,i,j} dP[f,2i+a,2j+b,co] * X[f,i+a-1+r,j+b-1+s,ci]
// MFMA view: D[m=co][n=ci] += A[m][k=pixel] B[k=pixel][n].  Both operands have the contraction (pixel) axis as the
// SLOW axis of their natural [pixel][channel] LDS tiles; the gfx950 LDS transpose read delivers, per lane (channel
// l&15), 4 consecutive pixels -- two of them form one 16x16x32 fragment (probe: tools/probes/tr16_probe.hip).
// The v1 kernel assembled fragments from 8 ds_read_u16 each and was LDS-bound (PMC: LDS active 184M cycles,
// 45 % conflicts vs 151M MFMA-busy cycles).  One block = (pixel strip, output phase, cout tile x cin tile), one wave =
// one of the phase's 4 taps; chunks of 4 low-res rows x 32 columns per barrier pair, next chunk prefetched in registers.
// =====================================================================================================
typedef __attribute__((ext_vector_type(4))) short ws_s16x4;
__device__ __forceinline__ ws_s16x4 lds_tr16(const bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ws_s16x4*)(p));
}
__device__ __forceinline__ s16x8 tr_frag(const bf16* p0, const bf16* p1) {
  const ws_s16x4 lo = lds_tr16(p0), hi = lds_tr16(p1);
  return (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// chunk = CR rows x CW columns of low-res pixels with CR * CW = 128; CW = 32 (wide layers) or 16 (the 16x16 bottleneck layer)
template <int FO, int FI, int CW>
__global__ __launch_bounds__(256, 2) void upconv_wgrad_tr_kernel(const bf16* __restrict__ X, const bf16* __restrict__ dP,
                                                              float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin,
                                                              int Cout, int chunks_per_block, int nstrips, int ntiles) {
  constexpr int WG2_W = CW, WG2_ROWS = 128 / CW, KROWS = 32 / CW;      // KROWS: chunk rows per 32-pixel k-step
  constexpr int BO = FO * 16, BI = FI * 16;
  // Row strides of the two [pixel][channel] images: 16 * odd elements = 8 * odd dwords.  A 32-lane pass of ds_read_b64_tr_b16 reads 8
  // pixels x 32 bytes; with the k-permutation below those are 8 CONSECUTIVE pixels, and a stride of 8 * odd dwords spreads them over
  // the 8 disjoint 8-bank groups: conflict-free (the strides BO + 8 / BI + 8 with pixels {0..3, 8..11} per pass measured 41-47 % conflict
  // cycles, profiles/r03_h_pmc_step.txt).
  constexpr int LDO = (BO / 16) % 2 ? BO : BO + 16, LDI = (BI / 16) % 2 ? BI : BI + 16;
  static_assert((LDO / 16) % 2 == 1 && (LDI / 16) % 2 == 1 && LDO % 16 == 0 && LDI % 16 == 0, "row strides must be 16 * odd elements");
  constexpr int XW = WG2_W + 2, XR = WG2_ROWS + 1;
  constexpr int NPX = WG2_ROWS * WG2_W;
  constexpr int DY_CH = NPX * (BO / 8), X_CH = XR * XW * (BI / 8);
  constexpr int NCH = (DY_CH + X_CH + 255) / 256;
  __shared__ __attribute__((aligned(16))) bf16 dYs[NPX * LDO];
  __shared__ __attribute__((aligned(16))) bf16 Xs[XR * XW * LDI];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // XCD-aware work map (1-D grid): workgroup L runs on XCD L % 8 (round-robin dispatch); the 4 output phases and the channel
  // tiles of ONE pixel strip read the same X rows and the same dP cache lines, so they get consecutive slots of the SAME
  // XCD and share them through that XCD's L2.  Before (phase = blockIdx.y): 1.68 GB fetched per launch for 0.60 GB of
  // operands (rocprofv3 FETCH_SIZE, profiles/r01_e_pmc_conv.txt) -- every phase streamed X and both dP column parities again.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int inner = 4 * ntiles;
  const int strip = (slot / inner) * 8 + xcd, phase = (slot % inner) & 3, ctile = (slot % inner) >> 2;
  if (strip >= nstrips) return;
  const int a = phase >> 1, b = phase & 1;
  const int r = w >> 1, s = w & 1;
  const int g = lane >> 4, p = lane & 15;
  const int cin_tiles = (Cin + BI - 1) / BI;
  const int co0 = (ctile / cin_tiles) * BO, ci0 = (ctile % cin_tiles) * BI;
  const int segs = Wi / WG2_W, rgs = Hi / WG2_ROWS;
  const int nchunks = F * rgs * segs;              // 32-bit on purpose: the per-chunk div / mod below is not free in 64 bits
  const int c_begin = strip * chunks_per_block;
  const int c_end = min(nchunks, c_begin + chunks_per_block);
  const int Ho = 2 * Hi, Wo = 2 * Wi;

  f32x4 acc[FO][FI];
#pragma unroll
  for (int m = 0; m < FO; ++m)
#pragma unroll
    for (int n = 0; n < FI; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // bias gradient db[co] = sum over pixels of dP[.., co]: the A fragments (m = co, k = pixel) are already in registers, so wave 0
  // of the blocks of the first cin tile multiplies them with an all-ones B fragment -- FO extra MFMAs per k-step on a matrix pipe
  // that is ~20 % busy -- instead of 32 dependent 2-byte LDS reads per chunk (that loop + the atomics below were 16 % of the
  // kernel).  Every column n of D then holds the row sums.
  const bool do_db = dbias != nullptr && ci0 == 0 && w == 0;
  f32x4 dbf[FO];
#pragma unroll
  for (int m = 0; m < FO; ++m) dbf[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const s16x8 ones = (s16x8){0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};      // bf16 1.0

  uint4 pre[NCH];
  auto prefetch = [&](int c) {
    const int seg = c % segs, t = c / segs;
    const int i0 = (t % rgs) * WG2_ROWS, f = t / rgs;
    const int j0 = seg * WG2_W;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int q = tid + u * 256;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q < DY_CH) {
        const int px = q / (BO / 8), ch = (q % (BO / 8)) * 8;
        const int ri = px / WG2_W, cj = px % WG2_W;
        if (co0 + ch < Cout)
          v = *reinterpret_cast<const uint4*>(dP + (((long long)f * Ho + 2 * (i0 + ri) + a) * Wo + 2 * (j0 + cj) + b) * Cout + co0 + ch);
      } else if (q < DY_CH + X_CH) {
        const int q2 = q - DY_CH;
        const int px = q2 / (BI / 8), ch = (q2 % (BI / 8)) * 8;
        const int gy = i0 + a - 1 + px / XW, gx = j0 + b - 1 + px % XW;
        if (gy >= 0 && gy < Hi && gx >= 0 && gx < Wi && ci0 + ch < Cin)
          v = *reinterpret_cast<const uint4*>(X + (((long long)f * Hi + gy) * Wi + gx) * Cin + ci0 + ch);
      }
      pre[u] = v;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int q = tid + u * 256;
      if (q < DY_CH) *reinterpret_cast<uint4*>(dYs + (q / (BO / 8)) * LDO + (q % (BO / 8)) * 8) = pre[u];
      else if (q < DY_CH + X_CH) { const int q2 = q - DY_CH; *reinterpret_cast<uint4*>(Xs + (q2 / (BI / 8)) * LDI + (q2 % (BI / 8)) * 8) = pre[u]; }
    }
  };

  if (c_begin < c_end) { prefetch(c_begin); commit(); }
  __syncthreads();
  // per-lane tr-read bases: lane p of group g addresses pixel (4g + p/4 [+16]) of the 32-pixel k-step and channels 4*(p%4).. of a
  // 16-channel block.  (Which 8 of the 32 pixels a lane group contributes is free as long as both operands agree: the MFMA sums
  // over k.  Pixels 4g .. 4g+3 and 16+4g .. make every 32-lane pass read 8 consecutive pixels.)
  const int kpx = 4 * g + (p >> 2), kch = 4 * (p & 3);
  constexpr int XHI = CW == 32 ? 16 * LDI : XW * LDI;          // + 16 pixels: same row (CW = 32) or the next chunk row (CW = 16)
  for (int c = c_begin; c < c_end; ++c) {
    if (c + 1 < c_end) prefetch(c + 1);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {              // k-step rr = pixels 32 rr .. 32 rr + 31 of the chunk (row-major)
      s16x8 af[FO], bfr[FI];
      const bf16* ab = dYs + (rr * 32 + kpx) * LDO + kch;
#pragma unroll
      for (int m = 0; m < FO; ++m) af[m] = tr_frag(ab + m * 16, ab + 16 * LDO + m * 16);
      const bf16* bb = Xs + ((rr * KROWS + r) * XW + kpx + s) * LDI + kch;
#pragma unroll
      for (int n = 0; n < FI; ++n) bfr[n] = tr_frag(bb + n * 16, bb + XHI + n * 16);
#pragma unroll
      for (int m = 0; m < FO; ++m)
#pragma unroll
        for (int n = 0; n < FI; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[m]), __builtin_bit_cast(bf16x8_t, bfr[n]), acc[m][n], 0, 0, 0);
      if (do_db) {
#pragma unroll
        for (int m = 0; m < FO; ++m)
          dbf[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[m]), __builtin_bit_cast(bf16x8_t, ones), dbf[m], 0, 0, 0);
      }
    }
    __syncthreads();
    if (c + 1 < c_end) commit();
    __syncthreads();
  }
  if (do_db && p == 0) {               // column n = 0: lane g holds rows m*16 + 4g + 0..3.  The blocks spread over db_parts copies
    float* dbp = dbias + (long long)(blockIdx.x % db_parts) * Cout;
#pragma unroll
    for (int m = 0; m < FO; ++m)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = co0 + m * 16 + g * 4 + rg;
        if (co < Cout) atomicAdd(dbp + co, dbf[m][rg]);
      }
  }
  const int pt = a * 8 + b * 4 + r * 2 + s;
#pragma unroll
  for (int m = 0; m < FO; ++m)
#pragma unroll
    for (int n = 0; n < FI; ++n) {
      const int ci = ci0 + n * 16 + p;
      if (ci >= Cin) continue;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = co0 + m * 16 + g * 4 + rg;
        if (co < Cout) atomicAdd(dWeff + ((long long)pt * Cout + co) * Cin + ci, acc[m][n][rg]);
      }
    }
}

// Weight gradient, v3: BOTH column parities of a row parity in one 512-thread workgroup.  In the kernel above a workgroup is
// (strip, phase, channel tile): the four phase blocks of a chunk each stage the same X halo (33 of their 45 KB) and their own quarter
// of dP, 1.47 GB of L1 fills per launch of the 96 -> 48 layer = 5.8 TB/s through L2 at 253 us -- the L2 -> L1 ceiling the 64 x 64 GEMM
// tiles run into as well.  Here a workgroup is (strip, row parity a, channel tile) and wave w = (column parity b = w >> 2, tap w & 3):
// X (CR + 1 rows) and the CR hi-res dP rows of parity a are staged once for both b (114 instead of 180 KB per chunk and row-parity
// pair of the 96 -> 48 layer); every wave reads its own column parity / tap through its transpose-read addresses.  (All four phases in
// one 1024-thread workgroup would stage 82 KB, but at 128 VGPRs per lane the 72 accumulator registers leave no room for the
// register-staged prefetch: 140-196 bytes of scratch per lane.)
// LDS layout of upconv_wgrad_tr4_kernel (bf16): TWO stages of BUF elements, each the dP image [CR][2 CW][LDO] and then the X image
// [CR + 1][CW + 2][LDI]; the strides are explained where the kernel takes them
template <int FO, int FI, int CW, int NPIX>
struct WgradTr4Geo {
  static constexpr int CR = NPIX / CW, BO = FO * 16, BI = FI * 16;
  static constexpr int LDO = BO + 8, LDI = (BI / 16) % 2 ? BI : BI + 16;
  static constexpr int YW = 2 * CW, YR = CR, XW = CW + 2, XR = CR + 1;
  static constexpr int BUF = YR * YW * LDO + XR * XW * LDI;
  static constexpr int LDS_BYTES = 2 * BUF * 2;
  static_assert(LDS_BYTES <= 160 * 1024, "the layout fits the CU's LDS");
};
template <int FO, int FI, int CW, int NPIX>
__global__ __launch_bounds__(512, 2) void upconv_wgrad_tr4_kernel(const bf16* __restrict__ X, const bf16* __restrict__ dP,
                                                                  float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin,
                                                                  int Cout, int chunks_per_block, int nstrips, int ntiles) {
  using G = WgradTr4Geo<FO, FI, CW, NPIX>;
  constexpr int CR = G::CR, KROWS = 32 / CW;              // NPIX low-res pixels per barrier pair (NPIX / 32 k-steps)
  constexpr int BO = G::BO, BI = G::BI;
  // row strides: consecutive low-res pixels lie 2 hi-res columns = LDO dwords apart in the dP image and LDI / 2 dwords apart in the X
  // image; both 8 * odd dwords, so the 8 consecutive pixels of a 32-lane transpose-read pass (k-permutation below) hit disjoint banks
  constexpr int LDO = G::LDO, LDI = G::LDI;
  static_assert((LDO / 8) % 2 == 1 && (LDI / 16) % 2 == 1 && LDI % 16 == 0, "conflict-free transpose-read strides");
  constexpr int YW = G::YW, YR = G::YR, XW = G::XW, XR = G::XR;
  constexpr int DY_CH = YR * YW * (BO / 8), X_CH = XR * XW * (BI / 8);
  constexpr int NCH = (DY_CH + X_CH + 511) / 512;
  extern __shared__ __attribute__((aligned(16))) unsigned char w4_smem[];
  constexpr int BUF = G::BUF;                              // elements of one stage; TWO stages: the next chunk is written while this one
  bf16* dYs = reinterpret_cast<bf16*>(w4_smem);            // is read -- one barrier per chunk.  [CR][2 CW][LDO]: hi-res dP rows 2 (i0 + ri) + a
  bf16* Xs = dYs + YR * YW * LDO;                          // [CR + 1][CW + 2][LDI]: X rows i0 + a - 1 .., columns j0 - 1 ..

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int inner = 2 * ntiles;
  const int strip = (slot / inner) * 8 + xcd, a = (slot % inner) & 1, ctile = (slot % inner) >> 1;      // same strip: same XCD, adjacent slots
  if (strip >= nstrips) return;
  const int b = w >> 2;
  const int r = (w >> 1) & 1, s = w & 1;
  const int g = lane >> 4, p = lane & 15;
  const int cin_tiles = (Cin + BI - 1) / BI;
  const int co0 = (ctile / cin_tiles) * BO, ci0 = (ctile % cin_tiles) * BI;
  const int segs = Wi / CW, rgs = Hi / CR;
  const int nchunks = F * rgs * segs;
  const int c_begin = strip * chunks_per_block;
  const int c_end = min(nchunks, c_begin + chunks_per_block);
  const int Ho = 2 * Hi, Wo = 2 * Wi;

  f32x4 acc[FO][FI];
#pragma unroll
  for (int m = 0; m < FO; ++m)
#pragma unroll
    for (int n = 0; n < FI; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bool do_db = dbias != nullptr && ci0 == 0 && (w & 3) == 0;         // one wave per phase sums its quarter of the pixels
  f32x4 dbf[FO];
#pragma unroll
  for (int m = 0; m < FO; ++m) dbf[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const s16x8 ones = (s16x8){0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  // this thread's staging chunks (geometry independent of the pixel chunk)
  int soff[NCH], slds[NCH], sryx[NCH];
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int q = tid + u * 512;
    if (q < DY_CH) {
      const int px = q / (BO / 8), ch = (q % (BO / 8)) * 8;
      const int ry = px / YW, rx = px % YW;
      soff[u] = ((2 * ry + a) * Wo + rx) * Cout + co0 + ch;
      slds[u] = (co0 + ch < Cout) ? px * LDO + ch : -1;
      sryx[u] = 0x40000000;                                               // dP chunk: always inside the image
    } else if (q < DY_CH + X_CH) {
      const int q2 = q - DY_CH;
      const int px = q2 / (BI / 8), ch = (q2 % (BI / 8)) * 8;
      const int ry = px / XW + a - 1, rx = px % XW - 1;
      soff[u] = (ry * Wi + rx) * Cin + ci0 + ch;
      slds[u] = (ci0 + ch < Cin) ? YR * YW * LDO + px * LDI + ch : -1;
      sryx[u] = (ry & 0xff) | ((rx & 0xffff) << 8);
    } else {
      soff[u] = 0; slds[u] = -1; sryx[u] = 0x40000000;
    }
  }
  uint4 pre[NCH];
  bool pin[NCH];
  auto prefetch = [&](int c) {
    const int seg = c % segs, t = c / segs;
    const int i0 = (t % rgs) * CR, f = t / rgs;
    const int j0 = seg * CW;
    const bf16* Pt = dP + (((long long)f * Ho + 2 * i0) * Wo + 2 * j0) * Cout;
    const bf16* Xt = X + (((long long)f * Hi + i0) * Wi + j0) * Cin;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const bool isx = !(sryx[u] & 0x40000000);
      const int gy = i0 + (signed char)(sryx[u] & 0xff), gx = j0 + (short)((sryx[u] >> 8) & 0xffff);
      pin[u] = slds[u] >= 0 && (!isx || ((unsigned)gy < (unsigned)Hi && (unsigned)gx < (unsigned)Wi));
      const bf16* src = isx ? Xt : Pt;
      pre[u] = *reinterpret_cast<const uint4*>(src + (pin[u] ? soff[u] : 0));      // unconditional (chunk origins are inside the image)
    }
  };
  auto commit = [&](int bo) {
#pragma unroll
    for (int u = 0; u < NCH; ++u)
      if (slds[u] >= 0) *reinterpret_cast<uint4*>(dYs + bo + slds[u]) = pin[u] ? pre[u] : make_uint4(0, 0, 0, 0);
  };
  // (Round 6: a SECOND register set, so that the chunk after next is in flight while this one is computed -- a chunk's loads then have a whole
  //  chunk period to land: 128-pixel chunks spill (588 us); 64-pixel chunks, one k-step unrolled: 334 us against 270 for 64-pixel chunks with one
  //  set and 240 for this kernel: the staging is not waiting on its prefetch distance.  profiles/r06_zf_tr4_deep_prefetch.txt.  The k-steps
  //  software-pipelined inside the wave -- the next k-step's 18 transpose reads under this one's 18 MFMAs, two fragment sets, 222 registers --:
  //  242 / 246 / 245 us against 244 / 246 / 242: the SIMD's other wave already covers the reads.  profiles/r06_zg_tr4_swp.txt)
  if (c_begin < c_end) { prefetch(c_begin); commit(0); }
  __syncthreads();
  const int kpx = 4 * g + (p >> 2), kch = 4 * (p & 3);        // pixels 4g + p/4 and 16 + 4g + p/4 of a 32-pixel k-step (see upconv_wgrad_tr_kernel)
  const int krow = 0, kcol = kpx;
  constexpr int XHI = CW == 32 ? 16 * LDI : XW * LDI;          // + 16 pixels: same row (CW = 32) or the next chunk row (CW = 16)
  for (int c = c_begin; c < c_end; ++c) {
    const int bo = ((c - c_begin) & 1) * BUF;
    if (c + 1 < c_end) prefetch(c + 1);
#pragma unroll 4
    for (int rr = 0; rr < NPIX / 32; ++rr) {              // k-step rr = low-res pixels 32 rr .. 32 rr + 31 of the chunk (row-major)
      s16x8 af[FO], bfr[FI];
      const bf16* ab = dYs + bo + ((rr * KROWS + krow) * YW + 2 * kcol + b) * LDO + kch;               // this wave's column parity
#pragma unroll
      for (int m = 0; m < FO; ++m) af[m] = tr_frag(ab + m * 16, ab + 32 * LDO + m * 16);         // + 16 low-res pixels = + 32 hi-res columns (CW = 16: = the next row, YW = 32)
      const bf16* bb = Xs + bo + ((rr * KROWS + krow + r) * XW + kcol + b + s) * LDI + kch;
#pragma unroll
      for (int n = 0; n < FI; ++n) bfr[n] = tr_frag(bb + n * 16, bb + XHI + n * 16);
#pragma unroll
      for (int m = 0; m < FO; ++m)
#pragma unroll
        for (int n = 0; n < FI; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[m]), __builtin_bit_cast(bf16x8_t, bfr[n]), acc[m][n], 0, 0, 0);
      if (do_db) {
#pragma unroll
        for (int m = 0; m < FO; ++m)
          dbf[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[m]), __builtin_bit_cast(bf16x8_t, ones), dbf[m], 0, 0, 0);
      }
    }
    if (c + 1 < c_end) commit(BUF - bo);                  // the other stage: last read one barrier ago
    __syncthreads();
  }
  if (do_db && p == 0) {
    float* dbp = dbias + (long long)((blockIdx.x * 2 + b) % db_parts) * Cout;
#pragma unroll
    for (int m = 0; m < FO; ++m)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = co0 + m * 16 + g * 4 + rg;
        if (co < Cout) atomicAdd(dbp + co, dbf[m][rg]);
      }
  }
  const int pt = a * 8 + b * 4 + r * 2 + s;
#pragma unroll
  for (int m = 0; m < FO; ++m)
#pragma unroll
    for (int n = 0; n < FI; ++n) {
      const int ci = ci0 + n * 16 + p;
      if (ci >= Cin) continue;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int co = co0 + m * 16 + g * 4 + rg;
        if (co < Cout) atomicAdd(dWeff + ((long long)pt * Cout + co) * Cin + ci, acc[m][n][rg]);
      }
    }
}

// Workgroup budget of the two large weight-gradient launches (an argument of stj_upconv_wgrad): 128 (half the CUs) for a step whose
// branches run concurrently, 256 when every kernel runs alone (serial mode).
template <int FO, int FI, int CW, int NPIX>
static bool wgrad_tr4_launch(const void* X, const void* dP, float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin, int Cout,
                             int tiles, int wg_budget, hipStream_t st) {
  constexpr int CR = NPIX / CW, lds = WgradTr4Geo<FO, FI, CW, NPIX>::LDS_BYTES;
  if (!stj_reserve_lds<upconv_wgrad_tr4_kernel<FO, FI, CW, NPIX>>(lds)) return false;
  const long long nchunks = (long long)F * (Hi / CR) * (Wi / CW);
  // Workgroups: HALF the CUs.  Alone the kernel is faster with one workgroup per CU (246 vs 344 us for the 96 -> 48 layer), but the
  // decoder's weight gradients are deferred (ops.py) and run next to the backward of the cross-attentions / FG-MSA / the encoder, chains
  // of short launches that then find the other half of the CUs free: 1085 -> 1130 scenes/s (256 -> 128 workgroups; 192: 1116, 96: 1121,
  // 64: 1131, 32: 842)
  const int budget = wg_budget > 0 ? wg_budget : 128;
  int strips = (int)min(nchunks, (long long)max(1, budget / (2 * tiles)));   // x 2 row parities x tiles workgroups
  const int cpb = (int)((nchunks + strips - 1) / strips);
  strips = (int)((nchunks + cpb - 1) / cpb);
  hipLaunchKernelGGL((upconv_wgrad_tr4_kernel<FO, FI, CW, NPIX>), dim3((strips + 7) / 8 * 8 * 2 * tiles), dim3(512), lds, st, (const bf16*)X, (const bf16*)dP,
                     dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, cpb, strips, tiles);
  return true;
}

// returns true when handled (bf16; Wi % 32 == 0 and Hi % 4 == 0, or Wi % 16 == 0 and Hi % 8 == 0; channels % 8 == 0)
template <int CW>
static bool wgrad_tr_launch(const void* X, const void* dP, float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin, int Cout, int wg_budget, hipStream_t st) {
  constexpr int CR = 128 / CW;
  const long long nchunks = (long long)F * (Hi / CR) * (Wi / CW);
  // (the two large layers only: at 32 x 32 and below a strip has too few chunks to amortise a 512-thread workgroup: 149 vs 113 us;
  //  128-pixel chunks: with 256 the register-staged prefetch spills)
  if (Hi % (256 / CW) == 0 && nchunks >= 2048) {
    if (Cout <= 48 && Cin <= 96) return wgrad_tr4_launch<3, 6, CW, 128>(X, dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, 1, wg_budget, st);
    // 128 -> 96: ALL 96 couts x 64 cins per workgroup (24 accumulator fragments per wave).  As 64 x 64 channel tiles the layer is 4 tiles,
    // the second cout tile half empty: every X slice staged twice, every dP slice twice, a quarter of the MFMAs on zero rows.
    // (B = 8, 64 x 64: 153 vs 188 us alone on the GPU)
    if (Cout == 96 && Cin % 64 == 0) return wgrad_tr4_launch<6, 4, CW, 128>(X, dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, Cin / 64, wg_budget, st);
    return wgrad_tr4_launch<4, 4, CW, 128>(X, dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, ((Cout + 63) / 64) * ((Cin + 63) / 64), wg_budget, st);
  }
  if (Cout <= 48 && Cin <= 96) {
    int strips = (int)min(nchunks, (long long)256);     // 128 and 512 measured within noise / slower
    const int cpb = (int)((nchunks + strips - 1) / strips);
    strips = (int)((nchunks + cpb - 1) / cpb);
    hipLaunchKernelGGL((upconv_wgrad_tr_kernel<3, 6, CW>), dim3((strips + 7) / 8 * 8 * 4), dim3(256), 0, st, (const bf16*)X, (const bf16*)dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, cpb, strips, 1);
  } else {
    const int tiles = ((Cout + 63) / 64) * ((Cin + 63) / 64);
    // workgroups (swept again in round 5, after the accumulation buffers' alignment fix: 256 / 512 / 768 / 1536 / 2048 = 209 / 110 / 123 / 124 /
    // 136 us for 384 -> 192 and 152 / 137 / 112 / 130 / 139 for 192 -> 128, against 111 / 113 for 1024; full-cout x 64-cin tiles (<6,4> / <8,4>:
    // 20 / 183 spilled registers at two workgroups per CU) 132-157 / 248-290 us).  Inside the step (same-box A/B, two boxes): 512 workgroups for
    // 384 -> 192 gave 1351-1353 vs 1330-1338 scenes/s on one box and 1332-1337 vs 1343-1348 on the other; 384 / 448 / 576 and 896 / 1280 / 1536
    // for 192 -> 128 inside the noise or below: 1024 stays)
    const int tgt = 1024;
    int strips = (int)min(nchunks, (long long)max(1, tgt / (4 * tiles)));
    const int cpb = (int)((nchunks + strips - 1) / strips);
    strips = (int)((nchunks + cpb - 1) / cpb);
    hipLaunchKernelGGL((upconv_wgrad_tr_kernel<4, 4, CW>), dim3((strips + 7) / 8 * 8 * 4 * tiles), dim3(256), 0, st, (const bf16*)X, (const bf16*)dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, cpb, strips, tiles);
  }
  return true;
}
bool upconv_wgrad_tr_try(const void* X, const void* dP, float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin, int Cout, int wg_budget, hipStream_t st) {
  if (Cin % 8 || Cout % 8) return false;
  if (Wi % 32 == 0 && Hi % 4 == 0) return wgrad_tr_launch<32>(X, dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, wg_budget, st);
  if (Wi % 16 == 0 && Hi % 8 == 0) return wgrad_tr_launch<16>(X, dP, dWeff, dbias, db_parts, F, Hi, Wi, Cin, Cout, wg_budget, st);
  return false;
}

// =====================================================================================================
// Output heads on MFMA (bf16): Conv2D 3x3 SAME 48 -> 2 (reference modules.py:767-770) written straight into the
// [B,H,W,32] f32 result, and its backward.  N = 2 is far too narrow for a GEMM tile, so the 2 output channels ride in
// rows 0..1 of a 16-row MFMA A operand that stays in registers (9 taps x (one 16x16x32 + one 16x16x16 step = 48
// channels exactly)); pixels are the N dimension and come from an 18x18 halo tile in LDS.  HBM-bound by design:
// 403 MB read per head at B=8.  The first (VALU) version ran at 0.48 ms fwd / 1.2 ms bwd per head (profiles/r01_b_*).
// =====================================================================================================
#define OCM_T 16
#define OCM_H 18
// Work index -> (tile column, tile row, frame).  The 8 waypoint frames of one scene write / read the SAME 128-byte lines of the
// [B,H,W,32] f32 tensor (a frame owns 8 bytes of each line).  Enumerated frame-major, those 8 frames ran on 8 different XCDs at
// unrelated times: rocprofv3 (profiles/r02_b_pmc_step.txt) counted 1080 MB fetched by the backward kernel for 420 MB of operands and
// 134 MB written by the forward one for 17 MB of results -- every frame pulled / pushed whole lines through its own L2.  Work items are
// dealt to the XCDs round-robin (index % 8), so the 8 frames of a spatial tile get indices c + 8 t + 64 u (same XCD c, adjacent in
// time): the lines are fetched once per tile into ONE L2 and the 8 partial writes merge there.
__device__ __forceinline__ void oc_decode(int i, int tiles_x, int tiles_y, int F, int inner, long long s_outer, long long s_inner,
                                          int& tx, int& ty, int& f) {
  const bool time_outer = s_outer < s_inner;                 // which component of f = outer * inner + in is the waypoint index
  const int nt = time_outer ? F / inner : inner, nb = F / nt;
  const int S = nb * tiles_x * tiles_y;
  int sp, t;
  if (nt == 8 && (S & 7) == 0) { const int c = i & 7, u = i >> 6; t = (i >> 3) & 7; sp = c + 8 * u; }
  else { t = i % nt; sp = i / nt; }
  tx = sp % tiles_x;
  const int s2 = sp / tiles_x;
  ty = s2 % tiles_y;
  const int b = s2 / tiles_y;
  f = time_outer ? t * inner + b : b * inner + t;
}
// v2 of the forward head (round 2).  The kernel above reads one LDS fragment pair per (output row, tap): 72 ds_read_b128 and 72
// MFMAs per wave and tile, of which 14 of 16 MFMA rows multiply zeros -- 288 KB of LDS reads per 31 KB tile, and LDS, not HBM, set its
// pace (2.2 us per tile and CU where the fragment reads alone need 1 us; profiles/r02_c_pmc_step.txt: 51 % of HBM peak).  Here the
// vertical taps move into the M dimension: A row m = 2 dy + o (6 of 16 rows), one A fragment pair per horizontal tap dx; a halo row is
// read once per dx (3 fragment pairs) and yields its contributions to the THREE output rows it touches (row - dy), which a lane
// accumulates in registers: 36 reads and 36 MFMAs per wave and tile.  The dy = 2 contributions sit in the lanes of group g = 1 and are
// added to those of g = 0 with one cross-lane move per output value.  Halo loads are unconditional (clamped address, zeroed on the
// way to LDS): no branch per 16-byte chunk.
template <typename T, int C>
__global__ __launch_bounds__(256, 3) void outconv_fwd_mfma2_kernel(const T* __restrict__ X, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, float* __restrict__ Y, int F, int Hh,
                                                                   int Ww, int Tn, long long y_bs, long long y_ts, long long y_ps, int dbg) {
  static_assert(C == 48, "specialised for 48 input channels (32 + 16)");
  constexpr int LDH = C + 32;                      // 160-byte pixels: conflict-free b128 fragment reads
  constexpr int CPP = C / 8, NCH = (OCM_H * OCM_H * CPP + 255) / 256;
  __shared__ __attribute__((aligned(16))) T halo[OCM_H * OCM_H * LDH + 64];   // pads + tail stay zero (read by the padded 2nd k-step)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ln = lane & 15;
  // stationary weights: A row m = ln = 2 dy + o (m < 6), one fragment pair per horizontal tap dx
  s16x8 a32[3], a16[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int t = (ln >> 1) * 3 + dx, o = ln & 1;
    float v[8], u[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ln < 6 ? W[(t * C + 8 * g + j) * 2 + o] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = (ln < 6 && g < 2) ? W[(t * C + 32 + 8 * g + j) * 2 + o] : 0.f;   // channels 32..47, rest zero
    a32[dx] = __builtin_bit_cast(s16x8, make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])));
    a16[dx] = __builtin_bit_cast(s16x8, make_uint4(pack2<T>(u[0], u[1]), pack2<T>(u[2], u[3]), pack2<T>(u[4], u[5]), pack2<T>(u[6], u[7])));
  }
  const float b0 = bias[0], b1 = bias[1];
  const int tiles_x = Ww / OCM_T, tiles_y = Hh / OCM_T, ntiles = F * tiles_x * tiles_y;
  // this thread's halo chunks: geometry is the same for every tile (computed once: the divisions by 6 and 18 per chunk and tile
  // were ~300 VALU instructions per tile, as much issue time as the MFMA loop)
  int rel[NCH], ryx[NCH], lds[NCH];
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int q = min(tid + u * 256, OCM_H * OCM_H * CPP - 1);
    const int px = q / CPP, ch = (q % CPP) * 8;
    const int ry = px / OCM_H - 1, rx = px % OCM_H - 1;
    rel[u] = (ry * Ww + rx) * C + ch;
    ryx[u] = (ry & 0xffff) | (rx << 16);
    lds[u] = tid + u * 256 < OCM_H * OCM_H * CPP ? px * LDH + ch : -1;
  }
  uint4 pre[NCH];
  bool pin[NCH];
  auto prefetch = [&](int tile) {
    int tx, ty, f;
    oc_decode(tile, tiles_x, tiles_y, F, Tn, y_bs, y_ts, tx, ty, f);
    const int y0 = ty * OCM_T, x0 = tx * OCM_T;
    const T* Xt = X + ((long long)f * Hh + y0) * Ww * C + (long long)x0 * C;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int gy = y0 + (short)(ryx[u] & 0xffff), gx = x0 + (ryx[u] >> 16);
      pin[u] = (unsigned)gy < (unsigned)Hh && (unsigned)gx < (unsigned)Ww;
      pre[u] = *reinterpret_cast<const uint4*>(Xt + (pin[u] ? rel[u] : 0));      // (the tile's own first pixel is always in the image)
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < NCH; ++u)
      if (lds[u] >= 0) *reinterpret_cast<uint4*>(halo + lds[u]) = pin[u] ? pre[u] : make_uint4(0, 0, 0, 0);
  };
  for (int i = tid; i < OCM_H * OCM_H * LDH + 64; i += 256) halo[i].v = 0;
  __syncthreads();
  int tile = blockIdx.x;
  if (tile < ntiles) { prefetch(tile); commit(); }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    if (next < ntiles && !(dbg & 4)) prefetch(next);
    int tx, ty, f;
    oc_decode(tile, tiles_x, tiles_y, F, Tn, y_bs, y_ts, tx, ty, f);
    const int bb = f / Tn, tt = f % Tn;
    float* Yb = Y + bb * y_bs + tt * y_ts;
    // halo rows 4w .. 4w+5 -> output rows 4w .. 4w+3.  acc rows: [0],[1] = dy 0 (g = 0) / dy 2 (g = 1);  [2],[3] = dy 1 (g = 0)
    float pa0[6], pa1[6], pb0[6], pb1[6];
#pragma unroll
    for (int hr = 0; hr < 6; ++hr) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (!(dbg & 1))
      {const T* hp = halo + ((4 * w + hr) * OCM_H + ln) * LDH;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const s16x8 x32 = *reinterpret_cast<const s16x8*>(hp + dx * LDH + 8 * g);
        const s16x8 x16 = *reinterpret_cast<const s16x8*>(hp + dx * LDH + 32 + 8 * g);
        acc = Mma<T>::mma(a32[dx], x32, acc);
        acc = Mma<T>::mma(a16[dx], x16, acc);
      }}
      pa0[hr] = acc[0]; pa1[hr] = acc[1]; pb0[hr] = acc[2]; pb1[hr] = acc[3];
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      // g = 0 lanes: dy 0 of halo row jj + dy 1 of halo row jj + 1;  g = 1 lanes: dy 2 of halo row jj + 2
      float v0 = g == 0 ? pa0[jj] + pb0[jj + 1] : pa0[jj + 2];
      float v1 = g == 0 ? pa1[jj] + pb1[jj + 1] : pa1[jj + 2];
      v0 += __shfl_xor(v0, 16);
      v1 += __shfl_xor(v1, 16);
      if (g == 0 && !(dbg & 2)) {
        float* dst = Yb + ((long long)(ty * OCM_T + 4 * w + jj) * Ww + tx * OCM_T + ln) * y_ps;
        *reinterpret_cast<float2*>(dst) = make_float2(v0 + b0, v1 + b1);
      }
    }
    __syncthreads();
    if (next < ntiles) commit();
    __syncthreads();
  }
}

// Both heads in one launch (round 2).  Ablation of the kernel above (tools/bench_outconv.py, STJ_OC_DBG): 124 us per head, of which
// the MFMA loop 8 us and the OUTPUT STORES 35 us -- 17 MB of results: a frame owns 8 bytes of every 128-byte line of the [B,H,W,32]
// tensor, so each line is written in 16 pieces by 16 different (head, waypoint) work items.  Here a work item is a SPATIAL tile of
// one scene: the workgroup runs the 16 (waypoint, head) sub-tiles over it back to back (same halo pipeline, 31 KB per sub-tile) and
// keeps the results in registers -- lane group g collects the 32 bytes of waypoints 2g, 2g+1 -- so every output pixel leaves as ONE
// full 128-byte line (4 lanes x 2 float4).  Output layout fixed to Tn = 8: channel 4 t + 2 head + o.
#ifndef OCP_MINB
#define OCP_MINB 2
#endif
template <typename T, int C>
__global__ __launch_bounds__(256, OCP_MINB) void outconv_pair_fwd_kernel(const T* __restrict__ X0, const T* __restrict__ X1,
                                                                  const float* __restrict__ W0, const float* __restrict__ W1,
                                                                  const float* __restrict__ bias0, const float* __restrict__ bias1,
                                                                  float* __restrict__ Y, int B, int Hh, int Ww, int t_major, int nsp) {
  static_assert(C == 48, "specialised for 48 input channels (32 + 16)");
  constexpr int LDH = C + 32;
  constexpr int CPP = C / 8, NCH = (OCM_H * OCM_H * CPP + 255) / 256;
  __shared__ __attribute__((aligned(16))) T halo[OCM_H * OCM_H * LDH + 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ln = lane & 15;
  s16x8 a32[2][3], a16[2][3];      // [head][dx]: A row m = ln = 2 dy + o
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float* W = h ? W1 : W0;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int t = (ln >> 1) * 3 + dx, o = ln & 1;
      float v[8], u[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ln < 6 ? W[(t * C + 8 * g + j) * 2 + o] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = (ln < 6 && g < 2) ? W[(t * C + 32 + 8 * g + j) * 2 + o] : 0.f;
      a32[h][dx] = __builtin_bit_cast(s16x8, make_uint4(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]), pack2<T>(v[4], v[5]), pack2<T>(v[6], v[7])));
      a16[h][dx] = __builtin_bit_cast(s16x8, make_uint4(pack2<T>(u[0], u[1]), pack2<T>(u[2], u[3]), pack2<T>(u[4], u[5]), pack2<T>(u[6], u[7])));
    }
  }
  const float bs[4] = {bias0[0], bias0[1], bias1[0], bias1[1]};       // per (head, o): channel 4 t + 2 head + o
  const int tiles_x = Ww / OCM_T, tiles_y = Hh / OCM_T;
  int rel[NCH], ryx[NCH], lds[NCH];
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int q = min(tid + u * 256, OCM_H * OCM_H * CPP - 1);
    const int px = q / CPP, ch = (q % CPP) * 8;
    const int ry = px / OCM_H - 1, rx = px % OCM_H - 1;
    rel[u] = (ry * Ww + rx) * C + ch;
    ryx[u] = (ry & 0xffff) | (rx << 16);
    lds[u] = tid + u * 256 < OCM_H * OCM_H * CPP ? px * LDH + ch : -1;
  }
  uint4 pre[NCH];
  bool pin[NCH];
  // sub-tile it of this workgroup: spatial tile sp = blockIdx.x + (it >> 4) gridDim.x, waypoint t = (it & 15) >> 1, head = it & 1
  auto prefetch = [&](int it) {
    const int sp = blockIdx.x + (it >> 4) * gridDim.x, t = (it & 15) >> 1, h = it & 1;
    const int tx = sp % tiles_x, s2 = sp / tiles_x, ty = s2 % tiles_y, b = s2 / tiles_y;
    const int f = t_major ? t * B + b : b * 8 + t;
    const int y0 = ty * OCM_T, x0 = tx * OCM_T;
    const T* Xt = (h ? X1 : X0) + ((long long)f * Hh + y0) * Ww * C + (long long)x0 * C;
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int gy = y0 + (short)(ryx[u] & 0xffff), gx = x0 + (ryx[u] >> 16);
      pin[u] = (unsigned)gy < (unsigned)Hh && (unsigned)gx < (unsigned)Ww;
      pre[u] = *reinterpret_cast<const uint4*>(Xt + (pin[u] ? rel[u] : 0));
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < NCH; ++u)
      if (lds[u] >= 0) *reinterpret_cast<uint4*>(halo + lds[u]) = pin[u] ? pre[u] : make_uint4(0, 0, 0, 0);
  };
  for (int i = tid; i < OCM_H * OCM_H * LDH + 64; i += 256) halo[i].v = 0;
  __syncthreads();
  const int nmine = blockIdx.x < nsp ? (nsp - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const int nit = nmine * 16;
  if (nit > 0) { prefetch(0); commit(); }
  __syncthreads();
  float keep[4][8] = {};           // this lane group's 32 bytes (waypoints 2g, 2g+1; both heads) of 4 pixels (rows 4w + jj, column ln)
  for (int it0 = 0; it0 < nit; it0 += 4) {
    const int d = (it0 & 15) >> 2;                 // lane group that collects these four sub-tiles
#pragma unroll
    for (int i = 0; i < 4; ++i) {                  // i = 2 (t & 1) + head
      const int it = it0 + i;
      if (it + 1 < nit) prefetch(it + 1);
      float pa0[6], pa1[6], pb0[6], pb1[6];
#pragma unroll
      for (int hr = 0; hr < 6; ++hr) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        const T* hp = halo + ((4 * w + hr) * OCM_H + ln) * LDH;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const s16x8 x32 = *reinterpret_cast<const s16x8*>(hp + dx * LDH + 8 * g);
          const s16x8 x16 = *reinterpret_cast<const s16x8*>(hp + dx * LDH + 32 + 8 * g);
          acc = Mma<T>::mma(a32[i & 1][dx], x32, acc);
          acc = Mma<T>::mma(a16[i & 1][dx], x16, acc);
        }
        pa0[hr] = acc[0]; pa1[hr] = acc[1]; pb0[hr] = acc[2]; pb1[hr] = acc[3];
      }
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        float v0 = g == 0 ? pa0[jj] + pb0[jj + 1] : pa0[jj + 2];
        float v1 = g == 0 ? pa1[jj] + pb1[jj + 1] : pa1[jj + 2];
        v0 += __shfl_xor(v0, 16);                  // lanes of groups 0 and 1 now hold the pixel's value
        v1 += __shfl_xor(v1, 16);
        v0 = __shfl(v0, ln);                       // ... and now every group does
        v1 = __shfl(v1, ln);
        keep[jj][2 * i] = g == d ? v0 + bs[2 * (i & 1)] : keep[jj][2 * i];          // (a select, not a conditional store: the array stays in VGPRs)
        keep[jj][2 * i + 1] = g == d ? v1 + bs[2 * (i & 1) + 1] : keep[jj][2 * i + 1];
      }
      __syncthreads();
      if (it + 1 < nit) commit();
      __syncthreads();
    }
    if (d == 3) {                                  // all 16 sub-tiles of the spatial tile done: 128-byte lines out
      const int sp = blockIdx.x + (it0 >> 4) * gridDim.x;
      const int tx = sp % tiles_x, s2 = sp / tiles_x, ty = s2 % tiles_y, b = s2 / tiles_y;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        float* dst = Y + ((((long long)b * Hh + ty * OCM_T + 4 * w + jj) * Ww) + tx * OCM_T + ln) * 32 + 8 * g;
        *reinterpret_cast<float4*>(dst) = make_float4(keep[jj][0], keep[jj][1], keep[jj][2], keep[jj][3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(keep[jj][4], keep[jj][5], keep[jj][6], keep[jj][7]);
      }
    }
  }
}

bool outconv_pair_fwd_try(const void* X0, const void* X1, const float* W0, const float* W1, const float* b0, const float* b1, float* Y,
                          int B, int Tn, int Hh, int Ww, int C, int t_major, int dtype, hipStream_t st) {
  if (C != 48 || Tn != 8 || Hh % OCM_T || Ww % OCM_T || (((uintptr_t)Y) & 15)) return false;
  const int nsp = B * (Hh / OCM_T) * (Ww / OCM_T);
  // OCP_MINB resident workgroups per CU; an equal number of spatial tiles for (nearly) every workgroup
  // (one / two spatial tiles per workgroup instead of four, i.e. 2048 / 1024 shorter-lived workgroups: 187-193 / 172-179 us against 172-175 in a hot loop)
  const int per = (nsp + 256 * OCP_MINB - 1) / (256 * OCP_MINB);
  const int nb = (nsp + per - 1) / per;
  return stj_with_dtype16(dtype, [&](auto t) { typedef typename decltype(t)::type T;
    hipLaunchKernelGGL((outconv_pair_fwd_kernel<T, 48>), dim3(nb), dim3(256), 0, st, (const T*)X0, (const T*)X1, W0, W1, b0, b1, Y, B, Hh, Ww, t_major, nsp);
  });
}

// Second half of the inference heads (first half: the HEAD epilogue of upconv_fwd_ws2_kernel): Y[b, y, x, 4 t + 2 h + o] = bias_h[o] +
// sum over the 9 neighbours (ky, kx) of Z_h[f(b, t), y + ky - 1, x + kx - 1, 2 (3 ky + kx) + o] (zero outside the image), Z_h the projected
// tensors [F, H, W, STJ_HEAD_CZ = 20] of the two decoder branches.  A workgroup owns a 16 x 16 spatial tile of one scene and walks its 16 (waypoint,
// head) planes through an 18 x 18 halo in LDS (next plane prefetched in registers); a thread keeps the 32 results of its pixel and writes
// one full 128-byte line.
// QUANT (stj_outconv_pair_gather_q): the same sums, but the epilogue turns the 32 results into the challenge format's bytes (quantize.h)
// and Y is the byte buffer of stj_quantize_waypoints, [B][obs u8 [8,H,W] | occ u8 [8,H,W] | flow i8 [8,H,W,2]]: the tile's 32 plane
// pieces (16 rows x 16 B, flow 32 B) are staged in the halo's LDS, which the last plane has finished with, and leave as 16-byte vectors.
template <typename T, bool QUANT>
__global__ __launch_bounds__(256) void outconv_pair_gather_kernel(const T* __restrict__ Z0, const T* __restrict__ Z1, const float* __restrict__ b0,
                                                                  const float* __restrict__ b1, std::conditional_t<QUANT, uint8_t, float>* __restrict__ Y,
                                                                  int B, int Hh, int Ww, int t_major, int nsp) {
  constexpr int CZ = STJ_HEAD_CZ, LDZ = STJ_HEAD_CZ, CPP = CZ / 4, NPX = OCM_H * OCM_H, NCHK = NPX * CPP, NCH = (NCHK + 255) / 256;      // 8-byte pieces
  __shared__ __attribute__((aligned(16))) T halo[NPX * LDZ];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int tiles_x = Ww / OCM_T, tiles_y = Hh / OCM_T;
  const float bias[2][2] = {{b0[0], b0[1]}, {b1[0], b1[1]}};
  for (int sp = blockIdx.x; sp < nsp; sp += gridDim.x) {
    const int tcx = sp % tiles_x, t2 = sp / tiles_x, tcy = t2 % tiles_y, b = t2 / tiles_y;
    const int y0 = tcy * OCM_T - 1, x0 = tcx * OCM_T - 1;
    uint2 pre[NCH];
    auto fetch = [&](int plane) {
      const int t = plane >> 1, h = plane & 1;
      const int f = t_major ? t * B + b : b * 8 + t;
      const T* Zf = (h ? Z1 : Z0) + (long long)f * Hh * Ww * CZ;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = tid + i * 256;
        const int px = c / CPP, cc = c % CPP;
        const int gy = y0 + px / OCM_H, gx = x0 + px % OCM_H;
        uint2 v = make_uint2(0, 0);
        if (c < NCHK && gy >= 0 && gy < Hh && gx >= 0 && gx < Ww) v = *reinterpret_cast<const uint2*>(Zf + ((long long)gy * Ww + gx) * CZ + cc * 4);
        pre[i] = v;
      }
    };
    float out[32];
    uint32_t qb[8] = {0, 0, 0, 0, 0, 0, 0, 0};           // QUANT: the bytes of waypoint t, obs | occ << 8 | flow_x << 16 | flow_y << 24
    fetch(0);
#pragma unroll 1
    for (int plane = 0; plane < 16; ++plane) {
      __syncthreads();                                   // the previous plane's reads are through
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = tid + i * 256;
        if (c < NCHK) *reinterpret_cast<uint2*>(halo + (c / CPP) * LDZ + (c % CPP) * 4) = pre[i];
      }
      __syncthreads();
      if (plane + 1 < 16) fetch(plane + 1);
      const int h = plane & 1;
      float s0 = bias[h][0], s1 = bias[h][1];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const uint32_t w = *reinterpret_cast<const uint32_t*>(halo + ((ty + ky) * OCM_H + tx + kx) * LDZ + 2 * (3 * ky + kx));
          float a0, a1;
          unpack2<T>(w, a0, a1);
          s0 += a0; s1 += a1;
        }
      // plane = 2 t + h -> channels 4 t + 2 h + {0, 1} = 2 plane + {0, 1}
      if constexpr (QUANT) {       // quantised here, not behind the loop: 8 packed registers live instead of 32 floats
        const uint32_t v = h ? (quant_flow(s0) | (quant_flow(s1) << 8)) << 16 : quant_prob(s0) | (quant_prob(s1) << 8);
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (q == (plane >> 1)) qb[q] |= v;
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
          if (q == plane) { out[2 * q] = s0; out[2 * q + 1] = s1; }
      }
    }
    if constexpr (QUANT) {
      static_assert(sizeof(halo) >= 32 * OCM_T * OCM_T, "the byte stage lives in the halo");
      uint8_t* stg = reinterpret_cast<uint8_t*>(halo);           // [obs 8 x 256 | occ 8 x 256 | flow 8 x 512], a plane piece = 16 rows of the tile
      __syncthreads();                                           // the last plane's reads are through
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        stg[t * 256 + tid] = (uint8_t)qb[t];
        stg[2048 + t * 256 + tid] = (uint8_t)(qb[t] >> 8);
        *reinterpret_cast<uint16_t*>(stg + 4096 + t * 512 + 2 * tid) = (uint16_t)(qb[t] >> 16);
      }
      __syncthreads();                                           // (the next tile's first halo write waits behind the barrier at the head of its plane loop)
      const long long HW = (long long)Hh * Ww;
      uint8_t* q = Y + (long long)b * 32 * HW;
      const long long cell = (long long)(tcy * OCM_T) * Ww + tcx * OCM_T;
      {       // threads 0..127: (observed plane, row), 128..255: (occluded plane, row): 16 B each
        const int p = tid >> 4, r = tid & 15;
        *reinterpret_cast<uint4*>(q + p * HW + cell + (long long)r * Ww) = *reinterpret_cast<const uint4*>(stg + 16 * tid);
      }
      {       // flow: (plane, row, half of the row's 32 B)
        const int p = tid >> 5, r = (tid >> 1) & 15, hf = tid & 1;
        *reinterpret_cast<uint4*>(q + 16 * HW + p * 2 * HW + 2 * (cell + (long long)r * Ww) + 16 * hf) = *reinterpret_cast<const uint4*>(stg + 4096 + 16 * tid);
      }
    } else {
      float* yp = Y + (((long long)b * Hh + tcy * OCM_T + ty) * Ww + tcx * OCM_T + tx) * 32;
#pragma unroll
      for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(yp + 4 * q) = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    }
  }
}
template <bool QUANT>
static bool outconv_pair_gather_launch(const void* Z0, const void* Z1, const float* b0, const float* b1, std::conditional_t<QUANT, uint8_t, float>* Y, int B,
                                       int Tn, int Hh, int Ww, int t_major, int dtype, hipStream_t st) {
  if (Tn != 8 || Hh % OCM_T || Ww % OCM_T || (((uintptr_t)Y | (uintptr_t)Z0 | (uintptr_t)Z1) & 15)) return false;
  const int nsp = B * (Hh / OCM_T) * (Ww / OCM_T);
  const int nb = nsp < 2048 ? nsp : 2048;
  return stj_with_dtype16(dtype, [&](auto t) { typedef typename decltype(t)::type T;
    hipLaunchKernelGGL((outconv_pair_gather_kernel<T, QUANT>), dim3(nb), dim3(256), 0, st, (const T*)Z0, (const T*)Z1, b0, b1, Y, B, Hh, Ww, t_major, nsp);
  });
}
bool outconv_pair_gather_try(const void* Z0, const void* Z1, const float* b0, const float* b1, float* Y, int B, int Tn, int Hh, int Ww, int t_major,
                             int dtype, hipStream_t st) {
  return outconv_pair_gather_launch<false>(Z0, Z1, b0, b1, Y, B, Tn, Hh, Ww, t_major, dtype, st);
}
bool outconv_pair_gather_q_try(const void* Z0, const void* Z1, const float* b0, const float* b1, uint8_t* Q, int B, int Tn, int Hh, int Ww, int t_major,
                               int dtype, hipStream_t st) {
  return outconv_pair_gather_launch<true>(Z0, Z1, b0, b1, Q, B, Tn, Hh, Ww, t_major, dtype, st);
}

// Backward.  Occupancy is what matters here (the first MFMA version held all 27 (tap, channel-block) dW accumulators in every
// wave: 332 VGPRs, one wave per SIMD, and 1.8 M same-address f32 atomics for dW -- 0.5-0.6 ms per head).  Now: wave w owns 7 of
// the 27 dW accumulators and walks all 16 rows of the tile, so a block needs 168 VGPRs and 39 KB LDS -> 3 blocks per CU (0.28 ms per head); dW/db
// partials leave as plain stores into a caller-provided workspace [blocks][866] and a small second kernel sums them.
#define OCB_PART (9 * 48 * 2 + 2)
#define OCB_MAXBLK 768
// Backward, v2 (round 2).  The weight gradient is re-associated: dW[t][c][o] = sum_p X[p + off(t)][c] dY[p][o] = sum_p' X[p'][c] dY[p' - off(t)][o],
// p' over the tile's OWN pixels -- so the taps move into the N dimension of the MFMA (B[k = pixel][n = (tap, o)], 18 of 32 columns, built
// from the 18 x 18 dY halo that the input gradient needs anyway) and the A operand is the UNSHIFTED X tile, read once per k-step for all
// nine taps: 6 transpose reads + 16 scalar reads + 6 MFMAs per 32-pixel k-step, where v1 (one accumulator per (tap, channel block),
// the X tile shifted per tap) needs 14 + 8 + 7 in each of its four waves -- and X needs no halo any more (256 instead of 324 pixels per
// tile).  A wave owns two of the eight k-steps (the four tile rows it also produces dX for); the four partial sums meet in LDS once,
// at the end of the kernel.
#define OCB_CH(mf, m) (12 * ((m) >> 2) + 4 * (mf) + ((m) & 3))
template <int C>
__global__ __launch_bounds__(256, 3) void outconv_bwd_mfma2_kernel(const bf16* __restrict__ X, const float* __restrict__ W,
                                                                   const float* __restrict__ dY, bf16* __restrict__ dX,
                                                                   float* __restrict__ part, int F, int Hh, int Ww, int Tn,
                                                                   long long y_bs, long long y_ts, long long y_ps, int elu_in) {
  static_assert(C == 48, "specialised for 48 channels");
  constexpr int LDH = C + 8;
  constexpr int CPP = C / 8, NCH = (OCM_T * OCM_T * CPP + 255) / 256;      // 6
  constexpr int NDY = (OCM_H * OCM_H + 255) / 256;                         // 2
  __shared__ __attribute__((aligned(16))) bf16 Xs[OCM_T * OCM_T * LDH];    // the tile's own pixels only
  __shared__ __attribute__((aligned(16))) float dys[OCM_H * OCM_H * 2];
  // [mf][nf][row 0..15][col 0..15] cross-wave sum of dW; padded to 10 KB so that the workgroup takes > 40 KB of LDS: with room for a
  // fourth workgroup per CU the compiler targets 128 VGPRs and keeps the prefetch registers in scratch (112 bytes per lane)
  __shared__ float wred[3 * 2 * 16 * 16 + 1024];
  __shared__ float dbs[2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, ln = lane & 15;
  // dX weights: A[m = c][k = (tap, o)], k = 2*tap + o < 18 ; lane row c = mf*16 + ln, k = 8g + j
  s16x8 ax[3];
#pragma unroll
  for (int mf = 0; mf < 3; ++mf) {
    float v[8];
#pragma unroll
    // row m = ln of fragment mf is channel 12 (ln >> 2) + 4 mf + (ln & 3): the three accumulator fragments of a lane are then 12 CONSECUTIVE
    // channels (12 g + 4 mf + r) of its pixel -- 24 contiguous bytes per lane, 96 per 4 lanes -- instead of three 8-byte pieces 32 bytes apart
    for (int j = 0; j < 8; ++j) { const int k = 8 * g + j; v[j] = k < 18 ? W[((k >> 1) * C + OCB_CH(mf, ln)) * 2 + (k & 1)] : 0.f; }
    ax[mf] = __builtin_bit_cast(s16x8, make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])));
  }
  f32x4 wacc[3][2];
#pragma unroll
  for (int mf = 0; mf < 3; ++mf) { wacc[mf][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; wacc[mf][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  for (int i = tid; i < 3 * 2 * 256; i += 256) wred[i] = 0.f;
  float db0 = 0.f, db1 = 0.f;
  if (tid < 2) dbs[tid] = 0.f;
  const int tiles_x = Ww / OCM_T, tiles_y = Hh / OCM_T, ntiles = F * tiles_x * tiles_y;
  // staging geometry of this thread (tile independent)
  int xrel[NCH], xlds[NCH], yrel[NDY], ylds[NDY], yryx[NDY];
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int q = tid + u * 256;
    const int px = q / CPP, ch = (q % CPP) * 8;
    xrel[u] = ((px / OCM_T) * Ww + px % OCM_T) * C + ch;
    xlds[u] = px * LDH + ch;
  }
#pragma unroll
  for (int u = 0; u < NDY; ++u) {
    const int q = min(tid + u * 256, OCM_H * OCM_H - 1);
    const int ry = q / OCM_H - 1, rx = q % OCM_H - 1;
    yrel[u] = ry * Ww + rx;
    yryx[u] = (ry & 0xffff) | (rx << 16);
    ylds[u] = tid + u * 256 < OCM_H * OCM_H ? 2 * q : -1;
  }
  // staging registers as NAMED scalars (as arrays they stayed in scratch here, 112 bytes per lane, whatever the loop structure)
  static_assert(NCH == 6 && NDY == 2, "staging code below is written out for 6 + 2 chunks");
  uint4 p0, p1, p2, p3, p4, p5;
  float2 q0, q1;
#define OCB2_PREFETCH(TILE)                                                                                              \
  do {                                                                                                                   \
    int tx_, ty_, f_;                                                                                                    \
    oc_decode(TILE, tiles_x, tiles_y, F, Tn, y_bs, y_ts, tx_, ty_, f_);                                                  \
    const int y0_ = ty_ * OCM_T, x0_ = tx_ * OCM_T;                                                                      \
    const bf16* Xt_ = X + (((long long)f_ * Hh + y0_) * Ww + x0_) * C;                                                   \
    const float* dYt_ = dY + (f_ / Tn) * y_bs + (f_ % Tn) * y_ts + ((long long)y0_ * Ww + x0_) * y_ps;                   \
    p0 = *reinterpret_cast<const uint4*>(Xt_ + xrel[0]); p1 = *reinterpret_cast<const uint4*>(Xt_ + xrel[1]);            \
    p2 = *reinterpret_cast<const uint4*>(Xt_ + xrel[2]); p3 = *reinterpret_cast<const uint4*>(Xt_ + xrel[3]);            \
    p4 = *reinterpret_cast<const uint4*>(Xt_ + xrel[4]); p5 = *reinterpret_cast<const uint4*>(Xt_ + xrel[5]);            \
    {                                                                                                                    \
      const int gy_ = y0_ + (short)(yryx[0] & 0xffff), gx_ = x0_ + (yryx[0] >> 16);                                      \
      const bool in_ = (unsigned)gy_ < (unsigned)Hh && (unsigned)gx_ < (unsigned)Ww;                                     \
      const float2 v_ = *reinterpret_cast<const float2*>(dYt_ + (in_ ? (long long)yrel[0] * y_ps : 0));                  \
      q0 = in_ ? v_ : make_float2(0.f, 0.f);                                                                             \
    }                                                                                                                    \
    {                                                                                                                    \
      const int gy_ = y0_ + (short)(yryx[1] & 0xffff), gx_ = x0_ + (yryx[1] >> 16);                                      \
      const bool in_ = (unsigned)gy_ < (unsigned)Hh && (unsigned)gx_ < (unsigned)Ww;                                     \
      const float2 v_ = *reinterpret_cast<const float2*>(dYt_ + (in_ ? (long long)yrel[1] * y_ps : 0));                  \
      q1 = in_ ? v_ : make_float2(0.f, 0.f);                                                                             \
    }                                                                                                                    \
  } while (0)
#define OCB2_COMMIT()                                                                                                    \
  do {                                                                                                                   \
    *reinterpret_cast<uint4*>(Xs + xlds[0]) = p0; *reinterpret_cast<uint4*>(Xs + xlds[1]) = p1;                          \
    *reinterpret_cast<uint4*>(Xs + xlds[2]) = p2; *reinterpret_cast<uint4*>(Xs + xlds[3]) = p3;                          \
    *reinterpret_cast<uint4*>(Xs + xlds[4]) = p4; *reinterpret_cast<uint4*>(Xs + xlds[5]) = p5;                          \
    if (ylds[0] >= 0) *reinterpret_cast<float2*>(dys + ylds[0]) = q0;                                                    \
    if (ylds[1] >= 0) *reinterpret_cast<float2*>(dys + ylds[1]) = q1;                                                    \
  } while (0)
  int tile = blockIdx.x;                             // (< ntiles: the launcher starts at most ntiles workgroups)
  OCB2_PREFETCH(tile);
  OCB2_COMMIT();
  __syncthreads();
  const int kpx = 8 * (g & 1) + (ln >> 2), kch = 4 * (ln & 3);
  // B operand of the weight gradient: column n = ln of fragment nf is (tap, o) = ((ln >> 1) + 8 nf, ln & 1); nf = 1 only has tap 8
  const int t0 = ln >> 1, o0 = ln & 1;
  const int sh0 = ((2 - t0 / 3) * OCM_H + 2 - t0 % 3) * 2 + o0;            // dys offset of tap t0 relative to pixel (row, col)
  const int sh1 = ((2 - 8 / 3) * OCM_H + 2 - 8 % 3) * 2 + o0;              // tap 8
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    OCB2_PREFETCH(min(next, ntiles - 1));            // unconditional; the last one re-reads the last tile
    int tx, ty, f;
    oc_decode(tile, tiles_x, tiles_y, F, Tn, y_bs, y_ts, tx, ty, f);
    bf16* dXf = dX + (long long)f * Hh * Ww * C;
    // ---- dX rows 4w .. 4w+3 ----
    // (unrolled: with the 12 stores of a tile in a rolled loop the waitcnt pass cannot count them and the commit of the prefetched tile below
    //  waits for most of the STORES to complete as well -- vmcnt(8..3) where 18 operations are younger than the first load)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = 4 * w + rr;
      float2 d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = 4 * g + j;
        d[j] = t < 9 ? *reinterpret_cast<const float2*>(dys + 2 * ((row + 2 - t / 3) * OCM_H + ln + 2 - t % 3)) : make_float2(0.f, 0.f);
      }
      const s16x8 bx = __builtin_bit_cast(s16x8, make_uint4(pack2bf(d[0].x, d[0].y), pack2bf(d[1].x, d[1].y), pack2bf(d[2].x, d[2].y), pack2bf(d[3].x, d[3].y)));
      bf16* orow = dXf + ((long long)(ty * OCM_T + row) * Ww + tx * OCM_T + ln) * C + 12 * g;      // 24 bytes of the lane: channels 12 g .. 12 g + 11
      uint32_t ow[6];
#pragma unroll
      for (int mf = 0; mf < 3; ++mf) {
        f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ax[mf]), __builtin_bit_cast(bf16x8_t, bx), (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        if (elu_in) {        // X is the ELU output of the producing conv: fold ELU'(x) = (x > 0 ? 1 : x + 1) into the input gradient
          const uint2 xv = *reinterpret_cast<const uint2*>(Xs + (row * OCM_T + ln) * LDH + 12 * g + 4 * mf);
          const float x0 = __uint_as_float(xv.x << 16), x1 = __uint_as_float(xv.x & 0xffff0000u);
          const float x2 = __uint_as_float(xv.y << 16), x3 = __uint_as_float(xv.y & 0xffff0000u);
          acc[0] *= x0 > 0.f ? 1.f : x0 + 1.f; acc[1] *= x1 > 0.f ? 1.f : x1 + 1.f;
          acc[2] *= x2 > 0.f ? 1.f : x2 + 1.f; acc[3] *= x3 > 0.f ? 1.f : x3 + 1.f;
        }
        ow[2 * mf] = pack2bf(acc[0], acc[1]); ow[2 * mf + 1] = pack2bf(acc[2], acc[3]);
      }
      // 24 bytes at an 8-byte aligned address: three 8-byte stores to consecutive addresses (the compiler may merge them; 96 contiguous bytes per 4 lanes either way)
      uint2* o2 = reinterpret_cast<uint2*>(orow);
      o2[0] = make_uint2(ow[0], ow[1]); o2[1] = make_uint2(ow[2], ow[3]); o2[2] = make_uint2(ow[4], ow[5]);
    }
    // ---- dW: this wave's k-steps 2w, 2w+1 (tile rows 4w .. 4w+3, 32 pixels each) ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = 2 * w + h;
      const int prow = 2 * kk + (g >> 1), pcol = 8 * (g & 1);              // this lane group's 8 pixels (k = 8g .. 8g+7 of the k-step)
      const float* dp = dys + 2 * (prow * OCM_H + pcol);
      float dv0[8], dv1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { dv0[j] = dp[2 * j + sh0]; dv1[j] = ln < 2 ? dp[2 * j + sh1] : 0.f; }
      const s16x8 bw0 = __builtin_bit_cast(s16x8, make_uint4(pack2bf(dv0[0], dv0[1]), pack2bf(dv0[2], dv0[3]), pack2bf(dv0[4], dv0[5]), pack2bf(dv0[6], dv0[7])));
      const s16x8 bw1 = __builtin_bit_cast(s16x8, make_uint4(pack2bf(dv1[0], dv1[1]), pack2bf(dv1[2], dv1[3]), pack2bf(dv1[4], dv1[5]), pack2bf(dv1[6], dv1[7])));
      const bf16* ap = Xs + (prow * OCM_T + kpx) * LDH + kch;
#pragma unroll
      for (int mf = 0; mf < 3; ++mf) {
        const s16x8 aw = tr_frag(ap + mf * 16, ap + mf * 16 + 4 * LDH);
        wacc[mf][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, aw), __builtin_bit_cast(bf16x8_t, bw0), wacc[mf][0], 0, 0, 0);
        wacc[mf][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, aw), __builtin_bit_cast(bf16x8_t, bw1), wacc[mf][1], 0, 0, 0);
      }
    }
    {
      const int py = tid / OCM_T, px = tid % OCM_T;
      const float2 v = *reinterpret_cast<const float2*>(dys + 2 * ((py + 1) * OCM_H + px + 1));
      db0 += v.x; db1 += v.y;
    }
    __syncthreads();
    OCB2_COMMIT();                                   // (after the last tile: the re-read tile, read by nobody)
    __syncthreads();
  }
  // cross-wave sum of the weight gradient: D[m = c][n = (tap, o)]: lane (g, ln) holds channels mf*16 + 4g + r, column ln
#pragma unroll
  for (int mf = 0; mf < 3; ++mf)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&wred[((mf * 2 + nf) * 16 + 4 * g + r) * 16 + ln], wacc[mf][nf][r]);
  db0 = wave_sum(db0); db1 = wave_sum(db1);
  if (lane == 0) { atomicAdd(&dbs[0], db0); atomicAdd(&dbs[1], db1); }
  __syncthreads();
  float* mypart = part + (long long)blockIdx.x * OCB_PART;
  for (int i = tid; i < 9 * C * 2; i += 256) {                             // i = (t * C + c) * 2 + o
    const int o = i & 1, c = (i >> 1) % C, t = (i >> 1) / C;
    const int nf = t >> 3, n = (t & 7) * 2 + o;
    mypart[i] = wred[(((c >> 4) * 2 + nf) * 16 + (c & 15)) * 16 + n];
  }
  if (tid < 2) mypart[9 * C * 2 + tid] = dbs[tid];
}
#undef OCB2_PREFETCH
#undef OCB2_COMMIT

// (Round 6 built a v3 of this kernel in short-lived workgroups -- one 4 x 16 pixel strip per wave, all loads in flight first, no barrier between a
// wave's loads and its stores, the last wave of a workgroup writing the partial -- because a bare copy of the tensor streams 5.8 TB/s in that
// form and 4.1-4.5 in this kernel's persistent one (tools/probes/tile_stream_probe.hip, profiles/r06_m_tile_stream_probe*.txt).  Measured at
// F = 64, 256 x 256: 614 us with the cross-wave sum as LDS float atomics (24 ds_add_f32 per lane cost ~23 us per wave there), 249 us with
// plain LDS stores, 220 us with no cross-wave sum at all, against 209 us for this kernel: per WAVE the strided dY halo (8 bytes of every
// 128-byte line: -35 us without it, -18 us with a compact dY) and the 24 weight loads (-18 us) are paid 65536 times instead of 3072.
// The same strips in a LOOP (a wave walks strips gw, gw + GW, ...; weights through LDS once per workgroup, eight loads in flight behind an
// operand-barrier asm statement, sums as plain LDS stores added up by the last wave): 205-214 us at 768 .. 3072 workgroups -- this
// kernel's time.  Not kept; profiles/r06_m_outconv_bwd_v3.txt.)
// sums the per-block partials: grid (ceil(866 / 64), 16 row groups) x 64 threads
__global__ __launch_bounds__(64) void outconv_bwd_reduce_kernel(const float* __restrict__ part, int nblk, float* dW, float* db) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= OCB_PART) return;
  float s = 0.f;
  for (int r = blockIdx.y; r < nblk; r += gridDim.y) s += part[(long long)r * OCB_PART + idx];
  atomicAdd(idx < OCB_PART - 2 ? dW + idx : db + (idx - (OCB_PART - 2)), s);
}

bool outconv_fwd_mfma_try(const void* X, const float* W, const float* bias, float* Y, int F, int Hh, int Ww, int C, int Tn,
                          long long y_bs, long long y_ts, long long y_ps, int dtype, hipStream_t st) {
  // the kernel moves float2 at Y + b*y_bs + t*y_ts + p*y_ps: every stride even and the base 8-byte aligned, or the generic kernel runs
  if (C != 48 || Hh % OCM_T || Ww % OCM_T || ((y_bs | y_ts | y_ps) & 1) || (((uintptr_t)Y) & 7)) return false;
  const int ntiles = F * (Hh / OCM_T) * (Ww / OCM_T);
  const int dbg = 0, nbm = 768;
  const int nb = min(ntiles, nbm);
  return stj_with_dtype16(dtype, [&](auto t) { typedef typename decltype(t)::type T;
    hipLaunchKernelGGL((outconv_fwd_mfma2_kernel<T, 48>), dim3(nb), dim3(256), 0, st, (const T*)X, W, bias, Y, F, Hh, Ww, Tn, y_bs, y_ts, y_ps, dbg);
  });
}
long long outconv_bwd_ws_bytes() { return (long long)OCB_MAXBLK * OCB_PART * sizeof(float); }
bool outconv_bwd_mfma_try(const void* X, const float* W, const float* dY, void* dX, float* dW, float* db, int F, int Hh, int Ww, int C,
                          int Tn, long long y_bs, long long y_ts, long long y_ps, int elu_in, void* ws, long long ws_bytes, hipStream_t st) {
  if (C != 48 || Hh % OCM_T || Ww % OCM_T || ((y_bs | y_ts | y_ps) & 1) || (((uintptr_t)dY) & 7)) return false;
  if (!ws || ws_bytes < outconv_bwd_ws_bytes()) return false;
  const int ntiles = F * (Hh / OCM_T) * (Ww / OCM_T);
  const int nblk = min(ntiles, OCB_MAXBLK);          // 3 resident blocks per CU (168 VGPRs, 39 KB LDS): measured best of 512/768/1024
  hipLaunchKernelGGL(outconv_bwd_mfma2_kernel<48>, dim3(nblk), dim3(256), 0, st, (const bf16*)X, W, dY, (bf16*)dX, (float*)ws, F, Hh, Ww, Tn,
                     y_bs, y_ts, y_ps, elu_in);
  hipLaunchKernelGGL(outconv_bwd_reduce_kernel, dim3((OCB_PART + 63) / 64, 16), dim3(64), 0, st, (const float*)ws, nblk, dW, db);
  return true;
}
// =====================================================================================================
// Input gradient of the folded up-conv, v2 (bf16): weight-stationary per INPUT phase + LDS reduction.
//   dX[f,i,j,:] = sum_{a,b} sum_{r,s} dP[f, 2i+u, 2j+v, :] . Weff[a,b,r,s]^T ,  u = 2-a-2r, v = 2-b-2s
// Wave (a,b) keeps Weff[a,b,*,*]^T (Cin-tile x Cout) in VGPRs as MFMA A fragments and consumes only the hi-res pixels of
// parity (a,b) from an 18 x 34 halo tile of dP in LDS; the four per-phase partial tiles are summed through LDS (f32)
// and leave as coalesced 8-byte segments.  v1 (conv.hip) re-staged 16 tap matrices through LDS per tile: 0.59 ms for
// 96<-48 @128x128 (profiles/r01_b_*).
// =====================================================================================================
// LDS layout of upconv_dgrad_ws_kernel (bf16): the dP halo [HPIX][LDK] (+64 elements of tail), then two partial stages
// [4 phases][2 rows][16 px][LDR]; the strides are explained where the kernel takes them
template <int KS, int NFI>
struct DgradWsGeo {
  static constexpr int LDK = KS * 32 + 8;
  static constexpr int HH = 2 * WS_TH + 2, HW = 2 * WS_TW + 2, HPIX = HH * HW;
  static constexpr int CT = NFI * 16, LDR = CT + 4;
  static constexpr int RED = 4 * 2 * 16 * LDR;
  static constexpr int HALO_BYTES = (HPIX * LDK + 64) * 2;
  static constexpr int LDS_BYTES = HALO_BYTES + 2 * RED * 2;
  static_assert(LDS_BYTES <= 160 * 1024, "the layout fits the CU's LDS");
};
template <int KS, int NFI, bool ELU, int COUT>
__global__ __launch_bounds__(512, 1) void upconv_dgrad_ws_kernel(const bf16* __restrict__ dP, const bf16* __restrict__ Wd,
                                                                 bf16* __restrict__ dX, const bf16* __restrict__ Xelu, int F, int Hi,
                                                                 int Wi, int Cin, int ntiles) {
  constexpr int Cout = COUT;                       // compile time: the halo loader divides by Cout / 8 forty times per tile (a runtime
                                                   // divisor cost ~1400 VALU instructions per tile, a quarter of the tile's time)
  // halo pixel stride.  A fragment read takes every OTHER halo pixel (low-res pixel ln <-> high-res 2 ln + v), so consecutive lanes are
  // 2 * LDK apart: conflict-free b128 reads need 2 * LDK = 2 (mod 4) 16-byte slots, i.e. an ODD number of slots per pixel -> +8 elements
  // (9 / 13 slots).  Channels >= Cout stay zero.
  using G = DgradWsGeo<KS, NFI>;
  constexpr int LDK = G::LDK;
  constexpr int HH = G::HH, HW = G::HW, HPIX = G::HPIX;
  constexpr int CT = G::CT;                        // cin tile of this workgroup
  constexpr int LDR = G::LDR;                      // partial-tile row stride (bf16): 34 dwords (two stages + the halo = 158.4 KB of the 160)
  constexpr int RED = G::RED;                      // one partial stage: [4 phases][2 rows][16 px][LDR]
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16* halo = reinterpret_cast<bf16*>(smem_raw);                         // [HPIX][LDK] (+64 tail)
  bf16* red0 = reinterpret_cast<bf16*>(smem_raw + G::HALO_BYTES);         // 2 stages
  constexpr int CPP = Cout / 8;                    // 16-byte chunks per halo pixel (Cout <= KS*32)
  static_assert(COUT % 8 == 0 && COUT <= KS * 32, "halo pixel holds KS*32 channels");
  // 8 waves: wave = (input phase (a,b), half of the cin tile), 96 weight VGPRs each, two waves per SIMD.  A pass (2 low-res rows) is ONE
  // barrier interval holding three things that used to be three serial phases (measured by ablation, 128 <- 96 @64x64 F = 64: 68 us of
  // MFMA + 37 us waiting for the halo prefetch + 14 us of phase reduction + 43 us of barriers and bookkeeping = the kernel's 154 us):
  //   * the MFMAs of pass p -> this wave's partial tile (bf16) into stage p & 1;
  //   * the phase reduction + ELU' + store of pass p - 1 from stage (p - 1) & 1 -- the waves of half 0 do it BEFORE their MFMAs, those
  //     of half 1 AFTER, so on every SIMD one wave reduces / stores while the other feeds the matrix pipe;
  //   * the next tile's halo rows for the rows this pass frees: loads issued at the top, written behind the barrier.
  constexpr int NT = 512, NFW = NFI / 2;
  static_assert(NFI % 2 == 0, "cin tile splits into two halves");
  const int tid = threadIdx.x, lane = tid & 63, w = (tid >> 6) & 3, half = tid >> 8;
  const int a = w >> 1, b = w & 1;
  const int g = lane >> 4, ln = lane & 15;
  const int n0 = blockIdx.y * CT;
  const int tiles_x = (Wi + WS_TW - 1) / WS_TW, tiles_y = (Hi + WS_TH - 1) / WS_TH;
  const int Ho = 2 * Hi, Wo = 2 * Wi;

  // stationary weights: A[m = cin][k = cout] = Wd[(u+1)*4 + (v+1)][cin][cout]
  s16x8 wd[4][NFW][KS];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = t >> 1, s = t & 1;
    const int uv = (2 - a - 2 * r + 1) * 4 + (2 - b - 2 * s + 1);
#pragma unroll
    for (int n = 0; n < NFW; ++n) {
      const int ci = n0 + (half * NFW + n) * 16 + ln;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int co = ks * 32 + g * 8;
        if (ci < Cin && co < Cout) wd[t][n][ks] = *reinterpret_cast<const s16x8*>(Wd + ((long long)uv * Cin + ci) * Cout + co);
        else wd[t][n][ks] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }
  // the weights are complete HERE on every path: without this the waitcnt pass carries "weight loads may be pending" into the tile
  // loop (through the path that skips the first tile's commit) and opens every pass's MFMA block with vmcnt(0) -- which also waits
  // for the halo prefetch issued a few instructions earlier, i.e. exposes the whole HBM latency once per pass
  __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
  for (int i = tid; i < (HPIX * LDK + 64) / 2; i += NT) reinterpret_cast<uint32_t*>(halo)[i] = 0u;
  __syncthreads();

  // rolling halo: pass mf reads halo rows 2 mf .. 2 mf + 5, so rows 2 mf .. 2 mf + 3 are dead once its fragments are read (the last pass
  // frees 6) and take the NEXT tile's rows: 5 uint4 of prefetch per thread instead of a whole tile's 15.
  constexpr int NPRE = (6 * HW * CPP + NT - 1) / NT;
  typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
  u32x4 pre[NPRE];
  auto tile_coords = [&](int tile, int& f, int& ty0, int& tx0) {
    const int tx = tile % tiles_x; const int t2 = tile / tiles_x;
    ty0 = (t2 % tiles_y) * WS_TH; f = t2 / tiles_y; tx0 = tx * WS_TW;
  };
  // raw buffer loads: a pixel outside the image (or a thread beyond the row group) asks for an offset past the end and gets the zero
  // padding from the hardware -- no guards, so the loads are straight-line code the waitcnt pass can count
  const __amdgpu_buffer_rsrc_t dPr = __builtin_amdgcn_make_buffer_rsrc((void*)dP, 0, (unsigned)((long long)F * Ho * Wo * Cout * 2), 0x00020000);
  auto prefetch = [&](int f, int ty0, int tx0, int r0, int nr) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int q = tid + i * NT;
      const int px = q / CPP, ch = (q % CPP) * 8;
      const int gy = 2 * ty0 + r0 + px / HW - 1, gx = 2 * tx0 + px % HW - 1;
      const bool ok = q < nr * HW * CPP && gy >= 0 && gy < Ho && gx >= 0 && gx < Wo;
      const unsigned off = ok ? (unsigned)((((f * Ho + gy) * Wo + gx) * Cout + ch) * 2) : 0xffffffe0u;
      pre[i] = __builtin_amdgcn_raw_buffer_load_b128(dPr, off, 0, 0);
    }
  };
  auto commit = [&](int r0, int nr) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int q = tid + i * NT;
      if (q < nr * HW * CPP) *reinterpret_cast<u32x4*>(halo + (r0 * HW + q / CPP) * LDK + (q % CPP) * 8) = pre[i];
    }
  };
  // phase reduction of one finished pass: thread = (row m, pixel, 4 cins); 4 x 8-byte partials -> f32 sum -> ELU' -> 8-byte store
  static_assert(2 * 16 * (CT / 4) == NT, "one reduction item per thread");
  const int rc4 = (tid % (CT / 4)) * 4, rp = tid / (CT / 4);            // rp = m * 16 + px
  auto reduce = [&](const bf16* red, int f, int ty0, int tx0, int mf, uint2 xin) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const uint2 t = *reinterpret_cast<const uint2*>(red + (ww * 32 + rp) * LDR + rc4);
      v[0] += __uint_as_float(t.x << 16); v[1] += __uint_as_float(t.x & 0xffff0000u);
      v[2] += __uint_as_float(t.y << 16); v[3] += __uint_as_float(t.y & 0xffff0000u);
    }
    const int oy = ty0 + mf + (rp >> 4), ox = tx0 + (rp & 15), ci = n0 + rc4;
    if (oy < Hi && ox < Wi && ci < Cin) {             // Cin % 8 == 0 (dispatch)
      if constexpr (ELU) {      // layer input is an ELU output: return the gradient w.r.t. the producer's pre-activation
        const uint32_t xw[2] = {xin.x, xin.y};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float x0 = __uint_as_float(xw[e] << 16), x1 = __uint_as_float(xw[e] & 0xffff0000u);
          v[2 * e] *= x0 > 0.f ? 1.f : x0 + 1.f;
          v[2 * e + 1] *= x1 > 0.f ? 1.f : x1 + 1.f;
        }
      }
      *reinterpret_cast<uint2*>(dX + ((long long)f * Hi * Wi + (long long)oy * Wi + ox) * Cin + ci) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
    }
  };
  auto load_xin = [&](int f, int ty0, int tx0, int mf) {
    uint2 x = make_uint2(0x3f803f80u, 0x3f803f80u);
    if constexpr (ELU) {
      const int oy = ty0 + mf + (rp >> 4), ox = tx0 + (rp & 15), ci = n0 + rc4;
      if (oy < Hi && ox < Wi && ci < Cin) x = *reinterpret_cast<const uint2*>(Xelu + ((long long)f * Hi * Wi + (long long)oy * Wi + ox) * Cin + ci);
    }
    return x;
  };
  f32x4 acc[2][NFW];
  auto mfma_taps = [&](int mf, const int r) {      // the two taps (r, 0), (r, 1) of this wave's phase
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int u1 = 2 - a - 2 * r + 1, v1 = 2 - b - 2 * s + 1;      // halo offsets (u+1, v+1)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        s16x8 xb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          xb[m] = *reinterpret_cast<const s16x8*>(halo + ((2 * (mf + m) + u1) * HW + 2 * ln + v1) * LDK + ks * 32 + g * 8);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < NFW; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wd[r * 2 + s][n][ks]),
                                                                __builtin_bit_cast(bf16x8_t, xb[m]), acc[m][n], 0, 0, 0);
      }
    }
  };
  auto acc_zero = [&]() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NFW; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  auto acc_store = [&](bf16* red) {      // partial tile of this phase -> LDS: lane holds cins (half*NFW + n)*16 + g*4 + 0..3 of pixel (mf+m, ln)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < NFW; ++n)
        *reinterpret_cast<uint2*>(red + ((w * 2 + m) * 16 + ln) * LDR + (half * NFW + n) * 16 + g * 4) =
            make_uint2(pack2bf(acc[m][n][0], acc[m][n][1]), pack2bf(acc[m][n][2], acc[m][n][3]));
  };

  int tile = blockIdx.x;              // < ntiles (launcher)
  {
    int f, ty0, tx0;
    tile_coords(tile, f, ty0, tx0);
    for (int r0 = 0; r0 < HH; r0 += 6) { prefetch(f, ty0, tx0, r0, 6); commit(r0, 6); }
  }
  __syncthreads();
  int pf = 0, pty0 = 0, ptx0 = 0, pmf = -1, stage = 0;      // the pass waiting for its reduction (pmf < 0: none)
  for (; tile < ntiles; tile += gridDim.x) {
    const int next = tile + gridDim.x;
    int f, ty0, tx0, nf = 0, nty0 = 0, ntx0 = 0;
    tile_coords(tile, f, ty0, tx0);
    if (next < ntiles) tile_coords(next, nf, nty0, ntx0);
#pragma unroll 1
    for (int mf = 0; mf < WS_TH; mf += 2) {
      const int pr0 = 2 * mf, pnr = mf == WS_TH - 2 ? 6 : 4;
      if (next < ntiles) prefetch(nf, nty0, ntx0, pr0, pnr);
      uint2 xin = make_uint2(0x3f803f80u, 0x3f803f80u);
      if (pmf >= 0) xin = load_xin(pf, pty0, ptx0, pmf);
      bf16* rcur = red0 + stage * RED;
      const bf16* rprev = red0 + (stage ^ 1) * RED;
      // half 0 reduces first, half 1 between its two tap rows: one wave of a SIMD reduces while the other runs MFMAs, and every store
      // is at least half a pass old when the commit behind the barrier waits for the prefetch (vmcnt(0) waits for stores too)
      acc_zero();
      if (half == 0) {
        if (pmf >= 0) reduce(rprev, pf, pty0, ptx0, pmf, xin);
        mfma_taps(mf, 0);
        mfma_taps(mf, 1);
      } else {
        mfma_taps(mf, 0);
        if (pmf >= 0) reduce(rprev, pf, pty0, ptx0, pmf, xin);
        mfma_taps(mf, 1);
      }
      acc_store(rcur);
      __syncthreads();
      if (next < ntiles) commit(pr0, pnr);
      pf = f; pty0 = ty0; ptx0 = tx0; pmf = mf; stage ^= 1;
    }
  }
  if (pmf >= 0) reduce(red0 + (stage ^ 1) * RED, pf, pty0, ptx0, pmf, load_xin(pf, pty0, ptx0, pmf));
}

template <int KS, int NFI, bool ELU, int COUT>
static bool dgrad_ws_launch2(const void* dP, const void* Wd, void* dX, const void* Xelu, int F, int Hi, int Wi, int Cin, int Cout, hipStream_t st) {
  constexpr int CT = NFI * 16, lds = DgradWsGeo<KS, NFI>::LDS_BYTES;
  if (!stj_reserve_lds<upconv_dgrad_ws_kernel<KS, NFI, ELU, COUT>>(lds)) return false;
  if ((long long)F * 4 * Hi * Wi * Cout * 2 >= (1LL << 31)) return false;      // the halo loader addresses dP through 32-bit (int) byte offsets
  const int ntiles = ((Wi + WS_TW - 1) / WS_TW) * ((Hi + WS_TH - 1) / WS_TH) * F;
  const int ct = (Cin + CT - 1) / CT;
  int nblk = 256 / ct;
  if (nblk > ntiles) nblk = ntiles;
  if (nblk < 1) nblk = 1;
  hipLaunchKernelGGL((upconv_dgrad_ws_kernel<KS, NFI, ELU, COUT>), dim3(nblk, ct), dim3(512), lds, st, (const bf16*)dP, (const bf16*)Wd, (bf16*)dX,
                     (const bf16*)Xelu, F, Hi, Wi, Cin, ntiles);
  return true;
}
// =====================================================================================================
// Wave-specialised input gradient for the 96 <- 48 layer (round 2; the largest kernel of the step: 2 x 373 us before).
// Same decomposition as upconv_dgrad_ws_kernel (a wave per INPUT phase, tap matrices stationary, partial tiles summed through LDS),
// re-organised like upconv_fwd_ws2_kernel:
//   * waves 0-3 compute: ds_read fragments -> MFMA -> partial tile (bf16) into a step-granular, double-buffered LDS stage.  K = Cout =
//     48 is one 16x16x32 + one 16x16x16 MFMA (no zero padding to 64: 144 weight VGPRs instead of 192, which is what lets two waves
//     share a SIMD);
//   * waves 4-7 move data: sum the 4 phase partials of the PREVIOUS step, apply ELU'(x) of the layer input, store 16-byte segments;
//     and keep the dP halo rolling: the 18 x 34 halo tile is ONE buffer whose rows are overwritten with the next tile's rows as soon
//     as the current tile's steps are done with them (step s reads hi-res rows 4s .. 4s+5), fetched one step ahead in 4-5 registers.
// One workgroup barrier per step (2 low-res rows).
// =====================================================================================================
typedef __attribute__((ext_vector_type(4))) short ws_bf16x4;
// LDS layout of upconv_dgrad_ws2_kernel (bf16, 96 <- 48): the dP halo [HPIX][LDK], then two stage buffers [4 phases][2 rows][16 px][LDR]
struct DgradWs2Geo {
  static constexpr int Cout = 48, Cin = 96;
  static constexpr int LDK = Cout + 8;             // halo pixel: 48 channels + 8 pad = 7 16-byte slots (odd: conflict-free stride-2 reads)
  static constexpr int HH = 2 * WS_TH + 2, HW = 2 * WS_TW + 2, HPIX = HH * HW;
  static constexpr int LDR = Cin + 8;              // partial-tile pixel stride (bf16)
  static constexpr int RED = 4 * 2 * 16 * LDR;
  static constexpr int HALO_BYTES = HPIX * LDK * 2;      // the stage buffers follow (the kernel's red0)
  static constexpr int LDS_BYTES = HALO_BYTES + 2 * RED * 2;
  static_assert(LDS_BYTES <= 160 * 1024, "the layout fits the CU's LDS");
};
template <bool ELU, bool V3>
__global__ __launch_bounds__(512, 1) void upconv_dgrad_ws2_kernel(const bf16* __restrict__ dP, const bf16* __restrict__ Wd,
                                                                  bf16* __restrict__ dX, const bf16* __restrict__ Xelu, int F, int Hi,
                                                                  int Wi, int ntiles, int dbg) {
  using G = DgradWs2Geo;
  constexpr int Cout = G::Cout, Cin = G::Cin, NFI = 6;
  constexpr int LDK = G::LDK;
  constexpr int HH = G::HH, HW = G::HW, HPIX = G::HPIX;
  constexpr int LDR = G::LDR;
  constexpr int RED = G::RED;                      // one stage buffer: [4 phases][2 rows][16 px][LDR]
  constexpr int CPP = Cout / 8;                    // 16-byte chunks per halo pixel
  constexpr int STEPS = WS_TH / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16* halo = reinterpret_cast<bf16*>(smem_raw);
  bf16* red0 = halo + HPIX * LDK;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool mover = w >= 4;
  const int mt = tid - 256;
  const int g = lane >> 4, ln = lane & 15;
  const int tiles_x = (Wi + WS_TW - 1) / WS_TW, tiles_y = (Hi + WS_TH - 1) / WS_TH;
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  auto tile_coords = [&](int tile, int& f, int& ty0, int& tx0) {
    const int tx = tile % tiles_x; const int t2 = tile / tiles_x;
    ty0 = (t2 % tiles_y) * WS_TH; f = t2 / tiles_y; tx0 = tx * WS_TW;
  };

  if (!mover) {
    const int a = w >> 1, b = w & 1;
    // stationary weights: A[m = cin][k = cout] = Wd[(u+1)*4 + (v+1)][cin][cout], k 0..31 (16x16x32) and 32..47 (16x16x16)
    s16x8 w32[4][NFI];
    ws_bf16x4 w16[4][NFI];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = t >> 1, s2 = t & 1;
      const int uv = (2 - a - 2 * r + 1) * 4 + (2 - b - 2 * s2 + 1);
#pragma unroll
      for (int n = 0; n < NFI; ++n) {
        const bf16* wp = Wd + ((long long)uv * Cin + n * 16 + ln) * Cout;
        w32[t][n] = *reinterpret_cast<const s16x8*>(wp + g * 8);
        w16[t][n] = *reinterpret_cast<const ws_bf16x4*>(wp + 32 + g * 4);
      }
    }
    __syncthreads();                                   // first halo committed
    int q = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
      for (int st = 0; st < STEPS; ++st, ++q) {
        const int mf = 2 * st;
        bf16* red = red0 + (q & 1) * RED;
        f32x4 acc[2][NFI];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < NFI; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // Halo-row-major order (as upconv_fwd_ws2_kernel): the step's two low-res rows take their four taps from THREE hi-res halo rows of this
        // wave's parity -- row 2 mf + 1 - a (row 0's r = 1 taps), 2 mf + 3 - a (row 0's r = 0 and row 1's r = 1 taps: read ONCE), 2 mf + 5 - a
        // (row 1's r = 0 taps) -- 6 fragment pairs instead of 8, fetched DG_PF groups ahead of their MFMAs through a ring; row 0's partial
        // tile is packed and staged in front of the last halo row's MFMAs.
        {
          constexpr int PF = DG_PF, NG = 6;
          auto fragp = [&](const int gi) { return halo + ((2 * mf + 2 * (gi >> 1) + 1 - a) * HW + 2 * ln + (2 - b - 2 * (gi & 1) + 1)) * LDK; };
          s16x8 x32r[PF + 1];
          ws_bf16x4 x16r[PF + 1];
#pragma unroll
          for (int i = 0; i < PF; ++i) { x32r[i] = *reinterpret_cast<const s16x8*>(fragp(i) + g * 8); x16r[i] = *reinterpret_cast<const ws_bf16x4*>(fragp(i) + 32 + g * 4); }
#pragma unroll
          for (int gi = 0; gi < NG; ++gi) {
            if (gi + PF < NG) {
              x32r[(gi + PF) % (PF + 1)] = *reinterpret_cast<const s16x8*>(fragp(gi + PF) + g * 8);
              x16r[(gi + PF) % (PF + 1)] = *reinterpret_cast<const ws_bf16x4*>(fragp(gi + PF) + 32 + g * 4);
            }
            const int hr = gi >> 1, s2 = gi & 1;
            const s16x8 x32 = x32r[gi % (PF + 1)];
            const ws_bf16x4 x16 = x16r[gi % (PF + 1)];
            if (hr >= 1) {            // tap row r = 0 of low-res row hr - 1
#pragma unroll
              for (int n = 0; n < NFI; ++n)
                acc[hr - 1][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w32[s2][n]), __builtin_bit_cast(bf16x8_t, x32), acc[hr - 1][n], 0, 0, 0);
#pragma unroll
              for (int n = 0; n < NFI; ++n) acc[hr - 1][n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w16[s2][n], x16, acc[hr - 1][n], 0, 0, 0);
            }
            if (hr <= 1) {            // tap row r = 1 of low-res row hr
#pragma unroll
              for (int n = 0; n < NFI; ++n)
                acc[hr][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w32[2 + s2][n]), __builtin_bit_cast(bf16x8_t, x32), acc[hr][n], 0, 0, 0);
#pragma unroll
              for (int n = 0; n < NFI; ++n) acc[hr][n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w16[2 + s2][n], x16, acc[hr][n], 0, 0, 0);
            }
            if (gi == 3 || gi == 5) {
              const int m = gi == 3 ? 0 : 1;
#pragma unroll
              for (int n = 0; n < NFI; ++n)
                *reinterpret_cast<uint2*>(red + ((w * 2 + m) * 16 + ln) * LDR + n * 16 + g * 4) =
                    make_uint2(pack2bf(acc[m][n][0], acc[m][n][1]), pack2bf(acc[m][n][2], acc[m][n][3]));
            }
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();
  } else if constexpr (V3) {
    // ------------------------------------------------------------------ mover role, straight-line version (whole tiles only)
    // The first mover (below) guards every load and store (image border, ragged tile, group size, end of the tile stream).  Each
    // guard is a branch, and with memory operations under divergent branches the compiler gives up counting: every use of a
    // prefetched register waits on vmcnt(0) -- i.e. on the loads issued a few instructions earlier, which were meant to stay in
    // flight for two steps (ablation: 318 us, of which the movers alone 277; without the sum 208).  Here every load, LDS write and
    // store of a step is unconditional: out-of-image addresses are clamped and the value zeroed when it is committed, a thread's
    // surplus chunk of a short group repeats its previous chunk (same address, same data), a tile index past the end is clamped to
    // the last tile (its groups are fetched and committed again: dead rows, never read), the 384 16-byte items of a step are one
    // item + one half item per thread.  The waits then carry exact counts and the two-step lookahead is real.
    constexpr int NP4 = (4 * HW * CPP + 255) / 256, NP6 = (6 * HW * CPP + 255) / 256;     // 4, 5 chunks per thread
    int cgeo[NP6];                                       // row | col << 8 | channel-chunk << 16 of chunk i (row < 6, col < 34)
#pragma unroll
    for (int i = 0; i < NP6; ++i) {
      const int c = mt + i * 256, px = c / CPP;
      cgeo[i] = (px / HW) | ((px % HW) << 8) | ((c % CPP) << 16);
    }
    uint4 preA[NP6], preB[NP6];
    int mskA = 0, mskB = 0;                              // bit i: chunk i of the set lies inside the image
    const int last_tile = ntiles - 1;
    // group n = 4 * (local tile) + j; J = n & 3 is a compile-time constant at every call site
    auto prefetch = [&](uint4 (&pre)[NP6], int& msk, int n, auto JC) {
      constexpr int J = decltype(JC)::value, NR = J == 3 ? 6 : 4, NP = J == 3 ? NP6 : NP4;
      int tile = blockIdx.x + (n >> 2) * (int)gridDim.x;
      tile = tile < last_tile ? tile : last_tile;
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
      const int y0 = 2 * ty0 + 4 * J - 1, x0 = 2 * tx0 - 1;
      const bf16* Pf = dP + (long long)f * Ho * Wo * Cout;
      int m = 0;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int ge = (i > 0 && (cgeo[i] & 0xff) >= NR) ? cgeo[i - 1] : cgeo[i];
        const int gy = y0 + (ge & 0xff), gx = x0 + ((ge >> 8) & 0xff), ch = (ge >> 16) * 8;
        const int cy = min(max(gy, 0), Ho - 1), cx = min(max(gx, 0), Wo - 1);
        m |= (cy == gy && cx == gx) ? (1 << i) : 0;
        pre[i] = *reinterpret_cast<const uint4*>(Pf + (cy * Wo + cx) * Cout + ch);
      }
      msk = m;
    };
    auto commit = [&](const uint4 (&pre)[NP6], int msk, auto JC) {
      constexpr int J = decltype(JC)::value, NR = J == 3 ? 6 : 4, NP = J == 3 ? NP6 : NP4;
      // the zeroing of out-of-image chunks must not be scheduled above the barrier that precedes this commit (it would wait for the
      // loads a step early): the mask goes through a volatile asm, which keeps its uses below it
      int m = msk;
      asm volatile("" : "+v"(m));
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int ge = (i > 0 && (cgeo[i] & 0xff) >= NR) ? cgeo[i - 1] : cgeo[i];
        const bool in = (m >> i) & 1;
        const uint4 v = make_uint4(in ? pre[i].x : 0u, in ? pre[i].y : 0u, in ? pre[i].z : 0u, in ? pre[i].w : 0u);
        *reinterpret_cast<uint4*>(halo + ((4 * J + (ge & 0xff)) * HW + ((ge >> 8) & 0xff)) * LDK + (ge >> 16) * 8) = v;
      }
    };
    // items of a step: A = 16 bytes (8 channels) of pixel mt / 12; B = 8 bytes (4 channels) of the remaining 128 items, two threads each
    const int ppA = mt / 12, cA = (mt % 12) * 8;
    const int itB = 256 + (mt >> 1), ppB = itB / 12, cB = (itB % 12) * 8 + (mt & 1) * 4;
    uint4 xA = make_uint4(0, 0, 0, 0);
    uint2 xB = make_uint2(0, 0);
    auto item_off = [&](int f, int ty0, int tx0, int st, int pp, int c) {
      return ((long long)f * Hi * Wi + (long long)(ty0 + 2 * st + (pp >> 4)) * Wi + tx0 + (pp & 15)) * Cin + c;
    };
    auto fetch_x = [&](int f, int ty0, int tx0, int st) {
      if constexpr (ELU) {
        xA = *reinterpret_cast<const uint4*>(Xelu + item_off(f, ty0, tx0, st, ppA, cA));
        xB = *reinterpret_cast<const uint2*>(Xelu + item_off(f, ty0, tx0, st, ppB, cB));
      }
    };
    auto elu2 = [](float& v0, float& v1, uint32_t xw) {      // v *= ELU'(x) = min(x, 0) + 1
      const float x0 = __uint_as_float(xw << 16), x1 = __uint_as_float(xw & 0xffff0000u);
      v0 = fmaf(v0, fminf(x0, 0.f), v0);
      v1 = fmaf(v1, fminf(x1, 0.f), v1);
    };
    auto reduce = [&](const bf16* red, int f, int ty0, int tx0, int st) {
      // x was fetched a step ago; without this pin its unpacking (pure register arithmetic) is scheduled ABOVE the preceding barrier,
      // into the step that issued the loads, and waits for them there
      uint4 xa = xA; uint2 xb = xB;
      if constexpr (ELU) asm volatile("" : "+v"(xa.x), "+v"(xa.y), "+v"(xa.z), "+v"(xa.w), "+v"(xb.x), "+v"(xb.y));
      {
        const bf16* rp = red + ((ppA >> 4) * 16 + (ppA & 15)) * LDR + cA;
        float v[8], t[8];
        ld16<bf16>(rp, v);
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
          ld16<bf16>(rp + ww * 2 * 16 * LDR, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += t[e];
        }
        if constexpr (ELU) { elu2(v[0], v[1], xa.x); elu2(v[2], v[3], xa.y); elu2(v[4], v[5], xa.z); elu2(v[6], v[7], xa.w); }
        *reinterpret_cast<uint4*>(dX + item_off(f, ty0, tx0, st, ppA, cA)) =
            make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
      }
      {
        const bf16* rp = red + ((ppB >> 4) * 16 + (ppB & 15)) * LDR + cB;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
          const uint2 u = *reinterpret_cast<const uint2*>(rp + ww * 2 * 16 * LDR);
          v[0] += __uint_as_float(u.x << 16); v[1] += __uint_as_float(u.x & 0xffff0000u);
          v[2] += __uint_as_float(u.y << 16); v[3] += __uint_as_float(u.y & 0xffff0000u);
        }
        if constexpr (ELU) { elu2(v[0], v[1], xb.x); elu2(v[2], v[3], xb.y); }
        *reinterpret_cast<uint2*>(dX + item_off(f, ty0, tx0, st, ppB, cB)) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
      }
    };
    using J0 = std::integral_constant<int, 0>; using J1 = std::integral_constant<int, 1>;
    using J2 = std::integral_constant<int, 2>; using J3 = std::integral_constant<int, 3>;
    // first tile of the block: whole halo, synchronously; groups 3 (again: step 0 commits it) and 4 go in flight
    prefetch(preA, mskA, 0, J0{}); commit(preA, mskA, J0{});
    prefetch(preA, mskA, 1, J1{}); commit(preA, mskA, J1{});
    prefetch(preA, mskA, 2, J2{}); commit(preA, mskA, J2{});
    prefetch(preB, mskB, 3, J3{}); commit(preB, mskB, J3{});
    prefetch(preA, mskA, 4, J0{});
    __syncthreads();
    int q = 0, pf = 0, pty = 0, ptx = 0;
    // one mover step: roll the halo (commit group q + 3, fetch group q + 5), sum + store the previous step's partials (their x
    // operand was fetched last step), fetch this step's x.  FIRST: there is no previous step.
    auto step = [&](uint4 (&pre)[NP6], int& msk, int f, int ty0, int tx0, auto STC, auto FIRSTC) {
      constexpr int ST = decltype(STC)::value;
      constexpr bool FIRST = decltype(FIRSTC)::value;
      commit(pre, msk, std::integral_constant<int, (ST + 3) & 3>{});
      prefetch(pre, msk, q + 5, std::integral_constant<int, (ST + 1) & 3>{});
      if constexpr (!FIRST) reduce(red0 + ((q - 1) & 1) * RED, pf, pty, ptx, (ST + 3) & 3);
      fetch_x(f, ty0, tx0, ST);
      pf = f; pty = ty0; ptx = tx0;
      ++q;
      __syncthreads();
    };
    using T_ = std::true_type; using F_ = std::false_type;
    int tile = blockIdx.x;
    if (tile < ntiles) {
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
      step(preB, mskB, f, ty0, tx0, J0{}, T_{});
      step(preA, mskA, f, ty0, tx0, J1{}, F_{});
      step(preB, mskB, f, ty0, tx0, J2{}, F_{});
      step(preA, mskA, f, ty0, tx0, J3{}, F_{});
      for (tile += gridDim.x; tile < ntiles; tile += gridDim.x) {
        tile_coords(tile, f, ty0, tx0);
        step(preB, mskB, f, ty0, tx0, J0{}, F_{});
        step(preA, mskA, f, ty0, tx0, J1{}, F_{});
        step(preB, mskB, f, ty0, tx0, J2{}, F_{});
        step(preA, mskA, f, ty0, tx0, J3{}, F_{});
      }
      reduce(red0 + ((q - 1) & 1) * RED, pf, pty, ptx, 3);
    }
    __syncthreads();
  } else {
    // ------------------------------------------------------------------ mover role
    // halo row groups: j = 0..2 -> rows 4j .. 4j+3 ; j = 3 -> rows 12 .. 17
    constexpr int NPF = (6 * HW * CPP + 255) / 256;      // chunks per thread of the largest group
    // Group n of the block's stream (n = 4 * local tile + j; j = 0..2 -> halo rows 4j .. 4j+3, j = 3 -> rows 12 .. 17) is committed at
    // step n - 3 -- step s of a tile reads rows 4s .. 4s+5, so the rows are dead for the current tile by then -- and FETCHED two steps
    // before that, into one of two register sets (n & 1): 2 x 20 KB of loads in flight per CU.  (One step of lookahead left the movers
    // latency-bound: movers alone 205 us against 147 us for the compute waves alone; two steps: 161 us.  Measured and rejected: the two
    // duties on separate wave pairs (250 vs 228 us), and an LDS-DMA roller -- global_load_lds_dwordx4 straight into the halo rows, counted
    // vmcnt, raw s_barrier: correct, but a group can only be ISSUED once its rows are dead, which leaves ~1 group in flight: 315 us.)
    uint4 preA[NPF], preB[NPF];
    auto grp_rows = [](int j, int& r0, int& nr) { r0 = 4 * j; nr = j == 3 ? 6 : 4; };
    auto grp_tile = [&](int n) { return blockIdx.x + (n >> 2) * (int)gridDim.x; };
    // chunk geometry of this thread inside a group (the same for every group and tile: the divisions by 6 and 34 per chunk, twice per
    // step, were a third of the movers' VALU instructions -- and the movers share their SIMDs with the compute waves)
    int cgeo[NPF];                                       // row | col << 8 | channel-chunk << 16 of chunk i (row < 6, col < 34)
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int c = mt + i * 256, px = c / CPP;
      cgeo[i] = (px / HW) | ((px % HW) << 8) | ((c % CPP) << 16);
    }
    auto prefetch = [&](uint4 (&pre)[NPF], int n) {
      const int tile = grp_tile(n);
      if (tile >= ntiles) return;
      int f, ty0, tx0, r0, nr;
      tile_coords(tile, f, ty0, tx0);
      grp_rows(n & 3, r0, nr);
      const int y0 = 2 * ty0 + r0 - 1, x0 = 2 * tx0 - 1;
      const bf16* Pf = dP + (long long)f * Ho * Wo * Cout;
#pragma unroll
      for (int i = 0; i < NPF; ++i) {
        const int row = cgeo[i] & 0xff, col = (cgeo[i] >> 8) & 0xff, ch = (cgeo[i] >> 16) * 8;
        const int gy = y0 + row, gx = x0 + col;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < nr && (unsigned)gy < (unsigned)Ho && (unsigned)gx < (unsigned)Wo) v = *reinterpret_cast<const uint4*>(Pf + ((long long)gy * Wo + gx) * Cout + ch);
        pre[i] = v;
      }
    };
    auto commit = [&](const uint4 (&pre)[NPF], int n) {
      if (grp_tile(n) >= ntiles) return;
      int r0, nr;
      grp_rows(n & 3, r0, nr);
#pragma unroll
      for (int i = 0; i < NPF; ++i) {
        const int row = cgeo[i] & 0xff, col = (cgeo[i] >> 8) & 0xff, ch = (cgeo[i] >> 16) * 8;
        if (row < nr) *reinterpret_cast<uint4*>(halo + ((r0 + row) * HW + col) * LDK + ch) = pre[i];
      }
    };
    constexpr int NIT = 2 * 16 * (Cin / 8);              // 8-channel items of one step
    constexpr int NEP = (NIT + 255) / 256;
    // ELU' operand (the layer input x) of step q's pixels: fetched during step q, used when step q's partials are summed (step q + 1)
    uint4 xin[ELU ? NEP : 1];
    auto fetch_x = [&](int f, int ty0, int tx0, int st) {
      if constexpr (ELU) {
#pragma unroll
        for (int i = 0; i < NEP; ++i) {
          const int c = mt + i * 256;
          const int c8 = (c % (Cin / 8)) * 8, pp = c / (Cin / 8);
          const int oy = ty0 + 2 * st + (pp >> 4), ox = tx0 + (pp & 15);
          xin[i] = make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
          if (c < NIT && oy < Hi && ox < Wi) xin[i] = *reinterpret_cast<const uint4*>(Xelu + ((long long)f * Hi * Wi + (long long)oy * Wi + ox) * Cin + c8);
        }
      }
    };
    auto reduce = [&](const bf16* red, int f, int ty0, int tx0, int st) {
      bf16* Xf = dX + (long long)f * Hi * Wi * Cin;
#pragma unroll
      for (int i = 0; i < NEP; ++i) {
        const int c = mt + i * 256;
        if (c >= NIT) break;
        const int c8 = (c % (Cin / 8)) * 8, pp = c / (Cin / 8);
        const int m = pp >> 4, px = pp & 15;
        const int oy = ty0 + 2 * st + m, ox = tx0 + px;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
          float t[8];
          ld16<bf16>(red + ((ww * 2 + m) * 16 + px) * LDR + c8, t);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += t[e];
        }
        if (oy < Hi && ox < Wi) {
          if constexpr (ELU) {
            const uint32_t xw[4] = {xin[i].x, xin[i].y, xin[i].z, xin[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float x0 = __uint_as_float(xw[e] << 16), x1 = __uint_as_float(xw[e] & 0xffff0000u);
              v[2 * e] *= x0 > 0.f ? 1.f : x0 + 1.f;
              v[2 * e + 1] *= x1 > 0.f ? 1.f : x1 + 1.f;
            }
          }
          *reinterpret_cast<uint4*>(Xf + ((long long)oy * Wi + ox) * Cin + c8) =
              make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
        }
      }
    };
    // first tile of the block: whole halo, synchronously; then the first group of the second tile goes in flight
    int tile = blockIdx.x;
    if (tile < ntiles)
      for (int j = 0; j < 4; ++j) { prefetch(preA, j); commit(preA, j); }
    prefetch(preA, 4);
    __syncthreads();
    int q = 0, pf = 0, pty = 0, ptx = 0, pst = 0;
    bool have = false;
    // one mover step: roll the halo, sum + store the previous step's partials (its x operand was fetched last step)
    auto step = [&](uint4 (&pre)[NPF], int f, int ty0, int tx0, int st) {
      if (q >= 1) commit(pre, q + 3);                    // rows dead for the current tile from this step on
      if (!(dbg & 8)) prefetch(pre, q + 5);
      if (have && !(dbg & 4)) reduce(red0 + ((q - 1) & 1) * RED, pf, pty, ptx, pst);
      fetch_x(f, ty0, tx0, st);
      pf = f; pty = ty0; ptx = tx0; pst = st; have = true;
      ++q;
      __syncthreads();
    };
    for (; tile < ntiles; tile += gridDim.x) {
      int f, ty0, tx0;
      tile_coords(tile, f, ty0, tx0);
      // group n lives in register set n & 1; step q handles groups q + 3 (commit) and q + 5 (fetch): set B on even q, set A on odd q
      step(preB, f, ty0, tx0, 0);
      step(preA, f, ty0, tx0, 1);
      step(preB, f, ty0, tx0, 2);
      step(preA, f, ty0, tx0, 3);
    }
    if (have) reduce(red0 + ((q - 1) & 1) * RED, pf, pty, ptx, pst);
    __syncthreads();
  }
}

template <bool ELU, bool V3>
static bool dgrad_ws2_launch(const void* dP, const void* Wd, void* dX, const void* Xelu, int F, int Hi, int Wi, hipStream_t st) {
  constexpr int lds = DgradWs2Geo::LDS_BYTES;
  if (!stj_reserve_lds<upconv_dgrad_ws2_kernel<ELU, V3>>(lds)) return false;
  const int ntiles = ((Wi + WS_TW - 1) / WS_TW) * ((Hi + WS_TH - 1) / WS_TH) * F;
  const int nblk = ntiles < 256 ? ntiles : 256;
  const int dbg = 0;      // (role-ablation mask of the kernel; profiling builds only)
  hipLaunchKernelGGL((upconv_dgrad_ws2_kernel<ELU, V3>), dim3(nblk), dim3(512), lds, st, (const bf16*)dP, (const bf16*)Wd, (bf16*)dX, (const bf16*)Xelu, F, Hi, Wi, ntiles, dbg);
  return true;
}

template <int KS, int NFI, int COUT>
static bool dgrad_ws_launch(const void* dP, const void* Wd, void* dX, const void* Xelu, int F, int Hi, int Wi, int Cin, int Cout, hipStream_t st) {
  return Xelu ? dgrad_ws_launch2<KS, NFI, true, COUT>(dP, Wd, dX, Xelu, F, Hi, Wi, Cin, Cout, st)
              : dgrad_ws_launch2<KS, NFI, false, COUT>(dP, Wd, dX, Xelu, F, Hi, Wi, Cin, Cout, st);
}
bool upconv_dgrad_ws_try(const void* dP, const void* Wd, void* dX, const void* Xelu, int F, int Hi, int Wi, int Cin, int Cout, hipStream_t st) {
  if (Cout % 8 || Cin % 8) return false;
  if (Cout == 48 && Cin == 96) {
    if (Hi % WS_TH == 0 && Wi % WS_TW == 0)      // whole tiles: straight-line movers (ragged ones: the guarded form)
      return Xelu ? dgrad_ws2_launch<true, true>(dP, Wd, dX, Xelu, F, Hi, Wi, st) : dgrad_ws2_launch<false, true>(dP, Wd, dX, Xelu, F, Hi, Wi, st);
    return Xelu ? dgrad_ws2_launch<true, false>(dP, Wd, dX, Xelu, F, Hi, Wi, st) : dgrad_ws2_launch<false, false>(dP, Wd, dX, Xelu, F, Hi, Wi, st);
  }
  if (Cout == 96 && Cin == 128) return dgrad_ws_launch<3, 4, 96>(dP, Wd, dX, Xelu, F, Hi, Wi, Cin, Cout, st);
  return false;
}
