// The model's inputs from agent tracks, on the device: the reference's L0 layer (data_preprocessing.py:145-213,262-273,360-363 and
// grid_utils.py:18-77,438-607) without TensorFlow.  Three launches, no floating-point atomics, no host sync, no allocation:
//   stj_raster_boxes    per (scene, agent, step) one box record in the SDC's frame + its pixel bounding box; per scene the frame and ok
//   stj_raster_grids    ogm [B,G,G,11,2] and vec_flow [B,G,G,2]: one workgroup per (scene, 64 x 16 pixel tile)
//   stj_raster_actors   the actor masks, distances, ranks, obs [B,48,11,8] and occ [B,16,11,8]: one workgroup per scene
// Semantics: strajnet_amd/raster.py, raster_reference; the rules and the workspace layout: raster.h.
#include "common.h"
#include "raster.h"

#define RST_NT 256
#define RST_CHUNK 1024                      // records culled per pass of a tile's workgroup
#define RST_TILE_PX (RST_TILE_W * RST_TILE_H)

__global__ __launch_bounds__(RST_NT) void raster_boxes_kernel(const float* __restrict__ state, const int* __restrict__ type,
                                                              const int* __restrict__ is_sdc, float* __restrict__ box, int* __restrict__ aabb,
                                                              float* __restrict__ frame, int* __restrict__ ok, int B, int A, int G, float ppm,
                                                              float sdc_px, float sdc_py) {
  __shared__ int s_sdc;
  const int b = blockIdx.y;
  if (threadIdx.x == 0) s_sdc = A;
  __syncthreads();
  for (int a = threadIdx.x; a < A; a += RST_NT)
    if (is_sdc[(long long)b * A + a] == 1) atomicMin(&s_sdc, a);      // the lowest index: the reference's gather assumes exactly one
  __syncthreads();
  const int sdc = s_sdc;
  const long long plane = (long long)B * A * RST_STEPS;      // state [8, B, A, 11]: x y yaw length width vx vy valid
  rst_frame_t f = rst_frame(0.f, 0.f, 0.f);
  if (sdc < A) {
    const long long at = ((long long)b * A + sdc) * RST_STEPS + RST_CUR;
    f = rst_frame(state[at], state[plane + at], state[2 * plane + at]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float* fr = frame + (long long)b * 8;
    const bool have = sdc < A;
    fr[0] = have ? f.x : 0.f; fr[1] = have ? f.y : 0.f; fr[2] = have ? f.yaw : 0.f; fr[3] = have ? f.angle : 0.f;
    fr[4] = have ? f.c : 0.f; fr[5] = have ? f.s : 0.f; fr[6] = have ? (float)sdc : -1.f; fr[7] = have ? 1.f : 0.f;
    ok[b] = have ? 1 : 0;
  }
  const int r = blockIdx.x * RST_NT + threadIdx.x;      // a * 11 + t
  if (r >= A * RST_STEPS) return;
  const long long at = (long long)b * A * RST_STEPS + r;
  float w[RST_BOX_WORDS];
  int q[4] = {0, 0, -1, -1};
  if (sdc < A) {
    const rst_box_t bx = rst_box(f, state[at], state[plane + at], state[2 * plane + at], state[3 * plane + at], state[4 * plane + at],
                                 state[5 * plane + at], state[6 * plane + at], type[(long long)b * A + r / RST_STEPS], state[7 * plane + at]);
    rst_box_store(bx, w);
    rst_aabb(bx, ppm, sdc_px, sdc_py, G, q);
  } else {
    for (int i = 0; i < RST_BOX_WORDS; ++i) w[i] = 0.f;      // a scene without an SDC: all-zero outputs, nothing is clamped
  }
  float4* dst = reinterpret_cast<float4*>(box + at * RST_BOX_WORDS);
  dst[0] = make_float4(w[0], w[1], w[2], w[3]);
  dst[1] = make_float4(w[4], w[5], w[6], w[7]);
  dst[2] = make_float4(w[8], w[9], w[10], w[11]);
  reinterpret_cast<int4*>(aabb)[at] = make_int4(q[0], q[1], q[2], q[3]);
}

__device__ __forceinline__ rst_box_t raster_load_box(const float* __restrict__ p) {
  const float4* s = reinterpret_cast<const float4*>(p);
  const float4 a = s[0], b = s[1], c = s[2];
  const float w[RST_BOX_WORDS] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
  return rst_box_load(w);
}

// One workgroup per (scene, tile).  LDS per pixel: the occupancy planes as bits, the flow count and the two displacement sums, all
// integers: OR and integer add commute, so the result does not depend on the order the waves arrive in.  The tile then leaves in whole rows.
__global__ __launch_bounds__(RST_NT) void raster_grids_kernel(const float* __restrict__ box, const int* __restrict__ aabb, float* __restrict__ ogm,
                                                              float* __restrict__ flow, int A, int G, float ppm, float sdc_px, float sdc_py, int nl,
                                                              int nw, int tiles_x) {
  __shared__ uint32_t s_occ[RST_TILE_PX];
  __shared__ uint32_t s_cnt[RST_TILE_PX];
  __shared__ unsigned long long s_sx[RST_TILE_PX], s_sy[RST_TILE_PX];
  __shared__ uint32_t s_list[RST_CHUNK];
  __shared__ uint32_t s_n;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = (blockIdx.x % tiles_x) * RST_TILE_W, ty0 = (blockIdx.x / tiles_x) * RST_TILE_H;
  const int tw = min(RST_TILE_W, G - tx0), th = min(RST_TILE_H, G - ty0);
  const int tx1 = tx0 + tw - 1, ty1 = ty0 + th - 1;
  for (int i = tid; i < RST_TILE_PX; i += RST_NT) { s_occ[i] = 0u; s_cnt[i] = 0u; s_sx[i] = 0ull; s_sy[i] = 0ull; }
  const int R = A * RST_STEPS, np = nl * nw;
  const float* sbox = box + (long long)b * R * RST_BOX_WORDS;
  const int4* sq = reinterpret_cast<const int4*>(aabb) + (long long)b * R;
  for (int r0 = 0; r0 < R; r0 += RST_CHUNK) {
    if (tid == 0) s_n = 0u;
    __syncthreads();
    for (int r = r0 + tid; r < min(R, r0 + RST_CHUNK); r += RST_NT) {
      const int4 q = sq[r];
      if (q.z >= q.x && q.x <= tx1 && q.z >= tx0 && q.y <= ty1 && q.w >= ty0) s_list[atomicAdd(&s_n, 1u)] = (uint32_t)r;      // at most RST_CHUNK per pass
    }
    __syncthreads();
    const int n = (int)s_n;
    for (int e = wave; e < n; e += RST_NT / 64) {
      const int r = (int)s_list[e], t = r % RST_STEPS;
      const rst_box_t bx = raster_load_box(sbox + (long long)r * RST_BOX_WORDS);
      const uint32_t planes = rst_plane_mask(t, bx.cls);
      // vec_flow (data_preprocessing.py:360-363): vehicles, valid at the current step and at step 0, rendered at the current step
      bool do_flow = t == RST_CUR && bx.cls == 0;
      rst_box_t b0 = bx;
      if (do_flow) {
        b0 = raster_load_box(sbox + (long long)(r - RST_CUR) * RST_BOX_WORDS);
        do_flow = b0.valid != 0;
      }
      for (int p = lane; p < np; p += 64) {
        const int i = p / nw, j = p - i * nw;
        float x, y, px, py;
        rst_point(bx, i, j, nl, nw, &x, &y);
        rst_pixel(x, y, ppm, sdc_px, sdc_py, &px, &py);
        if (!rst_in_grid(px, py, G, 0)) continue;
        const int ix = (int)px, iy = (int)py;
        if (ix < tx0 || ix > tx1 || iy < ty0 || iy > ty1) continue;
        const int pix = (iy - ty0) * RST_TILE_W + (ix - tx0);
        atomicOr(&s_occ[pix], planes);
        if (do_flow) {
          float x0, y0, px0, py0;
          rst_point(b0, i, j, nl, nw, &x0, &y0);
          rst_pixel(x0, y0, ppm, sdc_px, sdc_py, &px0, &py0);
          atomicAdd(&s_cnt[pix], 1u);
          atomicAdd(&s_sx[pix], (unsigned long long)((long long)px0 - (long long)ix));
          atomicAdd(&s_sy[pix], (unsigned long long)((long long)py0 - (long long)iy));
        }
      }
    }
    __syncthreads();
  }
  // ---- the tile leaves in whole rows: tw x 22 contiguous floats of ogm, tw x 2 of vec_flow
  const long long row0 = ((long long)b * G + ty0) * G + tx0;      // pixel index of the tile's first pixel
  const bool vec = (G & 1) == 0;                                  // then every run starts and ends on 16 bytes
  const int run = tw * RST_NPLANES;
  if (vec) {
    const int rq = run / 4;
    for (int idx = tid; idx < th * rq; idx += RST_NT) {
      const int row = idx / rq, f = (idx - row * rq) * 4;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = (f + k) / RST_NPLANES, pl = (f + k) - px * RST_NPLANES;
        v[k] = (float)((s_occ[row * RST_TILE_W + px] >> pl) & 1u);
      }
      *reinterpret_cast<float4*>(ogm + (row0 + (long long)row * G) * RST_NPLANES + f) = make_float4(v[0], v[1], v[2], v[3]);
    }
    const int fq = tw * 2 / 4;
    for (int idx = tid; idx < th * fq; idx += RST_NT) {
      const int row = idx / fq, px = (idx - row * fq) * 2;
      float v[4];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int pix = row * RST_TILE_W + px + k;
        const uint32_t c = s_cnt[pix];
        v[2 * k] = c ? (float)((double)(long long)s_sx[pix] / (double)c) : 0.f;      // divide_no_nan (grid_utils.py:398-435)
        v[2 * k + 1] = c ? (float)((double)(long long)s_sy[pix] / (double)c) : 0.f;
      }
      *reinterpret_cast<float4*>(flow + (row0 + (long long)row * G + px) * 2) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
    for (int idx = tid; idx < th * run; idx += RST_NT) {
      const int row = idx / run, f = idx - row * run, px = f / RST_NPLANES, pl = f - px * RST_NPLANES;
      ogm[(row0 + (long long)row * G) * RST_NPLANES + f] = (float)((s_occ[row * RST_TILE_W + px] >> pl) & 1u);
    }
    for (int idx = tid; idx < th * tw * 2; idx += RST_NT) {
      const int row = idx / (tw * 2), f = idx - row * tw * 2, pix = row * RST_TILE_W + (f >> 1);
      const uint32_t c = s_cnt[pix];
      const long long s = (long long)((f & 1) ? s_sy[pix] : s_sx[pix]);
      flow[(row0 + (long long)row * G) * 2 + f] = c ? (float)((double)s / (double)c) : 0.f;
    }
  }
}

// One workgroup per scene: grid_utils.py:555-584 (masks, actor_traj) and data_preprocessing.py:145-213 (selection), restated literally --
// including its index mix-up: the distance list of `obs` is compacted over the in_box agents WITH a valid step, yet valid_actor[d] and
// valid_type[d] index the in_box list that still holds the agents without one (data_preprocessing.py:154-174).
__global__ __launch_bounds__(RST_NT) void raster_actors_kernel(const float* __restrict__ box, const int* __restrict__ type, const int* __restrict__ ok,
                                                               int* __restrict__ mask, float* __restrict__ dist, int* __restrict__ rank,
                                                               float* __restrict__ obs, float* __restrict__ occ, int A, int Gf, float ppm,
                                                               float fov_px, float fov_py) {
  __shared__ uint8_t s_mask[RST_MAX_AGENTS];
  __shared__ float s_dl[RST_MAX_AGENTS];
  __shared__ int s_ulist[RST_MAX_AGENTS];                     // the in_box agents in index order
  __shared__ int s_src[RST_MAX_OBS + RST_MAX_OCC];            // the agent each output row is taken from, -1: zero padding
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* sbox = box + (long long)b * A * RST_STEPS * RST_BOX_WORDS;
  const int* stype = type + (long long)b * A;
  const bool live = ok[b] != 0;
  for (int i = tid; i < RST_MAX_OBS + RST_MAX_OCC; i += RST_NT) s_src[i] = -1;
  for (int a = tid; a < A; a += RST_NT) {
    int m = 0, first = -1, last = -1;
    float dl = 0.f, df = 0.f;
    if (live) {
      bool inbox = false;
      rst_box_t cur;
      for (int t = 0; t < RST_STEPS; ++t) {
        const rst_box_t bx = raster_load_box(sbox + ((long long)a * RST_STEPS + t) * RST_BOX_WORDS);
        for (int k = 0; k < 4; ++k) {      // no validity check here: grid_utils.py:562-575 has none
          float x, y, px, py;
          rst_corner(bx, k, &x, &y);
          rst_pixel(x, y, ppm, fov_px, fov_py, &px, &py);
          inbox |= rst_in_grid(px, py, Gf, 0);
        }
        if (bx.valid) {
          const float d = sqrtf(bx.cx * bx.cx + bx.cy * bx.cy);
          if (first < 0) { first = t; df = d; }
          last = t; dl = d;
        }
        if (t == RST_CUR) cur = bx;
      }
      float px, py;
      rst_pixel(cur.cx, cur.cy, ppm, fov_px, fov_py, &px, &py);
      const bool occu = rst_in_grid(px, py, Gf, RST_OCC_MARGIN) && !inbox;
      m = (inbox ? RST_MASK_INBOX : 0) | (occu ? RST_MASK_OCCU : 0) | (last >= 0 ? RST_MASK_VALID : 0) | (last >= 0 && df > dl ? RST_MASK_AWAY : 0);
    }
    s_mask[a] = (uint8_t)m;
    s_dl[a] = dl;
    mask[(long long)b * A + a] = m;
    dist[((long long)b * A + a) * 2] = dl;
    dist[((long long)b * A + a) * 2 + 1] = df;
  }
  __syncthreads();
  const int OBS = RST_MASK_INBOX | RST_MASK_VALID, OCC = RST_MASK_OCCU | RST_MASK_VALID | RST_MASK_AWAY;
  for (int a = tid; a < A; a += RST_NT) {
    const int m = s_mask[a];
    if (m & RST_MASK_INBOX) {
      int pu = 0;
      for (int o = 0; o < a; ++o) pu += s_mask[o] & RST_MASK_INBOX;
      s_ulist[pu] = a;
    }
  }
  __syncthreads();
  for (int a = tid; a < A; a += RST_NT) {
    const int m = s_mask[a];
    const float d = s_dl[a];
    int r_obs = -1, r_occ = -1;
    if ((m & OBS) == OBS) {      // ties break by agent index (np.argsort leaves them unspecified)
      int k = 0, r = 0;
      for (int o = 0; o < A; ++o) {
        if ((s_mask[o] & OBS) != OBS) continue;
        k += o < a;
        r += s_dl[o] < d || (s_dl[o] == d && o < a);
      }
      if (r < RST_MAX_OBS) { r_obs = r; s_src[r] = s_ulist[k]; }      // the compacted index k applied to the uncompacted list
    }
    if ((m & OCC) == OCC) {
      int r = 0;
      for (int o = 0; o < A; ++o) r += (s_mask[o] & OCC) == OCC && (s_dl[o] < d || (s_dl[o] == d && o < a));
      if (r < RST_MAX_OCC) { r_occ = r; s_src[RST_MAX_OBS + r] = a; }
    }
    rank[((long long)b * A + a) * 2] = r_obs;
    rank[((long long)b * A + a) * 2 + 1] = r_occ;
  }
  __syncthreads();
  const int row_words = RST_STEPS * 8;
  for (int idx = tid; idx < (RST_MAX_OBS + RST_MAX_OCC) * row_words; idx += RST_NT) {
    const int row = idx / row_words, e = idx - row * row_words, t = e >> 3, c = e & 7, src = s_src[row];
    float v = 0.f;
    if (src >= 0) {
      if (c < 5) {
        const float* w = sbox + ((long long)src * RST_STEPS + t) * RST_BOX_WORDS;
        const float val = c == 0 ? w[0] : c == 1 ? w[1] : c == 2 ? w[6] : c == 3 ? w[7] : w[8];
        v = w[10] * val;                                          // valid . [x, y, vx, vy, bbox_yaw] (grid_utils.py:582)
      } else {
        v = stype[src] == c - 4 ? 1.f : 0.f;                      // onehot3(type) tiled over the steps, zero outside {1, 2, 3}
      }
    }
    if (row < RST_MAX_OBS) obs[((long long)b * RST_MAX_OBS + row) * row_words + e] = v;
    else occ[((long long)b * RST_MAX_OCC + (row - RST_MAX_OBS)) * row_words + e] = v;
  }
}

static bool raster_cfg_ok(const char* who, int B, int A, int G, float ppm) {
  if (B < 0 || A < 1 || G < 1 || !(ppm > 0.f)) { stj_set_error("%s: B %d, A %d, grid %d, pixels per metre %g", who, B, A, G, (double)ppm); return false; }
  return true;
}

extern "C" long long stj_raster_workspace_bytes(int B, int A) { return B < 0 || A < 0 ? -1 : rst_ws_offset(B, A, RST_WS_PARTS); }

extern "C" long long stj_raster_workspace_offset(int B, int A, int part) {
  return B < 0 || A < 0 || part < 0 || part >= RST_WS_PARTS ? -1 : rst_ws_offset(B, A, part);
}

extern "C" int stj_raster_boxes(const float* state, const int* type, const int* is_sdc, void* ws, int B, int A, int grid, float ppm,
                                float sdc_x, float sdc_y, hipStream_t stream) {
  if (!raster_cfg_ok("stj_raster_boxes", B, A, grid, ppm)) return STJ_EINVAL;
  if (B == 0) return STJ_OK;
  if (!state || !type || !is_sdc || !ws) { stj_set_error("stj_raster_boxes: state / type / is_sdc / ws is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)state | (uintptr_t)type | (uintptr_t)is_sdc) & 3) || ((uintptr_t)ws & 15)) {
    stj_set_error("stj_raster_boxes: 4-byte aligned state / type / is_sdc, 16-byte aligned ws only");
    return STJ_EUNSUPPORTED;
  }
  const long long blocks = ((long long)A * RST_STEPS + RST_NT - 1) / RST_NT;
  if (B > 65535 || blocks > 0x7fffffffll) { stj_set_error("stj_raster_boxes: B %d, A %d are beyond the launch limit", B, A); return STJ_EUNSUPPORTED; }
  char* w = (char*)ws;
  hipLaunchKernelGGL(raster_boxes_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(RST_NT), 0, stream, state, type, is_sdc,
                     (float*)(w + rst_ws_offset(B, A, RST_WS_BOX)), (int*)(w + rst_ws_offset(B, A, RST_WS_AABB)),
                     (float*)(w + rst_ws_offset(B, A, RST_WS_FRAME)), (int*)(w + rst_ws_offset(B, A, RST_WS_OK)), B, A, grid, ppm, sdc_x, sdc_y);
  return stj_check_launch("stj_raster_boxes");
}

extern "C" int stj_raster_grids(const void* ws, float* ogm, float* flow, int B, int A, int grid, float ppm, float sdc_x, float sdc_y,
                                int points_length, int points_width, hipStream_t stream) {
  if (!raster_cfg_ok("stj_raster_grids", B, A, grid, ppm)) return STJ_EINVAL;
  if (points_length < 2 || points_width < 2 || (long long)points_length * points_width > (1 << 20)) {
    stj_set_error("stj_raster_grids: %d x %d points per box (2 .. per side, 2^20 in all)", points_length, points_width);
    return STJ_EINVAL;
  }
  if (B == 0) return STJ_OK;
  if (!ws || !ogm || !flow) { stj_set_error("stj_raster_grids: ws / ogm / flow is NULL"); return STJ_EINVAL; }
  if (((uintptr_t)ws | (uintptr_t)ogm | (uintptr_t)flow) & 15) { stj_set_error("stj_raster_grids: 16-byte aligned ws / ogm / flow only"); return STJ_EUNSUPPORTED; }
  const int tiles_x = (grid + RST_TILE_W - 1) / RST_TILE_W;
  const long long tiles = (long long)tiles_x * ((grid + RST_TILE_H - 1) / RST_TILE_H);
  if (B > 65535 || tiles > 0x7fffffffll || A > (1 << 20)) { stj_set_error("stj_raster_grids: B %d, A %d, grid %d are beyond the launch limit", B, A, grid); return STJ_EUNSUPPORTED; }
  const char* w = (const char*)ws;
  hipLaunchKernelGGL(raster_grids_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(RST_NT), 0, stream,
                     (const float*)(w + rst_ws_offset(B, A, RST_WS_BOX)), (const int*)(w + rst_ws_offset(B, A, RST_WS_AABB)), ogm, flow, A, grid, ppm,
                     sdc_x, sdc_y, points_length, points_width, tiles_x);
  return stj_check_launch("stj_raster_grids");
}

extern "C" int stj_raster_actors(void* ws, const int* type, float* obs, float* occ, int B, int A, int fov_grid, float ppm, float fov_sdc_x,
                                 float fov_sdc_y, hipStream_t stream) {
  if (!raster_cfg_ok("stj_raster_actors", B, A, fov_grid, ppm)) return STJ_EINVAL;
  if (A > RST_MAX_AGENTS) { stj_set_error("stj_raster_actors: %d agents per scene, at most %d", A, RST_MAX_AGENTS); return STJ_EUNSUPPORTED; }
  if (B == 0) return STJ_OK;
  if (!ws || !type || !obs || !occ) { stj_set_error("stj_raster_actors: ws / type / obs / occ is NULL"); return STJ_EINVAL; }
  if ((((uintptr_t)type | (uintptr_t)obs | (uintptr_t)occ) & 3) || ((uintptr_t)ws & 15)) {
    stj_set_error("stj_raster_actors: 4-byte aligned type / obs / occ, 16-byte aligned ws only");
    return STJ_EUNSUPPORTED;
  }
  char* w = (char*)ws;
  hipLaunchKernelGGL(raster_actors_kernel, dim3((unsigned)B), dim3(RST_NT), 0, stream, (const float*)(w + rst_ws_offset(B, A, RST_WS_BOX)), type,
                     (const int*)(w + rst_ws_offset(B, A, RST_WS_OK)), (int*)(w + rst_ws_offset(B, A, RST_WS_MASK)),
                     (float*)(w + rst_ws_offset(B, A, RST_WS_DIST)), (int*)(w + rst_ws_offset(B, A, RST_WS_RANK)), obs, occ, A, fov_grid, ppm,
                     fov_sdc_x, fov_sdc_y);
  return stj_check_launch("stj_raster_actors");
}
