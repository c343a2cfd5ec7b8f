// Rasterising agent tracks (stj_raster_boxes / stj_raster_grids / stj_raster_actors, csrc/raster.hip): the rules that do not need the
// device, as plain functions (RST_FN) a host program compiles as they stand (the semantics in NumPy: strajnet_amd/raster.py,
// raster_reference).
//
//   rst_frame        the scene's frame from the SDC's current x, y, yaw: angle = pi/2 - yaw and its cosine / sine (grid_utils.py:63-77,
//                    541-558).  Positions have the SDC's subtracted and are rotated by angle (rst_to_frame), velocities are rotated only
//                    (rst_rotate), the box yaw used for sampling is bbox_yaw + angle.
//   rst_box          one (agent, step) box record from its frame-relative state: centre, the two half-axis vectors
//                    hx = L/2 (cos, sin), hy = W/2 (-sin, cos), the rotated velocity and the UNROTATED yaw (grid_utils.py:580).
//   rst_point        point (i, j) of a box, i < nl, j < nw:  centre + R(yaw) (u_i L, v_j W),  u_i = i/(nl-1) - 0.5,  v_j = j/(nw-1) - 0.5
//                    = centre + 2 u_i hx + 2 v_j hy.  This is the published Waymo renderer's _sample_points_from_agent_boxes WRITTEN FROM
//                    MEMORY (the library is not part of the reference's tree): this statement, not the library, is the contract.
//   rst_pixel        px = rint(x ppm) + sdc_x, py = rint(-y ppm) + sdc_y (grid_utils.py:40-42); rint is round-half-even like tf.round.
//   rst_in_grid      0 <= px, py < grid + margin and >= -margin (grid_utils.py:45-58: margin 0, or 64 for the occluded-actor mask).
//   rst_corner       the four _rotate_box corners (grid_utils.py:587-607) of a record: centre +- hx +- hy.
//   rst_aabb         a conservative pixel bounding box of a record's points (one pixel of slack: it only culls).
//   rst_plane_at     the plane table of stj_raster_grids: output plane p of the occupancy tensor is set by boxes of class rst_plane_at(p).cls
//                    at step rst_plane_at(p).step.  Adding planes (future steps: the ground-truth grids) is adding rows.
//   rst_plane_mask   the planes one (step, class) sets, as bits.
//   rst_ws_*         the workspace's parts and their byte offsets for (B, A).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RST_FN __host__ __device__ __forceinline__
#else
#define RST_FN static inline
#endif

#define RST_STEPS 11                        // 10 past + 1 current (data_preprocessing.py:68)
#define RST_CUR 10                          // the current step
#define RST_BOX_WORDS 12                    // cx cy hxx hxy hyx hyy vx vy yaw cls valid pad
#define RST_MAX_AGENTS 1024                 // stj_raster_actors ranks a scene in one workgroup's LDS
#define RST_MAX_OBS 48
#define RST_MAX_OCC 16
#define RST_OCC_MARGIN 64                   // grid_utils.py:53-58 (larger_box)
#define RST_TILE_W 64                       // stj_raster_grids: pixels of a tile row (one contiguous run of 64 x 22 floats)
#define RST_TILE_H 16
#define RST_NPLANES 22
#define RST_MASK_INBOX 1
#define RST_MASK_OCCU 2
#define RST_MASK_VALID 4                    // at least one valid step
#define RST_MASK_AWAY 8                     // the first valid position is farther from the SDC than the last (data_preprocessing.py:193)

typedef struct { int step, cls; } rst_plane;
// ogm[y, x, t, c]: plane 2 t + c.  class 0 = type 1 (vehicles), class 1 = types 2 and 3 (pedestrians + cyclists, data_preprocessing.py:262-273)
RST_FN rst_plane rst_plane_at(int p) {
  constexpr rst_plane RST_PLANES[RST_NPLANES] = {
    {0, 0}, {0, 1}, {1, 0}, {1, 1}, {2, 0}, {2, 1}, {3, 0}, {3, 1}, {4, 0}, {4, 1}, {5, 0}, {5, 1},
    {6, 0}, {6, 1}, {7, 0}, {7, 1}, {8, 0}, {8, 1}, {9, 0}, {9, 1}, {10, 0}, {10, 1}};
  return RST_PLANES[p];
}

RST_FN uint32_t rst_plane_mask(int step, int cls) {
  uint32_t m = 0;
  for (int p = 0; p < RST_NPLANES; ++p) {
    const rst_plane r = rst_plane_at(p);
    if (r.step == step && r.cls == cls) m |= 1u << p;
  }
  return m;
}

RST_FN int rst_class(int type) { return type == 1 ? 0 : (type == 2 || type == 3) ? 1 : -1; }

typedef struct { float x, y, yaw, angle, c, s; } rst_frame_t;

RST_FN rst_frame_t rst_frame(float sdc_x, float sdc_y, float sdc_yaw) {
  rst_frame_t f;
  f.x = sdc_x; f.y = sdc_y; f.yaw = sdc_yaw;
  f.angle = 1.57079632679489661923f - sdc_yaw;
  f.c = cosf(f.angle); f.s = sinf(f.angle);
  return f;
}

RST_FN void rst_rotate(const rst_frame_t& f, float x, float y, float* ox, float* oy) {
  *ox = f.c * x - f.s * y;
  *oy = f.s * x + f.c * y;
}

RST_FN void rst_to_frame(const rst_frame_t& f, float x, float y, float* ox, float* oy) { rst_rotate(f, x - f.x, y - f.y, ox, oy); }

typedef struct { float cx, cy, hxx, hxy, hyx, hyy, vx, vy, yaw; int cls, valid; } rst_box_t;

RST_FN rst_box_t rst_box(const rst_frame_t& f, float x, float y, float yaw, float length, float width, float vx, float vy, int type, float valid) {
  rst_box_t b;
  rst_to_frame(f, x, y, &b.cx, &b.cy);
  const float a = yaw + f.angle, c = cosf(a), s = sinf(a);
  b.hxx = 0.5f * length * c; b.hxy = 0.5f * length * s;
  b.hyx = -0.5f * width * s; b.hyy = 0.5f * width * c;
  rst_rotate(f, vx, vy, &b.vx, &b.vy);
  b.yaw = yaw;
  b.cls = rst_class(type);
  b.valid = valid > 0.f ? 1 : 0;
  return b;
}

RST_FN void rst_box_store(const rst_box_t& b, float* w) {
  w[0] = b.cx; w[1] = b.cy; w[2] = b.hxx; w[3] = b.hxy; w[4] = b.hyx; w[5] = b.hyy; w[6] = b.vx; w[7] = b.vy; w[8] = b.yaw;
  w[9] = (float)b.cls; w[10] = (float)b.valid; w[11] = 0.f;
}

RST_FN rst_box_t rst_box_load(const float* w) {
  rst_box_t b;
  b.cx = w[0]; b.cy = w[1]; b.hxx = w[2]; b.hxy = w[3]; b.hyx = w[4]; b.hyy = w[5]; b.vx = w[6]; b.vy = w[7]; b.yaw = w[8];
  b.cls = (int)w[9]; b.valid = (int)w[10];
  return b;
}

RST_FN void rst_point(const rst_box_t& b, int i, int j, int nl, int nw, float* x, float* y) {
  const float u2 = 2.f * ((float)i / (float)(nl - 1) - 0.5f), v2 = 2.f * ((float)j / (float)(nw - 1) - 0.5f);
  *x = b.cx + u2 * b.hxx + v2 * b.hyx;
  *y = b.cy + u2 * b.hxy + v2 * b.hyy;
}

RST_FN void rst_pixel(float x, float y, float ppm, float sdc_x, float sdc_y, float* px, float* py) {
  *px = rintf(x * ppm) + sdc_x;
  *py = rintf(-y * ppm) + sdc_y;
}

RST_FN bool rst_in_grid(float px, float py, int grid, int margin) {
  return px >= (float)-margin && py >= (float)-margin && px < (float)(grid + margin) && py < (float)(grid + margin);
}

// corner k: 0 upper-left (+hx -hy), 1 upper-right (+hx +hy), 2 lower-left (-hx -hy), 3 lower-right (-hx +hy)
RST_FN void rst_corner(const rst_box_t& b, int k, float* x, float* y) {
  const float sl = k < 2 ? 1.f : -1.f, sw = (k & 1) ? 1.f : -1.f;
  *x = b.cx + sl * b.hxx + sw * b.hyx;
  *y = b.cy + sl * b.hxy + sw * b.hyy;
}

RST_FN int rst_clamp_lo(float v, int lo, int hi) { return !(v > (float)lo) ? lo : v > (float)hi ? hi : (int)v; }      // NaN -> lo
RST_FN int rst_clamp_hi(float v, int lo, int hi) { return !(v < (float)hi) ? hi : v < (float)lo ? lo : (int)v; }      // NaN -> hi: never culled wrongly

// pixel box [x0, x1] x [y0, y1] that holds every rendered point of the record, clamped to the grid; x1 < x0 when nothing can render
RST_FN void rst_aabb(const rst_box_t& b, float ppm, float sdc_x, float sdc_y, int grid, int* q) {
  const float ex = fabsf(b.hxx) + fabsf(b.hyx), ey = fabsf(b.hxy) + fabsf(b.hyy);
  float xa, ya, xb, yb;
  rst_pixel(b.cx - ex, b.cy + ey, ppm, sdc_x, sdc_y, &xa, &ya);
  rst_pixel(b.cx + ex, b.cy - ey, ppm, sdc_x, sdc_y, &xb, &yb);
  q[0] = rst_clamp_lo(xa - 1.f, 0, grid); q[1] = rst_clamp_lo(ya - 1.f, 0, grid);
  q[2] = rst_clamp_hi(xb + 1.f, -1, grid - 1); q[3] = rst_clamp_hi(yb + 1.f, -1, grid - 1);
  if (!(b.valid && b.cls >= 0) || q[3] < q[1]) { q[0] = 0; q[2] = -1; }
}

// ---- workspace: [box records | aabb | frame | ok | mask | dist | rank], every part 256-byte aligned
enum { RST_WS_BOX = 0, RST_WS_AABB = 1, RST_WS_FRAME = 2, RST_WS_OK = 3, RST_WS_MASK = 4, RST_WS_DIST = 5, RST_WS_RANK = 6, RST_WS_PARTS = 7 };

RST_FN long long rst_ws_part_bytes(long long B, long long A, int part) {
  switch (part) {
    case RST_WS_BOX: return B * A * RST_STEPS * RST_BOX_WORDS * 4;      // float [B, A, 11, 12]
    case RST_WS_AABB: return B * A * RST_STEPS * 16;                    // int   [B, A, 11, 4]
    case RST_WS_FRAME: return B * 32;                                   // float [B, 8]: sdc x, y, yaw, angle, cos, sin, sdc index, ok
    case RST_WS_OK: return B * 4;                                       // int   [B]
    case RST_WS_MASK: return B * A * 4;                                 // int   [B, A]: RST_MASK_* bits
    case RST_WS_DIST: return B * A * 8;                                 // float [B, A, 2]: |position| at the last / first valid step
    case RST_WS_RANK: return B * A * 8;                                 // int   [B, A, 2]: row in obs / occ, -1 for none
    default: return 0;
  }
}

RST_FN long long rst_ws_offset(long long B, long long A, int part) {      // part == RST_WS_PARTS: the whole size
  long long at = 0;
  for (int p = 0; p < part && p < RST_WS_PARTS; ++p) at += (rst_ws_part_bytes(B, A, p) + 255) / 256 * 256;
  return at;
}
