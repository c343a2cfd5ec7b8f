// Challenge-format quantisation of the model output (reference inference.py:160-182, _add_waypoints_to_scenario_prediction):
//   observed / occluded occupancy : uint8 np.round(sigmoid(logit) * 255)
//   flow                          : int8  np.clip(np.round(flow), -128, 127)
// np.round is round-half-to-even = rintf in the default rounding mode.  The sigmoid is the accurate one (expf + IEEE division), not
// loss.hip's sigmoidf (__expf + __frcp_rn): a byte flips where 255 * sigmoid sits on a rounding tie, and this is a pure stream
// (128 B read + 32 B written per cell), so the accurate form costs nothing.  NaN (occupancy logit or flow) -> 0.
//
// Q, per scene one block of 4 Tn H W bytes: [ obs u8 [Tn,H,W] | occ u8 [Tn,H,W] | flow i8 [Tn,H,W,2] ] -- the slice of (scene, waypoint,
// field) is byte for byte what the reference's .tobytes() yields for a batch of one.
#include "common.h"
#include "quantize.h"

// A workgroup takes a run of QZ_RUN = 256 consecutive cells of one scene (32 KB of logits): the 8 lanes (g, t = 0..7) of a lane group
// read the 128-byte line of cell 8 g + i in pass i, so a thread ends up with the four values of waypoint t at 8 CONSECUTIVE cells =
// 8 + 8 + 16 contiguous bytes of the three planes.  Those go through LDS (plane rows padded by 16 B: the 8 waypoints of a lane group land
// on 8 different bank quads) and leave as 16-byte vectors: 256 contiguous bytes per occupancy plane, 512 per flow plane.
// Short-lived workgroups, no persistent loop (5.8-6.0 TB/s against 4.0-4.5 for a read-modify-write stream).
__global__ __launch_bounds__(256) void quantize_waypoints_kernel(const float* __restrict__ Y, uint8_t* __restrict__ Q, long long HW) {
  constexpr int SO = QZ_RUN + 16, SF = 2 * QZ_RUN + 16;            // padded plane rows
  __shared__ __attribute__((aligned(16))) uint8_t st[2 * 8 * SO + 8 * SF];
  const int tid = threadIdx.x, g = tid >> 3, t = tid & 7;
  const long long runs = HW / QZ_RUN;
  const long long b = blockIdx.x / runs, c0 = (blockIdx.x % runs) * QZ_RUN;
  const float4* src = reinterpret_cast<const float4*>(Y + (b * HW + c0 + 8 * g) * 32) + t;
  float4 v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = src[8 * i];
  uint32_t o[2] = {0, 0}, c[2] = {0, 0}, f[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i >> 2] |= quant_prob(v[i].x) << (8 * (i & 3));
    c[i >> 2] |= quant_prob(v[i].y) << (8 * (i & 3));
    f[i >> 1] |= (quant_flow(v[i].z) | (quant_flow(v[i].w) << 8)) << (16 * (i & 1));
  }
  *reinterpret_cast<uint2*>(st + t * SO + 8 * g) = make_uint2(o[0], o[1]);
  *reinterpret_cast<uint2*>(st + (8 + t) * SO + 8 * g) = make_uint2(c[0], c[1]);
  *reinterpret_cast<uint4*>(st + 16 * SO + t * SF + 16 * g) = make_uint4(f[0], f[1], f[2], f[3]);
  __syncthreads();
  uint8_t* q = Q + b * 32 * HW;
  {       // threads 0..127: the 8 observed planes, 128..255: the 8 occluded ones; 16 vectors of 16 B per plane
    const int p = tid >> 4, j = tid & 15;
    *reinterpret_cast<uint4*>(q + p * HW + c0 + 16 * j) = *reinterpret_cast<const uint4*>(st + p * SO + 16 * j);
  }
  {       // flow: 8 planes x 32 vectors
    const int p = tid >> 5, j = tid & 31;
    *reinterpret_cast<uint4*>(q + 16 * HW + p * 2 * HW + 2 * c0 + 16 * j) = *reinterpret_cast<const uint4*>(st + 16 * SO + p * SF + 16 * j);
  }
}

extern "C" int stj_quantize_waypoints(const float* Y, uint8_t* Q, int B, int Tn, int Hh, int Ww, hipStream_t stream) {
  if (B <= 0 || Hh <= 0 || Ww <= 0) { stj_set_error("quantize_waypoints: empty problem"); return STJ_EINVAL; }
  const long long HW = (long long)Hh * Ww;
  if (Tn != 8 || HW % QZ_RUN || ((uintptr_t)Y | (uintptr_t)Q) & 15 || B * (HW / QZ_RUN) > 0x7fffffffLL) {
    stj_set_error("quantize_waypoints: Tn = 8, H * W a multiple of %d, 16-byte aligned buffers only (Tn %d, H %d, W %d)", QZ_RUN, Tn, Hh, Ww);
    return STJ_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(quantize_waypoints_kernel, dim3((unsigned)(B * (HW / QZ_RUN))), dim3(256), 0, stream, Y, Q, HW);
  return stj_check_launch("stj_quantize_waypoints");
}
