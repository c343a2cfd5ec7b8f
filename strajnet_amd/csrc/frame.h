// Protobuf framing of a scene's zlib streams (stj_compress_waypoints_framed, csrc/deflate.hip): the rules that do not need the device,
// as plain functions (FRM_FN) a host program compiles as they stand (the same rules in Python: strajnet_amd/submission.py,
// frame_reference).
//
// A scene's block is the wire form of its `repeated Waypoint waypoints`: for k = 0 .. 7
//     tag_wp   varint(Lk)
//     tag_obs  varint(l0) <obs stream>
//     tag_occ  varint(l1) <occ stream>
//     tag_flow varint(l2) <flow stream>                     Lk = sum_i (1 + varint_len(l_i) + l_i)
// The four tag bytes (field number << 3 | 2, field numbers 1 .. 15) come from the caller, packed into one uint32:
// tag_wp | tag_obs << 8 | tag_occ << 16 | tag_flow << 24.  All lengths are below 2^32 (the packed buffer's limit).
//
//   pb_varint_len      bytes of a uint32 as a base-128 varint (1 .. 5)
//   pb_put_varint      writes it, returns the count
//   frm_field_len      a length-delimited field of l payload bytes: tag, varint(l), payload
//   frm_waypoint_body  Lk from a waypoint's three stream lengths
//   frm_tag            tag byte i (0: waypoint, 1 .. 3: obs, occ, flow) of the packed four
//   frm_scene          lays out one scene from its 3 * FRM_WAYPOINTS stream lengths: every stream's start relative to the block, the header
//                      bytes into `out` when it is not null (the streams' own bytes are the caller's), returns the block's length
#pragma once
#include <stdint.h>

#define FRM_WAYPOINTS 8
#define FRM_MAX_HEADER 6                   // tag + the 5 bytes of a 32-bit varint: per stream and per waypoint

#if defined(__HIPCC__) || defined(__HIP__)
#define FRM_FN __host__ __device__ __forceinline__
#else
#define FRM_FN static inline
#endif

FRM_FN uint32_t pb_varint_len(uint32_t v) { return 1u + (v >= 1u << 7) + (v >= 1u << 14) + (v >= 1u << 21) + (v >= 1u << 28); }

FRM_FN uint32_t pb_put_varint(uint8_t* p, uint32_t v) {
  uint32_t n = 0;
  while (v >= 0x80u) { p[n++] = (uint8_t)(v | 0x80u); v >>= 7; }
  p[n++] = (uint8_t)v;
  return n;
}

FRM_FN uint32_t frm_field_len(uint32_t l) { return 1u + pb_varint_len(l) + l; }
FRM_FN uint32_t frm_waypoint_body(uint32_t l0, uint32_t l1, uint32_t l2) { return frm_field_len(l0) + frm_field_len(l1) + frm_field_len(l2); }
FRM_FN uint8_t frm_tag(uint32_t tags, int i) { return (uint8_t)(tags >> (8 * i)); }

FRM_FN uint32_t frm_scene(const uint32_t* lens, uint32_t tags, uint8_t* out, uint32_t* starts) {
  uint32_t at = 0;
  for (int k = 0; k < FRM_WAYPOINTS; ++k) {
    const uint32_t* l = lens + 3 * k;
    const uint32_t body = frm_waypoint_body(l[0], l[1], l[2]);
    if (out) { out[at] = frm_tag(tags, 0); pb_put_varint(out + at + 1, body); }
    at += 1u + pb_varint_len(body);
    for (int i = 0; i < 3; ++i) {
      if (out) { out[at] = frm_tag(tags, 1 + i); pb_put_varint(out + at + 1, l[i]); }
      at += 1u + pb_varint_len(l[i]);
      starts[3 * k + i] = at;
      at += l[i];
    }
  }
  return at;
}
