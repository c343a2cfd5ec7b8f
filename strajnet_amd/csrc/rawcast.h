// The conversion of one record element to float32 (reference train.py:87-103 / inference.py:84-96: tf.io.decode_raw + cast), shared by
// stj_decode_raw (util.hip) and stj_gather_raw (pool.h) so that both give the same bits.  kind 0: bool / uint8 -> (v != 0), 1: int8,
// 2: float32, 3: float64.  Plain C++ beyond __device__ / __forceinline__: a host program can compile it.
#pragma once

template <int KIND> __device__ __forceinline__ float raw_to_f32(const void* src, long long s) {
  if constexpr (KIND == 0) return reinterpret_cast<const unsigned char*>(src)[s] != 0 ? 1.f : 0.f;
  else if constexpr (KIND == 1) return (float)reinterpret_cast<const signed char*>(src)[s];
  else if constexpr (KIND == 2) return reinterpret_cast<const float*>(src)[s];
  else return (float)reinterpret_cast<const double*>(src)[s];
}
