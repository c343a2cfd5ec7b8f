// Per-scene scoring of the validation pass (stj_eval_scenes_fwd, csrc/eval.hip): the rules that do not need the device, as plain
// functions (EVS_FN) a host program compiles as they stand (the semantics in NumPy: strajnet_amd/evaluate.py, SceneScores.reference).
//
//   evs_grid     workgroups per scene, a function of (H, W) ALONE: a scene's partial sums are the same ones, added in the same order,
//                whatever the batch around it holds.
//   evs_finite   a float32 is neither NaN nor an infinity (by its bits: immune to fast-math folding of x == x).
//   evs_commit   one live scene's row float32[12] -> running state double[2][13], score table float32[capacity][12], cursor.
//                state[0][c] += row[c] (x loss_scale in the five loss columns), state[1][c] += 1 for every FINITE column c; a
//                non-finite column is added to neither (one scene without vehicles would turn the epoch's mean into NaN: this is where
//                the state departs from Keras Mean).  state[0][12] += 1 per scene, state[1][12] += 1 per scene with a non-finite column.
//                The row is stored at table[*cursor] only when 0 <= *cursor < capacity; *cursor advances all the same.
#pragma once
#include <stdint.h>
#include <string.h>

#define EVS_COLS 12                         // observed_xe, occluded_xe, flow, flow_warp_xe, their sum, the seven metrics
#define EVS_LOSS_COLS 5
#define EVS_STATE_COLS 13                   // the row's columns, then [0][12] scenes scored / [1][12] scenes with a non-finite column
#define EVS_THREADS 512                     // = EVAL_THREADS: work items of one workgroup per stride
#define EVS_MAXB 65534                      // blockIdx.y is the scene, and one more row of the AUC grid takes the pooled histograms
#ifndef EVS_MAXG
#define EVS_MAXG 64                         // workgroups per scene at most; measured against 16 and 32
#endif

#if defined(__HIPCC__) || defined(__HIP__)
#define EVS_FN __host__ __device__ __forceinline__
#else
#define EVS_FN static inline
#endif

EVS_FN int evs_grid(int H, int W) {
  const long long items = (long long)H * W * 8;
  if (H <= 0 || W <= 0) return 0;
  const long long g = (items + EVS_THREADS - 1) / EVS_THREADS;
  return (int)(g < EVS_MAXG ? g : EVS_MAXG);
}

EVS_FN bool evs_finite(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return (u & 0x7f800000u) != 0x7f800000u;
}

EVS_FN void evs_commit(const float* row, double* state, float* table, long long* cursor, long long capacity, float loss_scale) {
  if (state) {
    bool bad = false;
    for (int c = 0; c < EVS_COLS; ++c) {
      const float v = row[c];
      if (evs_finite(v)) {
        state[c] += c < EVS_LOSS_COLS ? (double)v * (double)loss_scale : (double)v;
        state[EVS_STATE_COLS + c] += 1.0;
      } else {
        bad = true;
      }
    }
    state[EVS_COLS] += 1.0;
    if (bad) state[EVS_STATE_COLS + EVS_COLS] += 1.0;
  }
  if (cursor) {
    const long long at = *cursor;
    if (table && at >= 0 && at < capacity)
      for (int c = 0; c < EVS_COLS; ++c) table[at * EVS_COLS + c] = row[c];
    *cursor = at + 1;
  }
}
