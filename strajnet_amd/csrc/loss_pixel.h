// Per-pixel device functions of the OGMFlow loss and the occupancy / flow metrics, shared by csrc/loss.hip (the training loss, the
// AUC gate, the metrics) and csrc/eval.hip (the validation step's one pass): the cross-entropy / focal terms, the warp-consistency
// term, the bilinear warp sample, the Keras AUC bucket and the Keras PR-AUC interpolation.  One definition each: the entry points of
// the two files agree bit for bit wherever they compute the same quantity.
#pragma once
#include "common.h"

#define NWP 8

__device__ __forceinline__ float xe_logits(float z, float x) {   // tf.nn.sigmoid_cross_entropy_with_logits
  return fmaxf(x, 0.f) - x * z + log1pf(__expf(-fabsf(x)));      // v_exp_f32 (1 ulp on a value in (0, 1]); log1p stays exact for small arguments
}
__device__ __forceinline__ float sigmoidf(float x) { return __frcp_rn(1.f + __expf(-x)); }
// XE + tfa focal term on a logit x with label y; *d = derivative w.r.t. x when d != NULL
__device__ __forceinline__ float xe_focal_logits(float y, float x, float* d) {
  const float ce = xe_logits(y, x), p = sigmoidf(x);
  const float pt = y * p + (1.f - y) * (1.f - p), at = y * 0.25f + (1.f - y) * 0.75f, om = 1.f - pt;
  if (d) {
    const float dce = p - y, dpt = (2.f * y - 1.f) * p * (1.f - p);
    *d = dce + at * (om * om * dce - 2.f * om * dpt * ce);
  }
  return ce + at * om * om * ce;
}
// Keras backend binary_crossentropy(from_logits=False): clip to [eps, 1-eps], -(y log(q+eps) + (1-y) log(1-q+eps));
// tf.clip_by_value passes the gradient for eps <= q <= 1-eps (bounds included)
__device__ __forceinline__ float bce_prob(float y, float q, float* d) {
  const float eps = 1e-7f, hi = 1.f - 1e-7f;
  const float qc = fminf(fmaxf(q, eps), hi);
  if (d) *d = (q >= eps && q <= hi) ? (1.f - y) / (1.f - qc + eps) - y / (qc + eps) : 0.f;
  return -(y * logf(qc + eps) + (1.f - y) * logf(1.f - qc + eps));
}
// tfa focal term on a probability q (pred_prob = q unclipped, ce = bce_prob)
__device__ __forceinline__ float focal_prob(float y, float q, float* d) {
  float dce;
  const float ce = bce_prob(y, q, &dce);
  const float pt = y * q + (1.f - y) * (1.f - q), at = y * 0.25f + (1.f - y) * 0.75f, om = 1.f - pt;
  if (d) *d = at * (om * om * dce - 2.f * om * (2.f * y - 1.f) * ce);
  return at * om * om * ce;
}
// the warp-consistency pixel term on the joint probability q with label ta; inv_hw = 1 / (H*W)
template <bool FOCAL, bool PRED>
__device__ __forceinline__ float warp_term(float ta, float q, float inv_hw, float* d) {
  if (PRED) {
    const float v = bce_prob(ta, q, d);
    if (d) *d *= inv_hw;
    return v * inv_hw;
  }
  if (FOCAL) {
    float d0, d1;
    const float v = focal_prob(ta, q, &d0) + bce_prob(ta, q, &d1) * inv_hw;
    if (d) *d = d0 + d1 * inv_hw;
    return v;
  }
  if (d) *d = sigmoidf(q) - ta;
  return xe_logits(ta, q);
}

// bilinear sample of a single-channel [H][W] image at (x,y) (sample(): pad 1, warp+1); optionally d/dx, d/dy
__device__ __forceinline__ float warp_sample(const float* img, int H, int W, float x, float y, float* ddx, float* ddy) {
  Bil c = bil_setup(x + 1.f, y + 1.f, H + 2, W + 2);
  const float tl = pad_at(img, H, W, 1, c.y0, c.x0), tr = pad_at(img, H, W, 1, c.y0, c.x0 + 1);
  const float bl = pad_at(img, H, W, 1, c.y0 + 1, c.x0), br = pad_at(img, H, W, 1, c.y0 + 1, c.x0 + 1);
  const float top = c.ax * (tr - tl) + tl, bot = c.ax * (br - bl) + bl;
  if (ddx) *ddx = c.gx ? (c.ay * (br - bl) + (1.f - c.ay) * (tr - tl)) : 0.f;
  if (ddy) *ddy = c.gy ? (bot - top) : 0.f;
  return c.ay * (bot - top) + top;
}

// Keras AUC bucket of a prediction: the number of thresholds strictly below it, thresholds t0 = -1e-7, t_i = i/99 (i = 1..98),
// t_99 = 1 + 1e-7 as float32 (tf.keras.metrics.AUC(num_thresholds=100))
__device__ __forceinline__ int auc_bucket(float pred) {
  int bk = 0;
  if (pred > -1e-7f) {
    bk = 1;
    int j = (int)(pred * 99.f);
    j = j < 0 ? 0 : (j > 98 ? 98 : j);
    // count i in 1..98 with t_i < pred, robust to rounding of pred*99
    int cnt = j;
    if (cnt >= 1 && !((float)((double)cnt / 99.0) < pred)) cnt -= 1;
    else if (cnt < 98 && ((float)((double)(cnt + 1) / 99.0) < pred)) cnt += 1;
    bk += cnt;
    if (pred > (float)(1.0 + 1e-7)) bk += 1;
  }
  return bk;
}

// Keras interpolate_pr_auc from one histogram h [2][101] (int): bucket = #thresholds strictly below pred; class 1 = label true.
// Called by ALL 128 threads of a block, thread i = threshold i; s = the block's LDS scratch.  The AUC comes back in thread 0.
// (v0 ran the whole recurrence in ONE thread per histogram with 1.6 KB of f64 scratch arrays: 82 us.)
struct AucScratch { int hn[101], hp[101]; double tp[100], pp[100], part[128]; };
__device__ __forceinline__ double auc_pr_block(const int* h, AucScratch& s) {
  const int i = threadIdx.x;
  if (i <= 100) { s.hn[i] = h[i]; s.hp[i] = h[101 + i]; }
  __syncthreads();
  double totp = 0, totn = 0;
  for (int j = 0; j <= 100; ++j) { totp += s.hp[j]; totn += s.hn[j]; }
  if (i < 100) {                       // positive at threshold i <=> bucket > i
    double cp = 0, cn = 0;
    for (int j = 0; j <= i; ++j) { cp += s.hp[j]; cn += s.hn[j]; }
    s.tp[i] = totp - cp;
    s.pp[i] = s.tp[i] + (totn - cn);
  }
  __syncthreads();
  double term = 0;
  if (i < 99) {
    const double dtp = s.tp[i] - s.tp[i + 1], dp = s.pp[i] - s.pp[i + 1];
    const double den = dp > 0 ? dp : 0;
    const double slope = den != 0 ? dtp / den : 0;
    const double icpt = s.tp[i + 1] - slope * s.pp[i + 1];
    double ratio = 1.0;
    if (s.pp[i] > 0 && s.pp[i + 1] > 0) ratio = s.pp[i] / s.pp[i + 1];
    const double d2 = totp > 0 ? totp : 0;    // tp + fn = all positives
    term = d2 != 0 ? slope * (dtp + icpt * log(ratio)) / d2 : 0;
  }
  s.part[i] = term;
  __syncthreads();
  double auc = 0;
  if (i == 0)
    for (int j = 0; j < 99; ++j) auc += s.part[j];          // same summation order as the serial recurrence
  return auc;
}
