// One element of the Keras-Nadam update (reference train.py:197,224), shared by nadam_kernel (csrc/rng.hip: the
// coefficients are kernel arguments) and nadam_apply_kernel (csrc/optim.hip: they are read from a device buffer):
//   gg = g * gscale ; m = b1 m + (1-b1) gg ; v = b2 v + (1-b2) gg^2
//   w -= lr * (cg gg + cm m) / (sqrt(v * vhat_scale) + eps)
#pragma once

__device__ __forceinline__ void nadam_update(float& w, float g, float& m, float& v, float lr, float b1, float b2, float eps, float cg,
                                             float cm, float vhat_scale, float gscale) {
  const float gg = g * gscale;
  m = b1 * m + (1.f - b1) * gg;
  v = b2 * v + (1.f - b2) * gg * gg;
  w -= lr * (cg * gg + cm * m) / (sqrtf(v * vhat_scale) + eps);
}
