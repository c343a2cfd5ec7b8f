// The validation step's loss AND metrics from ONE streaming pass over the [B,H,W,32] logits and the packed ground truth
// (reference train.py:252-282: OGMFlow_loss, then compute_occupancy_flow_metrics, every batch of the validation set).
// Assembled from the existing entry points the same numbers take three passes: stj_loss_auc_gate reads the ground truth, stj_loss_fwd
// the logits and the ground truth, stj_metrics both again (67 MB + 84 MB per pass at B = 8, 256 x 256), and the loss's warp term and
// the metric's flow-warped occupancy gather the same sample(origin, identity + pred_flow) twice.  Here:
//   eval_clear_kernel     zeroes the four-per-waypoint integer histograms in the workspace (the entry needs no zeroed memory);
//   eval_pass_kernel      thread = pixel * 8 + waypoint (loss_fwd_kernel's layout: a lane loads ITS float4 of the 128-byte logit line):
//                         15 float accumulators per thread (5 of the loss, 11 of the metrics, the flow count shared), the predicted-flow
//                         warp sample taken once for both, and 8 x 4 histograms (gate, observed, occluded, flow-warped) in LDS;
//   eval_auc_kernel       Keras PR-AUC of the 32 histograms (auc_pr_block, as auc_gate_kernel) and the use_gt gate;
//   eval_finalize_kernel  folds the workgroups' partial sums and writes loss[5], metrics[7] and the optional running state.
// No floating-point atomics anywhere: every workgroup STORES its 120 partial sums, the finalize kernel adds them in a fixed order in
// double, and the grid depends on the shape alone -- two calls on the same inputs give the same bits.  The histograms are integer
// (order-independent) atomics.  The per-pixel arithmetic is csrc/loss_pixel.h, shared with csrc/loss.hip: the histograms, and with
// them gate and AUCs, equal those of stj_loss_auc_gate / stj_metrics exactly.
// The second half of the file scores every scene of the batch on its own (stj_eval_scenes_fwd) with the same per-item body (eval_item),
// the same fold (eval_fold) and the same formulas (eval_scores): one definition each for both entries.
#include "loss_pixel.h"
#include "eval_scene.h"

#ifndef EVAL_THREADS
#define EVAL_THREADS 512        // 8 waves share one set of histograms (26 KB of LDS)
#endif
#ifndef EVAL_WAVES
#define EVAL_WAVES 6            // waves per SIMD the register allocator is held to: 80 VGPRs, no scratch (at 8: 64 VGPRs and 40 bytes of scratch per lane)
#endif
#ifndef EVAL_MAXG
#define EVAL_MAXG 512           // grid-stride beyond it: every workgroup ends with up to 6464 integer atomics and 120 stores.  Measured at
                                // B = 8 / B = 32, 256 x 256: 1536 workgroups 163 / 466 us, 768: 139 / 462 us, 512: 137 / 441 us
#endif
#define EVAL_NH 4               // histograms per waypoint
#define EVAL_HIST (NWP * EVAL_NH * 202)
#define EVAL_PSTRIDE 128        // floats between two workgroups' partial sums (120 used)
// accumulator slots per waypoint: the loss's five (loss.hip S_*), then the metrics' (loss.hip M_*; the flow count is E_EX for both)
enum { E_OBS = 0, E_OCC, E_L1, E_EX, E_WARP, E_IO, E_TO, E_PO, E_IC, E_TC, E_PC, E_EPE, E_IW, E_TW, E_PW, E_N };
enum { H_GATE = 0, H_OBS, H_OCC, H_WARP };
static_assert(EVS_THREADS == EVAL_THREADS, "eval: eval_scene.h sizes the per-scene grid for EVAL_THREADS");
static_assert(EVAL_THREADS % 64 == 0 && EVAL_THREADS >= NWP * E_N && NWP * E_N <= EVAL_PSTRIDE, "eval: block shape");

// workspace: int hist[EVAL_HIST] | float auc[32], gate[8] (256 bytes) | float partial[G][EVAL_PSTRIDE]
#define EVAL_WS_AUC (EVAL_HIST * 4)
#define EVAL_WS_PART (EVAL_WS_AUC + 256)
static inline int eval_grid(long long npix) {
  return npix <= 0 ? 0 : (int)min((long long)EVAL_MAXG, (npix * NWP + EVAL_THREADS - 1) / EVAL_THREADS);
}

__global__ __launch_bounds__(256) void eval_clear_kernel(int* hist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < EVAL_HIST) hist[i] = 0;
}

struct EvalArgs { const float *logits, *gt_obs, *gt_occ, *gt_flow, *origin; int H, W, loss_warp, met_warp, use_gt; };

// One work item `it` = (pixel of the batch) * 8 + waypoint k: two histogram bumps, the 15 accumulators, one warp gather for both
// consumers and the gate's gather.  The ONE per-item body of eval_pass_kernel and eval_scenes_pass_kernel; hk = waypoint k's four
// histograms in LDS.
template <bool FOCAL, bool PRED>
__device__ __forceinline__ void eval_item(const EvalArgs& a, long long it, int k, float inv_hw, int* hk, float (&acc)[E_N]) {
  const float *logits = a.logits, *gt_obs = a.gt_obs, *gt_occ = a.gt_occ, *gt_flow = a.gt_flow, *origin = a.origin;
  const int H = a.H, W = a.W, loss_warp = a.loss_warp, met_warp = a.met_warp, use_gt = a.use_gt;
  {
    const long long i = it >> 3;
    const int x = (int)(i % W); long long t = i / W;
    const int y = (int)(t % H); const long long b = t / H;
    const float4 lg = reinterpret_cast<const float4*>(logits)[it];
    const long long g = ((b * NWP + k) * H + y) * W + x;
    const float to = gt_obs[g], tc = gt_occ[g];
    const float2 fl = reinterpret_cast<const float2*>(gt_flow)[g];
    const float fx = fl.x, fy = fl.y;
    const float po = sigmoidf(lg.x), pc = sigmoidf(lg.y);
    // the loss's occupancy and flow terms (loss_fwd_kernel)
    acc[E_OBS] += FOCAL ? xe_focal_logits(to, lg.x, nullptr) : xe_logits(to, lg.x);
    acc[E_OCC] += FOCAL ? xe_focal_logits(tc, lg.y, nullptr) : xe_logits(tc, lg.y);
    const float ex = (fx != 0.f || fy != 0.f) ? 1.f : 0.f;
    acc[E_L1] += (fabsf(fx - lg.z) + fabsf(fy - lg.w)) * ex;
    acc[E_EX] += ex;
    // the metrics' occupancy and flow terms (metrics_kernel, pred_is_logits)
    atomicAdd(&hk[H_OBS * 202 + (to != 0.f ? 101 : 0) + auc_bucket(po)], 1);
    atomicAdd(&hk[H_OCC * 202 + (tc != 0.f ? 101 : 0) + auc_bucket(pc)], 1);
    acc[E_IO] += po * to; acc[E_TO] += to; acc[E_PO] += po;
    acc[E_IC] += pc * tc; acc[E_TC] += tc; acc[E_PC] += pc;
    const float dx = (fx - lg.z) * ex, dy = (fy - lg.w) * ex;
    acc[E_EPE] += sqrtf(dx * dx + dy * dy);
    const float ta = fminf(fmaxf(to + tc, 0.f), 1.f);
    const float* img = origin + (b * NWP + k) * (long long)H * W;
    if (loss_warp | met_warp) {
      // ONE gather of sample(origin, identity + pred_flow) for the loss's warp term and the metric's flow-warped occupancy
      const float wp = warp_sample(img, H, W, (float)x + lg.z, (float)y + lg.w, nullptr, nullptr);
      const float pj = fminf(fmaxf(po + pc, 0.f), 1.f);
      if (loss_warp) {
        const float sg = PRED ? pj : fminf(fmaxf(sigmoidf(to) + sigmoidf(tc), 0.f), 1.f);
        acc[E_WARP] += warp_term<FOCAL, PRED>(ta, sg * wp, inv_hw, nullptr);
      }
      if (met_warp) {
        const float fg = pj * wp;
        atomicAdd(&hk[H_WARP * 202 + (fg != 0.f ? 101 : 0) + auc_bucket(ta)], 1);     // y_true = grounded prediction, y_pred = true_all
        acc[E_IW] += ta * fg; acc[E_TW] += fg; acc[E_PW] += ta;
      }
    }
    if (use_gt) {       // the gate's histogram (auc_hist_kernel): it depends on the ground truth alone and multiplies per-waypoint sums at the end
      const float wg = warp_sample(img, H, W, (float)x + fx, (float)y + fy, nullptr, nullptr);
      const float pred = wg * ta;
      atomicAdd(&hk[H_GATE * 202 + (ta != 0.f ? 101 : 0) + auc_bucket(pred)], 1);
    }
  }
}

// The end of a pass workgroup: its 120 partial sums STORED to partial[0..120), its LDS histograms flushed into hist with integer atomics.
__device__ __forceinline__ void eval_pass_tail(const float (&acc)[E_N], const int* sh, float (*red)[NWP * E_N], float* partial, int* hist) {
  // lanes with equal (lane & 7) hold the same waypoint: reduce over lane bits 3..5, then the waves through LDS in a fixed order
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < E_N; ++i) {
    float v = acc[i];
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    if (lane < 8) red[w][lane * E_N + i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NWP * E_N) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int j = 1; j < EVAL_THREADS / 64; ++j) s += red[j][threadIdx.x];
    partial[threadIdx.x] = s;       // a store, not an atomic: the finalize kernels fold the workgroups
  }
  for (int i = threadIdx.x; i < EVAL_HIST; i += EVAL_THREADS)
    if (sh[i]) atomicAdd(hist + i, sh[i]);
}

template <bool FOCAL, bool PRED>
__global__ __launch_bounds__(EVAL_THREADS, EVAL_WAVES) void eval_pass_kernel(const float* logits, const float* gt_obs, const float* gt_occ,
                                                                 const float* gt_flow, const float* origin, int* hist, float* partial,
                                                                 int B, int H, int W, int loss_warp, int met_warp, int use_gt) {
  __shared__ int sh[EVAL_HIST];
  __shared__ float red[EVAL_THREADS / 64][NWP * E_N];
  for (int i = threadIdx.x; i < EVAL_HIST; i += EVAL_THREADS) sh[i] = 0;
  __syncthreads();
  const float inv_hw = 1.f / ((float)H * (float)W);
  float acc[E_N];
#pragma unroll
  for (int i = 0; i < E_N; ++i) acc[i] = 0.f;
  const long long nitem = (long long)B * H * W * NWP;
  const int k = threadIdx.x & 7;                       // EVAL_THREADS % 8 == 0 and the grid stride is a multiple of 8: k is fixed per thread
  int* hk = sh + k * (EVAL_NH * 202);
  const EvalArgs a = {logits, gt_obs, gt_occ, gt_flow, origin, H, W, loss_warp, met_warp, use_gt};
  for (long long it = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x; it < nitem; it += (long long)gridDim.x * EVAL_THREADS)
    eval_item<FOCAL, PRED>(a, it, k, inv_hw, hk, acc);
  eval_pass_tail(acc, sh, red, partial + (long long)blockIdx.x * EVAL_PSTRIDE, hist);
}

// The per-scene pass (stj_eval_scenes_fwd): grid (G, B), blockIdx.y = scene.  A workgroup walks ITS scene's H*W*8 items with stride
// G * EVAL_THREADS (a multiple of 8: k is fixed per thread) and never touches another scene's items, partial sums or histograms; the
// workgroups of a dead scene (live[b] == 0) return before any load.  partial [B][G][EVAL_PSTRIDE], hist [B][EVAL_HIST].
template <bool FOCAL, bool PRED>
__global__ __launch_bounds__(EVAL_THREADS, EVAL_WAVES) void eval_scenes_pass_kernel(const float* logits, const float* gt_obs, const float* gt_occ,
                                                                        const float* gt_flow, const float* origin, const int* live, int* hist,
                                                                        float* partial, int H, int W, int loss_warp, int met_warp, int use_gt) {
  __shared__ int sh[EVAL_HIST];
  __shared__ float red[EVAL_THREADS / 64][NWP * E_N];
  const int b = blockIdx.y;
  if (live && live[b] == 0) return;
  for (int i = threadIdx.x; i < EVAL_HIST; i += EVAL_THREADS) sh[i] = 0;
  __syncthreads();
  const float inv_hw = 1.f / ((float)H * (float)W);
  float acc[E_N];
#pragma unroll
  for (int i = 0; i < E_N; ++i) acc[i] = 0.f;
  const long long per = (long long)H * W * NWP, first = (long long)b * per;     // the scene as a batch of one: its planes are contiguous
  const int k = threadIdx.x & 7;
  int* hk = sh + k * (EVAL_NH * 202);
  const EvalArgs a = {logits + first * 4, gt_obs + first, gt_occ + first, gt_flow + first * 2, origin + first, H, W, loss_warp, met_warp, use_gt};
  for (long long it = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x; it < per; it += (long long)gridDim.x * EVAL_THREADS)
    eval_item<FOCAL, PRED>(a, it, k, inv_hw, hk, acc);
  eval_pass_tail(acc, sh, red, partial + ((long long)b * gridDim.x + blockIdx.x) * EVAL_PSTRIDE, hist + (long long)b * EVAL_HIST);
}

// block (k, h) = the PR-AUC of histogram h of waypoint k -> auc[k*4 + h]; h = 0 also decides the gate (1 everywhere without use_gt)
__global__ __launch_bounds__(128) void eval_auc_kernel(const int* hist, float* auc, float* gate, float* auc_out, float* gate_out, int use_gt) {
  __shared__ AucScratch s;
  const int kh = blockIdx.x;
  const double a = auc_pr_block(hist + kh * 202, s);
  if (threadIdx.x != 0) return;
  auc[kh] = (float)a;
  if (auc_out) auc_out[kh] = (float)a;
  if (kh % EVAL_NH == H_GATE) {
    const float gk = use_gt ? (((1.0 - a) < 1.0) ? 1.f : 0.f) : 1.f;
    gate[kh / EVAL_NH] = gk;
    if (gate_out) gate_out[kh / EVAL_NH] = gk;
  }
}

struct EvalCfg { float ogm_w, occ_w, fow, replica, loss_scale; int loss_warp, met_warp; };

// The workgroups' partial sums folded in a fixed order, in double: 1024 threads, eight per accumulator, each over every eighth workgroup,
// then the eight in order -> sums[NWP * E_N] in LDS.  Called by ALL 1024 threads of a block; ends behind a barrier.
__device__ __forceinline__ void eval_fold(const float* partial, int nparts, double (*part)[EVAL_PSTRIDE], double* sums) {
  const int slot = threadIdx.x % EVAL_PSTRIDE, j = threadIdx.x / EVAL_PSTRIDE;
  double a = 0.0;
  if (slot < NWP * E_N)
    for (int q = j; q < nparts; q += 8) a += (double)partial[(long long)q * EVAL_PSTRIDE + slot];
  part[j][slot] = a;
  __syncthreads();
  if (threadIdx.x < NWP * E_N) {
    const int t = threadIdx.x;
    sums[t] = ((((((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]) + part[4][t]) + part[5][t]) + part[6][t]) + part[7][t];
  }
  __syncthreads();
}

// loss[5] as loss_finalize_kernel, metrics[7] as metrics_finalize_kernel, from sums[8][E_N], auc[8][4] and gate[8], evaluated in double.
// The ONE statement of the formulas: the batch's (eval_finalize_kernel), a scene's and the live scenes' pooled (stj_eval_scenes_fwd).
__device__ __forceinline__ void eval_scores(const double* sums, const float* auc, const float* gate, double npix, const EvalCfg& c,
                                            float* loss, float* metrics) {
  double so = 0, sc = 0, sf = 0, sw = 0, fc = 0;
  double m[7] = {0, 0, 0, 0, 0, 0, 0};
  auto iou = [](double i, double t, double p) { const double d = p + t - i; return d != 0 ? i / d : 0.0; };   // divide_no_nan
  for (int k = 0; k < NWP; ++k) fc += gate[k];
  for (int k = 0; k < NWP; ++k) {
    const double* s = sums + k * E_N;
    so += c.ogm_w * s[E_OBS] / (npix * c.replica);
    sc += c.occ_w * s[E_OCC] / (npix * c.replica);
    const double den = s[E_EX] * c.replica / 2;
    sf += gate[k] * (den != 0 ? s[E_L1] / den : 0.0);
    sw += gate[k] * c.fow * s[E_WARP] / (npix * c.replica);
    m[0] += auc[k * EVAL_NH + H_OBS]; m[1] += auc[k * EVAL_NH + H_OCC];
    m[2] += iou(s[E_IO], s[E_TO], s[E_PO]); m[3] += iou(s[E_IC], s[E_TC], s[E_PC]);
    m[4] += s[E_EX] != 0 ? s[E_EPE] / s[E_EX] : 0.0;
    if (c.met_warp) { m[5] += auc[k * EVAL_NH + H_WARP]; m[6] += iou(s[E_IW], s[E_TW], s[E_PW]); }
  }
  loss[0] = (float)(so / NWP);
  loss[1] = (float)(sc / NWP);
  loss[2] = (float)(sf / fc);
  loss[3] = c.loss_warp ? (float)(sw / fc) : 0.f;
  loss[4] = loss[0] + loss[1] + loss[2] + loss[3];      // the sum of the four (train.py:273), in the order a host-side sum adds them
  for (int i = 0; i < 7; ++i) metrics[i] = (float)(m[i] / NWP);
}

// running (optional) double[12]: += 1, the four losses x loss_scale, the seven metrics (Keras Mean.update_state).
__global__ __launch_bounds__(1024) void eval_finalize_kernel(const float* partial, int nparts, const float* auc, const float* gate,
                                                            float* loss, float* metrics, double* running, double npix, EvalCfg c) {
  __shared__ double part[8][EVAL_PSTRIDE], sums[NWP * E_N];
  eval_fold(partial, nparts, part, sums);
  if (threadIdx.x != 0) return;
  eval_scores(sums, auc, gate, npix, c, loss, metrics);
  if (running) {
    running[0] += 1.0;
    for (int i = 0; i < 4; ++i) running[1 + i] += (double)loss[i] * c.loss_scale;
    for (int i = 0; i < 7; ++i) running[5 + i] += (double)metrics[i];
  }
}

extern "C" long long stj_eval_workspace_bytes(int B, int H, int W) {
  return (long long)EVAL_WS_PART + (long long)eval_grid((long long)B * H * W) * EVAL_PSTRIDE * 4;
}

extern "C" int stj_eval_fwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                            void* workspace, float* loss, float* metrics, float* gate, float* auc, double* running, int B, int H, int W,
                            float ogm_w, float occ_w, float flow_origin_w, float replica, float loss_scale, int flags, hipStream_t stream) {
  if (((uintptr_t)logits) & 15) { stj_set_error("eval: logits must be 16-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)gt_flow) & 7) { stj_set_error("eval: gt_flow must be 8-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)workspace) & 15) { stj_set_error("eval: the workspace must be 16-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)running) & 7) { stj_set_error("eval: running must be 8-byte aligned"); return STJ_EINVAL; }
  if (flags & ~31) { stj_set_error("eval: unknown flag bits %d", flags); return STJ_EINVAL; }
  const long long npix = (long long)B * H * W;
  if (npix <= 0) return STJ_OK;
  const int loss_warp = flags & 1, focal = (flags >> 1) & 1, pred = (flags >> 2) & 1, use_gt = (flags >> 3) & 1, met_warp = ((flags >> 4) & 1) ^ 1;
  int* hist = (int*)workspace;
  float* wauc = (float*)((char*)workspace + EVAL_WS_AUC);
  float* wgate = wauc + NWP * EVAL_NH;
  float* partial = (float*)((char*)workspace + EVAL_WS_PART);
  const int gx = eval_grid(npix);
  hipLaunchKernelGGL(eval_clear_kernel, dim3((EVAL_HIST + 255) / 256), dim3(256), 0, stream, hist);
#define EVAL_PASS(FO, PR) hipLaunchKernelGGL((eval_pass_kernel<FO, PR>), dim3(gx), dim3(EVAL_THREADS), 0, stream, logits, gt_obs, gt_occ, gt_flow, origin, hist, partial, B, H, W, loss_warp, met_warp, use_gt)
  if (focal && pred) EVAL_PASS(true, true); else if (focal) EVAL_PASS(true, false); else if (pred) EVAL_PASS(false, true); else EVAL_PASS(false, false);
#undef EVAL_PASS
  hipLaunchKernelGGL(eval_auc_kernel, dim3(NWP * EVAL_NH), dim3(128), 0, stream, hist, wauc, wgate, auc, gate, use_gt);
  EvalCfg c; c.ogm_w = ogm_w; c.occ_w = occ_w; c.fow = flow_origin_w; c.replica = replica; c.loss_scale = loss_scale;
  c.loss_warp = loss_warp; c.met_warp = met_warp;
  hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(1024), 0, stream, partial, gx, wauc, wgate, loss, metrics, running, (double)npix, c);
  return stj_check_launch("stj_eval_fwd");
}

// ------------------------------------------------------------------------------------------------ every scene of the batch on its own
// stj_eval_scenes_fwd: the pass above with nothing pooled across scenes (the rules that need no device: csrc/eval_scene.h).  Five launches:
//   eval_scenes_clear_kernel     zeroes hist[B][EVAL_HIST];
//   eval_scenes_pass_kernel      grid (G, B), above;
//   eval_scenes_auc_kernel       grid (32, B [+ 1]): the PR-AUC of histogram (k, h) of scene b and that scene's gates; row B of the grid adds
//                                the LIVE scenes' histograms (integers: the pooled histograms exactly) and takes the pooled AUCs and gates;
//   eval_scenes_finalize_kernel  one workgroup per scene: eval_fold over its G partials, eval_scores with npix = H*W -> rows[b][12];
//                                the folded sums are kept in double for the pooled result;
//   eval_scenes_commit_kernel    one workgroup: the pooled sums = the live scenes' sums added scene by scene in double, eval_scores on them
//                                with npix = live * H*W; then ONE thread goes through the live rows in batch order (evs_commit).
// A dead scene's row, gate and auc are written as zeros; none of its inputs is read and none of its partial sums used, and its
// histograms stay the zeros the clear kernel wrote.
// workspace: int hist[B][EVAL_HIST] | double ssums[B][EVAL_PSTRIDE] | float partial[B][G][EVAL_PSTRIDE] | float auc[B+1][32] |
//            float gate[B+1][8] | float rows[B][12]
#define EVS_PIECE 128               // scenes whose rows eval_scenes_commit_kernel stages in LDS at a time
struct EvalScenesWs { long long ssums, partial, auc, gate, rows, total; };
static inline EvalScenesWs eval_scenes_ws(int B, int H, int W) {
  const long long b = B > 0 ? B : 0, g = evs_grid(H, W);
  EvalScenesWs w;
  w.ssums = b * EVAL_HIST * 4;                                   // 25856 b: a multiple of 16
  w.partial = w.ssums + b * EVAL_PSTRIDE * 8;
  w.auc = w.partial + b * g * EVAL_PSTRIDE * 4;
  w.gate = w.auc + (b + 1) * NWP * EVAL_NH * 4;
  w.rows = w.gate + (b + 1) * NWP * 4;
  w.total = (w.rows + b * EVS_COLS * 4 + 15) / 16 * 16;
  return w;
}

__global__ __launch_bounds__(256) void eval_scenes_clear_kernel(int* hist, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0;
}

// block (kh, b): b < B the scene's histogram, b == B the sum of the live scenes' (pool > 0 only).  wauc [B+1][32], wgate [B+1][8].
__global__ __launch_bounds__(128) void eval_scenes_auc_kernel(const int* hist, const int* live, float* wauc, float* wgate, float* auc_out,
                                                              float* gate_out, float* bauc_out, float* bgate_out, int B, int use_gt) {
  __shared__ AucScratch s;
  __shared__ int pooled[202];
  const int kh = blockIdx.x, b = blockIdx.y;
  const int* h = pooled;
  bool any = false;
  if (b < B) {
    any = !live || live[b] != 0;
    h = hist + (long long)b * EVAL_HIST + kh * 202;
  } else {
    // a dead scene's histograms are the zeros of eval_scenes_clear_kernel (its pass workgroups return at once): every scene is added,
    // with no load that waits for a live flag
    const int i0 = threadIdx.x, i1 = threadIdx.x + 128;
    const int* hq = hist + kh * 202;
    int a0 = 0, a1 = 0, mine = live ? 0 : 1;
    for (int q = 0; q < B; ++q, hq += EVAL_HIST) {
      a0 += hq[i0];
      if (i1 < 202) a1 += hq[i1];
    }
    if (live)
      for (int q = threadIdx.x; q < B; q += 128) mine |= live[q] != 0 ? 1 : 0;
    pooled[i0] = a0;
    if (i1 < 202) pooled[i1] = a1;
    any = __syncthreads_or(mine) != 0;
  }
  float* ao = b < B ? auc_out : bauc_out;
  float* go = b < B ? gate_out : bgate_out;
  const long long ob = b < B ? b : 0;
  if (!any) {                     // a dead scene, or a pool without a live scene: zeros
    if (threadIdx.x == 0) {
      wauc[b * (NWP * EVAL_NH) + kh] = 0.f;
      if (ao) ao[ob * (NWP * EVAL_NH) + kh] = 0.f;
      if (kh % EVAL_NH == H_GATE) {
        wgate[b * NWP + kh / EVAL_NH] = 0.f;
        if (go) go[ob * NWP + kh / EVAL_NH] = 0.f;
      }
    }
    return;
  }
  const double a = auc_pr_block(h, s);
  if (threadIdx.x != 0) return;
  wauc[b * (NWP * EVAL_NH) + kh] = (float)a;
  if (ao) ao[ob * (NWP * EVAL_NH) + kh] = (float)a;
  if (kh % EVAL_NH == H_GATE) {
    const float gk = use_gt ? (((1.0 - a) < 1.0) ? 1.f : 0.f) : 1.f;
    wgate[b * NWP + kh / EVAL_NH] = gk;
    if (go) go[ob * NWP + kh / EVAL_NH] = gk;
  }
}

__global__ __launch_bounds__(1024) void eval_scenes_finalize_kernel(const float* partial, int G, const int* live, const float* wauc,
                                                                   const float* wgate, double* ssums, float* wrows, float* rows_out,
                                                                   double npix, EvalCfg c) {
  __shared__ double part[8][EVAL_PSTRIDE], sums[NWP * E_N];
  __shared__ float row[EVS_COLS];
  const int b = blockIdx.x;
  if (live && live[b] == 0) {
    if (threadIdx.x < EVS_COLS) {
      wrows[b * EVS_COLS + threadIdx.x] = 0.f;
      if (rows_out) rows_out[(long long)b * EVS_COLS + threadIdx.x] = 0.f;
    }
    return;
  }
  eval_fold(partial + (long long)b * G * EVAL_PSTRIDE, G, part, sums);
  if (threadIdx.x < NWP * E_N) ssums[(long long)b * EVAL_PSTRIDE + threadIdx.x] = sums[threadIdx.x];
  if (threadIdx.x != 0) return;
  eval_scores(sums, wauc + b * (NWP * EVAL_NH), wgate + b * NWP, npix, c, row, row + EVS_LOSS_COLS);
  for (int i = 0; i < EVS_COLS; ++i) {
    wrows[b * EVS_COLS + i] = row[i];
    if (rows_out) rows_out[(long long)b * EVS_COLS + i] = row[i];
  }
}

__global__ __launch_bounds__(128) void eval_scenes_commit_kernel(const double* ssums, const int* live, const float* wauc, const float* wgate,
                                                                 const float* wrows, float* batch_loss, float* batch_metrics, double* state,
                                                                 float* table, long long* cursor, long long capacity, int B, int pool,
                                                                 double npix_scene, EvalCfg c) {
  __shared__ double sums[NWP * E_N];
  __shared__ float out[EVS_COLS];
  // the rows come in in pieces of EVS_PIECE scenes, loaded by the whole workgroup, and the one thread that commits them in batch order
  // holds state and cursor in registers: it waits for no global load (a global read-modify-write per column and scene otherwise)
  double st[2 * EVS_STATE_COLS];
  long long cur = 0;
  __shared__ float srows[EVS_PIECE * EVS_COLS];
  __shared__ int slive[EVS_PIECE];
  double pooled = 0.0;                 // threads 0..119: the live scenes' sums, added scene by scene
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 2 * EVS_STATE_COLS; ++i) st[i] = state ? state[i] : 0.0;
    if (cursor) cur = *cursor;
  }
  int nlive = 0;                       // thread 0's
  for (int first = 0; first < B; first += EVS_PIECE) {
    const int n = min(EVS_PIECE, B - first);
    for (int i = threadIdx.x; i < n * EVS_COLS; i += 128) srows[i] = wrows[(long long)first * EVS_COLS + i];
    for (int i = threadIdx.x; i < n; i += 128) slive[i] = (!live || live[first + i] != 0) ? 1 : 0;
    __syncthreads();
    if (pool && threadIdx.x < NWP * E_N) {
      const double* sp = ssums + (long long)first * EVAL_PSTRIDE + threadIdx.x;
#pragma unroll 8
      for (int b = 0; b < n; ++b) {
        const double v = sp[(long long)b * EVAL_PSTRIDE];      // loaded whether live or not (a dead scene's slot holds anything): no load waits for a flag
        if (slive[b]) pooled += v;
      }
    }
    if (threadIdx.x == 0)
      for (int b = 0; b < n; ++b)
        if (slive[b]) {
          ++nlive;
          if (state || cursor) evs_commit(srows + b * EVS_COLS, st, table, &cur, capacity, c.loss_scale);      // the copies: written back only where asked for
        }
    __syncthreads();
  }
  if (pool && threadIdx.x < NWP * E_N) sums[threadIdx.x] = pooled;
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (state) {
#pragma unroll
    for (int i = 0; i < 2 * EVS_STATE_COLS; ++i) state[i] = st[i];
  }
  if (cursor) *cursor = cur;
  if (pool) {
    if (nlive) eval_scores(sums, wauc + (long long)B * (NWP * EVAL_NH), wgate + (long long)B * NWP, npix_scene * nlive, c, out, out + EVS_LOSS_COLS);
    else for (int i = 0; i < EVS_COLS; ++i) out[i] = 0.f;       // an empty pool: zeros (as its gates and AUCs)
    if (batch_loss) for (int i = 0; i < EVS_LOSS_COLS; ++i) batch_loss[i] = out[i];
    if (batch_metrics) for (int i = 0; i < 7; ++i) batch_metrics[i] = out[EVS_LOSS_COLS + i];
  }
}

extern "C" long long stj_eval_scenes_workspace_bytes(int B, int H, int W) { return eval_scenes_ws(B, H, W).total; }

extern "C" int stj_eval_scenes_grid(int H, int W) { return evs_grid(H, W); }

extern "C" int stj_eval_scenes_fwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                                   const int* live, void* workspace, float* rows, float* gate, float* auc, float* batch_loss,
                                   float* batch_metrics, float* batch_gate, float* batch_auc, double* state, float* table, long long* cursor,
                                   long long capacity, int B, int H, int W, float ogm_w, float occ_w, float flow_origin_w, float replica,
                                   float loss_scale, int flags, hipStream_t stream) {
  if (((uintptr_t)logits) & 15) { stj_set_error("eval_scenes: logits must be 16-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)gt_flow) & 7) { stj_set_error("eval_scenes: gt_flow must be 8-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)workspace) & 15) { stj_set_error("eval_scenes: the workspace must be 16-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)state) & 7) { stj_set_error("eval_scenes: state must be 8-byte aligned"); return STJ_EINVAL; }
  if (((uintptr_t)cursor) & 7) { stj_set_error("eval_scenes: cursor must be 8-byte aligned"); return STJ_EINVAL; }
  if (flags & ~31) { stj_set_error("eval_scenes: unknown flag bits %d", flags); return STJ_EINVAL; }
  if (capacity < 0) { stj_set_error("eval_scenes: capacity %lld is negative", capacity); return STJ_EINVAL; }
  if (table && !cursor) { stj_set_error("eval_scenes: a table needs a cursor"); return STJ_EINVAL; }
  if (B > EVS_MAXB) { stj_set_error("eval_scenes: B = %d is above %d scenes per call", B, EVS_MAXB); return STJ_EINVAL; }
  if ((long long)B * H * W <= 0 || B <= 0 || H <= 0 || W <= 0) return STJ_OK;
  const int loss_warp = flags & 1, focal = (flags >> 1) & 1, pred = (flags >> 2) & 1, use_gt = (flags >> 3) & 1, met_warp = ((flags >> 4) & 1) ^ 1;
  const EvalScenesWs w = eval_scenes_ws(B, H, W);
  char* base = (char*)workspace;
  int* hist = (int*)base;
  double* ssums = (double*)(base + w.ssums);
  float* partial = (float*)(base + w.partial);
  float *wauc = (float*)(base + w.auc), *wgate = (float*)(base + w.gate), *wrows = (float*)(base + w.rows);
  const int G = evs_grid(H, W);
  const int pool = (batch_loss || batch_metrics || batch_gate || batch_auc) ? 1 : 0;
  const long long nh = (long long)B * EVAL_HIST;
  hipLaunchKernelGGL(eval_scenes_clear_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, stream, hist, nh);
#define EVAL_PASS(FO, PR) hipLaunchKernelGGL((eval_scenes_pass_kernel<FO, PR>), dim3(G, B), dim3(EVAL_THREADS), 0, stream, logits, gt_obs, gt_occ, gt_flow, origin, live, hist, partial, H, W, loss_warp, met_warp, use_gt)
  if (focal && pred) EVAL_PASS(true, true); else if (focal) EVAL_PASS(true, false); else if (pred) EVAL_PASS(false, true); else EVAL_PASS(false, false);
#undef EVAL_PASS
  hipLaunchKernelGGL(eval_scenes_auc_kernel, dim3(NWP * EVAL_NH, B + pool), dim3(128), 0, stream, hist, live, wauc, wgate, auc, gate, batch_auc,
                     batch_gate, B, use_gt);
  EvalCfg c; c.ogm_w = ogm_w; c.occ_w = occ_w; c.fow = flow_origin_w; c.replica = replica; c.loss_scale = loss_scale;
  c.loss_warp = loss_warp; c.met_warp = met_warp;
  const double npix = (double)H * (double)W;
  hipLaunchKernelGGL(eval_scenes_finalize_kernel, dim3(B), dim3(1024), 0, stream, partial, G, live, wauc, wgate, ssums, wrows, rows, npix, c);
  if (pool || state || cursor)
    hipLaunchKernelGGL(eval_scenes_commit_kernel, dim3(1), dim3(128), 0, stream, ssums, live, wauc, wgate, wrows, batch_loss, batch_metrics,
                       state, table, cursor, capacity, B, pool, npix, c);
  return stj_check_launch("stj_eval_scenes_fwd");
}
