/* strajnet_hip.h -- C ABI of libstrajnet_hip.so (MI355X / gfx950 kernels of the STrajNet hot path).
 *
 * The reference (georgeliu233/STrajNet) has no FFI / plugin interface: its hot path is TensorFlow ops issued from
 * Python (modules.py, FG_MSA.py, trajNet.py, loss.py).  This header is therefore the boundary a maintainer would bind
 * (ctypes stub in INTEGRATION.md); each entry point names the reference op sequence it replaces (file:line relative
 * to the reference repo).
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (no allocation, no synchronisation inside; every call is
 *     one or a few stream-ordered launches on `stream` => hipGraph-capturable); 16-byte alignment where noted.
 *   - dtype: STJ_F32 = 0 (exact-f32 MFMA, parity mode), STJ_BF16 = 1 (bf16 storage, f32 accumulate: the training throughput
 *     mode) or STJ_F16 = 2 (fp16 storage, f32 accumulate: the inference mode of BASELINE config 4; every entry point accepts it,
 *     the backward ones without any loss scaling and through the generic conv kernels) selects the activation type `T`; parameters, biases, LN gamma/beta, tables and all gradients of parameters are f32.
 *   - return 0 on success, negative stj_status otherwise; message via stj_last_error() (thread local).  A `dtype` outside
 *     enum stj_dtype is STJ_EINVAL (nothing is launched) unless an entry documents STJ_EUNSUPPORTED for it.
 *   - tensors are NHWC / row-major exactly as in the reference.
 *   - "+=" outputs are ACCUMULATED with f32 atomics (they point into the flat gradient buffer).
 */
#ifndef STRAJNET_HIP_H
#define STRAJNET_HIP_H
#include <hip/hip_runtime_api.h>
#ifdef __cplusplus
extern "C" {
#endif

enum stj_status { STJ_OK = 0, STJ_EINVAL = -1, STJ_ELAUNCH = -2, STJ_EUNSUPPORTED = -3 };
enum stj_dtype { STJ_F32 = 0, STJ_BF16 = 1, STJ_F16 = 2 };
enum stj_act { STJ_ACT_NONE = 0, STJ_ACT_GELU = 1, STJ_ACT_ELU = 2 };
enum stj_unary { STJ_U_GELU = 1, STJ_U_ELU = 2, STJ_U_TANH_SCALE = 3 };
/* STJ_HEAD_CZ: channels of the inference heads' projected tensor Z (stj_upconv_fwd_head -> stj_outconv_pair_gather): 18 (9 taps x 2
 * outputs) + 2 zero channels = whole 8-byte pieces (24 until round 6: 17 % more z traffic) */
enum stj_shape { STJ_HEAD_CZ = 20 };

const char* stj_last_error(void);
int stj_abi_version(void);

/* Batched strided GEMM with fused epilogue:  C[z] = act(alpha * A[z] B[z] + bias[z]) + res[z],  z = z1*nb2 + z2.
 * Replaces Keras Dense (modules.py:36-37,76-79,270-271), 1x1 Conv2D (FG_MSA.py:54-64), tfa MultiHeadAttention
 * projections and q k^T / attn v einsums (trajNet.py:33,42,71,80,195,225; FG_MSA.py:147,176), the time-collapsed
 * Conv3D(8,1,1) skips (modules.py:693-717,750-765) and all their dgrad/wgrad (tape.gradient, train.py:223).
 * Element strides: A(m,k) at sAm*m + sAk*k (+ batch), B(k,n) at sBk*k + sBn*n; C row-major with ldc.
 * c_f32: C is f32; accumulate: C += (f32 atomics; splitk may be >1, 0 = auto); colsum (optional): colsum[z][n] +=
 * sum_k B[z](k,n) (the bias gradient belonging to dW = x^T dY), addressed with the bias batch strides.
 * nkb >= 1 K segments: the contraction also runs over nkb segments of A / B that lie sAkb / sBkb elements apart (the input
 * gradient of a layer applied with 8 per-waypoint weight sets to ONE shared input is a single GEMM with K' = 8 K). */
int stj_gemm(const void* A, const void* B, void* C, const float* bias, const void* res, float* colsum,
             int M, int N, int K, int nb1, int nb2,
             long long sAb1, long long sAb2, long long sAm, long long sAk,
             long long sBb1, long long sBb2, long long sBk, long long sBn,
             long long sCb1, long long sCb2, long long ldc,
             long long sBias1, long long sBias2, long long sRes1, long long sRes2, long long ldres,
             int act, float alpha, int dtype, int c_f32, int accumulate, int splitk,
             int nkb, long long sAkb, long long sBkb, void* group, hipStream_t stream);
/* Grouped launch.  `group` (last pointer argument of stj_gemm; NULL = launch at once) is CALLER-OWNED HOST memory of
 * stj_gemm_group_workspace_bytes() bytes, initialised by stj_gemm_group_begin: stj_gemm calls handed the group are RECORDED in it
 * (arguments validated) and launched by stj_gemm_group_end(group, stream) as ONE kernel per 4 problems of equal dtype (64x64 or 32x32
 * tiles): the input and weight gradient of a Dense layer (tape.gradient of modules.py:36-37 etc.), the q / k / v projections of a
 * tfa MultiHeadAttention (trajNet.py:33,71,195), dP / dV and dQ / dK of an attention.  The problems of a group must not depend on
 * each other.  The library keeps no state between calls: two host threads use two groups. */
long long stj_gemm_group_workspace_bytes(void);
int stj_gemm_group_begin(void* group);
int stj_gemm_group_end(void* group, hipStream_t stream);
/* Grouped stream-K weight gradients (csrc/wgrad_sk.hip): for every job  dw[z] += x[z]^T dy[z]  and, if db != NULL,
 * db[z] += column sums of dy[z]  (z = z1*nb2 + z2 < nb1*nb2) -- tape.gradient (train.py:223) w.r.t. the kernel / bias of the Keras
 * Dense layers, 1x1 convs and tfa-MHA projections (modules.py:36-37,76-83,270-272; trajNet.py:71-77,195-211; FG_MSA.py:54-64) --
 * ALL jobs of the list in ONE launch (per 28 jobs) on `wg_budget` workgroups (<= 0: one per CU).  x [rows, cin] with row stride ldx,
 * dy [rows, cout] with row stride lddy (activation dtype, 16-byte aligned), dw f32 [cin, cout] with row stride lddw, db f32 [cout];
 * s*1 / s*2 are the element strides of the two batch levels.  A workgroup owns a full-width 96 x 384 tile of a job, streams the rows
 * once through an LDS-DMA ring, and the launch's workgroups share the 32-row slabs of all jobs evenly (stream-K): f32 atomics only
 * where a workgroup leaves a tile.  Jobs must satisfy stj_wgrad_job_supported (16-bit dtype, rows % 32 == 0, cin, cout and all
 * strides of x / dy multiples of 8); anything else is stj_gemm's (accumulate = 1). */
typedef struct stj_wgrad_job {
  const void* x; const void* dy; float* dw; float* db;
  int rows, cin, cout, nb1, nb2;
  long long ldx, lddy, lddw;
  long long sx1, sx2, sdy1, sdy2, sdw1, sdw2, sdb1, sdb2;
} stj_wgrad_job;
int stj_wgrad_job_supported(const stj_wgrad_job* job, int dtype);
int stj_wgrad_group(const stj_wgrad_job* jobs, int njobs, int dtype, int wg_budget, hipStream_t stream);
/* out[n] += sum_m X[m,n]  (bias gradients of the conv heads). */
int stj_colsum(const void* X, float* out, int M, int N, long long ld, int dtype, hipStream_t stream);
/* f32 <-> bf16 / fp16 copy (16-bit compute copy of the flat parameter buffer). */
int stj_cast(const void* src, int sdtype, void* dst, int ddtype, long long n, hipStream_t stream);

/* Gelu (tanh form, modules.py:18-29 / FG_MSA.py:7-18), ELU (Keras activation='elu'), tanh*scale (FG_MSA.py:116-117).
 * bwd: saved = x for GELU, y for ELU / tanh. */
int stj_unary_fwd(const void* x, void* y, long long n, int op, float p0, int dtype, hipStream_t stream);
int stj_unary_bwd(const void* dy, const void* saved, void* dx, long long n, int op, float p0, int dtype, hipStream_t stream);
/* GlobalMaxPooling1D over the 11 time steps (trajNet.py:34,44); backward splits ties evenly like tf.reduce_max. */
int stj_maxpool_fwd(const void* x, void* y, int* idx, long long outer, int Tn, int C, int dtype, hipStream_t stream);
int stj_maxpool_bwd(const void* dy, const void* x, const void* y, void* dx, long long outer, int Tn, int C, int dtype, hipStream_t stream);

/* Keras LayerNormalization (modules.py:179,184,272,433,517,557 eps 1e-5; FG_MSA.py:52, trajNet.py:72-73,110-111,
 * 206-207 eps 1e-3).  gather_res != 0 fuses the PatchMerging 2x2 gather-concat (modules.py:282-287): x is
 * [B,res,res,C0], C = 4*C0.  group_rows/ngroups/gstride: row runs of group_rows rows use parameter set
 * (run % ngroups) at gamma + g*gstride (the 8 per-waypoint LayerNorms, trajNet.py:257). */
int stj_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                      long long rows, int C, float eps, int gather_res, int C0, long long group_rows, int ngroups,
                      long long gstride, int dtype, hipStream_t stream);
/* y = LayerNorm(x) + res (res [rows,C], type T; no gather): the norm followed by the sum with another branch in one pass
 * (vec + maps ahead of all_patch_norm, modules.py:589; Cross_AttentionT output + query, trajNet.py:305-317).  Backward:
 * stj_layernorm_bwd for x; the gradient of res is dy itself. */
int stj_layernorm_res_fwd(const void* x, const float* gamma, const float* beta, const void* res, void* y, float* mean,
                          float* rstd, long long rows, int C, float eps, long long group_rows, int ngroups,
                          long long gstride, int dtype, hipStream_t stream);
int stj_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                      void* dx, float* dgamma, float* dbeta, long long rows, int C, int gather_res, int C0,
                      long long group_rows, int ngroups, long long gstride, const void* dres, int nparts, long long part_stride,
                      int dtype, hipStream_t stream);
/* Two LayerNorm backward passes in one launch, for y = LN2(LN1(x1) [+ add]) (the stem: modules.py:437-446 with :578 / :590): d2 = dLN2(dy)
 * at x2 (written to d2 when non-NULL: the gradient of `add`), dx1 = dLN1(d2) at x1; d2 is rounded to T in between, as two stj_layernorm_bwd
 * calls hand it over.  Plain [rows, C] tensors, one parameter set per norm, nparts / part_stride as in stj_layernorm_bwd (per norm). */
int stj_layernorm_bwd_chain_supported(int C, int dtype);
int stj_layernorm_bwd_chain(const void* dy, const void* x2, const float* gamma2, const float* mean2, const float* rstd2, const void* x1,
                            const float* gamma1, const float* mean1, const float* rstd1, void* d2, void* dx1, float* dgamma2, float* dbeta2,
                            float* dgamma1, float* dbeta1, long long rows, int C, int nparts2, long long part_stride2, int nparts1,
                            long long part_stride1, int dtype, hipStream_t stream);
/* dres (optional, x's layout, no gather): gradient arriving over the residual connection that bypasses the norm; dx += dres.
 * nparts / part_stride: dgamma and dbeta are "+=" into nparts copies that lie part_stride floats apart (workgroups rotate over
 * them: 256 same-address atomics per channel otherwise); the caller sums the copies.  nparts = 1: plain [C] buffers. */

/* Fused (shifted-)window attention, window 8x8, head_dim 32: roll + window_partition + softmax(q k^T*scale +
 * relative_position_bias[+shift mask]) v + window_reverse + roll (modules.py:49-63,103-134,189-216,229-255).
 * qkv [B,res*res,3*heads*32] in original token order, table f32 [225,heads], out [B,res*res,heads*32]. */
int stj_win_attn_fwd(const void* qkv, const float* table, void* out, int B, int res, int heads, int shift,
                     int dtype, hipStream_t stream);
int stj_win_attn_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable, int nparts,
                     int B, int res, int heads, int shift, int dtype, hipStream_t stream);
/* bwd: dtable f32 [nparts][225,heads], "+=": workgroup i adds the bias-table gradient of its window into copy i % nparts and the
 * caller sums the copies (one copy = hundreds of same-address atomics per table entry on the 64x64 stage; nparts = 1 is valid). */

/* Fused MLP half of SwinTransformerBlock (modules.py:260 = x + drop_path(mlp(norm2(x))); Mlp.call :40-46; Gelu :18-29; drop_path
 * :137-151), ONE kernel per direction (csrc/swin_fused.hip).  x, y [M,C] (C in {96,192,384}); gamma/beta f32 [C] (LN eps);
 * w1 [C,4C], w2 [4C,C] activation dtype (Keras [in,out]); b1 [4C], b2 [C] f32.
 * DropPath: rng_state = device int64[2] {seed, step} (NULL or p_drop = 0: none), one draw per sample = run of rows_per_sample rows,
 * drawn exactly as stj_dropout(inner = rows_per_sample * C) draws it.
 *   fwd: y = x + dp * (gelu(LN(x) w1 + b1) w2 + b2)
 *   bwd: dx = dy + LN'(...), dgamma/dbeta "+=" (nparts copies part_stride floats apart, as stj_layernorm_bwd), and the operands
 *        of the two weight gradients written once: h = gelu(pre) [M,4C], dpre [M,4C], ln = LN(x) [M,C], dys = dp*dy [M,C]
 *        (dys may be NULL when there is no DropPath: use dy).  dW1 = ln^T dpre, db1 = colsum(dpre), dW2 = h^T dys,
 *        db2 = colsum(dys) are stj_gemm split-K launches.
 * ws: workspace of stj_swin_split_workspace_bytes(M, C) bytes (0 = this (M, C) takes none: pass NULL), ZERO-INITIALISED ONCE by the caller
 *   and then left to the kernels: where a stage has fewer row blocks / windows than the chip has CUs, a unit is cut into slices of the hidden
 *   dimension (MLP half) or of the heads (attention half) that run as separate workgroups:
 *     C = 384, many slices (the 2048-row stage: (row block, 1/8 of the hidden dimension) workgroups, 256 at B = 8 instead of 32, each
 *       streaming 1/8 of the weights): partial sums [slices][M][C] f32 that a second launch adds up and finishes (bias + DropPath +
 *       shortcut; LayerNorm backward + dgamma / dbeta);
 *     two slices (C = 192 below 32768 rows; C = 384 at 8192 rows): the slices meet INSIDE the launch -- each writes its accumulators as a
 *       slab (write-through stores) and draws a ticket from the unit's arrival counter; the workgroup that draws the last one adds the
 *       other slab and runs the epilogue.  The counters live behind the partial-sum region and re-arm themselves (hence "zeroed once").
 *   REQUIRED at C = 384 (STJ_EINVAL without it); at C = 192 NULL selects one workgroup per unit.  The four stj_swin_* entry points share
 *   the workspace layout (launches that share a workspace must be ordered on one stream); stj_swin_attn_* at C = 384 run (window, 2 of the
 *   12 heads) workgroups + a finishing launch (every dtype; in f32 the Wqkv slice of a head is staged in two halves), or two slices of six
 *   heads that meet inside the launch (16-bit, more than 48 windows).  The arrival counters are the last 16384 bytes of the workspace: 4096
 *   units per launch (stj_swin_attn_bwd at C = 384, 16-bit, with more windows: STJ_EUNSUPPORTED) and all zero again behind every call.
 * Preconditions the kernels rely on and the host does not check: every activation, weight and output pointer, gamma, b2, bproj and ws
 *   16-byte aligned (rows and vectors are read as 16-byte pieces); rows_per_sample a positive multiple of 16 (checked: STJ_EINVAL);
 *   part_stride >= C. */
long long stj_swin_split_workspace_bytes(long long M, int C);
int stj_swin_mlp_fwd(const void* x, const float* gamma, const float* beta, const void* w1, const float* b1, const void* w2,
                     const float* b2, void* y, long long M, int C, float eps, const long long* rng_state, int site,
                     float p_drop, long long rows_per_sample, int dtype, void* ws, hipStream_t stream);
int stj_swin_mlp_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const void* w1, const float* b1,
                     const void* w2, void* dx, void* h, void* dpre, void* ln, void* dys, float* dgamma, float* dbeta,
                     int nparts, long long part_stride, long long M, int C, float eps, const long long* rng_state, int site,
                     float p_drop, long long rows_per_sample, int dtype, void* ws, hipStream_t stream);

/* Fused attention half of SwinTransformerBlock, forward (modules.py:225-258: norm1, roll, window_partition, WindowAttention :103-134
 * with the shift mask :189-216, window_reverse, roll, drop_path + shortcut), one workgroup per 8x8 window (csrc/swin_fused.hip):
 *   y = x + dp * (proj(window_attention(LN(x) wqkv + bqkv)) + bproj);  x, y [B,res*res,C], C in {96,192,384}, heads = C/32;
 *   wqkv [C,3C], wproj [C,C] activation dtype (Keras [in,out]); bqkv [3C], bproj [C], gamma/beta [C], table [225,heads] f32.
 * Training hand-offs (all or none; NULL for inference): qkv [B,N,3C], a = attention output before proj [B,N,C], ln = LN(x) [B,N,C],
 * mean / rstd f32 [B*N] -- the operands stj_win_attn_bwd, stj_layernorm_bwd and the dgrad / wgrad stj_gemm launches of backward read.
 * DropPath: one draw per sample b at (rng_state, site), as stj_dropout(inner = N*C) draws it. */
int stj_swin_attn_fwd(const void* x, const float* gamma, const float* beta, const void* wqkv, const float* bqkv,
                      const float* table, const void* wproj, const float* bproj, void* y, void* qkv, void* a, void* ln,
                      float* mean, float* rstd, int B, int res, int C, int shift, float eps, const long long* rng_state,
                      int site, float p_drop, int dtype, void* ws, hipStream_t stream);

/* Backward of stj_swin_attn_fwd in one launch (one workgroup per window): dys = dp*dy, da = dys wproj^T, window-attention backward,
 * dLN = dqkv wqkv^T, dx = dy + LayerNorm'(dLN); "+=" outputs: dtable [tparts][225,heads] (workgroup i adds into copy i % tparts),
 * dgamma / dbeta (nparts copies part_stride floats apart).  Reads x, dy, the saved qkv / mean / rstd; writes dx, dqkv [B,N,3C] and
 * (when rng_state != NULL and p_drop > 0: else may be NULL) dys [B,N,C] -- the operands of the two weight gradients, which stay
 * stj_gemm launches: dWproj = a^T dys (+ colsum), dWqkv = ln^T dqkv (+ colsum), a / ln saved by the forward kernel.  C in {96,192,384}. */
int stj_swin_attn_bwd(const void* x, const void* dy, const void* qkv, const float* mean, const float* rstd, const float* gamma,
                      const void* wqkv, const void* wproj, const float* table, void* dx, void* dqkv, void* dys,
                      float* dtable, int tparts, float* dgamma, float* dbeta, int nparts, long long part_stride,
                      int B, int res, int C, int shift, const long long* rng_state, int site, float p_drop, int dtype, void* ws,
                      hipStream_t stream);

/* Fused Cross_AttentionT block: the 8 time-separated cross-attentions of TrajNetCrossAttention (trajNet.py:189-234 Cross_AttentionT --
 * tfa MultiHeadAttention(head 42 x 3, out 128, dropout .1), LayerNorm(1e-3), Dense(512, elu), Dropout, Dense(384), Dropout,
 * LayerNorm(1e-3) -- and :305-317, the loop over the waypoints with `+ query`) as ONE kernel per direction (csrc/xattn_fused.hip):
 * one workgroup per 64 tokens of a (set z, scene b), every intermediate chained in registers, weights streamed through LDS.
 *   stj_xattn_pack: the set's weights (f32 masters wq [3,384,42], wo [3,42,128], w1 [128,512], w2 [512,384] of set 0; set z lies
 *     zstride elements further) -> `pack`, Z streams of stj_xattn_pack_workspace_bytes(dtype) bytes in the activation dtype, laid out
 *     as the LDS images the kernels stage (once per step: the weights change).
 *   stj_xattn_fwd: y [Z,B,HW,384] = LN2(dropout(dropout(elu(LN1(MHA(query,k,v)) W1 + b1)) W2 + b2)) + query.  query [Z,B,HW,384];
 *     k, v [Z,B,64,126] = key Wk[z], key Wv[z] (stj_gemm); kvalid int32 [B,64] or NULL; bo/g1/be1 [128], b1 [512], b2/g2/be2 [384]
 *     f32 vectors of set 0.  rng_state != NULL: training, the three dropout sites draw with the layouts [Z,B,3,HW,64],
 *     [Z,B*HW,512], [Z,B*HW,384] (as stj_dropout would).  sq, so [Z,B,HW,144], sv1 [.,128], su2 [.,384]: saves for backward
 *     (all or none; NULL for inference).  HW % 64 == 0.  The f32 vectors bo, g1, be1, b1, b2, g2, be2 must be 16-byte aligned (here and in
 *     stj_xattn_bwd) and zstride % 4 == 0: the kernels read them as float4.
 *   stj_xattn_bwd: reads dy, query, k, v, sq, sv1, su2 and the pack; writes dquery, dk, dv (via the f32 per-tile partials dkp / dvp,
 *     stj_xattn_bwd_workspace_bytes(Z,B,HW) bytes each, reduced by a second launch) and the operands of the weight-gradient
 *     stj_gemm launches the caller makes: hd, dpre [Z,B,HW,512], du2 [.,384], n1, dv1 [.,128], dq [.,144]
 *     (dW2 = hd^T du2 + colsum, dW1 = n1^T dpre + colsum, dWo[h] = so_h^T dv1, dWq[h] = query^T dq_h);
 *     "+=": dg1, dbe1, dbo [128], dg2, dbe2 [384] of set z at + z * zstride. */
long long stj_xattn_pack_workspace_bytes(int dtype);
long long stj_xattn_pack_tail_workspace_bytes(int dtype);    /* once behind the Z streams: the kernels copy fixed-size pieces */
int stj_xattn_pack(const float* wq, const float* wo, const float* w1, const float* w2, long long zstride, int Z, void* pack, int dtype,
                   hipStream_t stream);
int stj_xattn_fwd(const void* query, const void* k, const void* v, const int* kvalid, const void* pack, const float* bo,
                  const float* g1, const float* be1, const float* b1, const float* b2, const float* g2, const float* be2,
                  long long zstride, void* y, void* sq, void* so, void* sv1, void* su2, int Z, int B, int HW,
                  const long long* rng_state, int site_a, int site_1, int site_2, float p_drop, int dtype, hipStream_t stream);
long long stj_xattn_bwd_workspace_bytes(int Z, int B, int HW);
int stj_xattn_bwd(const void* dy, const void* query, const void* k, const void* v, const int* kvalid, const void* pack,
                  const float* g1, const float* be1, const float* b1, const float* g2, long long zstride, const void* sq,
                  const void* sv1, const void* su2, void* dquery, void* dk, void* dv, float* dkp, float* dvp, void* hd,
                  void* dpre, void* du2, void* n1, void* dv1, void* dq, float* dg1, float* dbe1, float* dbo, float* dg2,
                  float* dbe2, int Z, int B, int HW, const long long* rng_state, int site_a, int site_1, int site_2,
                  float p_drop, int dtype, hipStream_t stream);

/* Row softmax of the global attentions: P = softmax(S + bias + (-10e9 where !(qvalid&kvalid))) (tfa MHA mask
 * semantics, f32 add); S f32 [batch,H,Nq,Nk] (Nk <= 256).  bwd: dS = P*(dP - sum(P dP)). */
int stj_softmax_fwd(const float* S, void* P, const int* qvalid, const int* kvalid, const float* bias,
                    long long batch, int H, int Nq, int Nk, int dtype, hipStream_t stream);
int stj_softmax_bwd(const void* P, const float* dP, void* dS, long long rows, int Nk, int dtype, hipStream_t stream);
/* Tiny attention (at most 16 queries / keys per batch element and head: the TrajEncoder's self-attention over 11 time steps, trajNet.py:33,42)
 * in one launch per direction: o [Bt,N,H*d] = dropout(softmax(scale q k^T, masked logits += -10e9)) v; q, k, v [Bt,N,H*d]; qvalid / kvalid
 * int32 [Bt,N] or NULL; dropout on the coefficients [Bt,H,N,N] at (rng_state, site), drawn as stj_dropout draws that tensor (NULL / p = 0:
 * none).  Backward recomputes the probabilities: dq, dk, dv written.  stj_small_attn_supported(N, H, d, dtype) = 1 for the geometries it
 * takes (otherwise: stj_gemm + stj_softmax_* + stj_dropout). */
int stj_small_attn_supported(int N, int H, int d, int dtype);
int stj_small_attn_fwd(const void* q, const void* k, const void* v, const int* qvalid, const int* kvalid, void* o, long long Bt, int N, int H,
                       int d, float scale, const long long* rng_state, int site, float p_drop, int dtype, hipStream_t stream);
int stj_small_attn_bwd(const void* q, const void* k, const void* v, const int* qvalid, const int* kvalid, const void* dO, void* dq, void* dk,
                       void* dv, long long Bt, int N, int H, int d, float scale, const long long* rng_state, int site, float p_drop, int dtype,
                       hipStream_t stream);
/* Fused agent branch (csrc/agent_fused.hip).
 * stj_agent_pack: transposed copies ([N][K], K contiguous, activation dtype) of the branch's eleven Dense / tfa kernels -- the layout
 * the forward kernels stream as MFMA A fragments -- into `out` (stj_agent_pack_workspace_bytes(dtype) bytes); once per step.
 * stj_agent_enc_fwd / _bwd: TrajEncoder.call (trajNet.py:38-48) for all B (n_obs + n_occ) agents in ONE launch per direction: Conv1D(5 -> 64)
 * + ELU, the 4-head tfa self-attention over the 11 steps with the (x != 0) mask and dropout on the coefficients, GlobalMaxPooling1D,
 * Dense(3 -> 64) on the step-0 type one-hot, concat, Dense(384 -> 384) + ELU.  Forward writes enc and the agent mask cmi, and, when the
 * five s_* pointers are given, what backward reads.  Backward writes the three dY tensors whose weight gradients are the CALLER's
 * (dW += X^T dY through stj_wgrad_group / stj_gemm with X = s_cat / s_att / s_nodes) and accumulates the 5 x 64, 64 and 3 x 64 ones itself.
 * A step is valid where its RAW float32 x differs from 0 (tf.not_equal(x, 0): -0.0 is invalid, a value that rounds to 0 in the activation
 * dtype is valid).  bo and bs are read as float4: 16-byte aligned; so are the d_enc_f32 slabs (each slab, i.e. B (n_obs + n_occ) 384 floats
 * from a 16-byte aligned base).  The pack, the natural-layout 16-bit kernels and every activation tensor are read or written 16 bytes at a time. */
typedef struct stj_agent_weights {          /* f32 masters (views of the flat parameter buffer), Keras / tfa layouts */
  const float* e_wq; const float* e_wk; const float* e_wv;     /* traj_encoder/node_attention query | key | value kernels [4][64][64] */
  const float* e_wo;                                            /* .../projection_kernel [4][64][320] */
  const float* e_ws;                                            /* traj_encoder/sublayer/kernel [384][384] */
  const float* i_wq; const float* i_wk; const float* i_wv;     /* cross_attention/mha query | key | value kernels [6][384][64] */
  const float* i_wo;                                            /* .../projection_kernel [6][64][384] */
  const float* i_w1; const float* i_w2;                         /* FFN1/kernel [384][1536], FFN2/kernel [1536][384] */
} stj_agent_weights;
typedef struct stj_agent_enc_args {
  const float* obs; const float* occ;        /* tracks [B][n_obs][11][8], [B][n_occ][11][8] f32 */
  int n_obs, n_occ, B, dtype;
  const void* pack;                          /* stj_agent_pack output */
  const float* wn; const float* bn;          /* node_feature kernel [1][5][64] + bias (f32 masters) */
  const float* wv3;                          /* vector_feature kernel [3][64] */
  const float* bo; const float* bs;          /* node_attention projection_bias [320], sublayer bias [384] */
  void* enc;                                 /* [B (n_obs + n_occ)][384] (forward: out; backward: in) */
  int* cmi;                                  /* [B (n_obs + n_occ)] agent has a valid step (forward: out) */
  void* s_nodes; void* s_qkv; void* s_att; void* s_pmask; void* s_cat;     /* saved for backward ([rows 11][64], [rows 11][768], [rows 11][256], uint16 [agents][320], [agents][384]); all NULL: inference */
  const long long* rng_state; int site; float p_drop;                    /* attention dropout, drawn as stj_dropout draws [agents][4][11][11] */
  /* backward only */
  const void* d_enc; int d_enc_f32;          /* [agents][384] in the activation dtype (d_enc_f32 = 0), or d_enc_f32 f32 slabs [d_enc_f32][agents][384] to be added */
  const void* wq; const void* wk; const void* wv; const void* wo; const void* ws;      /* the kernels in the activation dtype, natural layouts */
  void* dpre_s; void* dout; void* dqkv;      /* written: dY of sublayer [agents][384], projection [rows 11][320], q|k|v [rows 11][768] */
  float* dwn; float* dbn; float* dwv3;       /* += (atomics) */
} stj_agent_enc_args;
typedef struct stj_agent_int_args {
  const void* enc; const int* cmi;           /* stj_agent_enc_fwd outputs [B 64][384], [B 64] */
  int n_obs, n_occ, B, dtype;                /* n_obs + n_occ == 64; 16-bit dtypes */
  const void* pack;
  const void* seg;                           /* seg_embed kernel [2][384], ACTIVATION dtype */
  const float* bo; const float* g1; const float* be1; const float* b1; const float* b2; const float* g2; const float* be2;     /* cross_attention: projection_bias, norm1, FFN1 / FFN2 bias, norm2 (f32 masters) */
  const float* g_obs; const float* b_obs; const float* g_occ; const float* b_occ;                                             /* obs_norm | occ_norm */
  void* key;                                 /* out [B 64][384] */
  float* ws_v1; float* ws_u2;                /* forward workspaces: [6][B 64][384] and [4][B 64][384] f32 (per head / per hidden chunk partial sums, added in a fixed order: no atomics) */
  void* s_concat; void* s_qin; void* s_q; void* s_k; void* s_v; void* s_att; void* s_v1; void* s_n1; void* s_h; void* s_u2; void* s_out;   /* saved for backward ([B 64][384]; s_h [B 64][1536]); all NULL: inference */
  const long long* rng_state; int site_a, site_1, site_2; float p_drop;      /* dropout sites: coefficients [B][6][64][64], after FFN1 [B 64][1536], after FFN2 [B 64][384] */
  /* backward only */
  const void* dkey;
  const void* wq; const void* wk; const void* wv; const void* wo; const void* w1; const void* w2;      /* natural layouts, activation dtype */
  float* d_enc;                              /* written: gradient of enc as 7 slabs [7][B 64][384] f32 (stj_agent_enc_bwd with d_enc_f32 = 7 adds them) */
  float* ws_dn1;                             /* backward workspace [4][B 64][384] f32 */
  void* dq; void* dk; void* dv; void* dv1; void* dpre1; void* dz2;          /* written: dY of the q / k / v projections, the output projection, FFN1, FFN2 */
  float* dseg; float* dg1; float* dbe1; float* dg2; float* dbe2; float* dg_obs; float* db_obs; float* dg_occ; float* db_occ;      /* += (atomics) */
} stj_agent_int_args;
long long stj_agent_pack_workspace_bytes(int dtype);
int stj_agent_pack(const stj_agent_weights* w, void* out, int dtype, hipStream_t stream);
int stj_agent_enc_supported(int n_obs, int n_occ, int Tn, int dtype);
int stj_agent_enc_fwd(const stj_agent_enc_args* a, hipStream_t stream);
int stj_agent_enc_bwd(const stj_agent_enc_args* a, hipStream_t stream);
/* stj_agent_int_fwd / _bwd: the 64-agent interaction block of TrajNet.call (trajNet.py:135-187 with Cross_Attention.call :79-87) per scene in
 * ONE launch per direction: masked concat, segment embedding, the 6-head tfa attention (mask cm (x) cm, dropout on the coefficients), output
 * projection, LayerNorm(1e-3), Dense(1536, elu), Dropout, Dense(384), Dropout, LayerNorm(1e-3), enc + value + embed, obs_norm | occ_norm.
 * Three launches per direction: (scene, head) workgroups for the attention, (scene, hidden chunk) workgroups for the FFN -- their partial
 * sums are written as f32 slabs (ws_v1 [6][B 64][384], ws_u2 [4][..] forward; ws_dn1 [4][..], d_enc [7][..] backward) that the next launch adds
 * in a fixed order (no atomics on activations: bitwise reproducible) -- and a row-wise tail.  stj_agent_enc_bwd takes d_enc with d_enc_f32 = 7.
 * 16-bit dtypes, 64 agents per scene (stj_agent_int_supported); the f32 parity mode keeps the layer-by-layer chain.  Forward writes key
 * [B 64][384] and, when the eleven s_* pointers are given, what backward reads.  Backward writes d_enc and the six dY tensors whose weight
 * gradients are the caller's (X = s_qin / s_concat / s_concat / s_att / s_n1 / s_h), and accumulates seg_embed and the LayerNorm parameters.
 * The slabs ws_v1, ws_u2, ws_dn1 and d_enc need no zeroing: every element is written (plain stores) before the next launch reads it.
 * Alignment: b1 is read as float4 and the four slab workspaces as float4 / float2: 16-byte aligned; bo, g1, be1, b2, g2, be2 and the
 * obs_norm | occ_norm vectors are read one float at a time (4-byte aligned). */
int stj_agent_int_supported(int n_obs, int n_occ, int dtype);
int stj_agent_int_fwd(const stj_agent_int_args* a, hipStream_t stream);
int stj_agent_int_bwd(const stj_agent_int_args* a, hipStream_t stream);
/* Fused FG-MSA offset head (csrc/fgoff_fused.hip): offset = tanh(conv_offset(q)) * (H / 2) with conv_offset = grouped 3x3 conv
 * (8 groups of 48 channels, SAME) -> LayerNorm(eps) -> gelu -> per-group 1x1 conv 48 -> 2 without bias (FG_MSA.py:84-92,109-123), ONE launch
 * per direction instead of stj_im2col3 + stj_gemm + stj_layernorm_fwd + stj_unary_fwd + stj_fg_offset_fwd (and their backward).  One workgroup
 * per 16 or 32 pixels of whole image rows; the conv is an implicit GEMM over an LDS halo tile with the weights streamed as MFMA A fragments from the pack.
 * stj_fgoff_pack: w = conv_offset_0/kernel [3][3][48][384] f32 -> both directions' fragments (stj_fgoff_pack_workspace_bytes(dtype)
 * bytes), once per step.  Training (cols / c / mean / rstd given) also writes the im2col matrix and the saved tensors; the
 * backward writes dq and dc and ADDS the small parameter gradients; the conv kernel's gradient cols^T dc is the caller's GEMM.
 * C = 384, 8 groups; W = 16 (any dtype), W = 8 with even H (any dtype), W = 32 (16-bit dtypes): stj_fgoff_supported. */
typedef struct stj_fgoff_args {
  int B, H, W, dtype;                        /* q is [B][H][W][384]; W = 8 | 16 | 32 (stj_fgoff_supported) */
  float scale, eps;                          /* offset range (H / 2, FG_MSA.py:139) and the LayerNorm epsilon (1e-3) */
  const void* q;                             /* forward input [B][H][W][384], activation dtype */
  const void* pack;                          /* stj_fgoff_pack output */
  const float* bias;                         /* conv_offset_0/bias [384]                 (f32 masters) */
  const float* gamma; const float* beta;     /* conv_norm gamma / beta [384] */
  const void* w1;                            /* conv_offset_proj/kernel [48][2], ACTIVATION dtype */
  void* off;                                 /* [B][8][H W][2]   (forward: out; backward: in) */
  void* cols;                                /* training: im2col of q, [B H W][8][432] (the conv's weight gradient reads it); NULL: not written */
  void* c; float* mean; float* rstd;         /* training: conv output + bias [B H W][384] and its LayerNorm statistics [B H W]; NULL: inference */
  /* backward only */
  const void* doff;                          /* gradient of off [B][8][H W][2] */
  void* dc;                                  /* written: gradient of the conv output [B H W][384] (dW = cols^T dc is the caller's GEMM) */
  void* dq;                                  /* written: gradient of q [B][H][W][384] */
  float* d_w1; float* d_gamma; float* d_beta; float* d_bias;      /* += (atomics): [48][2], [384], [384], [384] f32 */
} stj_fgoff_args;
int stj_fgoff_supported(int H, int W, int C, int G, int dtype);
long long stj_fgoff_pack_workspace_bytes(int dtype);
int stj_fgoff_pack(const float* w, void* out, int dtype, hipStream_t stream);
int stj_fgoff_fwd(const stj_fgoff_args* a, hipStream_t stream);
int stj_fgoff_bwd(const stj_fgoff_args* a, hipStream_t stream);
/* FG-MSA relative-position bias: bilinear `sample` of rpe_table at (query - key - offset) displacements
 * (FG_MSA.py:150-172 via occu_metric.py:345-409 + tfa_image.py:87-173).  off [B,G,H*W,2], table f32 [2H-1,2W-1,G],
 * bias f32 [B,G,HW,HW]; bwd: dtable +=, doff f32 [B,G,HW,2] += (zeroed by the caller: query slices accumulate). */
int stj_fg_bias_fwd(const void* off, const float* table, float* bias, int B, int G, int Hh, int Ww, int dtype, hipStream_t stream);
int stj_fg_bias_bwd(const void* off, const float* table, const void* dbias, float* dtable, float* doff,
                    int B, int G, int Hh, int Ww, int dtype, hipStream_t stream);
/* Fused FG-MSA attention core (FG_MSA.py:138-178; csrc/fgattn.hip): a [B,HW,G*48] = softmax(scale q k^T + sampled bias) v per sample and
 * group, the bias sampled from `table` at the key's offsets as stj_fg_bias_fwd does -- the [B,G,HW,HW] logits / bias / probabilities
 * never reach HBM.  q, k, v [B,HW,G*48], off [B,G,HW,2] (activation dtype), table f32 [2Hh-1,2Ww-1,G]; lse f32 [B,G,HW] (log-sum-exp of
 * each row, the backward's input) or NULL.  Hh = Ww in {8, 16} (any other map: STJ_EUNSUPPORTED); STJ_F32, STJ_BF16 and STJ_F16 all run
 * the fused kernel (f32 with exact-f32 MFMA; its backward takes 16 queries per workgroup on the 16 x 16 map).
 * Backward: dq, dk, dv written (dk / dv through the f32 per-tile partials dkp / dvp, stj_fg_attn_bwd_workspace_bytes() bytes each, which
 * need no zeroing, and a second launch); dtable f32 "+="; doff f32 [B,G,HW,2] is WRITTEN when the backward has a single query tile per
 * (sample, group) -- the 8 x 8 map, every dtype -- and "+=" (zeroed by the caller) otherwise -- the 16 x 16 map: 4 tiles, f32 16. */
int stj_fg_attn_fwd(const void* q, const void* k, const void* v, const void* off, const float* table, void* a, float* lse, int B, int G,
                    int Hh, int Ww, float scale, int dtype, hipStream_t stream);
long long stj_fg_attn_bwd_workspace_bytes(int B, int G, int Hh, int Ww);
int stj_fg_attn_bwd(const void* q, const void* k, const void* v, const void* off, const float* table, const void* a, const float* lse,
                    const void* da, void* dq, void* dk, void* dv, float* dkp, float* dvp, float* dtable, float* doff, int B, int G,
                    int Hh, int Ww, float scale, int dtype, hipStream_t stream);
/* FG-MSA offset head: off[b,g,hw,:] = tanh(o[b,hw,g,:] . W1) * scale (1x1 conv gc -> 2, no bias) and, when fh != NULL,
 * fh = off . W2 + b2 (1x1 conv 2 -> C2) in one launch (FG_MSA.py:136-146).  o [B,HW,G,gc] (the offset conv's own layout, no
 * regrouped copy), W1 [gc,2], W2 [2,C2] (T), b2 f32 [C2] or NULL, off [B,G,HW,2]; fh [B,G,HW,C2], or with zmajor [G,B,HW,C2];
 * qres [B,HW,C2] or NULL is added to every group's fh (zmajor + qres = the decoder query of modules.py:827-831).
 * o == NULL: off is an input and only fh is produced.  HW % 16 == 0, G <= 8.
 * bwd: doff / dfh (either may be NULL) -> dO [B,HW,G,gc] (written), dq [B,HW,C2] (sum of dfh over the groups, written; NULL to
 * skip), dW1 / dW2 / db2 f32 += (db2 may be NULL).  dO == NULL: only the fh half is differentiated and the offset gradient
 * (doff + dfh . W2^T) is written to doff_out [B,G,HW,2]. */
int stj_fg_offset_fwd(const void* o, const void* W1, const void* W2, const float* b2, const void* qres, void* off, void* fh,
                      int B, int HW, int G, int gc, int C2, float scale, int zmajor, int dtype, hipStream_t stream);
int stj_fg_offset_bwd(const void* o, const void* off, const void* W1, const void* W2, const void* doff, const void* dfh,
                      void* dO, void* dq, void* doff_out, float* dW1, float* dW2, float* db2, int B, int HW, int G, int gc,
                      int C2, float scale, int zmajor, int dtype, hipStream_t stream);

/* Decoder: UpSampling3D(1,2,2) nearest + Conv2D 3x3 SAME + bias + ELU (modules.py:746-748,732-735) with the upsample
 * folded into 16 effective 2x2-tap matrices.  prep: W f32 [3,3,Cin,Cout] -> Wf [16,Cout,Cin], Wd [16,Cin,Cout] (T).
 * fwd: X [F,Hi,Wi,Cin] -> Y [F,2Hi,2Wi,Cout].  dgrad: dP (= dY*ELU') -> dX (times ELU'(Xelu) when Xelu != NULL:
 * the layer input is itself an ELU output and its producer skips its own ELU' pass).  wgrad: dWeff f32 [16,Cout,Cin] += (zeroed
 * by the caller), dbias f32 [Cout] += ; fold: dW [3,3,Cin,Cout] += fold(dWeff). */
int stj_upconv_prep(const float* W, void* Wf, void* Wd, int Cin, int Cout, int dtype, hipStream_t stream);
int stj_upconv_fold(const float* dWeff, float* dW, int Cin, int Cout, hipStream_t stream);
int stj_upconv_fwd(const void* X, const void* Wf, const float* bias, void* Y, int F, int Hi, int Wi, int Cin,
                   int Cout, int act, int dtype, hipStream_t stream);
/* Up-conv with the decoder skip sums in the epilogue (modules.py:750-765: x = upconv(x) + skip): Y = ELU(conv + bias) + R1 and, when
 * Y2 / R2 are not NULL, Y2 = Y + R2; every sum rounded to the activation dtype like a separate add.  16-bit dtypes, Cin in {192, 384, ...}
 * (multiple of 32 above 128), Cout multiple of 32; STJ_EUNSUPPORTED otherwise.  Backward of the sums + ELU: stj_elu_res_bwd:
 * g = dy (+ dy2, then g is also written to gsum: the gradient of R1), dpre = g * ELU'(Y - R1) (r == NULL: y is the ELU output itself). */
int stj_upconv_fwd_res(const void* X, const void* Wf, const float* bias, void* Y, const void* R1, void* Y2, const void* R2, int F, int Hi,
                       int Wi, int Cin, int Cout, int dtype, hipStream_t stream);
int stj_elu_res_bwd(const void* dy, const void* dy2, const void* y, const void* r, void* dpre, void* gsum, long long n, int dtype,
                    hipStream_t stream);
/* Backward junction of a decoder level whose skips R1 / R2 are ELU outputs themselves (the time-collapsed Conv3D + ELU of an encoder stage,
 * modules.py:750-765), one pass: g = dy1 (+ dy2, rounded), dpre = g ELU'(y) (y = the up-conv's ELU output), dr1 = g ELU'(r1) and
 * dr2 = dy2 ELU'(r2) -- the gradients of the skips' PRE-activations -- in place of stj_elu_res_bwd + one stj_unary_bwd per skip.
 * dy2 / r2 / dr2 all NULL: a level with one skip. */
int stj_skip_junction_bwd(const void* dy1, const void* dy2, const void* y, const void* r1, const void* r2, void* dpre, void* dr1,
                          void* dr2, long long n, int dtype, hipStream_t stream);
int stj_upconv_dgrad(const void* dP, const void* Wd, void* dX, const void* Xelu, int F, int Hi, int Wi, int Cin, int Cout,
                     int dtype, hipStream_t stream);
/* wg_budget: workgroups the two large weight-gradient launches (>= 64x64 inputs) may occupy.  0 = 128: half the CUs, because in a
 * step whose branches run on concurrent streams these launches are deferred next to chains of short kernels, which then find the
 * other half free (alone the kernel is 1.5x faster on 256).  A host that runs every kernel alone (serial / per-kernel timing) passes
 * 256.  An argument, not library state: the ABI is stateless and re-entrant. */
int stj_upconv_wgrad(const void* X, const void* dP, float* dWeff, float* dbias, int db_parts, int F, int Hi, int Wi, int Cin,
                     int Cout, int wg_budget, int dtype, hipStream_t stream);
/* wgrad: dbias (optional) is f32 [db_parts][Cout], "+=": workgroup i adds its share of the bias gradient into copy i % db_parts
 * and the caller sums the copies (db_parts = 1: plain [Cout]).
 * What tests/test_upconv_wgrad_abi_gpu.py pins down: Cin and Cout are multiples of 8 in the 16-bit types and of 4 in f32, F, Hi and Wi
 * positive, db_parts >= 1 with a dbias, 0 <= wg_budget <= 4096 (STJ_EINVAL otherwise, nothing launched).  X and dP are 16-byte aligned
 * (rows are read as 16-byte pieces; not checked) and are only read, and never outside their own extents.  dWeff is ACCUMULATED, like dbias:
 * the kernels add with f32 atomics to whatever the buffers hold (the caller zeroes dWeff because the fold adds all of it to dW).  The copies
 * of dbias are contiguous, copy i at dbias + i * Cout, and are selected by workgroup index (512-thread kernel: by 2 * index + column
 * parity), so which copy holds what depends on the launch geometry and only the sum over the copies is defined.
 * Kernels: bf16 with Wi % 32 == 0 and Hi % 4 == 0 (128-pixel chunks of 4 rows x 32 columns), or else Wi % 16 == 0 and Hi % 8 == 0 (8 rows x
 * 16 columns), takes the transpose-read kernels: the 512-thread one when there are at least 2048 chunks and Hi % 8 == 0 (Hi % 16 == 0 for
 * the 16-column chunks), the 256-thread one below; channel tile 48 x 96 for Cout <= 48 and Cin <= 96, all 96 couts x 64 cins for Cout == 96
 * and Cin % 64 == 0 (512-thread kernel only), 64 x 64 otherwise.  Every other shape, f32 and fp16 take the generic kernel (row segments of
 * 32 columns, any Hi and Wi) with the 48 x 96 or the 64 x 64 channel tile.  wg_budget is read by the 512-thread kernel alone. */
/* Output heads: Conv2D 3x3 SAME C->2, no activation (modules.py:767-770), written with strides straight into the
 * [B,H,W,32] f32 model output (concat + transpose of modules.py:770,838).  Y element (b,t,y,x,o) at
 * Y + b*y_bstride + t*y_tstride + (y*W+x)*y_pstride + o.  bwd with elu_in != 0: X is an ELU output, dX is multiplied by
 * ELU'(x) (gradient w.r.t. the producing conv's pre-activation; the producer then skips its own ELU' pass). */
int stj_outconv_fwd(const void* X, const float* W, const float* bias, float* Y, int F, int Hh, int Ww, int C, int Tn,
                    long long y_bstride, long long y_tstride, long long y_pstride, int dtype, hipStream_t stream);
/* Both heads in ONE launch (the pair of Conv2D 48->2 of modules.py:767-770 + concat + transpose :838): Y [B,H,W,4*Tn] f32, channel
 * 4 t + 2 head + o; X0 / X1 the two decoder branches [F,H,W,48], frames f = b*Tn + t (t_major = 0) or t*B + b (t_major = 1).  A
 * workgroup runs all 16 (waypoint, head) frames of a spatial tile and writes whole 128-byte output lines.  16-bit dtypes, C = 48,
 * Tn = 8 only (STJ_EUNSUPPORTED otherwise: call stj_outconv_fwd per head). */
int stj_outconv_pair_fwd(const void* X0, const void* X1, const float* W0, const float* W1, const float* bias0, const float* bias1,
                         float* Y, int B, int Tn, int H, int W, int C, int t_major, int dtype, hipStream_t stream);
/* Inference form of the last decoder level + both heads (modules.py:746-748 at 96 -> 48, then :767-770,838) without the [F,H,W,48]
 * tensor between them: out[p][o] = sum_taps z[p + tap][tap, o] with z[q][tap, o] = sum_c Whead[tap][c][o] ELU(upconv)[q][c].
 * stj_upconv_fwd_head: the up-conv of stj_upconv_fwd (same X, Wf, bias) whose epilogue projects every output pixel onto the head kernel
 * Whead f32 [3,3,48,2] and writes Z [F,2Hi,2Wi,20] (18 + 2 zero channels; 24 until round 6) in the activation dtype; stj_outconv_pair_gather: Y [B,H,W,32]
 * f32, channel 4 t + 2 head + o = bias + the 9-neighbour sum of Z0 / Z1 (the two decoder branches; frames as in stj_outconv_pair_fwd).
 * 16-bit dtypes, Cin = 96, Cout = 48, whole 8 x 16 tiles, Tn = 8; STJ_EUNSUPPORTED otherwise. */
int stj_upconv_fwd_head(const void* X, const void* Wf, const float* bias, const float* Whead, void* Z, int F, int Hi, int Wi, int Cin,
                        int Cout, int dtype, hipStream_t stream);
int stj_outconv_pair_gather(const void* Z0, const void* Z1, const float* bias0, const float* bias1, float* Y, int B, int Tn, int H, int W,
                            int t_major, int dtype, hipStream_t stream);
/* Challenge-format quantisation of the model output (inference.py:160-182).  Y [B,H,W,4*Tn] f32 logits, channel 4 t + {obs, occ,
 * flow_x, flow_y}; Q one contiguous block of 4*Tn*H*W bytes per scene: [ obs u8 [Tn,H,W] | occ u8 [Tn,H,W] | flow i8 [Tn,H,W,2] ], so
 * the slice of (scene, waypoint, field) is what the reference's .tobytes() yields for a batch of one.  obs / occ = (uint8)
 * rintf(255 * sigmoid(x)), sigmoid in f32 with the accurate expf and an IEEE division; flow = (int8) clamp(rintf(x), -128, 127); rintf
 * = round-half-to-even = np.round.  A NaN input is written as 0.  Tn = 8, H * W a multiple of 256, 16-byte aligned buffers;
 * STJ_EUNSUPPORTED otherwise.  stj_outconv_pair_gather_q: stj_outconv_pair_gather (same sums, bit for bit) whose epilogue writes Q. */
int stj_quantize_waypoints(const float* Y, uint8_t* Q, int B, int Tn, int H, int W, hipStream_t stream);
int stj_outconv_pair_gather_q(const void* Z0, const void* Z1, const float* bias0, const float* bias1, uint8_t* Q, int B, int Tn, int H,
                              int W, int t_major, int dtype, hipStream_t stream);
/* Q (the layout above) as zlib streams, on the device: one stream per (scene, waypoint, field) plane -- 78 01, one DEFLATE block per
 * segment of 8192 bytes (fixed Huffman code; runs of equal bytes (occupancy) or equal byte pairs (flow) as matches at distance 1 / 2 of up
 * to 258; a segment that would not shrink as a stored block), Adler-32.  The format is stated by compress_reference in
 * strajnet_amd/submission.py.  out: the streams back to back in the order scene, waypoint, (obs, occ, flow); offsets uint32 [B*Tn*3 + 1]:
 * stream s is out[offsets[s] .. offsets[s + 1]).  stj_compress_sizes: the bytes of the caller-owned scratch `work` (not zeroed) and the
 * capacity `out` must have (n + 5 ceil(n / 8192) + 6 per plane of n bytes).  Tn = 8, H * W a multiple of 256, 16-byte aligned buffers,
 * less than 4 GiB of capacity; STJ_EUNSUPPORTED otherwise.  No host synchronisation, no allocation: three launches on `stream`.
 * stj_compress_waypoints_level: level 1 is stj_compress_waypoints, launch for launch; level 2 writes every segment in the shortest of
 * three forms -- stored, the fixed code, or a dynamic Huffman code (BTYPE 10) built for that segment over the same tokens
 * (compress_reference(level=2) states it) -- with another encode kernel in front of the same two; same sizes, workspace and shape
 * limits, never a longer stream than level 1's.  Any other level: STJ_EINVAL. */
int stj_compress_sizes(int B, int Tn, int H, int W, long long* work_bytes, long long* out_capacity);
int stj_compress_waypoints(const uint8_t* Q, void* work, uint8_t* out, uint32_t* offsets, int B, int Tn, int H, int W, hipStream_t stream);
int stj_compress_waypoints_level(const uint8_t* Q, void* work, uint8_t* out, uint32_t* offsets, int B, int Tn, int H, int W, int level,
                                 hipStream_t stream);
/* The same streams inside their protobuf framing (strajnet_amd/csrc/frame.h; frame_reference in strajnet_amd/submission.py): per scene and
 * waypoint `tag_wp varint(Lk)`, then per field `tag varint(l) <stream>` -- a scene's block is the wire form of its repeated Waypoint
 * field as it stands.  tags: the four tag bytes, tag_wp | tag_obs << 8 | tag_occ << 16 | tag_flow << 24.  table uint32
 * [6*B*Tn + B + 1]: stream starts [3*B*Tn] (of the zlib bytes, behind their header), stream lengths [3*B*Tn], scene starts [B + 1]
 * (the last: the total).  stj_compress_framed_sizes: scratch bytes (= stj_compress_sizes'), the capacity of `out` (stj_compress_sizes'
 * + 6 per stream and 6 per waypoint) and the table's words.  Level, shape limits and codes of stj_compress_waypoints_level; the same
 * encode and pack launches with another offsets kernel between them: three launches, no host synchronisation, no allocation. */
int stj_compress_framed_sizes(int B, int Tn, int H, int W, long long* work_bytes, long long* out_capacity, long long* table_words);
int stj_compress_waypoints_framed(const uint8_t* Q, void* work, uint8_t* out, uint32_t* table, int B, int Tn, int H, int W, int level,
                                  uint32_t tags, hipStream_t stream);
int stj_outconv_bwd(const void* X, const float* W, const float* dY, void* dX, float* dW, float* db, int F, int Hh, int Ww,
                    int C, int Tn, long long y_bstride, long long y_tstride, long long y_pstride, int elu_in, void* ws,
                    long long ws_bytes, int dtype, hipStream_t stream);
long long stj_outconv_bwd_workspace_bytes(void);   /* size of the caller-owned scratch `ws` (not zeroed; may be NULL: slower path) */
/* What tests/test_heads_abi_gpu.py pins down for the output heads (statements and dispatch mirrors: tests/_heads_cases.py).
 * Arguments.  stj_outconv_fwd / _bwd: H, W multiples of 16, C of 8, F >= 1, Tn >= 1 and F a multiple of Tn (a frame is split f / Tn,
 * f % Tn), a known dtype, bwd: dW and db not NULL -- STJ_EINVAL otherwise, before any launch; C beyond the generic kernels' LDS (and, bwd,
 * 9 C > 1024; C = 112 is the largest) is STJ_EUNSUPPORTED.  stj_outconv_pair_fwd, stj_outconv_pair_gather(_q): B < 1 or Tn < 1 is
 * STJ_EINVAL; f32, Tn != 8, H or W no multiple of 16, C != 48 (pair), a Y / Q / Z that is not 16-byte aligned are STJ_EUNSUPPORTED.
 * stj_upconv_fwd_head: the argument checks of stj_upconv_fwd, then STJ_EUNSUPPORTED for f32, Cin != 96, Cout != 48, Hi % 8, Wi % 16.  A
 * refused call writes nothing.
 * Kernels.  stj_outconv_fwd: bf16 / fp16 with C = 48, even y_bstride, y_tstride and y_pstride and an 8-byte aligned Y take the MFMA kernel
 * (its stores are float2 at Y + b*y_bstride + t*y_tstride + p*y_pstride), at most 768 workgroups walking the tiles; every other legal call
 * the generic one, a workgroup per tile.  stj_outconv_bwd: the same conditions on dY, bf16 only, and a ws of at least
 * stj_outconv_bwd_workspace_bytes() take the MFMA kernel; fp16, f32, ws == NULL or shorter, an odd stride or a 4-byte aligned dY the
 * generic one (at most 1024 workgroups).  The frame order is read from y_bstride < y_tstride (t-major callers hand Tn = B and the two
 * strides exchanged); any Tn and any whole number of scenes is legal, Tn = 8 with a multiple of 8 spatial tiles is dealt to the XCDs
 * per tile.
 * Semantics.  A head writes the two floats of its own (b, t, pixel) positions and no other byte of Y: the other 30 channels of the
 * interleaved [B,H,W,32] tensor keep what they held.  dW and db are "+=" into what the buffers hold; the contents of ws are irrelevant on
 * entry and undefined afterwards.  Z channels 18 and 19 are written as +0 by stj_upconv_fwd_head and never read by the gather: its Y and
 * Q do not depend on them.  Q of stj_outconv_pair_gather_q equals stj_quantize_waypoints of stj_outconv_pair_gather's Y byte for byte. */
/* PatchEmbed Conv2D k=4 s=4 VALID as im2col (+ f32->T cast, + stride-2 pick of ogm[...,0]; modules.py:430-431,572). */
int stj_im2col_patch(const float* src, void* dst, int B, int H, int W, int Cin, long long pix_stride, int ch_stride,
                     int dtype, hipStream_t stream);
/* Fused PatchEmbed + the stem's sums / norms (modules.py:430-446 PatchEmbed.call: Conv2D k=4 s=4 VALID -> reshape -> LayerNorm(1e-5);
 * modules.py:572-590: patch_embed_vecicle(ogm[...,0]) + patch_embed_map(map) -> all_patch_norm; :576-578 patch_embed_flow -> flow_norm):
 *   pre = cols(src) @ w + bias ; x2 = LN(pre; gamma, beta) [+ add] ; y = gamma2 ? LN(x2; gamma2, beta2) : x2
 * src f32 rasters read as src[((b*H+y)*W+x)*pix_stride + c*ch_stride] (as stj_im2col_patch); w [16*Cin, Cout] type T (Keras kernel
 * [4,4,Cin,Cout] flattened); bias / gamma / beta f32; add, pre, x2, y [B*(H/4)*(W/4), Cout] type T; cols [.., 16*Cin] type T.
 * Optional outputs (NULL = not written): cols (the im2col rows, for dW = cols^T dpre), pre + mean + rstd, x2 + mean2 + rstd2 (what
 * stj_layernorm_bwd needs).  pre and x2 are rounded to T before they are normalised.  Built for Cin in {11, 3, 2}, Cout = 96. */
int stj_patch_embed_supported(int Cin, int Cout, int dtype);
int stj_patch_embed_fwd(const float* src, const void* w, const float* bias, const float* gamma, const float* beta, const void* add,
                        const float* gamma2, const float* beta2, void* cols, void* pre, void* x2, void* y, float* mean, float* rstd,
                        float* mean2, float* rstd2, int B, int H, int W, int Cin, long long pix_stride, int ch_stride, int Cout,
                        float eps, int dtype, hipStream_t stream);
/* grouped 3x3 SAME conv of FG-MSA (FG_MSA.py:51) as im2col / col2im around the batched GEMM. */
int stj_im2col3(const void* x, void* cols, int N, int H, int W, int G, int Cg, int dtype, hipStream_t stream);
int stj_col2im3(const void* dcols, void* dx, int N, int H, int W, int G, int Cg, int dtype, hipStream_t stream);

/* OGMFlow_loss (loss.py:50-170 with train.py:195-196 flags).  All tensors f32: logits [B,H,W,32] (channel 4k+{0,1,2,3},
 * train.py:105-123), gt_obs/gt_occ/origin [B,8,H,W,1], gt_flow [B,8,H,W,2].
 * auc_gate: res_k = [Keras PR-AUC(true_all, warp(origin, id+gt_flow)*true_all) > 0] (loss.py:127-137); hist int[8*202] scratch, zero on entry.
 * fwd: sums f32[32*40] scratch (32 copies of the 40 accumulators the workgroups spread their atomics over; zero on entry), loss f32[5] = observed_xe, occluded_xe, flow, flow_warp_xe, their sum (train.py:221); coef f32[32] for bwd.
 * bwd: dlogits = sum_j upstream[j] * dloss_j/dlogits; with flag bit 3 (bwd only) upstream is ONE value for all four terms.
 * flags: bit 0 = flow-warp term on (not no_use_warp), bit 1 = use_focal_loss (tfa SigmoidFocalCrossEntropy added to the three
 * occupancy terms, loss.py:183-190,212-219,244-245), bit 2 = use_pred (loss.py:151-154,253-268); the same value goes to fwd and bwd. */
int stj_loss_auc_gate(const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                      int* hist, float* gate, float* auc_out, int B, int H, int W, hipStream_t stream);
int stj_loss_fwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                 const float* gate, float* sums, float* loss, float* coef, int B, int H, int W, float ogm_w, float occ_w,
                 float flow_origin_w, float replica, int flags, hipStream_t stream);
int stj_loss_bwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                 const float* coef, const float* upstream, float* dlogits, int B, int H, int W, int flags, hipStream_t stream);
/* The same two passes as ONE (round 6): every backward coefficient of loss.py:161-170 under train.py:221-223 (unit gradient on the sum of
 * the four terms) depends on the ground truth alone -- weights, pixel count, the AUC gate, the per-waypoint count of pixels with a
 * non-zero true flow (loss.py:279-291) -- so
 * coef:    coef f32[32] = what stj_loss_fwd would write, from gt_flow and the gate (cnt int[8] scratch, zero on entry);
 * fwd_bwd: loss f32[5], coef_out f32[32] as stj_loss_fwd, AND dlogits as stj_loss_bwd with upstream == 1 (flag bit 3), on one read of
 *          the logits and the ground truth; coef_in = coef's output; sums f32[128*40] scratch, zero on entry.  loss == NULL: the pass
 *          alone; stj_loss_finalize (any stream behind it) then writes loss and coef_out from sums. */
int stj_loss_coef(const float* gt_flow, const float* gate, int* cnt, float* coef, int B, int H, int W, float ogm_w, float occ_w,
                  float flow_origin_w, float replica, int flags, hipStream_t stream);
int stj_loss_finalize(const float* sums, const float* gate, float* loss, float* coef_out, int B, int H, int W, float ogm_w,
                      float occ_w, float flow_origin_w, float replica, int flags, hipStream_t stream);
/* auc_gate + coef on one pass over the ground truth: hist int[8*202 + 8] scratch (zero on entry; the last 8 collect the flow counts) */
int stj_loss_gate_coef(const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin, int* hist, float* gate,
                       float* auc_out, float* coef, int B, int H, int W, float ogm_w, float occ_w, float flow_origin_w,
                       float replica, int flags, hipStream_t stream);
int stj_loss_fwd_bwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                     const float* gate, const float* coef_in, float* sums, float* loss, float* coef_out, float* dlogits,
                     int B, int H, int W, float ogm_w, float occ_w, float flow_origin_w, float replica, int flags, hipStream_t stream);

/* TFRecord feature decode (train.py:87-103, inference.py:84-96 _parse_image_function: tf.io.decode_raw + reshape + centre crop
 * + cast).  src: the raw feature bytes of a batch, [n_outer][H][W][C] elements of kind 0 bool/uint8 (v != 0), 1 int8,
 * 2 float32, 3 float64; dst f32 [n_outer][Ho][Wo][C] = scale * src[:, y0:y0+Ho, x0:x0+Wo, :]. */
int stj_decode_raw(const void* src, int kind, float* dst, long long n_outer, int H, int W, int C, int y0, int x0, int Ho,
                   int Wo, float scale, hipStream_t stream);

/* Packed record features expanded on the device (csrc/unpack.hip; the format is stated by pack_bits / pack_sparse / unpack_reference in
 * strajnet_amd/data.py).  A scene's decoded array (after the reshape and centre crop, before the cast) is flattened to n elements.
 * stj_unpack_bits: element i is bit i & 7 of byte i >> 3; dst f32 [n_total] = 1.0f / 0.0f (scenes back to back: n_total = B n).
 * stj_unpack_sparse: per scene mask uint32 [n / 32] (same bit order), offs uint32 [ceil(n / 8192) + 1] (exclusive prefix of the present
 * counts per block of 8192 elements, relative to the scene), and its present 32-bit words in element order; val_base uint32 [B + 1] the
 * scenes' prefix into vals [n_vals].  dst f32 [B][n]: the present words unchanged (-0.0, NaN payloads, denormals), +0.0f elsewhere.
 * Gather indices are clamped to n_vals - 1, so a malformed stream reads nothing outside its buffers.  n a multiple of 32, fewer than
 * 2^32 elements and values, 4-byte aligned streams, 16-byte aligned dst; STJ_EUNSUPPORTED otherwise, STJ_OK for zero sizes.  No host
 * synchronisation, no allocation, no atomics: one launch each on `stream`. */
int stj_unpack_bits(const uint32_t* bits, float* dst, long long n_total, hipStream_t stream);
int stj_unpack_sparse(const uint32_t* mask, const uint32_t* offs, const uint32_t* val_base, const float* vals, long long n_vals,
                      float* dst, int B, long long n, hipStream_t stream);

/* Batches gathered from a pool of N packed scenes that stays on the device (csrc/pool.hip; the format is stated by PoolLayout.reference_gather
 * in strajnet_amd/data.py).  idx: int32 [B] ON THE DEVICE, read by the kernel; scene b of dst (f32 [B][n]) is pool scene
 * clamp(idx[b], 0, N - 1), so no index value reads outside the pool.
 * stj_gather_bits: pool uint32 [N][n / 32]; the scene as stj_unpack_bits expands it.
 * stj_gather_sparse: mask uint32 [N][n / 32], offs uint32 [N][ceil(n / 8192) + 1] (relative to the scene), val_base int64 [N + 1] (a pool's
 * value words can pass 2^32), vals [n_vals]; the scene as stj_unpack_sparse expands it.  Gather indices are clamped to n_vals - 1; nothing is
 * gathered when n_vals == 0.
 * stj_gather_raw: pool [N][n] elements of `kind` as in stj_decode_raw; dst[b][i] = scale * cast(pool[idx[b]][i]), the bits of stj_decode_raw
 * without a crop.  Any n >= 0, pool aligned to its element size.
 * STJ_EUNSUPPORTED: n % 32 != 0 (bits, sparse), n >= 2^32, N < 1 with B > 0, misaligned pointers (4-byte streams and idx, 8-byte val_base,
 * 16-byte dst), more workgroups than a launch takes; STJ_OK with nothing launched for B == 0.  One launch each on `stream`: no host
 * synchronisation, no allocation, no atomics. */
int stj_gather_bits(const uint32_t* pool, const int* idx, int N, float* dst, int B, long long n, hipStream_t stream);
int stj_gather_sparse(const uint32_t* mask, const uint32_t* offs, const long long* val_base, const float* vals, long long n_vals,
                      const int* idx, int N, float* dst, int B, long long n, hipStream_t stream);
int stj_gather_raw(const void* pool, int kind, const int* idx, int N, float* dst, int B, long long n, float scale, hipStream_t stream);

/* Raw record bytes packed on the device into the slots of such a pool (csrc/pack.hip; the semantics are stated by
 * PoolLayout.replace_reference in strajnet_amd/data.py).  src: the record's own bytes of B scenes, [B][T][H][W][C] elements; decoded element i
 * of a scene (n = T Ho Wo C of them) is source element (t, y0 + y, x0 + x, c) as in stj_decode_raw, uncropped T = H = C = 1, W = n.  slots:
 * int32 [B] ON THE DEVICE, scene b goes to pool slot slots[b]; ok: int32 [B] on the device, 1 = the scene lands.  A scene with ok[b] == 0
 * or a slot outside [0, N) is skipped by every entry point (never clamped); duplicate slots are the caller's error (the result is
 * unspecified, every access stays inside the pool arrays).
 * stj_pack_bits: src bool bytes (non-zero = set) -> pool_words uint32 [N][n / 32] in pack_bits' order.
 * stj_pack_sparse_count: src float32 words, present iff the 32-bit pattern is non-zero -> offs_stage uint32 [B][ceil(n / 8192) + 1], the
 * present words of every block of 8192 elements.
 * stj_pool_admit (one launch per sparse key, between its count and the commits): offs_stage[b][0 .. nblk] becomes the exclusive prefix with the
 * total at [nblk], in place; ok[b] = (first ? 0 <= slots[b] < N : ok[b]) && total <= val_base[s + 1] - val_base[s].  offs_stage NULL: the
 * range check alone (a pool without a sparse key).
 * stj_pack_sparse_commit: the slot's mask words uint32 [N][n / 32], its offs row [N][nblk + 1] (copied from offs_stage) and the present words
 * at vals[val_base[s] + offs_stage[b][blk] + rank] in element order (-0.0, NaN payloads and denormals unchanged).  Index arithmetic into
 * vals is 64-bit and every store is inside [val_base[s], min(val_base[s + 1], n_vals)), whatever offs_stage and val_base hold.
 * stj_pool_put_raw: rows of n elements of `itemsize` (1, 4 or 8) bytes, src [B][n] -> pool [N][n]; any n >= 0, no crop.
 * STJ_EUNSUPPORTED: n % 32 != 0 (bits, sparse), n >= 2^32, misaligned pointers (4-byte streams, slots and ok, 8-byte val_base, src / pool of
 * stj_pool_put_raw to the element size), more workgroups than a launch takes; STJ_EINVAL: NULL, negative sizes, a crop outside the source;
 * STJ_OK with nothing launched for B == 0.  One launch each on `stream`: no host synchronisation, no allocation, no atomics. */
int stj_pack_bits(const uint8_t* src, const int* ok, const int* slots, int N, uint32_t* pool_words, int B, int T, int H, int W, int C, int y0,
                  int x0, int Ho, int Wo, hipStream_t stream);
int stj_pack_sparse_count(const float* src, uint32_t* offs_stage, int B, int T, int H, int W, int C, int y0, int x0, int Ho, int Wo,
                          hipStream_t stream);
int stj_pool_admit(uint32_t* offs_stage, int nblk, const long long* val_base, const int* slots, int N, int* ok, int B, int first,
                   hipStream_t stream);
int stj_pack_sparse_commit(const float* src, const uint32_t* offs_stage, const int* ok, const int* slots, int N, uint32_t* mask_pool,
                           uint32_t* offs_pool, const long long* val_base, float* vals, long long n_vals, int B, int T, int H, int W, int C,
                           int y0, int x0, int Ho, int Wo, hipStream_t stream);
int stj_pool_put_raw(const void* src, int itemsize, const int* ok, const int* slots, int N, void* pool, int B, long long n, hipStream_t stream);

/* A shuffle window over such a pool (csrc/window.hip; the semantics are stated by ShuffleWindow.reference and
 * PoolLayout.replace_packed_reference in strajnet_amd/data.py).
 * stj_pool_draw: perm int32 [N] and idx int32 [B] ON THE DEVICE, u uint32 [B] random words on the device.  The live slots are
 * perm[tail : tail + n_live) (circular mod N); for i = 0 .. B - 1: j = (u[i] * (n_live - i)) >> 32, swap perm[(tail + i) % N] and
 * perm[(tail + i + j) % N], idx[i] = perm[(tail + i) % N] clamped to [0, N - 1].  One workgroup, one lane.  STJ_EINVAL with nothing launched
 * for n_live < B, B < 0, N < 1 or tail outside [0, N); STJ_OK with nothing launched for B == 0.
 * stj_pool_admit_packed (one launch per sparse key, all of them before any put): offs_src uint32 [B][nblk + 1], the scene-relative offs rows
 * as pack_sparse writes them, nblk = ceil(n / 8192); src_base int64 [B + 1] the scenes' first words in the staged values.
 * ok[b] = (first ? 0 <= slots[b] < N : ok[b]) && offs_src[b][0] == 0 && the row does not decrease && no block holds more present words than
 * elements && total == src_base[b + 1] - src_base[b] && total <= val_base[s + 1] - val_base[s], total = offs_src[b][nblk].
 * stj_pool_put_vals: scene b's words vals_src[src_base[b] .. src_base[b + 1]) -> vals[val_base[s] ..), s = slots[b]; 64-bit indices, every
 * store inside [val_base[s], min(val_base[s + 1], n_vals)) whatever src_base and val_base hold; vals_src is read inside
 * [src_base[b], src_base[b + 1]) only.  A scene with ok[b] == 0 or a slot outside [0, N) is skipped, never clamped.  The fixed-length rows
 * of a packed record (bits words, mask and offs rows as itemsize 4, raw rows) go through stj_pool_put_raw.
 * STJ_EUNSUPPORTED: misaligned pointers (4-byte words, slots, ok, perm, idx; 8-byte src_base / val_base), n % 32 != 0, n >= 2^32, nblk not
 * ceil(n / 8192), more workgroups than a launch takes; STJ_EINVAL: NULL, negative sizes.  One launch each on `stream`: no host
 * synchronisation, no allocation, no atomics. */
int stj_pool_draw(int* perm, int N, int tail, int n_live, const uint32_t* u, int* idx, int B, hipStream_t stream);
int stj_pool_admit_packed(const uint32_t* offs_src, int nblk, long long n, const long long* src_base, const long long* val_base,
                          const int* slots, int N, int* ok, int B, int first, hipStream_t stream);
int stj_pool_put_vals(const uint32_t* vals_src, const long long* src_base, const int* ok, const int* slots, int N,
                      const long long* val_base, uint32_t* vals, long long n_vals, int B, hipStream_t stream);

/* trajNet input plumbing (trajNet.py:125-140), one launch: obs [B,n_obs,Tn,8] and occ [B,n_occ,Tn,8] (f32, 16-byte aligned) ->
 * x5 [B*A*Tn,5] node features, v3 [B*A,3] vector features of step 0, vt [B*A,Tn] int32 step-valid (feature 0 != 0), cmi [B*A] int32 /
 * cmf [B*A] (type T) agent-valid (any step valid); A = n_obs + n_occ, obs rows first. */
int stj_agent_prep(const float* obs, const float* occ, int n_obs, int n_occ, int B, int Tn, void* x5, void* v3, int* vt, int* cmi,
                   void* cmf, int dtype, hipStream_t stream);
/* trajNet branch sums (trajNet.py:166-171), enc / value / concat / qin / out [B,A,C], embed [A,C], cm [B,A], all type T:
 * mix: concat = enc * cm, qin = concat + embed;  bwd: denc = (dconcat + dqin) * cm, dembed = sum_b dqin (either gradient may be NULL).
 * sum: out = enc + value + embed;                bwd: dembed = sum_b dout (the gradients of enc and value are dout itself). */
int stj_agent_mix_fwd(const void* enc, const void* embed, const void* cm, void* concat, void* qin, int B, int A, int C, int dtype,
                      hipStream_t stream);
int stj_agent_mix_bwd(const void* dconcat, const void* dqin, const void* cm, void* denc, void* dembed, int B, int A, int C, int dtype,
                      hipStream_t stream);
int stj_agent_sum_fwd(const void* enc, const void* value, const void* embed, void* out, int B, int A, int C, int dtype, hipStream_t stream);
int stj_agent_sum_bwd(const void* dout, void* dembed, int B, int A, int C, int dtype, hipStream_t stream);
/* The tail of TrajNet.call in one launch per direction (trajNet.py:171-187): out = enc + value + embed (rounded like stj_agent_sum_fwd), then
 * LayerNorm(eps) with parameters (g0, b0) on the first n0 agents of every scene (obs_norm) and (g1, b1) on the others (occ_norm): y [B,A,C].
 * Saves out [B,A,C], mean / rstd f32 [B*A].  Backward: dout [B,A,C] (= d_enc = d_value), dembed [A,C] = sum over scenes of dout (written);
 * dg0 / db0 / dg1 / db1 f32 "+=".  C = 384. */
int stj_agent_out_fwd(const void* enc, const void* value, const void* embed, const float* g0, const float* b0, const float* g1, const float* b1,
                      void* out, void* y, float* mean, float* rstd, int B, int A, int n0, int C, float eps, int dtype, hipStream_t stream);
int stj_agent_out_bwd(const void* dy, const void* out, const float* mean, const float* rstd, const float* g0, const float* g1, void* dout,
                      void* dembed, float* dg0, float* db0, float* dg1, float* db1, int B, int A, int n0, int C, int dtype, hipStream_t stream);
/* Time-kernel collapse of the decoder's Conv3D(8,1,1) SAME skips (modules.py:693-698,709-716,750-765): the
 * input is the same frame at all 8 steps, so step t needs W_t = sum_{j=max(0,3-t)}^{min(7,10-t)} W[j].  W f32 [8][n] (n = Cin*Cout),
 * Wz T [8][n].  fold (backward): dW[j] += sum over the t whose window contains j of dWz[t]. */
int stj_time_collapse(const float* W, void* Wz, long long n, int dtype, hipStream_t stream);
int stj_time_fold(const float* dWz, float* dW, long long n, hipStream_t stream);
/* g[idx[i]] += parts[i]; parts[i] = 0 for i < n: the partial-gradient copies some backward kernels rotate their atomics over
 * (LayerNorm gamma / beta, bias tables, conv biases) folded into the flat gradient buffer and re-zeroed, one launch. */
int stj_fold_parts(float* g, const long long* idx, float* parts, long long n, hipStream_t stream);

/* Host-side CRC-32C (Castagnoli) for the two TensorFlow file formats on either side of the hot path: TFRecord framing
 * (train.py:75-78) and the checkpoint bundle written / read by save_weights / load_weights (train.py:358,366,372;
 * inference.py:283).  *crc is the running, unmasked CRC: 0 before the first chunk, the checksum after the last.  Runs on the
 * calling thread; touches no device state. */
int stj_crc32c(const void* data, long long n, unsigned int* crc);

/* Evaluation metrics (occu_metric.py:26-140, evaluated every train / validation step: train.py:243-249,280-282): observed and
 * occluded PR-AUC + soft IoU, flow EPE, flow-warped occupancy AUC + IoU, means over the 8 waypoints.  pred [B,H,W,32]
 * (channel 4k+{obs,occ,flow_x,flow_y}); pred_is_logits: sigmoid is applied to the occupancy channels (train.py:142-154).
 * hist int[8*3*202] and sums f32[8*11] MUST BE ZERO on entry; auc f32[24] scratch; out f32[7] in the order of the proto
 * fields at occu_metric.py:130-139. */
int stj_metrics(const float* pred, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                int* hist, float* sums, float* auc, float* out, int B, int H, int W, int pred_is_logits, int use_warp,
                hipStream_t stream);

/* The validation step (train.py:252-282) behind the model: OGMFlow_loss AND the metrics above from ONE pass over the logits [B,H,W,32]
 * (f32) and the ground truth [B,8,H,W,{1,1,2,1}], instead of stj_loss_auc_gate + stj_loss_fwd + stj_metrics (three passes).
 * loss f32[5] = observed_xe, occluded_xe, flow, flow_warp_xe, their sum (as stj_loss_fwd); metrics f32[7] (as stj_metrics with
 * pred_is_logits); gate f32[8] and auc f32[8*4] ([k][gate's, observed, occluded, flow-warped]) optional (NULL).
 * flags: bits 0-2 as stj_loss_fwd (flow-warp term on, use_focal_loss, use_pred), bit 3 = use_gt (off: every gate 1 and the gate's
 * AUC 0), bit 4 = the metrics' no_warp (metrics[5], [6] = 0).
 * workspace: stj_eval_workspace_bytes(B, H, W) bytes, 16-byte aligned, ANY contents on entry (the entry clears what it needs on
 * `stream`; nothing is read back from an earlier call).
 * running: optional double[12] = count, the four losses x loss_scale (train.py:275-278 `* REPLICA`), the seven metrics: this
 * call's values are ADDED and the count incremented (Keras Mean.update_state) by the launch that writes loss and metrics.
 * No floating-point atomics: two calls on the same inputs give the same bits.  B*H*W <= 0: nothing is launched or written. */
long long stj_eval_workspace_bytes(int B, int H, int W);
int stj_eval_fwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                 void* workspace, float* loss, float* metrics, float* gate, float* auc, double* running, int B, int H, int W,
                 float ogm_w, float occ_w, float flow_origin_w, float replica, float loss_scale, int flags, hipStream_t stream);

/* Every scene of a validation batch scored ON ITS OWN, from one pass over the same inputs as stj_eval_fwd (same flags, weights and
 * replica); stj_eval_fwd itself is unchanged.  Nothing is pooled across scenes and there is no floating-point atomic.
 * rows f32[B][12]: per scene observed_xe, occluded_xe, flow, flow_warp_xe, their sum, then the seven metrics -- what OGMFlow_loss and
 * the metrics give for that scene as a batch of one.  A row depends on its scene alone: the same scene gives the same bits alone, in a
 * batch of any size and at any position (stj_eval_scenes_grid(H, W) workgroups per scene, a function of the shape only; partial sums
 * added in a fixed order).  A scene without vehicle occupancy has every gate 0 under use_gt: its flow, flow_warp_xe and sum are NaN (the
 * reference divides 0 by 0, loss.py:164,167), the other columns finite.  gate f32[B][8] and auc f32[B][8][4] per scene, optional.
 * live: optional device int32[B] (NULL: every scene is live).  A scene with live[b] == 0 is not scored, none of its inputs is read;
 * its row, gate and auc are written as zeros and it enters neither state, table nor the pooled result.
 * batch_loss f32[5], batch_metrics f32[7], batch_gate f32[8], batch_auc f32[32]: optional, the POOLED result of the live scenes =
 * what stj_eval_fwd computes for the sub-batch of the live scenes: gate and auc equal to it (the pooled histograms are the integer
 * sums of the scenes'), the float sums folded in double scene by scene, so loss and metrics differ from it in summation order only.
 * Without a live scene all four are written as zeros.
 * state: optional device double[2][13], added to by the last launch, live scenes in batch order: [0][c] the sum and [1][c] the count
 * of column c of the rows (the five loss columns x loss_scale); a NON-FINITE value is added to neither (unlike Keras Mean: one empty
 * scene must not turn an epoch's mean into NaN); [0][12] = scenes scored, [1][12] = scenes with at least one non-finite column.
 * table f32[capacity][12] with cursor (device long long[1]): live rows are appended in batch order at *cursor, which advances by the
 * number of live scenes even when the table is full; rows at or beyond capacity are dropped, nothing is stored outside the table.
 * A cursor without a table only counts.
 * workspace: stj_eval_scenes_workspace_bytes(B, H, W) bytes, 16-byte aligned, ANY contents on entry.  Five launches on `stream` (four
 * without state, cursor and pooled outputs), no allocation, no host synchronisation.  STJ_EINVAL before any launch, nothing written:
 * logits not 16-byte, gt_flow / state / cursor not 8-byte, workspace not 16-byte aligned; unknown flag bits; capacity < 0; a table
 * without a cursor; B > 65534.  B*H*W <= 0: nothing is launched or written. */
long long stj_eval_scenes_workspace_bytes(int B, int H, int W);
int stj_eval_scenes_grid(int H, int W);
int stj_eval_scenes_fwd(const float* logits, const float* gt_obs, const float* gt_occ, const float* gt_flow, const float* origin,
                        const int* live, void* workspace, float* rows, float* gate, float* auc, float* batch_loss, float* batch_metrics,
                        float* batch_gate, float* batch_auc, double* state, float* table, long long* cursor, long long capacity,
                        int B, int H, int W, float ogm_w, float occ_w, float flow_origin_w, float replica, float loss_scale,
                        int flags, hipStream_t stream);

/* Training-time randomness.  Keras Dropout / tfa-MHA attention dropout (trajNet.py:33,71,75,77,195,209,211) and DropPath
 * (modules.py:137-151) share one rule: y = [res +] keep(draw) * x / (1 - p), keep = U[0,1) >= p, draw(i) = i / inner
 * (inner = 1: per element; inner = elements per sample: DropPath with p = drop_prob).  U comes from Philox-4x32-10 keyed by
 * state = device int64[2] {seed, step} and `site`; backward calls stj_dropout on dY with the same (state, site).
 * stj_dropout_mask writes the keep bytes of the first ndraw draws (test hook: the oracle is fed the same masks). */
int stj_rng_advance(long long* state, hipStream_t stream);
/* stj_rng_advance that also writes the advanced {seed, step} to snap[2] (one launch instead of the advance + a device copy). */
int stj_rng_advance_snap(long long* state, long long* snap, hipStream_t stream);
int stj_dropout(const void* x, const void* res, void* y, long long n, long long inner, float p, const long long* state,
                int site, int dtype, hipStream_t stream);
int stj_dropout_mask(unsigned char* mask, long long ndraw, float p, const long long* state, int site, hipStream_t stream);
/* Keras Nadam (train.py:197,224) over flat f32 buffers: one fused pass.  Host-side scalars:
 * cg = (1-mu_t)/(1-prod_t), cm = mu_{t+1}/(1-prod_{t+1}), vhat_scale = 1/(1-b2^t); g is multiplied by gscale first. */
int stj_nadam_step(float* w, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps,
                   float cg, float cm, float vhat_scale, float gscale, hipStream_t stream);

/* The same Nadam step with its scalar state ON THE DEVICE (train.py:199-230 as one captured graph: by-value coefficients would freeze
 * at capture time).  Three launches ordered by kernel boundaries alone -- no flag, ticket or spin between workgroups:
 *   stj_gradnorm_partials   partials[b] = sum of (double)g[i]^2 over workgroup b's grid-stride share, b < STJ_GRADNORM_PARTS.  The grid
 *                           is fixed, every slot is stored by every call (0.0 where a workgroup has no element) and the fold order is
 *                           fixed: the same g gives the same bits.  The sum of the slots is non-finite exactly when some g is NaN or
 *                           +-inf (no term is negative; FLT_MAX^2 is a finite double).
 *   stj_nadam_prepare       one workgroup, all in double: folds the partials (sumsq), norm = gscale * sqrt(sumsq), decides whether the
 *                           step is skipped, evaluates the learning-rate schedule at `iterations` (0-based: the first update uses
 *                           schedule(0)), advances the Keras recurrences with t = iterations + 1
 *                             mu_t = b1 (1 - 0.5 0.96^(0.004 t)) ; prod_t = m_schedule mu_t ; prod_{t+1} = prod_t mu_{t+1}
 *                             cg = (1 - mu_t) / (1 - prod_t) ; cm = mu_{t+1} / (1 - prod_{t+1}) ; vhat_scale = 1 / (1 - b2^t)
 *                             m_schedule <- prod_t ; iterations <- t
 *                           (b1, b2: the f32 values passed, the ones the element update multiplies by) and writes coef.
 *                           clipnorm > 0 (tf.clip_by_global_norm): coef.gscale = gscale * clipnorm / max(norm, clipnorm), which IS
 *                           gscale when norm <= clipnorm.  flags bit 0 (STJ_NADAM_SKIP_NONFINITE): a non-finite sumsq makes
 *                           coef.apply = 0, skipped += 1 and leaves iterations, m_schedule and state[4] as they were (without the flag the
 *                           non-finite gradient propagates, as in Keras).  partials == NULL: no norm, no clip, no skip.
 *                           losses (f32[4]) and running go together (both or neither): running[0] += 1, running[1 + i] +=
 *                           losses[i] * loss_scale, on EVERY call, skipped or not (train.py:226-229 updates its means unconditionally).
 *   stj_nadam_apply         stj_nadam_step's element update (csrc/nadam.h) with lr, cg, cm, vhat_scale, gscale read from coef; when
 *                           coef.apply == 0 no thread reads or writes w, g, m or v.
 * Device buffers (doubles 8-byte aligned; g, w, m, v and coef 16-byte aligned):
 *   state   double[8]  [0] iterations (updates applied, 0 at start); [1] m_schedule (product of mu_1..mu_t, 1.0 at start); [2] skipped-
 *                      step count; [3] last gradient norm (after gscale, before clipping; 0 when not computed); [4] lr of the last
 *                      applied step; the rest 0
 *   sched   double[8]  [0] kind (enum stj_optim); STJ_SCHED_CONSTANT {lr}; STJ_SCHED_COSINE_RESTARTS {lr0, first_decay_steps, t_mul,
 *                      m_mul, alpha} (lr_schedule.py:37-76); STJ_SCHED_CUSTOM {d_model, warmup_steps} (lr_schedule.py:13-17), from [1] on
 *   coef    float[8]   lr, cg, cm, vhat_scale, gscale, apply (1 or 0), rest 0
 *   running double[5]  count, then the sums of the four loss terms x loss_scale
 * n < 0, a null or misaligned buffer, unknown flag bits: STJ_EINVAL, nothing launched.  n == 0: stj_gradnorm_partials still stores
 * its zeros, stj_nadam_apply launches nothing. */
enum stj_optim { STJ_GRADNORM_PARTS = 256, STJ_SCHED_CONSTANT = 0, STJ_SCHED_COSINE_RESTARTS = 1, STJ_SCHED_CUSTOM = 2,
                 STJ_NADAM_SKIP_NONFINITE = 1, STJ_TENSOR_CHUNK = 4096, STJ_TENSOR_GRID = 1024 };
int stj_gradnorm_partials(const float* g, long long n, double* partials, hipStream_t stream);
int stj_nadam_prepare(double* state, const double* sched, const double* partials, float* coef, const float* losses, double* running,
                      float b1, float b2, float gscale, float clipnorm, float loss_scale, int flags, hipStream_t stream);
int stj_nadam_apply(float* w, const float* g, float* m, float* v, long long n, const float* coef, float b1, float b2, float eps,
                    hipStream_t stream);

/* The device-state Nadam step over a TABLE OF TENSORS (csrc/tensorstats.hip): the flat buffers of n floats hold S >= 1 tensors, tensor s
 * owning [start_s, start_s + len_s) (len_s >= 1, start_0 = 0, start_s % 4 == 0, ascending, disjoint); [start_s + len_s, start_{s+1})
 * (start_S = n) is its slot's padding, counted in no statistic and updated with tensor s's multiplier.  The host cuts every slot into
 * chunks of at most STJ_TENSOR_CHUNK elements that never straddle a tensor (strajnet_amd/optim.py: chunk_table) and uploads
 *   chunks  int[n_chunks][4]  {start / 4, n_stat, n_apply, tensor}: the chunk's first element, how many elements from there are the
 *                             tensor's own (0 <= n_stat <= n_apply), how many belong to the slot (<= STJ_TENSOR_CHUNK), the tensor's
 *                             index; tensor-major, ascending.  16-byte aligned.  A record that fails these bounds, or reaches past n,
 *                             is treated as empty.
 *   chunk0  int[S + 1]        tensor s's chunks are [chunk0[s], chunk0[s + 1]).
 * Same rules as above: no floating-point atomics, every partial stored, f64 accumulation, grids (min(n_chunks, STJ_TENSOR_GRID)
 * workgroups striding over the chunks) and fold orders that are functions of the table alone, launches only.
 *   stj_tensor_partials        gpart[c] = sum of (double)g[i]^2 over chunk c's n_stat elements.
 *   stj_nadam_prepare_tensors  one workgroup folds every tensor's chunk partials: a tensor of one chunk takes the partial as it is
 *                              (one lane each); a tensor of more is folded by a wave (lane l adds chunk0[s] + l, + 64, ... in that
 *                              order, then the wave's xor tree).  tsum[s] = the sum of g^2, gnorm_s = gscale sqrt(tsum[s]).  The
 *                              total of tsum (thread-strided in index order, then the workgroup's tree) goes through the scalar step
 *                              of stj_nadam_prepare: the same coef, state[0..4] and running for the same total, global_clipnorm and
 *                              STJ_NADAM_SKIP_NONFINITE included.  Besides:
 *                                mult[s]     clipnorm > 0 (Keras clipnorm, tf.clip_by_norm per variable):
 *                                            (float)(gscale * clipnorm / max(gnorm_s, clipnorm)), which IS gscale when gnorm_s <=
 *                                            clipnorm; else coef.gscale.  global_clipnorm and clipnorm together: STJ_EUNSUPPORTED
 *                                state[5]    the lowest s whose tsum is non-finite (it holds a NaN or an infinity), -1 for none;
 *                                state[6]    how many tensors are; nfcount[s] += 1 for each; state[7] (calls) += 1
 *   stj_nadam_apply_tensors    stj_nadam_apply per chunk with gscale = mult[tensor].  coef.apply == 0: nothing is read or written.
 * S < 1, n_chunks < 1 (S tensors have at least S chunks), n < 0, a null or misaligned buffer, unknown flag bits, n / 4 >= 2^31:
 * STJ_EINVAL, nothing launched. */
int stj_tensor_partials(const float* g, long long n, const int* chunks, int n_chunks, int S, double* gpart, hipStream_t stream);
int stj_nadam_prepare_tensors(double* state, const double* sched, const double* gpart, const int* chunk0, int n_chunks, int S, float* coef,
                              float* mult, double* tsum, int* nfcount, const float* losses, double* running, float b1, float b2,
                              float gscale, float global_clipnorm, float clipnorm, float loss_scale, int flags, hipStream_t stream);
int stj_nadam_apply_tensors(float* w, const float* g, float* m, float* v, long long n, const int* chunks, int n_chunks, int S,
                            const float* coef, const float* mult, float b1, float b2, float eps, hipStream_t stream);

/* The model's inputs from agent tracks (csrc/raster.hip; rules: csrc/raster.h; semantics in NumPy: strajnet_amd/raster.py, raster_reference):
 * the reference's L0 layer -- create_ground_truth_timestep_grids at 512 (data_preprocessing.py:262-273), the index-0 backward flow of the
 * vehicles (:360-363), rotate_all_from_inputs (grid_utils.py:438-584) and actor_traj_process (data_preprocessing.py:145-213) -- as three
 * launches on `stream`.  No host sync, no allocation, no floating-point atomics: the same inputs give the same bits.
 *   state   float [8, B, A, 11]  x, y, bbox_yaw, length, width, velocity_x, velocity_y, valid (> 0 is valid) over 10 past + 1 current step
 *   type    int   [B, A]         1 vehicle, 2 pedestrian, 3 cyclist;  is_sdc int [B, A]: the SDC is the lowest agent with is_sdc == 1
 *   ws      stj_raster_workspace_bytes(B, A) bytes, 16-byte aligned; its parts lie at stj_raster_workspace_offset(B, A, part):
 *             STJ_RASTER_BOX   float [B, A, 11, 12]  cx cy | half axis hx (2) | half axis hy (2) | vx vy (rotated) | bbox_yaw (unrotated) |
 *                                                    class (0 vehicle, 1 pedestrian or cyclist, -1 none) | valid | 0
 *             STJ_RASTER_AABB  int   [B, A, 11, 4]   x0 y0 x1 y1: a pixel box that holds every rendered point; x1 < x0: none
 *             STJ_RASTER_FRAME float [B, 8]          SDC x, y, yaw, angle = pi/2 - yaw, cos, sin, SDC index (-1: none), ok
 *             STJ_RASTER_OK    int   [B]             0: no SDC in the scene -> every output of the scene is zero
 *             STJ_RASTER_MASK  int   [B, A]          bit 0 in_box, 1 occu_mask, 2 has a valid step, 3 first valid position farther than the last
 *             STJ_RASTER_DIST  float [B, A, 2]       |position| at the last / first valid step
 *             STJ_RASTER_RANK  int   [B, A, 2]       the agent's place among the nearest of obs / occ, -1: not kept
 * stj_raster_boxes writes BOX, AABB, FRAME, OK.  stj_raster_grids reads them and writes ogm float [B, grid, grid, 11, 2] and flow float
 * [B, grid, grid, 2] (every element, 16-byte aligned); points_length x points_width points per box.  stj_raster_actors (the FOV grid and its
 * SDC pixel; A <= 1024) reads BOX and OK and writes MASK, DIST, RANK, obs float [B, 48, 11, 8] and occ float [B, 16, 11, 8] (every element). */
enum stj_raster_part { STJ_RASTER_BOX = 0, STJ_RASTER_AABB = 1, STJ_RASTER_FRAME = 2, STJ_RASTER_OK = 3, STJ_RASTER_MASK = 4, STJ_RASTER_DIST = 5,
                       STJ_RASTER_RANK = 6 };
long long stj_raster_workspace_bytes(int B, int A);
long long stj_raster_workspace_offset(int B, int A, int part);
int stj_raster_boxes(const float* state, const int* type, const int* is_sdc, void* ws, int B, int A, int grid, float ppm,
                     float sdc_x, float sdc_y, hipStream_t stream);
int stj_raster_grids(const void* ws, float* ogm, float* flow, int B, int A, int grid, float ppm, float sdc_x, float sdc_y,
                     int points_length, int points_width, hipStream_t stream);
int stj_raster_actors(void* ws, const int* type, float* obs, float* occ, int B, int A, int fov_grid, float ppm, float fov_sdc_x,
                      float fov_sdc_y, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
