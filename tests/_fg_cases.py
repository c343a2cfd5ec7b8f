"""Cases, flat-buffer layout, float64 references and the judge shared by test_fg_abi_gpu.py (the FG-MSA kernels of csrc/fgattn.hip and the FG
part of csrc/attn.hip through the C ABI) and test_fg_ref.py (the references and the judge themselves, on the CPU).  Nothing here needs a GPU
or the library.

A case is a dict (acase: one stj_fg_attn_fwd / _bwd pair, bcase: one stj_fg_bias_fwd / _bwd pair, ocase: one stj_fg_offset_fwd / _bwd pair
with the MODES below, fcase: one stj_fgoff_fwd / _bwd pair).  prepare(cs, dt, kind) lays every tensor of one call into its own flat CPU allocation filled with the NaN pattern of
test_gemm_gpu.PAT, GUARD elements in front and behind (a multiple of 16 bytes in every type: each tensor starts 16-byte aligned).  Written
outputs keep the pattern until the call, "+=" outputs start from non-zero values, the partial-sum workspaces dkp / dvp are scratch (any
content afterwards, guards intact).

Inputs: wherever a floor depends on a value it is exactly representable in bf16 -- the offsets are multiples of 1/8 below 16 in magnitude
(or 40.5), so float64 and the kernels take the same cell and the same alpha, bit for bit.  In the cases with G = 8 three groups are MARKED:
    group 0  LATTICE: every offset an integer in [-Hh/2, Hh/2] (both ends present: what tanh(.) Hh/2 saturates to in the 16-bit types), and
             keys 0..3 at -Hh, -Hh - 1, 1 - 2 Hh, 2 - 2 Hh, where the sample point reaches the last padded cell (alpha == 1, below);
    group 1  FAR: every offset 40.5 -- every sample point beyond the padded table: the bias is 0 and a is the plain softmax;
    group 2  PEAKED (attention only): the table of this group has spread 30 (normal), so that one key carries a row; references() asserts
             that rows with their maximum in the first 32 keys and rows with it in the last 32 keys both occur (the running maximum of the
             first step and the last slice of Split<16>::KS = 4 in the LDS merge).
The other groups draw offsets randint(-9, 9) + randint(2, 6) / 8 (off the lattice), q, k of spread 2, the table of spread 1.

R64 (reference): the module text in float64 torch with a HAND-WRITTEN backward.
    bias  FG_MSA.py:150-172 -- q_grid = pos' grid = _get_ref_points (:95-104): meshgrid(range(H), range(W)) in its default 'xy' indexing,
          so point n = (i, j) of the row-major map carries (j, i); displacement = q_grid - (offset + reference) (:134, :157), its two
          components swapped (:160) into sample's (x, y): x = (i_q - i_k) - off[k, 1] runs along the table's WIDTH, y = (j_q - j_k) -
          off[k, 0] along its HEIGHT.  (With H != W the text itself cannot run: offset [H, W, 2] + reference [W, H, 2].  The C ABI states
          the non-square form it accepts -- table [2 Hh - 1, 2 Ww - 1, G], tokens row-major -- and that is what R64 states for 8 x 16.)
          sample (occu_metric.py:345-409, pixel_type = 0, BILINEAR, ZERO): pad the table by one zero cell, warp + 1, then
          interpolate_bilinear (tfa_image.py:87-173): floor = min(max(0, floor(query)), size - 2) (:126-128), alpha = query - floor
          clipped to [0, 1] (:136-139), the four corners gathered (:162-165) and lerped along x, then y (:169-171).
    core  :144-148, :172-176: S = 48^-1/2 q k^T + bias, P = softmax(S), a = P v per (sample, group); lse = log sum exp S.
    offset head  :84-92 / :109-123 as the header states the hand-offs: off = tanh(o . W1) scale, fh = off . W2 + b2 (+ qres); fused
          (fgoff_statement): o = gelu(LayerNorm_1e-3(conv3x3, 8 groups, SAME (q) + bias)) in front of it, backward by hand (test_fg_ref.py:
          equal to autograd through F.conv2d / F.layer_norm / F.gelu(tanh)).
    The backward, by hand (test_fg_ref.py: equal to autograd through oracle.torch_ref._sample wherever no alpha is 0 or 1):
          dS = P (dP - sum_k P dP), dP = da v^T;  dq = 48^-1/2 dS k, dk = 48^-1/2 dS^T q, dv = P^T da;  d bias = dS;
          d table: dS times the four lerp weights, scattered to the corners that lie inside the table;
          d off[k, 0] = - sum_q dS (bottom - top) [alpha_y passes],  d off[k, 1] = - sum_q dS (ay (br - bl) + (1 - ay) (tr - tl)) [alpha_x passes].
    ON THE LATTICE the rule is TF's, derived from the text: the alpha is minimum(maximum(min_alpha, a), max_alpha) with a = query - floor
          (tfa_image.py:136-139).  floor() has no gradient, so d a / d query = 1.  TF's MaximumGrad hands the gradient to its FIRST operand
          where first >= second and MinimumGrad where first <= second: a tie goes to the first operand.  In maximum(min_alpha, a) the first
          operand is the constant, so a receives the gradient iff a > 0; in minimum(., max_alpha) the first operand is the running value,
          so it passes iff a <= 1.  Together: a receives a gradient iff 0 < a <= 1.  An integer sample point inside the table has a == 0:
          no offset gradient, although the value is continuous there and its one-sided derivatives are not zero.  a == 1 happens only at
          query == size - 1 (floor clipped to size - 2): the gradient passes, and it is the slope towards the zero pad.
Rdt (twin): the same statement with rd() applied where the kernels turn an f32 value into the storage type T; rd = identity reproduces R64.
    Rounding points, found in the kernels:
    fgattn forward   P~ = exp(S - running max) (Ch<T>::from_acc in front of O^T = V^T P^T; the row sum l adds the unrounded values in f32);
                     a = O / l (st4).  S, the bias, the merge of the four key slices and lse are f32.  The twin walks the keys as the kernel
                     does (_stepwise: 32 at a time per key slice, running maximum, merge): WHICH value is rounded depends on the running
                     maximum.
    fgattn backward  P = exp(S - lse) into its LDS tile (operand of dV = P^T dO);  48^-1/2 dS into its LDS tile and through from_acc
                     (operand of dK and dq);  dq;  dk, dv (the reduce kernel, after the f32 partial sums).  sum_k P dP is read as
                     dO . a from the STORED a;  dS, the table and offset gradients are f32.  Behind the forward kernel the twin is
                     evaluated end to end, its backward on its own forward's saves, as in _xattn_cases / _swin_cases (E2E_TOL below).
    fg_bias_*        none: offsets and d bias are read in T, everything else is f32.  (The twin is R64.)
    fgoff forward    c = conv + bias (acc_to_tile: the LDS tile, the save, and what mean / rstd are taken from);  LN(c);  gelu(.);  off.
                     The conv weights are the pack's: the f32 kernel rounded to T (the cases draw it exact in T).  mean / rstd f32.
    fgoff backward   LN(c) and gelu(.) recomputed from the saved c, mean, rstd as in the forward;  d gelu = ds . w1^T;  d LN = d gelu gelu'(LN);
                     dc (halo tile = operand of the transposed conv, the store, and what d_bias sums);  dq.  ds = doff (scale - off^2 / scale)
                     from the stored off, d_w1, d_gamma, d_beta are f32 sums of the rounded factors.
    fg_offset_fwd    off (stored, and the ROUNDED value feeds fh);  fh.
    fg_offset_bwd    dO, dq, doff_out.  d off = doff + dfh . W2^T, the tanh factor scale - off^2 / scale (from the stored off) and the
                     weight gradients are f32.
judge(): per output tensor and per ROW  ||got[r] - R64[r]|| <= bound[r], the one of _xattn_cases.judge / _swin_cases.judge:
    f32     bound[r] = tol (max(||R64[r]||, rms_r ||R64[r]||) + ||start[r]||)
    16 bit  bound[r] = 2 max(e_twin[r], rms_r e_twin[r]) + the f32 bound,  e_twin[r] = ||Rdt[r] - R64[r]||
    tol = TOL_FWD = 2e-5 for forward values (a, lse, bias, off, fh), TOL_BWD = 2e-4 for gradients: _xattn_cases' figures; the CPU float32
    statement of test_fg_ref.py stays at ratio <= 0.5 under them on every case (the largest measured is written there).  The one
    exception, measured there too: the 16-bit gradients judged behind the forward kernel, E2E_TOL.
    Rows: a, dq, dk, dv the 48-vector of one (b, token, group);  lse one (b, g);  doff one (b, g, key);  dtable one table row of one group;
    bias one (b, g, query);  off one (b, g);  fh, dO, dq, c, dc of the offset heads one pixel row;  mean, rstd one sample;  a parameter
    gradient the vector.  cols of the fused offset head is a copy: bit for bit the im2col matrix of q.
    "+=" outputs are judged as the sum start + R64.  Every byte that is no output is bit-identical afterwards, no output element keeps the
    pattern.  check_edges(): doff is EXACTLY its start value (0 where written) for every (key, component) no query of which passes the
    rule above, and the FAR group leaves its column of dtable bit-identical.

Dispatch table (csrc/fgattn.hip: dispatch / Split<>; csrc/attn.hip); T in float, bf16, f16:
  attn  a8_1, a8_3, a8_1_g1         fgattn_fwd_kernel<T, 4>, fgattn_bwd_kernel<T, 4> (one query tile: doff written), fgattn_dkv_reduce_kernel<T>
        a16_1, a16_2                fgattn_fwd_kernel<T, 16>, fgattn_bwd_kernel<T, 16> (4 query tiles, f32: 16; doff "+="), fgattn_dkv_reduce_kernel<T>
  bias  every case                  fg_bias_fwd_kernel<T>, fg_bias_bwd_kernel<T>; QS = 8 (b8x8_1, b8x16_1), 7 (b8x8_9, b8x16_9: ragged query
                                    slices, doff "+="), 1 (b8x8_33, b8x16_33: doff written)
  offset  every case                fg_offset_fwd_kernel<T>, fg_offset_bwd_kernel<T>
  fgoff (rows per workgroup R: fgoff_rows)   fgoff_fwd_kernel<T, W, R>, fgoff_bwd_kernel<T, W, R>, fgoff_pack_kernel<T>
        f1_2_8, f3_6_8              <T, 8, 2>   (f1_2_8: both rows are borders)
        f2_1_16, f2_5_16            <T, 16, 1>  (f2_1_16: the halo is all padding)
        f128_4_16                   16b <T, 16, 2> (B H / 2 = 256 workgroups: the threshold); f32 <float, 16, 1>
        f127_4_16 (16b)             <T, 16, 1>  (just under the threshold)
        f2_3_32, f1_32_32 (16b)     <T, 32, 1>
"""
import math
import zlib

import torch
import torch.nn.functional as F

from test_gemm_gpu import GUARD, bits, draw, pattern
from _xattn_cases import TOL_BWD, TOL_FWD, Prep, report_lines        # noqa: F401  (report_lines: for the two test modules)
from _swin_cases import dgelu, gelu

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
ALL3, B16 = (F32, BF16, F16), (BF16, F16)
D = 48
FC_C = 384                 # channels of the fused offset head: 8 groups of 48
LATTICE, FAR, PEAKED = 0, 1, 2
FAR_OFF = 40.5
FWD_LIKE = ('a', 'lse', 'bias', 'off', 'fh', 'c', 'mean', 'rstd')
IDENT = lambda t: t
# Behind the forward kernel (prepare(saves_from=)) the 16-bit rows are judged against the END-TO-END twin: its backward on its own forward's
# saves.  Which way a stored a rounds is then part of the statement, and in a peaked row, where sum_k P dP = dO . a cancels against dP of the
# leading key, one rounding of a that falls the other way moves a gradient row by more than the twin's distance from float64.  The float32
# CPU statement of that form (test_fg_ref.py: test_float32_statement_forward_into_backward) shows it; an output it leaves above ratio 0.5
# has its tolerance TOL_BWD multiplied here, in that form and in 16 bit only, by the smallest factor (rounded up) that brings the statement
# to 0.5.  Measured: factor needed, ratio without it, case.
E2E_TOL = {('attn', 'dq'): 16.0,        # 15.11  0.710  a16_2 bf16  (f16: 6.14, 0.750)
           ('attn', 'dk'): 21.0,        # 20.35  0.800  a16_2 bf16
           ('attn', 'dv'): 1.3,         #  1.24  0.529  a8_3 f16
           ('attn', 'dtable'): 1.5,     #  1.48  0.536  a8_3 bf16
           ('attn', 'doff'): 50.0,      # 49.22  1.501  a16_2 bf16
           ('fgoff', 'dc'): 1.5}        #  1.43  0.536  f127_4_16 f16


def acase(name, B, Hh, G=8, dts=ALL3):
    return dict(name=name, fam='attn', B=B, G=G, Hh=Hh, Ww=Hh, HW=Hh * Hh, dts=dts, marked=G == 8, scale=D ** -0.5)


def bcase(name, B, Hh, Ww, G=8, dts=ALL3):
    qs = min(8, max(1, 512 // (B * G)))
    return dict(name=name, fam='bias', B=B, G=G, Hh=Hh, Ww=Ww, HW=Hh * Ww, dts=dts, marked=G == 8, QS=qs)


# the offset head's modes: forward (fh, zmajor, qres, b2, o) and backward (doff, dfh, dO, dq, db2) present or not
FMODES = {'off_only': dict(fh=0, zmajor=0, qres=0, b2=0, o=1), 'fh': dict(fh=1, zmajor=0, qres=0, b2=1, o=1),
          'fh_z_qres': dict(fh=1, zmajor=1, qres=1, b2=1, o=1), 'fh_z_nob2': dict(fh=1, zmajor=1, qres=0, b2=0, o=1),
          'fh_qres_nob2': dict(fh=1, zmajor=0, qres=1, b2=0, o=1), 'fh_from_off': dict(fh=1, zmajor=0, qres=0, b2=1, o=0)}
BMODES = {'doff_only': dict(doff=1, dfh=0, dO=1, dq=0, db2=0, zmajor=0), 'dfh_only': dict(doff=0, dfh=1, dO=1, dq=1, db2=1, zmajor=0),
          'both': dict(doff=1, dfh=1, dO=1, dq=1, db2=1, zmajor=0), 'both_z': dict(doff=1, dfh=1, dO=1, dq=1, db2=1, zmajor=1),
          'no_dO': dict(doff=1, dfh=1, dO=0, dq=1, db2=1, zmajor=0), 'no_dq': dict(doff=1, dfh=1, dO=1, dq=0, db2=1, zmajor=1),
          'no_db2': dict(doff=1, dfh=1, dO=1, dq=1, db2=0, zmajor=0)}


def ocase(name, G, gc, C2, HW, B=2, dts=ALL3):
    return dict(name=name, fam='offset', B=B, G=G, gc=gc, C2=C2, HW=HW, dts=dts, scale=4.0)


def fcase(name, B, H, W, dts=ALL3):
    """one stj_fgoff_fwd / _bwd pair: q [B, H, W, 384]; sample B - 1 is all zeros when B > 1"""
    return dict(name=name, fam='fgoff', B=B, G=8, H=H, W=W, HW=H * W, dts=dts, scale=H / 2.0, eps=1e-3)


def cases():
    return [fcase('f1_2_8', 1, 2, 8), fcase('f3_6_8', 3, 6, 8), fcase('f2_1_16', 2, 1, 16), fcase('f2_5_16', 2, 5, 16), fcase('f128_4_16', 128, 4, 16),
            fcase('f127_4_16', 127, 4, 16, B16), fcase('f2_3_32', 2, 3, 32, B16), fcase('f1_32_32', 1, 32, 32, B16),
            acase('a8_1', 1, 8), acase('a8_3', 3, 8), acase('a16_1', 1, 16), acase('a16_2', 2, 16), acase('a8_1_g1', 1, 8, G=1),
            bcase('b8x8_1', 1, 8, 8, G=1), bcase('b8x16_1', 1, 8, 16, G=1), bcase('b8x8_9', 9, 8, 8), bcase('b8x16_9', 9, 8, 16),
            bcase('b8x8_33', 33, 8, 8), bcase('b8x16_33', 33, 8, 16),
            ocase('o8_48_384_64', 8, 48, 384, 64), ocase('o4_24_64_16', 4, 24, 64, 16), ocase('o1_100_8_80', 1, 100, 8, 80),
            ocase('o8_256_1024_16', 8, 256, 1024, 16, dts=(F32,))]


_CASES = {c['name']: c for c in cases()}
CASE_DT = [(c['name'], dt) for c in cases() for dt in c['dts']]


def case(name):
    return _CASES[name]


def family(fam):
    return [(n, dt) for n, dt in CASE_DT if case(n)['fam'] == fam]


def case_id(v):
    return v if isinstance(v, str) else str(v).replace('torch.', '')


def modes(cs, kind):
    if cs['fam'] != 'offset':
        return (None,)
    return tuple(FMODES) if kind == 'fwd' else tuple(BMODES)


# ------------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def _offsets(cs, g):
    B, G, HW, Hh = cs['B'], cs['G'], cs['HW'], cs['Hh']
    shape = (B, G, HW, 2)
    off = torch.randint(-9, 10, shape, generator=g) + torch.randint(2, 7, shape, generator=g) / 8.0
    if cs['marked']:
        lat = torch.randint(-Hh // 2, Hh // 2 + 1, (B, HW, 2), generator=g).float()
        lat[:, 4] = Hh // 2
        lat[:, 5] = -(Hh // 2)
        lat[:, 6] = torch.tensor([Hh // 2, -(Hh // 2)], dtype=torch.float32)
        for i, v in enumerate((-Hh, -Hh - 1, 1 - 2 * Hh, 2 - 2 * Hh)):
            lat[:, i] = v
        off[:, LATTICE] = lat
        off[:, FAR] = FAR_OFF
    assert float(off[off != FAR_OFF].abs().max()) < 32
    return off


def make_inputs(cs, dt):
    """name -> CPU tensor as stored: activations and offsets in dt, the table and every start value f32"""
    g = torch.Generator().manual_seed(7000 + zlib.crc32(cs['name'].encode()) % 100000)
    d = lambda shape, scale=1.0, t=F32: draw(math.prod(shape), t, g, False, scale=scale).reshape(shape)
    B, G, HW = cs['B'], cs['G'], cs['HW']
    if cs['fam'] == 'fgoff':
        q = d((B, cs['H'], cs['W'], FC_C), 1.0, dt)
        if B > 1:
            q[B - 1] = 0           # c = the bias there: a LayerNorm variance (~1e-3) comparable with eps
        return dict(q=q, w=d((3, 3, D, FC_C), 1.5 / math.sqrt(9 * D), dt).float(), bias=d((FC_C,), 0.05), gamma=1.0 + d((FC_C,), 0.3), beta=d((FC_C,), 0.3),
                    w1=d((D, 2), 0.3, dt), doff=d((B, G, HW, 2), 1.0, dt), start_d_w1=d((D, 2)), start_d_gamma=d((FC_C,)), start_d_beta=d((FC_C,)),
                    start_d_bias=d((FC_C,)))
    if cs['fam'] == 'offset':
        gc, C2 = cs['gc'], cs['C2']
        o = d((B, HW, G, gc), 1.0 / math.sqrt(gc))
        o[:, 1::7] *= 40.0                           # pixels whose |o . W1| saturates tanh in every storage type (and mostly in f32)
        I = dict(o=o.to(dt), W1=d((gc, 2), 1.0, dt), W2=d((2, C2), 0.5, dt), b2=d((C2,), 0.3), qres=d((B, HW, C2), 1.0, dt),
                 doff=d((B, G, HW, 2), 1.0, dt), dfh=d((B, G, HW, C2), 1.0, dt), start_dW1=d((gc, 2)), start_dW2=d((2, C2)), start_db2=d((C2,)))
        I['dfh_z'] = I['dfh'].permute(1, 0, 2, 3).contiguous()
        return I
    TH, TW = 2 * cs['Hh'] - 1, 2 * cs['Ww'] - 1
    I = dict(off=_offsets(cs, g).to(dt), table=d((TH, TW, G)), start_dtable=d((TH, TW, G)), start_doff=d((B, G, HW, 2)))
    assert torch.equal(I['off'].double(), _offsets(cs, torch.Generator().manual_seed(g.initial_seed())).double()), 'an offset is not exact in ' + str(dt)
    if cs['fam'] == 'attn':
        C = G * D
        I.update(q=d((B, HW, C), 2.0, dt), k=d((B, HW, C), 2.0, dt), v=d((B, HW, C), 1.0, dt), da=d((B, HW, C), 1.0, dt))
        if cs['marked']:
            I['table'][:, :, PEAKED] = 30.0 * torch.randn(TH, TW, generator=g)
    else:
        I['dbias'] = d((B, G, HW, HW), 1.0, dt)
    return I


# ------------------------------------------------------------------------------------------------------------------------------------------
# The module text, in `dtype` (float64: R64; float32: the CPU statement of test_fg_ref.py), rd: the twin's rounding
# ------------------------------------------------------------------------------------------------------------------------------------------
def _axis(coord, size_p):
    """interpolate_bilinear's floor / alpha of one axis (tfa_image.py:124-139) and where the alpha passes a gradient (TF's tie rule)"""
    f = coord.floor().clamp(0, size_p - 2)
    a = coord - f
    return f.long(), a.clamp(0, 1), (a > 0) & (a <= 1)


def sample_parts(cs, off, table):
    """everything the bias and its gradients need; [B, G, query, key] tensors"""
    B, G, HW, Hh, Ww = cs['B'], cs['G'], cs['HW'], cs['Hh'], cs['Ww']
    TH, TW = 2 * Hh - 1, 2 * Ww - 1
    Hp, Wp = TH + 2, TW + 2
    n = torch.arange(HW)
    i, j = (n // Ww).to(off.dtype), (n % Ww).to(off.dtype)
    x = (i[:, None] - i[None, :])[None, None] - off[..., 1][:, :, None, :] + 1
    y = (j[:, None] - j[None, :])[None, None] - off[..., 0][:, :, None, :] + 1
    x0, ax, gx = _axis(x, Wp)
    y0, ay, gy = _axis(y, Hp)
    tp = torch.zeros(G, Hp, Wp, dtype=table.dtype)
    tp[:, 1:-1, 1:-1] = table.permute(2, 0, 1)
    tpf = tp.reshape(1, G, Hp * Wp).expand(B, -1, -1)
    at = lambda yy, xx: tpf.gather(2, (yy * Wp + xx).reshape(B, G, -1)).reshape(B, G, HW, HW)
    S = dict(x0=x0, y0=y0, ax=ax, ay=ay, gx=gx, gy=gy, tl=at(y0, x0), tr=at(y0, x0 + 1), bl=at(y0 + 1, x0), br=at(y0 + 1, x0 + 1), Hp=Hp, Wp=Wp)
    S['top'] = ax * (S['tr'] - S['tl']) + S['tl']
    S['bot'] = ax * (S['br'] - S['bl']) + S['bl']
    S['bias'] = ay * (S['bot'] - S['top']) + S['top']
    return S


def sample_grads(cs, S, go):
    """(doff [B, G, key, 2], dtable [TH, TW, G]) of d bias = go [B, G, query, key]"""
    B, G, Hp, Wp = cs['B'], cs['G'], S['Hp'], S['Wp']
    ax, ay = S['ax'], S['ay']
    d0 = -(go * (S['bot'] - S['top']) * S['gy']).sum(2)
    d1 = -(go * (ay * (S['br'] - S['bl']) + (1 - ay) * (S['tr'] - S['tl'])) * S['gx']).sum(2)
    dtp = torch.zeros(B, G, Hp * Wp, dtype=go.dtype)
    for dy, dx, w in ((0, 0, (1 - ay) * (1 - ax)), (0, 1, (1 - ay) * ax), (1, 0, ay * (1 - ax)), (1, 1, ay * ax)):
        dtp.scatter_add_(2, ((S['y0'] + dy) * Wp + S['x0'] + dx).reshape(B, G, -1), (go * w).reshape(B, G, -1))
    dtable = dtp.sum(0).reshape(G, Hp, Wp)[:, 1:-1, 1:-1].permute(1, 2, 0)
    return torch.stack((d0, d1), -1), dtable


def _heads(t, cs):
    return t.reshape(cs['B'], cs['HW'], cs['G'], D).permute(0, 2, 1, 3)


def _tokens(t, cs):
    return t.permute(0, 2, 1, 3).reshape(cs['B'], cs['HW'], cs['G'] * D)


def key_slice(cs):
    """the keys of the second of the forward's key slices (16 x 16: Split<16>::KS = 4 slices of 64) or of its second 32-key step (8 x 8)"""
    return slice(64, 128) if cs['HW'] == 256 else slice(32, 64)


def _stepwise(cs, logit, v, rd):
    """O / l as the forward kernel forms it: every key slice (Split<NKF>::KS: 4 slices of 64 keys on the 16 x 16 map, one on 8 x 8) visits its
    keys 32 at a time with a running maximum, rounds exp(S - running maximum) in front of the product with V (the row sum adds the
    unrounded values) and rescales; the slices merge at the end.  Without a rounding this is the softmax."""
    HW = cs['HW']
    ks = 4 if HW == 256 else 1
    parts = []
    for sl in range(ks):
        m = torch.full_like(logit[..., :1], -float('inf'))
        l, O = torch.zeros_like(m), torch.zeros_like(v)
        for k0 in range(sl * HW // ks, (sl + 1) * HW // ks, 32):
            s = logit[..., k0:k0 + 32]
            mn = torch.maximum(m, s.max(-1, keepdim=True).values)
            alpha, x = torch.exp(m - mn), torch.exp(s - mn)
            l, O, m = l * alpha + x.sum(-1, keepdim=True), O * alpha + rd(x) @ v[:, :, k0:k0 + 32], mn
        parts.append((m, l, O))
    M = torch.stack([m for m, _, _ in parts]).max(0).values
    l = sum(l * torch.exp(m - M) for m, l, _ in parts)
    return sum(O * torch.exp(m - M) for m, _, O in parts) / l


def attn_statement(cs, I, dtype=F64, rd=IDENT, saves=None, fault=None, stepwise=None):
    """name -> every output of stj_fg_attn_fwd and _bwd ("+=" outputs WITHOUT start values).  saves: (a, lse) the backward reads instead of
    this function's own forward.  fault: 'slice_dropped' -- group (0, 3 mod G) loses one key slice's share of the sum and the row sum."""
    c = lambda t: t.to(dtype)
    q, k, v, da = (_heads(c(I[n]), cs) for n in ('q', 'k', 'v', 'da'))
    S = sample_parts(cs, c(I['off']), c(I['table']))
    logit = cs['scale'] * (q @ k.transpose(-1, -2)) + S['bias']
    if fault == 'slice_dropped':
        logit = logit.clone()
        logit[0, 3 % cs['G'], :, key_slice(cs)] = -float('inf')
    m = logit.max(-1, keepdim=True).values
    E = torch.exp(logit - m)
    l = E.sum(-1, keepdim=True)
    lse = (m + torch.log(l))[..., 0]
    a = rd(_stepwise(cs, logit, v, rd) if (rd is not IDENT if stepwise is None else stepwise) else (E @ v) / l)
    out = dict(a=_tokens(a, cs), lse=lse, _P=E / l)
    if saves is not None:
        a, lse = _heads(c(saves[0]), cs), c(saves[1]).reshape(lse.shape)
    P = torch.exp(logit - lse[..., None])
    go = P * (da @ v.transpose(-1, -2) - (da * a).sum(-1, keepdim=True))
    dS = rd(go * cs['scale'])
    doff, dtable = sample_grads(cs, S, go)
    out.update(dq=_tokens(rd(dS @ k), cs), dk=_tokens(rd(dS.transpose(-1, -2) @ q), cs), dv=_tokens(rd(rd(P).transpose(-1, -2) @ da), cs),
               doff=doff, dtable=dtable, _passes=torch.stack((S['gy'].any(2), S['gx'].any(2)), -1))
    return out


def bias_statement(cs, I, dtype=F64, rd=IDENT, saves=None, fault=None):
    S = sample_parts(cs, I['off'].to(dtype), I['table'].to(dtype))
    doff, dtable = sample_grads(cs, S, I['dbias'].to(dtype))
    return dict(bias=S['bias'], doff=doff, dtable=dtable, _passes=torch.stack((S['gy'].any(2), S['gx'].any(2)), -1))


def fh_rows(t, cs, zmajor):
    """[B, G, HW, C2] in the logical order -> the stored order"""
    return t.permute(1, 0, 2, 3) if zmajor else t


def offset_statement(cs, I, dtype=F64, rd=IDENT, saves=None, fault=None):
    """every mode's outputs under the mode's name: 'fwd:<mode>' -> dict, 'bwd:<mode>' -> dict"""
    c = lambda t: t.to(dtype)
    o, W1, W2, b2, qres = (c(I[n]) for n in ('o', 'W1', 'W2', 'b2', 'qres'))
    s = cs['scale']
    u = torch.einsum('bhgc,co->bgho', o, W1)
    off = rd(torch.tanh(u) * s)
    out = {}
    for name, m in FMODES.items():
        src = off if m['o'] else c(rd(I['doff']))           # o == NULL: any given off (the case's doff tensor serves as one)
        r = {}
        if m['o']:
            r['off'] = off
        if m['fh']:
            fh = torch.einsum('bgho,oc->bghc', src, W2)
            if m['b2']:
                fh = fh + b2
            if m['qres']:
                fh = fh + qres[:, None]
            r['fh'] = fh_rows(rd(fh), cs, m['zmajor'])
        out['fwd:' + name] = r
    offs = c(saves) if saves is not None else off             # the backward reads the stored off
    for name, m in BMODES.items():
        dfh = c(I['dfh']) if m['dfh'] else None
        dof = c(I['doff']) if m['doff'] else torch.zeros_like(off)
        r = {}
        if dfh is not None:
            dof = dof + torch.einsum('bghc,oc->bgho', dfh, W2)
            r['dW2'] = torch.einsum('bgho,bghc->oc', offs, dfh)
            if m['db2']:
                r['db2'] = dfh.sum((0, 1, 2))
            if m['dq']:
                r['dq'] = rd(dfh.sum(1))
        if not m['dO']:
            r['doff_out'] = rd(dof)
        else:
            du = dof * (s - offs * offs / s)
            r['dO'] = rd(torch.einsum('bgho,co->bhgc', du, W1))
            r['dW1'] = torch.einsum('bhgc,bgho->co', o, du)
        out['bwd:' + name] = r
    out['_sat'] = u.abs() > 4.0                               # tanh(4) = 1 - 6.7e-4: rounds to 1 in bf16 and fp16
    return out


def im2col(q):
    """[B H W, 8, 9 * 48] (tap-major inside a group) of q [B, H, W, 384], zero outside the image: what the forward saves as cols"""
    B, H, W, _ = q.shape
    u = F.unfold(q.permute(0, 3, 1, 2).float(), 3, padding=1)              # [B, 384 * 9, HW], (channel, tap)
    return u.reshape(B, 8, D, 9, H * W).permute(0, 4, 1, 3, 2).reshape(B * H * W, 8, 9 * D).to(q.dtype)


def fgoff_statement(cs, I, dtype=F64, rd=IDENT, saves=None, fault=None):
    """name -> every output of stj_fgoff_fwd and _bwd.  saves: (c, mean, rstd, off) the backward reads instead of this function's forward.
    fault 'halo': the conv of sample 0's last row reads sample 1's first row as its lower halo (and the other way round)."""
    c_ = lambda t: t.to(dtype)
    B, H, W, G, s, eps = cs['B'], cs['H'], cs['W'], cs['G'], cs['scale'], cs['eps']
    q, bias, gam, bet, w1 = (c_(I[n]) for n in ('q', 'bias', 'gamma', 'beta', 'w1'))
    wt = c_(I['w']).permute(3, 2, 0, 1)                                 # [out channel, in channel of the group, ky, kx]
    x = q.permute(0, 3, 1, 2)
    conv = F.conv2d(x, wt, padding=1, groups=G)
    if fault == 'halo':
        tall = F.conv2d(torch.cat((x[0], x[1]), 1)[None], wt, padding=1, groups=G)[0]
        conv = conv.clone()
        conv[0], conv[1] = tall[:, :H], tall[:, H:]
    cc = rd(conv.permute(0, 2, 3, 1) + bias)
    mu = cc.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(((cc - mu) ** 2).mean(-1, keepdim=True) + eps)

    def tail(cc, mu, rs):
        xh = (cc - mu) * rs
        y = rd(xh * gam + bet)
        return xh, y, rd(gelu(y))

    xh, y, act = tail(cc, mu, rs)
    u = torch.einsum('bngc,co->bgno', act.reshape(B, H * W, G, D), w1)
    off = rd(torch.tanh(u) * s)
    out = dict(c=cc, mean=mu[..., 0], rstd=rs[..., 0], off=off)
    if saves is not None:
        cc, mu, rs, off = c_(saves[0]).reshape(cc.shape), c_(saves[1]).reshape(mu.shape), c_(saves[2]).reshape(rs.shape), c_(saves[3]).reshape(off.shape)
        xh, y, act = tail(cc, mu, rs)
    ds = c_(I['doff']) * (s - off * off / s)
    da = rd(torch.einsum('bgno,co->bngc', ds, w1)).reshape(cc.shape)
    dy = rd(da * dgelu(y))
    dxh = dy * gam
    dc = rd(rs * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True)))
    out.update(d_w1=torch.einsum('bngc,bgno->co', act.reshape(B, H * W, G, D), ds), d_gamma=(dy * xh).sum((0, 1, 2)), d_beta=dy.sum((0, 1, 2)),
               d_bias=dc.sum((0, 1, 2)), dc=dc, dq=rd(F.conv_transpose2d(dc.permute(0, 3, 1, 2), wt, padding=1, groups=G).permute(0, 2, 3, 1)))
    return out


STATEMENT = dict(attn=attn_statement, bias=bias_statement, offset=offset_statement, fgoff=fgoff_statement)


# ------------------------------------------------------------------------------------------------------------------------------------------
# One call: buffers, reference, bounds
# ------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """one flat allocation: GUARD | n | GUARD elements, the pattern everywhere except the values put in"""
    def __init__(self, n, dt, values=None, scratch=False):
        self.init, self.n, self.scratch = pattern(GUARD + n + GUARD, dt), n, scratch
        if values is not None:
            self.init[GUARD:GUARD + n] = values.reshape(-1).to(dt)


ROWS = dict(a=lambda t: t.reshape(-1, D), dq=lambda t: t.reshape(-1, D), dk=lambda t: t.reshape(-1, D), dv=lambda t: t.reshape(-1, D),
            lse=lambda t: t.reshape(-1, t.shape[-1]), doff=lambda t: t.reshape(-1, 2), dtable=lambda t: t.permute(0, 2, 1).reshape(-1, t.shape[1]),
            bias=lambda t: t.reshape(-1, t.shape[-1]))
VECTORS = ('dW1', 'dW2', 'db2', 'd_w1', 'd_gamma', 'd_beta', 'd_bias')


def rows(name, t, fam='attn'):
    """the judge's row view of output `name` (logical shape) of family `fam`"""
    if name in VECTORS:
        return t.reshape(1, -1)
    if fam == 'fgoff' and name in ('mean', 'rstd'):
        return t.reshape(t.shape[0], -1)
    if fam in ('offset', 'fgoff'):
        return t.reshape(t.shape[0] * t.shape[1], -1) if name == 'off' else t.reshape(-1, t.shape[-1])
    return ROWS[name](t)


_REF = {}


def references(cs, dt):
    """(inputs, R64, Rdt) of one case and dtype, computed once per process and left unchanged.  Rdt's backward reads the reference's saves
    rounded (a to dt, lse to f32; off to dt), as the backward judged alone does."""
    key = (cs['name'], dt)
    if key not in _REF:
        I = make_inputs(cs, dt)
        st = STATEMENT[cs['fam']]
        R = st(cs, I)
        if cs['fam'] == 'attn':
            top = R['_P'].max(-1)
            plain = [g for g in range(cs['G']) if not cs['marked'] or g > PEAKED]
            peak = float(top.values[:, plain].mean())
            assert 2.0 / cs['HW'] <= peak <= 0.7, f'{cs["name"]}: mean max_key P = {peak:.3f}: the attention is uniform or one-hot'
            if cs['marked']:
                pk = top.values[:, PEAKED] > 0.9
                first, last = (top.indices[:, PEAKED] < 32) & pk, (top.indices[:, PEAKED] >= cs['HW'] - 32) & pk
                assert float(pk.double().mean()) > 0.5 and int(first.sum()) >= 2 and int(last.sum()) >= 2, \
                    f'{cs["name"]}: peaked rows {float(pk.double().mean()):.2f}, maximum in the first step {int(first.sum())}, in the last {int(last.sum())}'
        if cs['fam'] == 'offset':
            sat = float(R['_sat'].double().mean())
            assert 0.02 <= sat <= 0.5, f'{cs["name"]}: {sat:.3f} of the offsets are saturated'
        tw = None
        if dt != F32:
            rd = lambda t: t.to(dt).double()
            sv = dict(attn=lambda: (rd(R['a']), R['lse'].float()), bias=lambda: None, offset=lambda: rd(R['fwd:off_only']['off']),
                      fgoff=lambda: (rd(R['c']), R['mean'].float(), R['rstd'].float(), rd(R['off'])))[cs['fam']]()
            tw = st(cs, I, rd=rd, saves=sv)
        _REF[key] = (I, R, tw)
    return _REF[key]


def ws_elems(cs):
    """floats of each of dkp, dvp: stj_fg_attn_bwd_workspace_bytes / 4"""
    return cs['B'] * cs['G'] * (cs['HW'] // 16) * cs['HW'] * D


def doff_written(cs):
    """whether the backward writes doff (one query tile / one query slice) instead of adding to it"""
    return cs['HW'] == 64 if cs['fam'] == 'attn' else cs['QS'] == 1


def prepare(cs, dt, kind, mode=None, saves_from=None, with_lse=True):
    """kind 'fwd' / 'bwd'; mode: a key of FMODES / BMODES (offset head).  saves_from: what the backward is handed instead of the reference's
    rounded saves -- (a, lse) of the attention, off of the offset head, (c, mean, rstd, off) of the fused one (forward into backward; the
    twin is then evaluated end to end and the tolerances of E2E_TOL apply).  with_lse False: the inference form of the attention forward."""
    assert kind in ('fwd', 'bwd')
    I, R, tw = references(cs, dt)
    fam = cs['fam']
    if dt != F32 and saves_from is not None:
        key = (cs['name'], dt, 'e2e')
        if key not in _REF:
            _REF[key] = STATEMENT[fam](cs, I, rd=lambda t: t.to(dt).double())
        tw = _REF[key]
    p = Prep()
    p.cs, p.dt, p.kind, p.mode, p.I, p.bufs, p.outs, p.start, p.with_saves = cs, dt, kind, mode, I, {}, {}, {}, with_lse
    p.e2e = saves_from is not None
    R_all = R
    if fam == 'offset':
        R, tw = R[f'{kind}:{mode}'], (tw[f'{kind}:{mode}'] if tw is not None else None)
    p.R, p.tw = R, tw

    def tensor(name, shape, t, values=None, out=False, scratch=False, start=None):
        p.bufs[name] = Buf(math.prod(shape), t, values if start is None else start, scratch)
        if out:
            p.outs[name] = tuple(shape)
            if start is not None:
                p.start[name] = start.double().reshape(shape)

    B, G, HW = cs['B'], cs['G'], cs['HW']
    if fam in ('attn', 'bias'):
        tensor('off', I['off'].shape, dt, I['off'])
        tensor('table', I['table'].shape, F32, I['table'])
    if fam == 'attn':
        for n in ('q', 'k', 'v'):
            tensor(n, I[n].shape, dt, I[n])
        if kind == 'fwd':
            tensor('a', I['q'].shape, dt, out=True)
            tensor('lse', (B, G, HW), F32, out=with_lse)
        else:
            sa, sl = saves_from if saves_from is not None else (R['a'], R['lse'])
            tensor('a', I['q'].shape, dt, sa)
            tensor('lse', (B, G, HW), F32, sl)
            tensor('da', I['da'].shape, dt, I['da'])
            for n in ('dq', 'dk', 'dv'):
                tensor(n, I['q'].shape, dt, out=True)
            for n in ('dkp', 'dvp'):
                tensor(n, (ws_elems(cs),), F32, scratch=True)
    elif fam == 'bias':
        if kind == 'fwd':
            tensor('bias', (B, G, HW, HW), F32, out=True)
        else:
            tensor('dbias', I['dbias'].shape, dt, I['dbias'])
    if fam in ('attn', 'bias') and kind == 'bwd':
        tensor('dtable', I['table'].shape, F32, out=True, start=I['start_dtable'])
        tensor('doff', (B, G, HW, 2), F32, out=True, start=None if doff_written(cs) else I['start_doff'])
    if fam == 'offset':
        gc, C2 = cs['gc'], cs['C2']
        tensor('W2', (2, C2), dt, I['W2'])
        if kind == 'fwd':
            m = FMODES[mode]
            tensor('W1', (gc, 2), dt, I['W1'])
            tensor('o', I['o'].shape, dt, I['o'])
            tensor('b2', (C2,), F32, I['b2'])
            tensor('qres', I['qres'].shape, dt, I['qres'])
            tensor('off', (B, G, HW, 2), dt, None if m['o'] else I['doff'], out=bool(m['o']))
            tensor('fh', (G, B, HW, C2) if m['zmajor'] else (B, G, HW, C2), dt, out=bool(m['fh']))
        else:
            m = BMODES[mode]
            tensor('W1', (gc, 2), dt, I['W1'])
            tensor('o', I['o'].shape, dt, I['o'])
            tensor('off', (B, G, HW, 2), dt, saves_from if saves_from is not None else R_all['fwd:off_only']['off'])
            tensor('doff', (B, G, HW, 2), dt, I['doff'])
            tensor('dfh', I['dfh'].shape, dt, I['dfh_z'] if m['zmajor'] else I['dfh'])
            tensor('dO', I['o'].shape, dt, out=bool(m['dO']))
            tensor('dq', (B, HW, C2), dt, out=bool(m['dq'] and m['dfh']))
            tensor('doff_out', (B, G, HW, 2), dt, out=not m['dO'])
            tensor('dW1', (gc, 2), F32, out=bool(m['dO']), start=I['start_dW1'])
            tensor('dW2', (2, C2), F32, out=bool(m['dfh']), start=I['start_dW2'])
            tensor('db2', (C2,), F32, out=bool(m['db2'] and m['dfh']), start=I['start_db2'])
    if fam == 'fgoff':
        M = B * HW
        for n in ('bias', 'gamma', 'beta'):
            tensor(n, (FC_C,), F32, I[n])
        tensor('w1', (D, 2), dt, I['w1'])
        if kind == 'fwd':
            tensor('q', I['q'].shape, dt, I['q'])
            tensor('off', (B, G, HW, 2), dt, out=True)
            tensor('cols', (M, G, 9 * D), dt, out=False, scratch=with_lse)       # judged bit for bit by check_edges, not by rows
            tensor('c', (B, cs['H'], cs['W'], FC_C), dt, out=with_lse)
            tensor('mean', (B, HW), F32, out=with_lse)
            tensor('rstd', (B, HW), F32, out=with_lse)
        else:
            S = saves_from if saves_from is not None else (R['c'], R['mean'], R['rstd'], R['off'])
            for n, t, v in (('c', dt, S[0]), ('mean', F32, S[1]), ('rstd', F32, S[2]), ('off', dt, S[3]), ('doff', dt, I['doff'])):
                tensor(n, v.shape, t, v)
            tensor('dc', (B, cs['H'], cs['W'], FC_C), dt, out=True)
            tensor('dq', (B, cs['H'], cs['W'], FC_C), dt, out=True)
            for n in ('d_w1', 'd_gamma', 'd_beta', 'd_bias'):
                tensor(n, I['start_' + n].shape, F32, out=True, start=I['start_' + n])
    # bounds
    p.bound = {}
    for n, shape in p.outs.items():
        ref = rows(n, R[n].reshape(shape), fam)
        norms = ref.norm(dim=1)
        b = torch.maximum(norms, (norms ** 2).mean().sqrt())
        if n in p.start:
            b = b + rows(n, p.start[n], fam).norm(dim=1)
        tol = TOL_FWD if n in FWD_LIKE else TOL_BWD
        if dt != F32 and saves_from is not None:
            tol = tol * E2E_TOL.get((fam, n), 1.0)
        b = tol * b
        if dt != F32:
            e = (rows(n, tw[n].reshape(shape), fam) - ref).norm(dim=1)
            b = 2.0 * torch.maximum(e, (e ** 2).mean().sqrt()) + b
        p.bound[n] = b
    return p


def value(p, after, name):
    """output `name` as the call left it, in its logical shape"""
    return after[name][GUARD:GUARD + p.bufs[name].n].reshape(p.outs[name])


def expected(p, name):
    ref = p.R[name].reshape(p.outs[name])
    return ref + p.start[name] if name in p.start else ref


def pack(p, values):
    """the flat buffers a call that computed `values` (name -> tensor, "+=" outputs without start values) would leave"""
    after = {k: b.init.clone() for k, b in p.bufs.items()}
    for n, shape in p.outs.items():
        t = values[n].reshape(shape).double()
        if n in p.start:
            t = t + p.start[n]
        after[n][GUARD:GUARD + p.bufs[n].n] = t.reshape(-1).to(after[n].dtype)
    if 'cols' in p.bufs and p.bufs['cols'].scratch:
        after['cols'][GUARD:-GUARD] = values['cols'].reshape(-1) if 'cols' in values else im2col(p.I['q']).reshape(-1)
    return after


def judge(p, after, ratios=None, label=''):
    """after: name -> the flat CPU buffer as the call left it.  Raises AssertionError; appends (entry point, dtype, output, case, largest e / bound)."""
    cs = p.cs
    label = f"{cs['name']} {p.kind}{' ' + p.mode if p.mode else ''}{'' if p.with_saves else ' (no lse)'}{label}"
    for name, b in p.bufs.items():
        same = bits(after[name]) == bits(b.init)
        if name in p.outs or b.scratch:
            same[GUARD:GUARD + b.n] = True
        bad = (~same).nonzero()
        assert bad.numel() == 0, f'{label}: {bad.numel()} elements of {name} outside the outputs changed, first at flat index {int(bad[0]) - GUARD}'
    for name in p.outs:
        raw = value(p, after, name)
        left = bits(raw) == int(bits(pattern(1, raw.dtype))[0])
        assert not bool(left.any()), f'{label}: {int(left.sum())} elements of {name} still hold the fill pattern, first at {tuple(left.nonzero()[0].tolist())}'
        err = rows(name, raw.double() - expected(p, name), cs['fam']).norm(dim=1)
        ok = err <= p.bound[name]            # False for NaN
        ratio = float((err / (p.bound[name] + 1e-300)).nan_to_num(nan=float('inf')).max())
        if ratios is not None:
            ratios.append((f'{cs["fam"]} {p.kind}{" e2e" if p.e2e else ""}', case_id(p.dt), name, cs['name'] + (':' + p.mode if p.mode else ''), ratio))
        assert bool(ok.all()), (f'{label}: {name}: {int((~ok).sum())} of {ok.numel()} rows over their bound, largest ||err|| / bound = {ratio:.3e}, '
                                f'first row {int((~ok).nonzero()[0])}')
    check_edges(p, after, label)


def check_edges(p, after, label=''):
    """what must hold EXACTLY: no offset gradient where no query's alpha passes one (the lattice and the far group), the far group's column
    of dtable untouched; the saturated offsets of the offset head are +-scale exactly"""
    cs = p.cs
    if cs['fam'] == 'fgoff':
        if p.kind == 'fwd' and p.with_saves:
            got = after['cols'][GUARD:-GUARD].reshape(-1, 8, 9 * D)
            assert torch.equal(bits(got), bits(im2col(p.I['q']))), f'{label}: cols is not the im2col matrix of q'
        return
    if cs['fam'] == 'offset':
        if 'off' in p.outs and p.dt != F32:
            sat = p.tw['off'].abs() == cs['scale']
            got = value(p, after, 'off').double()
            assert bool(sat.any()) and bool((got[sat] == p.tw['off'][sat]).all()), f'{label}: a saturated offset is not +-scale'
        if 'dO' in p.outs:
            B, G, HW = cs['B'], cs['G'], cs['HW']
            flat = (p.bufs['off'].init[GUARD:-GUARD].double().reshape(B, G, HW, 2).abs() == cs['scale']).all(-1)
            dO = value(p, after, 'dO').double().permute(0, 2, 1, 3)[flat]
            assert dO.numel() > 0 and not bool((dO != 0).any()), f'{label}: dO is not exactly zero behind a saturated tanh'
        return
    if p.kind != 'bwd':
        return
    dead = ~p.R['_passes']
    got, start = value(p, after, 'doff'), (p.start['doff'].float() if 'doff' in p.start else torch.zeros(p.outs['doff']))
    wrong = dead & (got != start)
    assert not bool(wrong.any()), (f'{label}: doff moved at {int(wrong.sum())} (key, component) places where no alpha passes a gradient, first at '
                                   f'(b, g, key, component) {tuple(wrong.nonzero()[0].tolist())}')
    if cs['marked']:
        assert bool(dead[:, FAR].all()) and int(dead[:, LATTICE].sum()) >= cs['HW'] and not bool(dead[:, LATTICE].all()), 'the marked groups are not what they claim'
        got, start = value(p, after, 'dtable')[:, :, FAR], p.start['dtable'].float()[:, :, FAR]
        assert torch.equal(bits(got.contiguous()), bits(start.contiguous())), f'{label}: the far group changed its column of dtable'
