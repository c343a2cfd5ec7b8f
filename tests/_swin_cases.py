"""Cases, flat-buffer layout, float64 references and the judge shared by test_swin_abi_gpu.py (the kernels of csrc/swin_fused.hip through
the C ABI) and test_swin_ref.py (the references and the judge themselves, on the CPU).  Nothing here needs a GPU or the library.

A case is a dict (mcase: one stj_swin_mlp_fwd / _bwd pair, acase: one stj_swin_attn_fwd / _bwd pair).  prepare(cs, dt, kind) lays every
tensor of one call into flat CPU allocations filled with the NaN pattern of test_gemm_gpu.PAT, GUARD elements in front and behind (GUARD
elements are a multiple of 16 bytes in every type: each tensor starts 16-byte aligned).  The "+=" outputs dgamma / dbeta lie as nparts
copies part_stride = C + 32 floats apart, dtable as tparts tight copies; every copy starts from non-zero values and the gaps between the
copies keep the pattern.  The split workspace is not part of a Prep: the GPU module owns one per (M, C).

Inputs: activations of spread ~2 around 0.75; every fifth row is QUIET (0.25 +- 0.03: variance ~4e-4, where eps = 1e-5 moves rstd by 1 %).
Weights in the storage type (the rounded compute copy the kernels see), vectors and the bias table f32.

R64 (reference): the module text in float64 torch -- Gelu modules.py:18-29, Mlp :40-46, WindowAttention.call :103-134 with the relative
    position index of :88-98, drop_path :137-151, the shift mask :189-216 (label image, window_partition, differences -> -100) and
    SwinTransformerBlock.call :225-260 (roll, window_partition :49-55, window_reverse :58-63, roll back) -- gradients by autograd,
    the hand-offs as the header of include/strajnet_hip.h defines them: h = gelu(pre), dpre = dL/dpre, ln = LN(x), dys = dp dy (MLP);
    qkv [B,N,3C] in token order, a = attention output before proj, ln, mean, rstd (attention forward); dqkv = dL/dqkv, dys (backward).
Rdt (twin): the same statement with a hand-written backward, in float64 with rd() applied where the kernels turn an f32 value into the
    storage type T.  rd = identity reproduces R64 and its autograd gradients (test_swin_ref.py).  Rounding points, found in the kernels:
    MLP forward   ln = LN(x) (ln_rows packs the B fragments);  h = gelu(pre) (Chain16::from_acc; pre = b1 + W1^T ln stays f32);  y.
                  The hidden groups' (LDS) and hidden slices' (slab / partial-sum) sums are f32.
    MLP backward  ln (and its store);  dys = dp dy (frag_pack: operand of dh and the store);  h (store only);  dpre = dh gelu'(pre) (from_acc
                  and the store);  dx.  d LN(x), its slice sums, dgamma and dbeta are f32; mean / rstd are recomputed from x in f32.
    attention forward   ln (and the save);  the q|k|v tile in LDS (= the save qkv; bias added in f32 before);  P (from_acc, after the f32
                  softmax);  O (from_acc before proj, and the save a);  y.  The head slices' projection sums are f32.
    attention backward  dys = dp dy;  dO = dys Wproj^T (dO tile in LDS and from_acc);  P and dS in their LDS tiles (dV = P^T dO,
                  dK = dS^T Q, dQ = dS K through from_acc; dS = P (dP - sum P dP) is formed from the f32 P);  the bias-table gradient sums
                  the rounded dS tile in f32;  dq, dk (scaled in f32) and dv into the tile (= dqkv, operand of d LN(x) and the store);  dx.
                  d LN(x) and its slice sums, dtable, dgamma, dbeta are f32; mean / rstd are read as saved.
    The 16-bit GELU (x sigmoid(2u) on v_exp / v_rcp) and __expf are the same functions to ~1e-6 and are not modelled.
judge(): per output tensor and per ROW (a token, a bias-table row, a parameter vector)  ||got[r] - R64[r]|| <= bound[r], the one of
    _xattn_cases.judge:
    f32     bound[r] = tol (max(||R64[r]||, rms_r ||R64[r]||) + sum over copies ||start[r]||)
    16 bit  bound[r] = 2 max(e_twin[r], rms_r e_twin[r]) + the f32 bound,  e_twin[r] = ||Rdt[r] - R64[r]||
            (this rms runs over the LIVE rows, ||R64[r]|| > 1e-20 max_r ||R64[r]||: the rows of a dropped sample are exactly zero in dys, dpre
            and dqkv, and with one shifted 8 x 8 window 176 of the 225 bias-table bins collect only pairs the -100 mask takes to e^-100;
            such rows carry no rounding error and say nothing about the error scale of the rows that are computed.  Counting them, one
            three-element table row of a96_1_8_4's float32 layer-by-layer statement stood at 1.15 of its bf16 bound.  The kernels do not
            need the restriction: with the rms over all rows their largest 16-bit ratio was 0.64 as well, measured once.)
    tol = TOL_FWD = 2e-5 for forward values (y, qkv, a, ln, mean, rstd and the recomputed h, ln, dys of the backward calls), TOL_BWD = 2e-4
    for gradients: _xattn_cases' figures.  K reaches 1536 here instead of 512; the CPU float32 statement of test_swin_ref.py stays at
    ratio <= 0.5 on every case below 32768 rows with them (largest measured: 0.13, on ln, qkv and h), so they are kept.
    For "+=" outputs the SUM over the copies is judged, and with at least as many units (row blocks / windows) as copies more than one
    copy must have changed -- in the cases without DropPath: a unit of dropped rows adds zeros, and where two slices meet inside the
    launch the unit adds into the copy of whichever slice arrives last (block 2u or 2u + 1), so two contributing neighbours may share a
    copy while three cannot (m192_3x80_p with one sample kept changed one copy in one run of four).
    Every element that is no output is bit-identical, no output element (tail rows included) keeps the pattern.

Dispatch table (csrc/swin_fused.hip: mlp_dispatch, attn_dispatch, attn_split384, attnb_192, attnb_split384); 16b = bf16 and fp16:
  MLP   m96_80, m96_3x80_p          16b mlp<T,96,1>            f32 mlp<float,96,1>                         (fwd and bwd kernel each)
        m96_32848                   bf16 mlp<T,96,1,0,8,1,192>  f32 mlp<float,96,2>
        m96_131072                  bf16 mlp<T,96,1,0,8>
        m192_80, _3x80_p, _8192     16b mlp<T,192,1,2,8,2> (two slices meet in the launch)   f32 mlp<float,192,1>
        m192_80_nows, m192_256_nows 16b mlp<T,192,1,0,8,2> (two hidden groups meet in LDS)   f32 (80 only) mlp<float,192,1>
        m192_32848                  bf16 mlp<T,192,1,0,8>      f32 mlp<float,192,2>
        m384_80, _3x80_p, m384_2048 mlp<T,384,1,1> x 8 slices + swin_split_fwd_epi / swin_split_bwd_epi<T,384,2>
        m384_2064, m384_4096        the same x 4 slices
        m384_4112, m384_8176        16b mlp<T,384,1,2> (two slices meet in the launch); f32 mlp<float,384,1,1> x 2 slices + epi
        m384_8272                   16b fwd mlp<T,384,1,1,8> x 4 slices + fwd epi, bwd mlp<T,384,1,2>; f32 as m384_8176
  attn  a96_*                       attn<T,96> / attnb<T,96>
        a192_2_16_4                 16b attn<T,192,2,1> / attnb<T,192,2,1,true>; f32 attn<float,192> / attnb<float,192>
        a192_255w (bf16)            attn<T,192,2,1> / attnb<T,192,2,1,true>
        a192_1_8_4_nows, a192_2_16_0_nows, a192_256w   attn<T,192> (two heads per pass) / attnb<T,192>
        a384_1_8_4, a384_48w        16b attn<T,384,1> x 6 slices + fwd epi / attnb<T,384,6> + bwd epi
        a384_49w, a384_52w_p        16b attn<T,384,2> / attnb<T,384,2,0,true> (two slices of six heads meet in the launch)
        a384_1_8_4, a384_2_16_4 f32 attn<float,384,1> x 6 (KH = 2) + fwd epi / attnb<float,384,6> + bwd epi
  Not covered: the 16-bit C = 384 kernels above 4096 units (forward attn<T,384,1> x 2 slices + epi, MLP backward mlp<T,384,1,1> x 2 + epi):
  the arrival counters hold 4096 units, so these need more than 262144 rows (> 400 MB of f32 partial sums) -- too large for a test.
"""
import math
import zlib

import torch

from test_gemm_gpu import GUARD, bits, draw, pattern
from _xattn_cases import TOL_BWD, TOL_FWD, Prep, report_lines        # noqa: F401  (report_lines: for the two test modules)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL3, B16 = (F32, BF16, F16), (BF16, F16)
EPS = 1e-5
SCALE = 32.0 ** -0.5
PSTRIDE_EXTRA = 32
LIVE_REL = 1e-20           # a row counts for the rms of the twin's error when its reference norm exceeds this share of the largest
FWD_LIKE = ('y', 'qkv', 'a', 'ln', 'mean', 'rstd', 'h', 'dys')
OUTS = {('mlp', 'fwd'): ('y',), ('mlp', 'bwd'): ('dx', 'h', 'dpre', 'ln', 'dys', 'dgamma', 'dbeta'),
        ('attn', 'fwd'): ('y', 'qkv', 'a', 'ln', 'mean', 'rstd'), ('attn', 'bwd'): ('dx', 'dqkv', 'dys', 'dtable', 'dgamma', 'dbeta')}
ADDED = ('dgamma', 'dbeta', 'dtable')
INPUTS = {('mlp', 'fwd'): ('x', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2'), ('mlp', 'bwd'): ('x', 'gamma', 'beta', 'w1', 'b1', 'w2'),
          ('attn', 'fwd'): ('x', 'gamma', 'beta', 'wqkv', 'bqkv', 'table', 'wproj', 'bproj'), ('attn', 'bwd'): ('x', 'gamma', 'wqkv', 'wproj', 'table')}


def mcase(name, C, M, dts=ALL3, ws=True, rps=None, p=0.0, nparts=1):
    rps = rps or M
    assert M % rps == 0 and rps % 16 == 0
    return dict(name=name, half='mlp', C=C, M=M, B=M // rps, rps=rps, dts=dts, ws=ws, p=p, nparts=nparts, tparts=1,
                units=(M + 63) // 64)


def acase(name, C, B, res, shift, dts=ALL3, ws=True, p=0.0, nparts=1, tparts=1):
    return dict(name=name, half='attn', C=C, M=B * res * res, B=B, res=res, shift=shift, rps=res * res, dts=dts, ws=ws, p=p,
                nparts=nparts, tparts=tparts, units=B * (res // 8) ** 2)


def cases():
    big = (BF16, F32)
    out = [mcase('m96_80', 96, 80, nparts=3), mcase('m96_3x80_p', 96, 240, rps=80, p=0.3), mcase('m96_32848', 96, 32848, big, nparts=3),
           mcase('m96_131072', 96, 131072, (BF16,)),
           mcase('m192_80', 192, 80), mcase('m192_3x80_p', 192, 240, rps=80, p=0.3, nparts=3), mcase('m192_8192', 192, 8192, nparts=3),
           mcase('m192_80_nows', 192, 80, ws=False, nparts=3), mcase('m192_256_nows', 192, 256, B16, ws=False),
           mcase('m192_32848', 192, 32848, big, nparts=3)]
    for i, M in enumerate((80, 2048, 2064, 4096, 4112, 8176, 8272)):
        out.append(mcase(f'm384_{M}', 384, M, nparts=(3, 1)[i % 2]))
    out.append(mcase('m384_3x80_p', 384, 240, rps=80, p=0.3))
    out += [acase('a96_1_8_0', 96, 1, 8, 0), acase('a96_1_8_4', 96, 1, 8, 4, nparts=3, tparts=3), acase('a96_2_16_3', 96, 2, 16, 3, tparts=3),
            acase('a96_3_16_4_p', 96, 3, 16, 4, p=0.3, nparts=3),
            acase('a192_2_16_4', 192, 2, 16, 4, nparts=3, tparts=3), acase('a192_255w', 192, 255, 8, 0, (BF16,)),
            acase('a192_1_8_4_nows', 192, 1, 8, 4, B16, ws=False), acase('a192_2_16_0_nows', 192, 2, 16, 0, B16, ws=False, nparts=3, tparts=3),
            acase('a192_256w', 192, 1, 128, 4, (BF16,), tparts=3),
            acase('a384_1_8_4', 384, 1, 8, 4, nparts=3), acase('a384_48w', 384, 3, 32, 4, B16, tparts=3), acase('a384_49w', 384, 49, 8, 0, B16, nparts=3),
            acase('a384_52w_p', 384, 13, 16, 4, B16, p=0.3, nparts=3, tparts=3), acase('a384_2_16_4', 384, 2, 16, 4, (F32,), nparts=3, tparts=3)]
    return out


_CASES = {c['name']: c for c in cases()}
CASE_DT = [(c['name'], dt) for c in cases() for dt in c['dts']]


def case(name):
    return _CASES[name]


def small(cs):
    return cs['M'] < 32768


def case_id(v):
    return v if isinstance(v, str) else str(v).replace('torch.', '')


def cpu_keep(cs, seed=99):
    """any fixed keep flags with one sample kept and one dropped (the GPU tests hand in the ones stj_dropout_mask states)"""
    if not cs['p'] > 0:
        return None
    g = torch.Generator().manual_seed(seed)
    while True:
        k = (torch.rand(cs['B'], generator=g) >= cs['p']).to(torch.uint8)
        if 0 < int(k.sum()) < cs['B']:
            return k


# ------------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def _acts(M, C, dt, g):
    x = draw(M * C, F32, g, False, scale=2.0).reshape(M, C)
    quiet = torch.arange(M) % 5 == 3
    x[quiet] *= 0.015
    x[quiet] += 0.25
    x[~quiet] += 0.75
    return x.to(dt)


def make_inputs(cs, dt):
    """name -> CPU tensor as stored: activations and weight matrices in dt, vectors, table and start values f32"""
    C, M = cs['C'], cs['M']
    g = torch.Generator().manual_seed(4000 + zlib.crc32(cs['name'].encode()) % 100000)
    d = lambda shape, scale=1.0, t=F32: draw(math.prod(shape), t, g, False, scale=scale).reshape(shape)
    I = dict(x=_acts(M, C, dt, g), dy=d((M, C), t=dt), gamma=1.0 + d((C,), 0.3), beta=d((C,), 0.3))
    for n in ('dgamma', 'dbeta'):
        I['start_' + n] = d((cs['nparts'], C))
    if cs['half'] == 'mlp':
        I.update(w1=d((C, 4 * C), 1.5 / math.sqrt(C), dt), b1=d((4 * C,), 0.3), w2=d((4 * C, C), 0.75 / math.sqrt(C), dt), b2=d((C,), 0.3))
    else:
        H = C // 32
        I.update(wqkv=d((C, 3 * C), 1.6 / math.sqrt(C), dt), bqkv=d((3 * C,), 0.2), table=d((225, H), 0.5), wproj=d((C, C), 1.5 / math.sqrt(C), dt),
                 bproj=d((C,), 0.2), start_dtable=d((cs['tparts'], 225 * H)))
    return I


def _f64(I):
    return {k: v.double() for k, v in I.items()}


def dp_rows(cs, keep):
    """[M, 1] float64 DropPath factor of every row: keep / (1 - p) of its sample (modules.py:137-151)"""
    if keep is None:
        return torch.ones(cs['M'], 1, dtype=torch.float64)
    return (keep.double() / (1.0 - cs['p'])).repeat_interleave(cs['rps'])[:, None]


# ------------------------------------------------------------------------------------------------------------------------------------------
# The module text in float64
# ------------------------------------------------------------------------------------------------------------------------------------------
K0 = math.sqrt(2.0 / math.pi)


def gelu(x, erf=False):
    if erf:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x * (0.5 * (1.0 + torch.tanh(K0 * (x + 0.044715 * x ** 3))))


def dgelu(x):
    t = torch.tanh(K0 * (x + 0.044715 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * K0 * (1.0 + 3 * 0.044715 * x * x)


def ln_stats(x, eps=EPS):
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True)
    return m, 1.0 / torch.sqrt(var + eps)


def mlp_graph(D, dp, fault=None):
    """x + drop_path(fc2(gelu(fc1(norm2(x)))));  fault: a single error for test_swin_ref.py's judge test"""
    x = D['x']
    m, r = ln_stats(x, 0.0 if fault == 'eps' else EPS)
    T = dict(ln=(x - m) * r * D['gamma'] + D['beta'])
    T['pre'] = T['ln'] @ D['w1'] + D['b1']
    T['h'] = gelu(T['pre'], erf=fault == 'erf')
    T['t'] = T['h'] @ D['w2'] + D['b2']
    if fault == 'hidden_twice':
        T['t'] = T['t'] + T['h'][:, :96] @ D['w2'][:96]
    T['y'] = x + dp * T['t']
    return T


def relative_position_index():
    c = torch.stack(torch.meshgrid(torch.arange(8), torch.arange(8), indexing='ij')).reshape(2, -1)
    rc = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).clone()
    rc[:, :, 0] += 7
    rc[:, :, 1] += 7
    rc[:, :, 0] *= 15
    return rc.sum(-1)


def window_partition(t):
    B, H, W, C = t.shape
    return t.reshape(B, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 8, C)


def window_reverse(w, H, W):
    C = w.shape[-1]
    return w.reshape(-1, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, H, W, C)


def shift_mask(res, shift, fault=None):
    img = torch.zeros(1, res, res, 1, dtype=torch.float64)
    sl = (slice(0, -8), slice(-8, -shift), slice(-shift, None))
    cnt = 0
    for h in sl:
        for w in sl:
            img[:, h, w, :] = cnt
            cnt += 1
    if fault == 'label':                       # in the last window row, region 5 takes the label of its left neighbour
        img[:, sl[1], sl[2], :] = 4
    mw = window_partition(img).reshape(-1, 64)
    am = mw[:, None, :] - mw[:, :, None]
    return torch.where(am != 0, torch.full_like(am, -100.0), torch.zeros_like(am))


def to_windows(t, B, res, shift):
    t = t.reshape(B, res, res, -1)
    if shift > 0:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    return window_partition(t).reshape(-1, 64, t.shape[-1])


def from_windows(w, B, res, shift, fault=None):
    t = window_reverse(w.reshape(-1, 8, 8, w.shape[-1]), res, res)
    if shift > 0:
        s = -shift if fault == 'roll_back' else shift
        t = torch.roll(t, shifts=(s, s), dims=(1, 2))
    return t.reshape(B * res * res, -1)


def _split_heads(w, H):
    """[nWB, 64, 3C] -> q, k, v [nWB, H, 64, 32]"""
    q = w.reshape(w.shape[0], 64, 3, H, 32).permute(2, 0, 3, 1, 4)
    return q[0], q[1], q[2]


def _logits(cs, q, k, table, fault=None):
    H, res, shift = cs['C'] // 32, cs['res'], cs['shift']
    idx = relative_position_index()
    if fault == 'swap_qk':
        idx = idx.t()
    bias = table[idx.reshape(-1)].reshape(64, 64, H).permute(2, 0, 1)
    s = (q * SCALE) @ k.transpose(-1, -2) + bias[None]
    if shift > 0:
        nW = (res // 8) ** 2
        s = (s.reshape(-1, nW, H, 64, 64) + shift_mask(res, shift, fault)[None, :, None]).reshape(-1, H, 64, 64)
    return s


def attn_graph(cs, D, dp, fault=None):
    """x + drop_path(roll(window_reverse(WindowAttention(window_partition(roll(norm1(x)))))));  rows [M = B N, C]"""
    B, res, shift, C = cs['B'], cs['res'], cs['shift'], cs['C']
    x = D['x']
    m, r = ln_stats(x, 0.0 if fault == 'eps' else EPS)
    T = dict(mean=m, rstd=r, ln=(x - m) * r * D['gamma'] + D['beta'])
    T['qkv'] = T['ln'] @ D['wqkv'] + D['bqkv']
    q, k, v = _split_heads(to_windows(T['qkv'], B, res, shift), C // 32)
    T['P'] = torch.softmax(_logits(cs, q, k, D['table'], fault), -1)
    o = (T['P'] @ v).permute(0, 2, 1, 3).reshape(-1, 64, C)
    T['a'] = from_windows(o, B, res, shift, fault)
    a = T['a']
    if fault == 'head_dropped':                  # the projection loses the share of heads 0 and 1
        a = torch.cat([torch.zeros_like(a[:, :64]), a[:, 64:]], 1)
    T['t'] = a @ D['wproj'] + D['bproj']
    T['y'] = x + dp * T['t']
    return T


def r64(cs, I, keep, fault=None, dp=None):
    """name -> float64 value of every output of the case's two entry points (the "+=" outputs WITHOUT their start values)"""
    D = _f64(I)
    leaves = ('x', 'gamma', 'beta') + (('table',) if cs['half'] == 'attn' else ())
    for n in leaves:
        D[n] = D[n].clone().requires_grad_(True)
    dp = dp_rows(cs, keep) if dp is None else dp
    T = mlp_graph(D, dp, fault) if cs['half'] == 'mlp' else attn_graph(cs, D, dp, fault)
    mids = ('pre', 't') if cs['half'] == 'mlp' else ('qkv', 't')
    for n in mids:
        T[n].retain_grad()
    (T['y'] * D['dy']).sum().backward()
    out = dict(y=T['y'], ln=T['ln'], dx=D['x'].grad, dys=T['t'].grad, dgamma=D['gamma'].grad[None], dbeta=D['beta'].grad[None])
    if cs['half'] == 'mlp':
        out.update(h=T['h'], dpre=T['pre'].grad, _pre=T['pre'])
    else:
        out.update(qkv=T['qkv'], a=T['a'], mean=T['mean'], rstd=T['rstd'], dqkv=T['qkv'].grad, dtable=D['table'].grad, _P=T['P'])
    return {k: v.detach() for k, v in out.items()}


def _ln_bwd(dln, xh, r, gamma):
    a = dln * gamma
    return r * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))


def twin(cs, I, keep, rd, saves=None):
    """The statement as the kernels evaluate it (see the module docstring for the rounding points), backward written by hand.
    saves (attention): dict qkv, mean, rstd the backward reads instead of this function's own forward."""
    D = _f64(I)
    x, dy, gamma, beta = D['x'], D['dy'], D['gamma'], D['beta']
    dp = dp_rows(cs, keep)
    m, r = ln_stats(x)
    ln = rd((x - m) * r * gamma + beta)
    dys = rd(dp * dy)
    out = dict(ln=ln, dys=dys)
    if cs['half'] == 'mlp':
        pre = ln @ D['w1'] + D['b1']
        h = rd(gelu(pre))
        dpre = rd((dys @ D['w2'].t()) * dgelu(pre))
        dln = dpre @ D['w1'].t()
        xh = (x - m) * r
        out.update(y=rd(x + dp * (h @ D['w2'] + D['b2'])), h=h, dpre=dpre, dx=rd(dy + _ln_bwd(dln, xh, r, gamma)),
                   dgamma=(dln * xh).sum(0)[None], dbeta=dln.sum(0)[None])
        return out
    B, res, shift, C = cs['B'], cs['res'], cs['shift'], cs['C']
    H = C // 32
    qkv = rd(ln @ D['wqkv'] + D['bqkv'])
    q, k, v = _split_heads(to_windows(qkv, B, res, shift), H)
    P = torch.softmax(_logits(cs, q, k, D['table']), -1)
    a = rd(from_windows((rd(P) @ v).permute(0, 2, 1, 3).reshape(-1, 64, C), B, res, shift))
    out.update(qkv=qkv, a=a, mean=m, rstd=r, y=rd(x + dp * (a @ D['wproj'] + D['bproj'])))
    # backward
    if saves is not None:
        qkv, m, r = (saves[n].double().reshape(s.shape) for n, s in (('qkv', qkv), ('mean', m), ('rstd', r)))
        q, k, v = _split_heads(to_windows(qkv, B, res, shift), H)
        P = torch.softmax(_logits(cs, q, k, D['table']), -1)
    dO = rd(dys @ D['wproj'].t())
    dO = to_windows(dO, B, res, shift).reshape(-1, 64, H, 32).permute(0, 2, 1, 3)
    dP = dO @ v.transpose(-1, -2)
    dS = rd(P * (dP - (P * dP).sum(-1, keepdim=True)))
    Pr = rd(P)
    dq, dk, dv = rd(SCALE * (dS @ k)), rd(SCALE * (dS.transpose(-1, -2) @ q)), rd(Pr.transpose(-1, -2) @ dO)
    w = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(-1, 64, 3 * C)          # [nWB, 64, (3, H, 32)]
    dqkv = from_windows(w, B, res, shift)
    dtable = torch.zeros(225, H, dtype=torch.float64)
    dtable.index_add_(0, relative_position_index().reshape(-1), dS.sum(0).permute(1, 2, 0).reshape(64 * 64, H))
    dln = dqkv @ D['wqkv'].t()
    xh = (x - m) * r
    out.update(dqkv=dqkv, dtable=dtable, dx=rd(dy + _ln_bwd(dln, xh, r, gamma)), dgamma=(dln * xh).sum(0)[None], dbeta=dln.sum(0)[None])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# One call: buffers, reference, bounds
# ------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """one flat allocation: pattern everywhere, values put at offsets relative to base = GUARD; `spans`: what the call may write"""
    def __init__(self, n, dt):
        self.init, self.n, self.spans = pattern(GUARD + n + GUARD, dt), n, []

    def put(self, off, values):
        self.init[GUARD + off:GUARD + off + values.numel()] = values.reshape(-1).to(self.init.dtype)

    def quiet(self):
        """the (begin, end) ranges of the allocation that no call may change: guards and the gaps between copies"""
        out, at = [], 0
        for b, e in sorted(self.spans):
            out.append((at, GUARD + b))
            at = GUARD + e
        out.append((at, GUARD + self.n + GUARD))
        return [(b, e) for b, e in out if e > b]


_REF = {}


def references(cs, dt, keep, tag):
    """(inputs, R64, Rdt on the reference's saves) of one case and dtype, computed once per process and left unchanged"""
    key = (cs['name'], dt, tag)
    if key not in _REF:
        I = make_inputs(cs, dt)
        R = r64(cs, I, keep)
        if cs['half'] == 'attn':             # a softmax that is neither uniform nor one-hot
            peak = float(R.pop('_P').max(-1).values.mean())
            assert 0.1 <= peak <= 0.7, f'{cs["name"]}: mean max_key P = {peak:.3f}: the attention is uniform or one-hot'
        else:                                # GELU on both sides of zero
            pos = float((R.pop('_pre') > 0).double().mean())
            assert 0.2 <= pos <= 0.8, f'{cs["name"]}: {pos:.2f} of the fc1 pre-activations are positive'
        if cs['p'] > 0:
            assert 0 < int(keep.sum()) < cs['B'], f'{cs["name"]}: DropPath keeps {keep.tolist()}: need one kept and one dropped sample'
        tw = None
        if dt != F32:
            sv = {k: R[k].to(F32 if k != 'qkv' else dt) for k in ('qkv', 'mean', 'rstd')} if cs['half'] == 'attn' else None
            tw = twin(cs, I, keep, lambda t: t.to(dt).double(), sv)
        _REF[key] = (I, R, tw)
    return _REF[key]


def _row_norms(t):
    return t.reshape(-1, t.shape[-1]).norm(dim=1)


def prepare(cs, dt, kind, keep=None, tag='cpu', with_saves=True, saves_from=None, nparts=None, tparts=None):
    """kind 'fwd' / 'bwd'.  keep: the DropPath keep flags [B] when cs['p'] > 0 (default: cpu_keep).  with_saves False: the inference form
    of the attention forward.  saves_from: dict qkv, mean, rstd the attention backward is handed instead of the reference's (forward into
    backward; the twin is then evaluated end to end).  nparts / tparts: override the case's (the start values are cut or repeated)."""
    assert kind in ('fwd', 'bwd')
    if cs['p'] > 0 and keep is None:
        keep, tag = cpu_keep(cs), 'cpu'
    I, R, tw = references(cs, dt, keep if cs['p'] > 0 else None, tag)
    C, M, half = cs['C'], cs['M'], cs['half']
    p = Prep()
    p.cs, p.dt, p.kind, p.I, p.R, p.keep, p.bufs, p.outs, p.with_saves = cs, dt, kind, I, R, keep if cs['p'] > 0 else None, {}, {}, with_saves
    p.nparts, p.tparts, p.pstride = nparts or cs['nparts'], tparts or cs['tparts'], C + PSTRIDE_EXTRA
    if dt != F32 and saves_from is not None:
        key = (cs['name'], dt, tag, 'e2e')
        if key not in _REF:
            _REF[key] = twin(cs, I, p.keep, lambda t: t.to(dt).double())
        tw = _REF[key]
    p.tw, p.start = tw, {}

    def tensor(name, shape, t, values=None, out=False):
        n = math.prod(shape)
        b = p.bufs[name] = Buf(n, t)
        if values is not None:
            b.put(0, values)
        if out:
            b.spans.append((0, n))
            p.outs[name] = (name, [0], n // shape[-1], shape[-1])

    def added(name, ncopy, stride, rows, width):
        b = p.bufs[name] = Buf((ncopy - 1) * stride + rows * width, F32)
        st = I['start_' + name]
        st = st[torch.arange(ncopy) % st.shape[0]].clone()
        for c in range(ncopy):
            b.put(c * stride, st[c])
            b.spans.append((c * stride, c * stride + rows * width))
        p.outs[name] = (name, [c * stride for c in range(ncopy)], rows, width)
        p.start[name] = st.double().reshape(ncopy, rows, width)

    for n in INPUTS[half, kind]:
        tensor(n, I[n].shape, I[n].dtype, I[n])
    if kind == 'fwd':
        tensor('y', (M, C), dt, out=True)
        if half == 'attn' and with_saves:
            for n, w, t in (('qkv', 3 * C, dt), ('a', C, dt), ('ln', C, dt), ('mean', 1, F32), ('rstd', 1, F32)):
                tensor(n, (M, w), t, out=True)
    else:
        tensor('dy', (M, C), dt, I['dy'])
        tensor('dx', (M, C), dt, out=True)
        tensor('dys', (M, C), dt, out=True)
        if half == 'mlp':
            for n, w in (('h', 4 * C), ('dpre', 4 * C), ('ln', C)):
                tensor(n, (M, w), dt, out=True)
        else:
            S = saves_from if saves_from is not None else {k: R[k] for k in ('qkv', 'mean', 'rstd')}
            tensor('qkv', (M, 3 * C), dt, S['qkv'])
            tensor('mean', (M, 1), F32, S['mean'])
            tensor('rstd', (M, 1), F32, S['rstd'])
            tensor('dqkv', (M, 3 * C), dt, out=True)
            added('dtable', p.tparts, 225 * (C // 32), 225, C // 32)
        added('dgamma', p.nparts, p.pstride, 1, C)
        added('dbeta', p.nparts, p.pstride, 1, C)
    # bounds
    p.bound = {}
    for n in p.outs:
        ref = R[n].reshape(-1, p.outs[n][3])
        norms = _row_norms(ref)
        b = torch.maximum(norms, (norms ** 2).mean().sqrt())
        if n in ADDED:
            b = b + p.start[n].norm(dim=2).sum(0)
        b = (TOL_FWD if n in FWD_LIKE else TOL_BWD) * b
        if dt != F32:
            e = _row_norms(tw[n].reshape(ref.shape) - ref)
            live = norms > LIVE_REL * norms.max()         # (see the module docstring: rows the statement leaves at zero)
            b = 2.0 * torch.maximum(e, (e[live] ** 2).mean().sqrt() if bool(live.any()) else e) + b
        p.bound[n] = b
    return p


def copies(p, after, name):
    """[ncopy, rows, width]: every copy of output `name` as the call left it"""
    bname, offs, rows, width = p.outs[name]
    return torch.stack([after[bname][GUARD + o:GUARD + o + rows * width].reshape(rows, width) for o in offs])


def expected(p, name):
    """[rows, width] float64: R64 of the output (the sum of the start values of its copies included)"""
    ref = p.R[name].reshape(-1, p.outs[name][3])
    return ref + p.start[name].sum(0) if name in ADDED else ref


def judge(p, after, ratios=None, label=''):
    """after: name -> the flat CPU buffer as the call left it.  Raises AssertionError; appends (kind, dtype, output, case, largest e / bound)."""
    cs = p.cs
    label = f"{cs['name']} {p.kind}{'' if p.with_saves else ' (no saves)'}{label}"
    for name, b in p.bufs.items():
        for lo, hi in b.quiet():
            bad = (bits(after[name][lo:hi]) != bits(b.init[lo:hi])).nonzero()
            assert bad.numel() == 0, f'{label}: {bad.numel()} elements of {name} outside the outputs changed, first at flat index {lo + int(bad[0]) - GUARD}'
    for name in p.outs:
        raw = copies(p, after, name)
        left = bits(raw) == int(bits(pattern(1, raw.dtype))[0])
        assert not bool(left.any()), f'{label}: {int(left.sum())} elements of {name} still hold the fill pattern, first at (copy, row, column) {tuple(left.nonzero()[0].tolist())}'
        if raw.shape[0] > 1 and cs['units'] >= raw.shape[0] and p.keep is None:
            moved = int((raw.double() != p.start[name]).flatten(1).any(1).sum())
            assert moved > 1, f'{label}: {name}: {moved} of {raw.shape[0]} copies changed with {cs["units"]} units'
        err = (raw.double().sum(0) - expected(p, name)).norm(dim=1)
        ok = err <= p.bound[name]            # False for NaN
        ratio = float((err / (p.bound[name] + 1e-300)).nan_to_num(nan=float('inf')).max())
        if ratios is not None:
            ratios.append((f'{cs["half"]} {p.kind}', case_id(p.dt), name, cs['name'], ratio))
        assert bool(ok.all()), (f'{label}: {name}: {int((~ok).sum())} of {ok.numel()} rows over their bound, largest ||err|| / bound = {ratio:.3e}, '
                                f'first row {int((~ok).nonzero()[0])}')
