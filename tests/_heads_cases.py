"""The output heads (stj_outconv_fwd, stj_outconv_pair_fwd, stj_outconv_bwd, stj_upconv_fwd_head, stj_outconv_pair_gather, stj_outconv_pair_gather_q;
csrc/conv.hip, csrc/conv_ws.hip): float64 statements from the header formulas, a plain Python copy of the launchers' dispatch conditions with
the launch facts the rows are chosen for, the case tables with the kernel each row is meant to reach, the judgement, and the mutants the
judgement must reject.  No GPU is needed to import or test this module (test_heads_ref.py); test_heads_abi_gpu.py runs the tables through the
C ABI.  The helpers of the up-conv twins (_upconv_cases.py, _upconv_fwd_cases.py) are used, not copied.

Layouts: X, dX [F,H,W,C] (T), zero outside the map; W, dW f32 [3,3,C,2], taps (ky,kx); bias, db f32 [2]; frames f = b*Tn + t or t*B + b.
    fwd     Y[f/Tn, f%Tn, y, x, o] = bias[o] + sum_{ky,kx,c} W[ky,kx,c,o] X[f,y+ky-1,x+kx-1,c], the element at
            Y + (f/Tn) y_bstride + (f%Tn) y_tstride + (y W + x) y_pstride + o; every other element of Y untouched.  (t-major callers hand
            Tn = B and the two strides exchanged, as ops._OutConvPair does.)
    pair    channel 4t + 2h + o of a contiguous [B,H,W,32]
    bwd     dX[f,y,x,c] = elu'(X) sum_{ky,kx,o} dY[.,y-ky+1,x-kx+1,o] W[ky,kx,c,o];  dW[ky,kx,c,o] += sum_{f,y,x} X[f,y+ky-1,x+kx-1,c] dY[f,y,x,o];
            db[o] += sum dY;  elu'(x) = x > 0 ? 1 : x + 1, and 1 when elu_in == 0
    head    Z[f,q,2(3ky+kx)+o] = RN_T(sum_c RN_T(Wh[ky,kx,c,o]) RN_T(ELU(pre[f,q,c]))), pre = _upconv_fwd_cases.fwd_pre;  Z[...,18:20] = +0
    gather  Y[b,y,x,4t+2h+o] = bias_h[o] + sum_{ky,kx} Z_h[f,y+ky-1,x+kx-1,2(3ky+kx)+o];  gather_q: the bytes of stj_quantize_waypoints of that Y

Judgement, per row and element type, on two data sets:
  * exact twin: X, dY, W, Wh, bias from {-1, 0, 1} (under elu_in X from {-0.5, 0, 1, 2}); every f32 partial sum is an exact integer or
    half-integer (|sum| <= 9*C + 1 forward, <= 18 for dX; dW, db far below 2^24), so Y, dW, db and the gather's Y must EQUAL the statement
    and dX RN_T of it; dW and db start from non-zero integers, ws from NaN pattern.  For Z the operands are non-negative and sparse: pre >= 0
    and pre, z are integers T represents (<= 256 in bf16, 2048 in fp16; test_heads_ref.py asserts the maxima), Z must EQUAL, 18-19 bitwise +0.
  * random twin: +-U[0.25, 1) rounded to T (W, Wh: f32 values T represents, scaled by 0.05 for the head's up-conv kernel; dY likewise, the
    MFMA backward packs it to bf16); per element |got - ref| <= gate(path, T) * S, S the same statement on absolute operands without elu'.
    gate: EPS_ELEM[T] of test_ops_gpu.py -- and EPS_ELEM[float32] where the output is f32 (Y, dW, db: exact products of T values summed in
    f32, the case EPS_ELEM[float32] is stated for) -- or four times the measured ratio where that is smaller (MEASURED).
Every operand and output lies between GUARD NaN-pattern elements in a flat buffer; outputs start as pattern and the judgement takes the flat
buffer with the positions the statement writes: an unwritten element, a write anywhere else or a touched guard fails it.
"""
import zlib

import torch

from _upconv_cases import ALL, BF16, BIG, F16, F32, F64, GUARD, bits, case_id, cdiv, draw_on, pad_ring, pattern, prep_ref   # noqa: F401
from _upconv_fwd_cases import B16, EPS_ELEM, U_T, elu, elu_prime, fwd_pre                                           # noqa: F401

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
U_ROUND = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}          # unit round-off: the kernel's own rounding of an unrounded W
F32_OUT = ('FM', 'FG', 'PAIR', 'GATHER', 'BM/dW', 'BG/dW')              # paths whose judged output is f32
PATHS = F32_OUT + ('BM/dX', 'BG/dX', 'HEAD')
Z_LIMIT = {BF16: 256, F16: 2048}
OCB_WS_BYTES = 768 * (9 * 48 * 2 + 2) * 4                               # stj_outconv_bwd_workspace_bytes()

# Largest |err| / S of the random twin per (path, element type) over two runs on an MI355X (dW and db arrive through atomics, whose order
# differs from run to run: 8.7e-09 and 1.1e-08 on BM/dW), over the path's rows, head offsets and elu_in modes (the run with
# an unrounded W has its own bound and is not in it); profiles/test_heads_ratios.txt is a later run under the gates these give.  What sets
# the ratio: f32 outputs (Y, dW, db) are exact products summed in f32 -- the order of the sums, far below 2^-17 of sum |terms|, so every
# such gate is four times its own figure; dX is one rounding of the stored result, up to the unit round-off 2^-8 (bf16) / 2^-11 (fp16) of an
# element that is a single term, which leaves those gates at EPS_ELEM; Z is two roundings (ELU(pre) and z), small against sum |terms|.
MEASURED = {
    ('FM', 'bfloat16'): 1.311e-08, ('FM', 'float16'): 4.369e-08,
    ('FG', 'bfloat16'): 1.287e-08, ('FG', 'float16'): 1.377e-07, ('FG', 'float32'): 2.111e-07,
    ('PAIR', 'bfloat16'): 1.542e-08, ('PAIR', 'float16'): 4.507e-08,
    ('GATHER', 'bfloat16'): 7.447e-08, ('GATHER', 'float16'): 7.388e-08,
    ('HEAD', 'bfloat16'): 2.100e-04, ('HEAD', 'float16'): 2.666e-05,
    ('BM/dX', 'bfloat16'): 3.800e-03, ('BM/dW', 'bfloat16'): 1.124e-08,
    ('BG/dX', 'bfloat16'): 3.291e-03, ('BG/dX', 'float16'): 4.455e-04, ('BG/dX', 'float32'): 1.698e-07,
    ('BG/dW', 'bfloat16'): 9.441e-09, ('BG/dW', 'float16'): 1.194e-07, ('BG/dW', 'float32'): 1.343e-07,
}


def bound(path, dt):
    return EPS_ELEM[F32] if path in F32_OUT else EPS_ELEM[dt]


def gate(path, dt):
    """the bound, or four times the measured ratio where that is smaller (the rule of _upconv_cases.GATE)"""
    m = MEASURED.get((path, case_id(dt)))
    return 4 * m if m is not None and 4 * m < bound(path, dt) else bound(path, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# statements (float64, on whatever device the operands are on)
# ---------------------------------------------------------------------------------------------------------------------------------------
def conv3_from_padded(Xp, W):
    """[F,H,W,2] = sum_{ky,kx,c} W[ky,kx,c,o] Xp[f,y+ky,x+kx,c] from the ringed map Xp [F,H+2,W+2,C]"""
    F, Hp, Wp, C = Xp.shape
    H, Wd = Hp - 2, Wp - 2
    out = Xp.new_zeros(F, H, Wd, 2)
    for ky in range(3):
        for kx in range(3):
            out += (Xp[:, ky:ky + H, kx:kx + Wd].reshape(-1, C) @ W[ky, kx]).view(F, H, Wd, 2)
    return out


def fwd_ref(X, W, bias):
    return conv3_from_padded(pad_ring(X.double()), W.double()) + bias.double()


def dx_sum(G, W):
    """sum_{ky,kx,o} G[f,y-ky+1,x-kx+1,o] W[ky,kx,c,o]: [F,H,W,C] from the head's gradient G [F,H,W,2]"""
    F, H, Wd, _ = G.shape
    Gp, W = pad_ring(G.double()), W.double()
    out = G.new_zeros(F, H, Wd, W.shape[2], dtype=F64)
    for ky in range(3):
        for kx in range(3):
            out += (Gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + Wd].reshape(-1, 2) @ W[ky, kx].t()).view(F, H, Wd, -1)
    return out


def dw_sum_from_padded(Xp, G):
    F, H, Wd, _ = G.shape
    C = Xp.shape[3]
    Gm = G.double().reshape(-1, 2)
    dW = Xp.new_zeros(3, 3, C, 2)
    for ky in range(3):
        for kx in range(3):
            dW[ky, kx] = Xp[:, ky:ky + H, kx:kx + Wd].reshape(-1, C).t() @ Gm
    return dW


def dw_sum(X, G):
    return dw_sum_from_padded(pad_ring(X.double()), G)


def frames_to_pair(y, B, t_major):
    """[F,H,W,2] of one head -> [B,H,W,8,2] (waypoint, o)"""
    F, H, Wd, _ = y.shape
    v = y.view(8, B, H, Wd, 2).permute(1, 2, 3, 0, 4) if t_major else y.view(B, 8, H, Wd, 2).permute(0, 2, 3, 1, 4)
    return v


def pair_of(y0, y1, B, t_major):
    """contiguous [B,H,W,32], channel 4t + 2h + o, from the two heads' [F,H,W,2]"""
    v = torch.stack((frames_to_pair(y0, B, t_major), frames_to_pair(y1, B, t_major)), dim=4)          # [B,H,W,8,2(h),2(o)]
    return v.reshape(v.shape[0], v.shape[1], v.shape[2], 32)


def head_proj(y48, Wh):
    """[...,18] = sum_c Wh[ky,kx,c,o] y48[...,c] at channel 2(3ky+kx)+o"""
    return y48 @ Wh.double().reshape(9, 48, 2).permute(1, 0, 2).reshape(48, 18)


def head_ref(X, Wf, bias, Wh, dt):
    """(Z [F,2Hi,2Wi,20] float64 of T values, S, pre)"""
    pre = fwd_pre(X, Wf, bias)
    y = elu(pre).to(dt).double()
    z = head_proj(y, Wh.to(dt)).to(dt).double()
    Z = z.new_zeros(*z.shape[:3], 20)
    Z[..., :18] = z
    S = Z.new_zeros(Z.shape)
    S[..., :18] = head_proj(fwd_pre(X.abs(), Wf.abs(), bias.abs()), Wh.abs())
    return Z, S, pre


def gather_taps(Z):
    """[F,H,W,2] = sum_{ky,kx} Z[f,y+ky-1,x+kx-1,2(3ky+kx)+o]; channels 18, 19 are never read"""
    F, H, Wd, _ = Z.shape
    Zp = pad_ring(Z[..., :18].double())
    out = Zp.new_zeros(F, H, Wd, 2)
    for ky in range(3):
        for kx in range(3):
            k = 2 * (3 * ky + kx)
            out += Zp[:, ky:ky + H, kx:kx + Wd, k:k + 2]
    return out


def gather_ref(Z0, Z1, b0, b1, B, t_major):
    return pair_of(gather_taps(Z0) + b0.double(), gather_taps(Z1) + b1.double(), B, t_major)


# ---------------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors.  Tiles are 16 x 16 pixels (the head epilogue of the up-conv: 8 x 16 low-res pixels).
# ---------------------------------------------------------------------------------------------------------------------------------------
def oc_check(F, H, W, C, Tn):
    """outconv_check of conv.hip"""
    if H % 16 or W % 16 or C % 8 or F < 1 or H < 1 or W < 1 or C < 1 or Tn < 1 or F % Tn:
        return EINVAL
    return OK


def oc_decode(i, tiles_x, tiles_y, F, inner, s_outer, s_inner):
    """oc_decode of conv_ws.hip: work index -> (tx, ty, f)"""
    time_outer = s_outer < s_inner
    nt = F // inner if time_outer else inner
    nb = F // nt
    S = nb * tiles_x * tiles_y
    if nt == 8 and S % 8 == 0:
        c, u, t = i & 7, i >> 6, (i >> 3) & 7
        sp = c + 8 * u
    else:
        t, sp = i % nt, i // nt
    tx, s2 = sp % tiles_x, sp // tiles_x
    ty, b = s2 % tiles_y, s2 // tiles_y
    return tx, ty, (t * inner + b if time_outer else b * inner + t)


def decode_facts(F, H, W, inner, ybs, yts):
    time_outer = ybs < yts
    nt = F // inner if time_outer else inner
    S = F // nt * (H // 16) * (W // 16)
    return dict(decode='swizzled' if nt == 8 and S % 8 == 0 else 'plain', time_outer=time_outer, nt=nt, S=S)


def walk(ntiles, grid):
    """tiles per workgroup (the most) and how many workgroups walk that many"""
    per = cdiv(ntiles, grid)
    return dict(ntiles=ntiles, grid=grid, per=per, full=grid if ntiles % grid == 0 else ntiles % grid)


def mfma_ok(C, H, W, ybs, yts, yps, base_bytes):
    """the shape / stride / alignment part of outconv_fwd_mfma_try and outconv_bwd_mfma_try: float2 at Y + b ybs + t yts + p yps"""
    return C == 48 and H % 16 == 0 and W % 16 == 0 and not ((ybs | yts | yps) & 1) and base_bytes % 8 == 0


def outconv_fwd_geometry(dt, F, H, W, C, Tn, ybs, yts, yps, base_bytes=0, ws_on=True):
    st = oc_check(F, H, W, C, Tn)
    if st:
        return dict(status=st)
    nt = F * (H // 16) * (W // 16)
    if dt in B16 and ws_on and mfma_ok(C, H, W, ybs, yts, yps, base_bytes):
        return dict(status=OK, path='FM', **walk(nt, min(nt, 768)), **decode_facts(F, H, W, Tn, ybs, yts))
    if (18 * 18 * (C + 1) + 9 * C * 2) * 4 > 160 * 1024:
        return dict(status=EUNSUPPORTED)
    if dt not in ALL:
        return dict(status=EINVAL)
    return dict(status=OK, path='FG', **walk(nt, nt), decode=None)


def outconv_bwd_geometry(dt, F, H, W, C, Tn, ybs, yts, yps, base_bytes=0, ws=True, ws_bytes=OCB_WS_BYTES, dW=True, db=True, ws_on=True):
    st = oc_check(F, H, W, C, Tn)
    if st:
        return dict(status=st)
    if not (dW and db):
        return dict(status=EINVAL)
    nt = F * (H // 16) * (W // 16)
    if dt == BF16 and ws_on and mfma_ok(C, H, W, ybs, yts, yps, base_bytes) and ws and ws_bytes >= OCB_WS_BYTES:
        return dict(status=OK, path='BM', **walk(nt, min(nt, 768)), **decode_facts(F, H, W, Tn, ybs, yts))
    if (18 * 18 * (C + 1) + 9 * C * 2 + 18 * 18 * 2) * 4 > 160 * 1024 or 9 * C > 1024:
        return dict(status=EUNSUPPORTED)
    if dt not in ALL:
        return dict(status=EINVAL)
    return dict(status=OK, path='BG', **walk(nt, min(nt, 1024)), decode=None)


def pair_geometry(dt, B, Tn, H, W, C, y_bytes=0, ws_on=True):
    """outconv_pair_fwd_try; per: spatial tiles per workgroup, nb: workgroups"""
    if B <= 0 or Tn <= 0:
        return dict(status=EINVAL)
    if not (dt in B16 and ws_on and C == 48 and Tn == 8 and H % 16 == 0 and W % 16 == 0 and y_bytes % 16 == 0):
        return dict(status=EUNSUPPORTED)
    nsp = B * (H // 16) * (W // 16)
    per = cdiv(nsp, 512)
    return dict(status=OK, path='PAIR', nb=cdiv(nsp, per), **walk(nsp, cdiv(nsp, per)))


def head_geometry(dt, F, Hi, Wi, Cin, Cout, ws_on=True):
    """upconv_check, then upconv_fwd_head_try"""
    vn = 4 if dt == F32 else 8
    if F <= 0 or Hi <= 0 or Wi <= 0 or Cin % vn or Cout % vn:
        return dict(status=EINVAL)
    if not (dt in B16 and ws_on and Cin == 96 and Cout == 48 and Hi % 8 == 0 and Wi % 16 == 0):
        return dict(status=EUNSUPPORTED)
    nt = F * (Hi // 8) * (Wi // 16)
    return dict(status=OK, path='HEAD', **walk(nt, min(nt, 256)))


def gather_geometry(dt, B, Tn, H, W, misaligned=False):
    """outconv_pair_gather_launch (both forms)"""
    if B <= 0 or Tn <= 0:
        return dict(status=EINVAL)
    if not (dt in B16 and Tn == 8 and H % 16 == 0 and W % 16 == 0 and not misaligned):
        return dict(status=EUNSUPPORTED)
    nsp = B * (H // 16) * (W // 16)
    return dict(status=OK, path='GATHER', **walk(nsp, min(nsp, 2048)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes at which each regime exists
# ---------------------------------------------------------------------------------------------------------------------------------------
def _oc(shape, fwd, bwd, note, order='b', yps=32, yts=4, ybs_extra=0, mis=0, offs=(0,), ws='full', raw_w=False):
    """one row of stj_outconv_fwd / stj_outconv_bwd: shape (F,H,W,C,Tn as handed in); fwd / bwd: {element type: path}; order 't': frames
    t*B + b with Tn = B and the strides exchanged; mis: floats the Y / dY base is off a 16-byte boundary; ws: 'full' | 'null' | 'short'"""
    F, H, W, C, Tn = shape
    name = 'x'.join(str(v) for v in shape) + ('-tmajor' if order == 't' else '') + (f'-{note}' if note else '')
    return dict(kind='oc', shape=shape, fwd=fwd, bwd=bwd, name=name, order=order, yps=yps, yts=yts, ybs_extra=ybs_extra, mis=mis, offs=offs,
                ws=ws, raw_w=raw_w, path='oc')


_FM = {BF16: 'FM', F16: 'FM'}
_BM = {BF16: 'BM'}
_FG16, _BG16 = {BF16: 'FG', F16: 'FG'}, {BF16: 'BG', F16: 'BG'}
OC_CASES = [
    _oc((8, 16, 16, 48, 8), _FM, _BM, '', offs=(0, 2), raw_w=True),                 # one tile, every halo edge outside, S = 1
    _oc((16, 32, 48, 48, 8), _FM, _BM, '', offs=(0, 2)),                            # rectangular, S = 12, plain decode
    _oc((8, 32, 64, 48, 8), _FM, _BM, '', offs=(0, 2)),                             # S = 8, swizzled
    _oc((16, 32, 32, 48, 2), _FM, _BM, '', order='t', offs=(0, 2)),                 # strides as ops._OutConvPair passes them, swizzled
    _oc((8, 16, 32, 48, 4), _FM, _BM, '', offs=(0, 2)),                             # nt = 4
    _oc((8, 128, 208, 48, 8), _FM, _BM, '', offs=(0, 2)),                           # 832 tiles on 768 workgroups, swizzled
    _oc((3, 16, 32, 8, 3), {F32: 'FG'}, {F32: 'BG'}, '', yps=12),
    _oc((1, 16, 16, 112, 1), {F32: 'FG'}, {F32: 'BG'}, '', yps=4),                  # largest C both limits admit; it = 3 partial row of dW
    _oc((8, 128, 272, 8, 8), {F32: 'FG'}, {F32: 'BG'}, ''),                         # 1088 tiles: the backward's grid-stride loop
    _oc((2, 16, 32, 40, 2), _FG16, _BG16, '', yps=8),                               # C != 48
    _oc((1, 16, 16, 48, 1), _FG16, _BG16, 'pstride3', yps=3, yts=2),                # odd y_pstride: the third element stays pattern
    _oc((8, 16, 16, 48, 8), _FG16, _BG16, 'base4', mis=1),                          # Y / dY 4 bytes off
    _oc((8, 16, 16, 48, 8), {}, {BF16: 'BG'}, 'wsnull', ws='null'),
    _oc((8, 16, 16, 48, 8), {}, {BF16: 'BG'}, 'wsshort', ws='short'),
    _oc((8, 16, 16, 48, 8), {}, {F16: 'BG'}, 'f16bwd'),
    _oc((2, 16, 16, 48, 2), _FG16, _BG16, 'tstride5', yps=12, yts=5),               # odd y_tstride: generic (the mfma_try conditions)
    _oc((4, 16, 16, 48, 2), _FG16, _BG16, 'bstrideodd', yps=12, ybs_extra=1),       # odd y_bstride: generic
]


def _row(kind, path, shape, note=''):
    return dict(kind=kind, path=path, shape=shape, name='x'.join(str(v) for v in shape) + (f'-{note}' if note else ''), dts=B16, nan=note == 'nan1819')


PAIR_CASES = [_row('pair', 'PAIR', s) for s in ((1, 16, 16, 0), (2, 32, 48, 1), (3, 16, 32, 0), (3, 144, 304, 1))]        # (B,H,W,t_major)
HEAD_CASES = [_row('head', 'HEAD', s) for s in ((1, 8, 16), (3, 16, 48), (3, 56, 208))]                                  # (F,Hi,Wi), 96 -> 48
GATHER_CASES = [_row('gather', 'GATHER', s) for s in ((1, 16, 16, 0), (2, 32, 48, 1), (3, 16, 32, 0), (2, 400, 656, 0))] + \
               [_row('gather', 'GATHER', (2, 32, 48, 1), 'nan1819')]
ELU_MODES = (0, 1)


def oc_rows(which):
    return [(cs, dt) for cs in OC_CASES for dt in cs[which]]


def rows(table):
    return [(cs, dt) for cs in table for dt in cs['dts']]


def strides(cs):
    """(y_bstride, y_tstride, y_pstride) as handed to the entry point, and the elements of the Y / dY tensor"""
    F, H, W, C, Tn = cs['shape']
    img = H * W * cs['yps'] + cs['ybs_extra']
    if cs['order'] == 't':
        return (cs['yts'], img, cs['yps']), Tn * img
    return (img, cs['yts'], cs['yps']), F // Tn * img


def oc_geometry(cs, dt, which, off=0):
    (ybs, yts, yps), _ = strides(cs)
    base = 4 * (cs['mis'] + off)
    if which == 'fwd':
        return outconv_fwd_geometry(dt, *cs['shape'], ybs, yts, yps, base)
    return outconv_bwd_geometry(dt, *cs['shape'], ybs, yts, yps, base, ws=cs['ws'] != 'null',
                                ws_bytes=OCB_WS_BYTES - (1 if cs['ws'] == 'short' else 0))


def geometry(cs, dt):
    s = cs['shape']
    if cs['kind'] == 'pair':
        return pair_geometry(dt, s[0], 8, s[1], s[2], 48)
    if cs['kind'] == 'head':
        return head_geometry(dt, s[0], s[1], s[2], 96, 48)
    return gather_geometry(dt, s[0], 8, s[1], s[2])


def y_index(cs, off, device='cpu'):
    """int64 [F,H,W,2]: the position in the flat Y / dY tensor of element (f, y, x, o) of a head at channel offset off"""
    F, H, W, C, Tn = cs['shape']
    (ybs, yts, yps), _ = strides(cs)
    f = torch.arange(F, device=device)
    base = (f // Tn) * ybs + (f % Tn) * yts + off + cs['mis']
    return (base.view(F, 1, 1) + (torch.arange(H * W, device=device) * yps).view(1, H * W, 1) + torch.arange(2, device=device).view(1, 1, 2)).view(F, H, W, 2)


def y_numel(cs):
    return strides(cs)[1] + cs['mis']


def frames_px(cs):
    s = cs['shape']
    if cs['kind'] == 'oc':
        return s[0] * s[1] * s[2]
    if cs['kind'] == 'head':
        return s[0] * 4 * s[1] * s[2]
    return 16 * s[0] * s[1] * s[2]


def on_device(cs):
    """rows whose statement is evaluated on float64 device tensors: more than BIG output pixels over all frames"""
    return frames_px(cs) > BIG


# ---------------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seed(cs, dt, exact, salt=0):
    return (zlib.crc32(f"{cs['kind']}{cs['shape']}".encode()) & 0xFFFFFF) + 1000003 * salt + 2 * ALL.index(dt) + int(exact)


def _val(dev, n, dt, seed, exact, scale=1.0):
    """{-1, 0, 1} or +-U[0.25, 1) * scale, values T represents, as f32"""
    return draw_on(dev, n, F32, seed, exact, lim=1, scale=scale).to(dt).float()


def _elu_x(dev, n, dt, seed, exact):
    if exact:
        return torch.tensor([-0.5, 0.0, 1.0, 2.0, 1.0], device=dev)[draw_on(dev, n, F32, seed, True, lim=2).long() + 2].to(dt)
    return elu(draw_on(dev, n, F32, seed, False)).to(dt)


def _sparse01(dev, n, seed, p):
    """1 with probability p, else 0 (f32)"""
    return (draw_on(dev, n, F32, seed, False).abs() < 0.25 + 0.75 * p).float()


class Ops:
    pass


def oc_operands(cs, dt, exact, which, elu_in=0, device='cpu'):
    """X (T) [F,H,W,C]; W f32 [3,3,C,2] of T values (Wraw: before that rounding); bias; bwd: G f32 [F,H,W,2] of T values, dW0, db0"""
    F, H, W, C, Tn = cs['shape']
    s = _seed(cs, dt, exact, 1 + elu_in if which == 'bwd' else 0)
    o = Ops()
    n = F * H * W * C
    o.X = (_elu_x(device, n, dt, s, exact) if elu_in else draw_on(device, n, F32, s, exact, lim=1).to(dt)).view(F, H, W, C)
    o.Wraw = draw_on(device, 18 * C, F32, s + 11, exact, lim=1).view(3, 3, C, 2)
    o.W = o.Wraw.to(dt).float()
    o.bias = _val(device, 2, F32, s + 12, exact)
    if which == 'bwd':
        o.G = _val(device, F * H * W * 2, dt, s + 13, exact).view(F, H, W, 2)
        o.dW0 = draw_on(device, 18 * C, F32, s + 14, exact, lim=3).view(3, 3, C, 2)
        o.db0 = draw_on(device, 2, F32, s + 15, exact, lim=3)
        if exact:                                      # the "+=" shows on every element
            o.dW0 = torch.where(o.dW0 == 0, torch.full_like(o.dW0, 2.0), o.dW0)
            o.db0 = torch.where(o.db0 == 0, torch.full_like(o.db0, 2.0), o.db0)
    return o


def pair_operands(cs, dt, exact, device='cpu'):
    B, H, W, _ = cs['shape']
    s = _seed(cs, dt, exact)
    o = Ops()
    n = 8 * B * H * W * 48
    o.X = [draw_on(device, n, F32, s + h, exact, lim=1).to(dt).view(8 * B, H, W, 48) for h in (0, 1)]
    o.W = [_val(device, 18 * 48, dt, s + 11 + h, exact).view(3, 3, 48, 2) for h in (0, 1)]
    o.bias = [_val(device, 2, F32, s + 21 + h, exact) for h in (0, 1)]
    return o


def head_operands(cs, dt, exact, device='cpu'):
    """X (T) [F,Hi,Wi,96]; Wf (T) = prep_ref(W3) cast; bias f32 [48]; Wh f32 [3,3,48,2] of T values"""
    F, Hi, Wi = cs['shape']
    s = _seed(cs, dt, exact)
    o = Ops()
    n = F * Hi * Wi * 96
    if exact:
        o.X = _sparse01(device, n, s, 1 / 8).to(dt).view(F, Hi, Wi, 96)
        W3 = _sparse01('cpu', 9 * 96 * 48, s + 11, 1 / 24).view(3, 3, 96, 48)
        o.bias = _sparse01(device, 48, s + 12, 1 / 2)
        o.Wh = _sparse01(device, 18 * 48, s + 13, 1 / 8).view(3, 3, 48, 2)
    else:
        o.X = draw_on(device, n, F32, s, False).to(dt).view(F, Hi, Wi, 96)
        W3 = draw_on('cpu', 9 * 96 * 48, F32, s + 11, False, scale=0.05).view(3, 3, 96, 48)
        o.bias = _val(device, 48, F32, s + 12, False)
        o.Wh = _val(device, 18 * 48, dt, s + 13, False).view(3, 3, 48, 2)
    o.Wf = prep_ref(W3)[0].to(dt).to(device)
    return o


def gather_operands(cs, dt, exact, device='cpu'):
    """Z0, Z1 (T) [F,H,W,20], channels 18-19 +0 (the nan row: NaN pattern there); bias f32"""
    B, H, W, _ = cs['shape']
    s = _seed(cs, dt, exact)
    o = Ops()
    o.Z = []
    for h in (0, 1):
        z = draw_on(device, 8 * B * H * W * 20, F32, s + h, exact, lim=1).to(dt).view(8 * B, H, W, 20)
        z[..., 18:] = pattern(1, dt)[0].to(device) if cs['nan'] else 0
        o.Z.append(z)
    o.bias = [_val(device, 2, F32, s + 21 + h, exact) for h in (0, 1)]
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------------
class Ref:
    pass


def oc_reference(o, which, elu_in=0, W=None):
    W = o.W if W is None else W
    R = Ref()
    if which == 'fwd':
        R.Y, R.S = fwd_ref(o.X, W, o.bias), fwd_ref(o.X.abs(), W.abs(), o.bias.abs())
        return R
    Xd = o.X.double()
    R.dX = dx_sum(o.G, W) * (elu_prime(Xd) if elu_in else 1.0)
    R.SdX = dx_sum(o.G.abs(), W.abs())
    R.dW, R.SdW = o.dW0.double() + dw_sum(Xd, o.G), o.dW0.double().abs() + dw_sum(Xd.abs(), o.G.abs())
    R.db, R.Sdb = o.db0.double() + o.G.double().sum((0, 1, 2)), o.db0.double().abs() + o.G.double().abs().sum((0, 1, 2))
    return R


def pair_reference(cs, o):
    B, t_major = cs['shape'][0], cs['shape'][3]
    R = Ref()
    R.Y = pair_of(fwd_ref(o.X[0], o.W[0], o.bias[0]), fwd_ref(o.X[1], o.W[1], o.bias[1]), B, t_major)
    R.S = pair_of(fwd_ref(o.X[0].abs(), o.W[0].abs(), o.bias[0].abs()), fwd_ref(o.X[1].abs(), o.W[1].abs(), o.bias[1].abs()), B, t_major)
    return R


def head_reference(o, dt):
    R = Ref()
    R.Z, R.S, R.pre = head_ref(o.X, o.Wf, o.bias, o.Wh, dt)
    return R


def gather_reference(cs, o):
    B, t_major = cs['shape'][0], cs['shape'][3]
    R = Ref()
    R.Y = gather_ref(o.Z[0], o.Z[1], o.bias[0], o.bias[1], B, t_major)
    R.S = gather_ref(o.Z[0][..., :18].abs(), o.Z[1][..., :18].abs(), o.bias[0].abs(), o.bias[1].abs(), B, t_major)
    return R


# ---------------------------------------------------------------------------------------------------------------------------------------
# judgement.  got / init: the flat buffer [GUARD][tensor][GUARD] after the call and as it started, on the device of the reference.
# ---------------------------------------------------------------------------------------------------------------------------------------
def judge(label, name, got, init, idx, want, S, exact, g, ratios, rn=None, bitwise=None):
    """idx: positions (in the tensor, guards not counted) of the elements the statement writes, want / S their float64 values; every other
    element of the flat buffer, the guards included, must hold its first bits.  exact: got == want (RN_rn of it); else |got - want| <= g S.
    bitwise: (positions, int bits) that must hold exactly these bits (Z's zero channels)"""
    fails = []
    pos = idx.reshape(-1).to(got.device) + GUARD
    own = torch.zeros(got.numel(), dtype=torch.bool, device=got.device)
    own[pos] = True
    changed = (bits(got) != bits(init)) & ~own
    if bool(changed.any()):
        at = int(changed.nonzero()[0]) - GUARD
        fails.append(f'{label}: {name}: {int(changed.sum())} elements outside the statement changed (guards included), first at {at}')
    v, w, S = got[pos].double(), want.reshape(-1).double().to(got.device), (S.to(got.device) if S is not None else None)
    if exact:
        if rn is not None:
            w = w.to(rn).double()
        ne = v != w                                    # NaN != anything: an element nobody wrote differs
        if bool(ne.any()):
            k = int(ne.nonzero()[0])
            fails.append(f'{label}: {name}: {int(ne.sum())} of {ne.numel()} elements differ from the exact result, first #{k} (at {int(pos[k]) - GUARD}): '
                         f'got {float(v[k])}, want {float(w[k])}')
    else:
        r = float(torch.nan_to_num((v - w).abs() / (S.reshape(-1).double() + 1e-300), nan=float('inf')).max())
        ratios[name] = max(r, ratios.get(name, 0.0))
        if not r <= g:
            fails.append(f'{label}: {name}: max |err| / sum |terms| = {r:.3e} over the gate {g:.3e}')
    if bitwise is not None:
        bp, bv = bitwise
        if not bool((bits(got)[bp.reshape(-1).to(got.device) + GUARD] == bv).all()):
            fails.append(f'{label}: {name}: the zero channels do not hold +0 bit for bit')
    return fails


def whole(n, device='cpu'):
    return torch.arange(n, device=device)


def z_zero_index(shape, device='cpu'):
    """positions of channels 18, 19 in a contiguous [F,H,W,20]"""
    n = shape[0] * shape[1] * shape[2]
    return (torch.arange(n, device=device).view(n, 1) * 20 + torch.tensor([18, 19], device=device)).reshape(-1)


def flat_with(n, dt, idx=None, vals=None, device='cpu'):
    """(flat, init): an all-pattern buffer of n elements between guards, and the same with vals (rounded to dt) at positions idx"""
    init = pattern(GUARD + n + GUARD, dt).to(device)
    flat = init.clone()
    if idx is not None:
        flat[idx.reshape(-1) + GUARD] = vals.reshape(-1).to(dt)
    return flat, init


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would leave in its output buffers.  Each returns (name of the output, flat, init, idx, want, S, rn,
# bitwise) for judge() on the exact twin of the row it is made for; kind None: the correct output.
# ---------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ('kykx_transposed', 'dw_convolution', 'tiles_xy_swapped', 'tile_unwritten', 'bt_swapped', 'head_offset_0_for_2', 'elu_dropped',
           'border_wrapped', 'db_tile_missing', 'dw_assigned', 'z_channel18', 'gather_plane_other_branch')
MUTANT_ROW = {'kykx_transposed': ('oc', 1), 'dw_convolution': ('oc', 1), 'tiles_xy_swapped': ('oc', 1), 'tile_unwritten': ('oc', 1),
              'bt_swapped': ('pair', 1), 'head_offset_0_for_2': ('oc', 0), 'elu_dropped': ('oc', 0), 'border_wrapped': ('oc', 0),
              'db_tile_missing': ('oc', 1), 'dw_assigned': ('oc', 0), 'z_channel18': ('head', 0), 'gather_plane_other_branch': ('gather', 1)}
TABLES = {'oc': OC_CASES, 'pair': PAIR_CASES, 'head': HEAD_CASES, 'gather': GATHER_CASES}


def _wrap_ring(X):
    Xp = pad_ring(X)
    Xp[:, 0], Xp[:, -1] = Xp[:, -2].clone(), Xp[:, 1].clone()
    Xp[:, :, 0], Xp[:, :, -1] = Xp[:, :, -2].clone(), Xp[:, :, 1].clone()
    return Xp


def _tiles_swapped(y):
    """every 16 x 16 tile of [F,H,W,2] holds the tile a decode with tiles_x and tiles_y exchanged would have computed there"""
    F, H, W, _ = y.shape
    tx_n, ty_n = W // 16, H // 16
    out = y.clone()
    for l in range(tx_n * ty_n):
        ty, tx = divmod(l, tx_n)
        l2 = ((l // ty_n) * tx_n + l % ty_n) % (tx_n * ty_n)
        sy, sx = divmod(l2, tx_n)
        out[:, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = y[:, 16 * sy:16 * sy + 16, 16 * sx:16 * sx + 16]
    return out


def mutant(kind, dt=BF16):
    """the arguments of judge() (after label) for the exact twin of the mutant's row, wrong in one way (kind None + a row: see correct())"""
    table, k = MUTANT_ROW[kind]
    return produce(TABLES[table][k], dt, kind)


def produce(cs, dt, kind=None, elu_in=1):
    """a list of judge() argument tuples (name, flat, init, idx, want, S, exact, gate, rn, bitwise), the outputs of the row's exact twin as a
    kernel that is wrong in the way `kind` names would leave them (None: as the statement has them)"""
    out = []
    if cs['kind'] == 'oc':
        F, H, W, C, Tn = cs['shape']
        off = cs['offs'][-1]
        if kind in (None, 'kykx_transposed', 'tiles_xy_swapped', 'tile_unwritten', 'head_offset_0_for_2', 'border_wrapped') and cs['fwd']:
            o = oc_operands(cs, dt, True, 'fwd')
            R = oc_reference(o, 'fwd')
            y = R.Y
            if kind == 'kykx_transposed':
                y = fwd_ref(o.X, o.W.transpose(0, 1), o.bias)
            if kind == 'tiles_xy_swapped':
                y = _tiles_swapped(y)
            if kind == 'border_wrapped':
                y = conv3_from_padded(_wrap_ring(o.X.double()), o.W.double()) + o.bias.double()
            idx = y_index(cs, off)
            widx, wy = idx, y
            if kind == 'tile_unwritten':
                keep = torch.ones(F, H, W, 2, dtype=torch.bool)
                keep[F - 1, H - 16:, W - 16:] = False
                widx, wy = idx[keep], y[keep]
            if kind == 'head_offset_0_for_2':
                widx = y_index(cs, 0)
            flat, init = flat_with(y_numel(cs), F32, widx, wy)
            out.append(('Y', flat, init, idx, R.Y, R.S, True, 0.0, None, None))
        if kind in (None, 'dw_convolution', 'elu_dropped', 'db_tile_missing', 'dw_assigned') and cs['bwd']:
            o = oc_operands(cs, dt, True, 'bwd', elu_in)
            R = oc_reference(o, 'bwd', elu_in)
            dX, dW, db = R.dX, R.dW, R.db
            if kind == 'dw_convolution':
                dW = o.dW0.double() + dw_sum(o.X, o.G).flip(0, 1)
            if kind == 'elu_dropped':
                dX = dx_sum(o.G, o.W)
            if kind == 'db_tile_missing':
                db = db - o.G[F - 1, H - 16:, W - 16:].double().sum((0, 1))
            if kind == 'dw_assigned':
                dW = dW - o.dW0.double()
            for name, t, want, S, tdt in (('dX', dX, R.dX, R.SdX, dt), ('dW', dW, R.dW, R.SdW, F32), ('db', db, R.db, R.Sdb, F32)):
                flat, init = flat_with(t.numel(), tdt, whole(t.numel()), t)
                out.append((name, flat, init, whole(t.numel()), want, S, True, 0.0, dt if name == 'dX' else None, None))
    elif cs['kind'] == 'pair':
        o = pair_operands(cs, dt, True)
        R = pair_reference(cs, o)
        y = R.Y
        if kind == 'bt_swapped':
            y = pair_of(fwd_ref(o.X[0], o.W[0], o.bias[0]), fwd_ref(o.X[1], o.W[1], o.bias[1]), cs['shape'][0], 1 - cs['shape'][3])
        flat, init = flat_with(y.numel(), F32, whole(y.numel()), y)
        out.append(('Y', flat, init, whole(y.numel()), R.Y, R.S, True, 0.0, None, None))
    elif cs['kind'] == 'head':
        o = head_operands(cs, dt, True)
        R = head_reference(o, dt)
        z = R.Z.clone()
        if kind == 'z_channel18':
            z[0, 0, 0, 18] = 1.0
        flat, init = flat_with(z.numel(), dt, whole(z.numel()), z)
        out.append(('Z', flat, init, whole(z.numel()), R.Z, R.S, True, 0.0, dt, (z_zero_index(z.shape), 0)))
    else:
        o = gather_operands(cs, dt, True)
        R = gather_reference(cs, o)
        y = R.Y
        if kind == 'gather_plane_other_branch':            # waypoint 3, head 1 summed from branch 0's Z
            y = y.clone()
            y[..., 14:16] = gather_ref(o.Z[0], o.Z[0], o.bias[0], o.bias[1], cs['shape'][0], cs['shape'][3])[..., 14:16]
        flat, init = flat_with(y.numel(), F32, whole(y.numel()), y)
        out.append(('Y', flat, init, whole(y.numel()), R.Y, R.S, True, 0.0, None, None))
    return out


def judge_all(label, outs):
    fails = []
    for name, flat, init, idx, want, S, exact, g, rn, bw in outs:
        fails += judge(label, name, flat, init, idx, want, S, exact, g, {}, rn, bw)
    return fails
