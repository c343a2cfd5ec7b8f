"""The up-conv forward and input gradient (stj_upconv_fwd, stj_upconv_fwd_res, stj_upconv_dgrad; csrc/conv.hip, conv_ws.hip, conv_ps.hip):
float64 statements from the header formulas, a plain Python copy of the launchers' dispatch conditions, the case tables with the kernel each
row is meant to reach, the judgement, and the mutated statements the judgement must reject.  No GPU is needed to import or test this module
(test_upconv_fwd_ref.py); test_upconv_fwd_abi_gpu.py runs the tables through the C ABI.  The weight gradient's twin is _upconv_cases.py, whose
prep_ref, pad_ring, upsample_pad, phases and draw helpers are used here.

Layouts (NHWC): X, dX, Xelu [F,Hi,Wi,Cin]   Y, Y2, R1, R2, dP [F,2Hi,2Wi,Cout]   bias f32 [Cout]   Wf [16,Cout,Cin]   Wd [16,Cin,Cout]
Statements, pt = a*8 + b*4 + r*2 + s:
    pre[f,2i+a,2j+b,co] = bias[co] + sum_{r,s,ci} Wf[pt][co][ci] * X[f,i+a-1+r,j+b-1+s,ci]                     (X zero outside the map)
    Y = act(pre), act 0: none, 2: ELU (x > 0 ? x : expm1(x));   res: Y = RN_T(RN_T(ELU(pre)) + R1), Y2 = RN_T(Y + R2)
    dX[f,i,j,ci] = elu'(Xelu[f,i,j,ci]) * sum_{u,v in -1..2} sum_co dP[f,2i+u,2j+v,co] * Wd[(u+1)*4+(v+1)][ci][co]  (dP zero outside the map;
                   elu'(x) = x > 0 ? 1 : x + 1, and 1 when Xelu == NULL)
The kernels are handed Wf / Wd = prep_ref(W) cast to the element type T, so they are judged independently of stj_upconv_prep.

Judgement, per row and element type, on two data sets:
  * exact twin: X, dP, bias, R1, R2 and W (before the fold) from {-1, 0, 1}, Xelu from {-0.5, 0, 1, 2}: |Wf|, |Wd| <= 4, elu' is 0.5 or 1, every
    product and f32 partial sum an exact integer.  Forward: Y EQUALS RN_T(pre) where pre > 0 (everywhere with act 0); where pre <= 0,
    |Y - expm1(pre)| <= 2 u_T |expm1(pre)| + 2^-22.  res: Y2 EQUALS RN_T(Y + R2) of the kernel's own Y everywhere, Y EQUALS
    RN_T(RN_T(pre) + R1) where pre > 0 and lies within 2 u_T (|expm1(pre)| + |expm1(pre) + R1|) + 2^-22 elsewhere (two roundings).  dgrad: dX
    EQUALS RN_T(elu' * sum).  The bf16 wave-specialised input gradients hand their phase partials through LDS in bf16: on their rows dP is
    zero with probability 1/2 and W with 2/3, so that per element the sum over the 16 taps of |that tap's partial| stays <= 256 and every
    grouping of taps is an exactly representable integer (test_upconv_fwd_ref.py asserts it on every such row).
  * random twin: +-U[0.25, 1) rounded to T, W scaled by 0.05 before the fold, Xelu = ELU of such a draw; per element
    |got - ref| <= gate(path, T) * S, S the same statement on absolute operands without act and elu' (plus |bias|, |R1|, |R2|).
Every operand and output lies between GUARD NaN-pattern elements in one flat buffer; the judgement takes the flat output, so a changed guard
or an element nobody wrote (still NaN) fails it.
"""
import zlib

import torch

from _upconv_cases import (ALL, BF16, BIG, F16, F32, F64, GUARD, bits, case_id, cdiv, draw_on, pad_ring, pattern, phases,  # noqa: F401
                           prep_ref, upsample_pad)
from test_ops_gpu import EPS_ELEM

B16 = (BF16, F16)
NONE, ELU = 0, 2
U_T = {F32: 2.0 ** -25, BF16: 2.0 ** -9, F16: 2.0 ** -12}      # 2 u_T is the unit round-off of T
EXP_ABS = 2.0 ** -22                                           # an accurate expm1f of an exact f32 argument, absolute
MACS_BIG = 2 ** 31                                             # multiply-adds from which the statement is evaluated on the device too

FWD_PATHS = ('FG3', 'FG4', 'FWS96/E', 'FWS96/R', 'FWS128/E', 'FWS128/E+X3', 'FWS128/R', 'FWS128/R+X3', 'FPS8', 'FPS16')
RES_PATHS = ('RES/FPS8', 'RES/FPS16')
DGRAD_PATHS = ('DG4', 'DG6', 'DWS2/V3', 'DWS2/G', 'DWS', 'DPF')

# Largest |err| / S of the random twin per (path, element type) on an MI355X, over the path's rows, both Xelu modes and both outputs of res
# (the runs with stj_upconv_prep on the device have their own bound and are not in it); profiles/test_upconv_fwd_ratios.txt is a later run
# under the gates these give.  What sets the ratio is the one rounding of the stored result, at most 2^-8 (bf16) / 2^-11 (fp16) of the
# element and far less of S wherever terms cancel; the bf16 partials of the wave-specialised input gradients and the second rounding of the
# skip sums do not show above it.  f32: the order of the f32 sums.  The kernels are deterministic, so a run repeats these figures.
MEASURED = {
    ('FG3', 'bfloat16'): 2.149e-03, ('FG3', 'float16'): 2.725e-04, ('FG3', 'float32'): 1.824e-07,
    ('FG4', 'bfloat16'): 2.397e-03, ('FG4', 'float16'): 2.707e-04, ('FG4', 'float32'): 1.973e-07,
    ('FWS96/E', 'bfloat16'): 1.604e-03, ('FWS96/E', 'float16'): 1.481e-04, ('FWS96/R', 'bfloat16'): 1.331e-03, ('FWS96/R', 'float16'): 1.509e-04,
    ('FWS128/E', 'bfloat16'): 1.264e-03, ('FWS128/E', 'float16'): 1.324e-04, ('FWS128/E+X3', 'bfloat16'): 1.453e-03, ('FWS128/E+X3', 'float16'): 1.242e-04,
    ('FWS128/R', 'bfloat16'): 8.361e-04, ('FWS128/R', 'float16'): 1.181e-04, ('FWS128/R+X3', 'bfloat16'): 9.913e-04, ('FWS128/R+X3', 'float16'): 1.429e-04,
    ('FPS8', 'bfloat16'): 8.790e-04, ('FPS8', 'float16'): 1.101e-04, ('FPS16', 'bfloat16'): 9.977e-04, ('FPS16', 'float16'): 1.329e-04,
    ('RES/FPS8', 'bfloat16'): 1.838e-03, ('RES/FPS8', 'float16'): 2.395e-04, ('RES/FPS16', 'bfloat16'): 2.187e-03, ('RES/FPS16', 'float16'): 2.489e-04,
    ('DG4', 'bfloat16'): 7.573e-04, ('DG4', 'float16'): 1.251e-04, ('DG4', 'float32'): 2.378e-07,
    ('DG6', 'bfloat16'): 7.682e-04, ('DG6', 'float16'): 8.903e-05, ('DG6', 'float32'): 2.216e-07,
    ('DWS2/V3', 'bfloat16'): 1.150e-03, ('DWS2/G', 'bfloat16'): 9.243e-04, ('DWS', 'bfloat16'): 7.527e-04,
    ('DPF', 'bfloat16'): 6.915e-04, ('DPF', 'float16'): 9.971e-05,
}


def gate(path, dt):
    """EPS_ELEM[T], the project's per-element bound, or four times the measured ratio where that is smaller (the rule of _upconv_cases.GATE)"""
    m = MEASURED.get((path, case_id(dt)))
    return 4 * m if m is not None and 4 * m < EPS_ELEM[dt] else EPS_ELEM[dt]


# ---------------------------------------------------------------------------------------------------------------------------------------
# statements (float64, on whatever device the operands are on)
# ---------------------------------------------------------------------------------------------------------------------------------------
def fwd_pre_from_padded(Xp, Wf, bias, tap=None):
    """pre [F,2Hi,2Wi,Cout] from the zero-ringed map Xp [F,Hi+2,Wi+2,Cin]; tap(pt, a, b, r, s, t) may alter one tap's contribution t [F,Hi,Wi,Cout]"""
    F, Hp, Wp, Cin = Xp.shape
    Hi, Wi, Cout = Hp - 2, Wp - 2, Wf.shape[1]
    pre = Xp.new_zeros(F, 2 * Hi, 2 * Wi, Cout)
    for pt, a, b, r, s in phases():
        t = (Xp[:, a + r:a + r + Hi, b + s:b + s + Wi].reshape(-1, Cin) @ Wf[pt].t()).view(F, Hi, Wi, Cout)   # X row i + a - 1 + r is padded row i + a + r
        if tap is not None:
            t = tap(pt, a, b, r, s, t)
        pre[:, a::2, b::2] += t
    return pre + bias


def fwd_pre(X, Wf, bias, tap=None):
    return fwd_pre_from_padded(pad_ring(X.double()), Wf.double(), bias.double(), tap)


def elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))


def elu_prime(x):
    return torch.where(x > 0, torch.ones_like(x), x + 1)


def dgrad_sum_from_padded(Pp, Wd, tap=None, tap_abs=False):
    """sum_{u,v,co} [F,Hi,Wi,Cin] from the zero-ringed gradient Pp [F,2Hi+2,2Wi+2,Cout] (padded row 2i + u + 1); with tap_abs the sum over the
    16 taps of |that tap's partial| as well (the condition of the bf16 hand-over)"""
    F, Hp, Wp, Cout = Pp.shape
    Hi, Wi, Cin = (Hp - 2) // 2, (Wp - 2) // 2, Wd.shape[1]
    out, mag = Pp.new_zeros(F, Hi, Wi, Cin), Pp.new_zeros(F, Hi, Wi, Cin)
    for u1 in range(4):
        for v1 in range(4):
            t = (Pp[:, u1:u1 + 2 * Hi:2, v1:v1 + 2 * Wi:2].reshape(-1, Cout) @ Wd[u1 * 4 + v1].t()).view(F, Hi, Wi, Cin)
            if tap is not None:
                t = tap(u1 - 1, v1 - 1, t)
            out += t
            if tap_abs:
                mag += t.abs()
    return (out, mag) if tap_abs else out


def dgrad_sum(dP, Wd, tap=None, tap_abs=False):
    return dgrad_sum_from_padded(pad_ring(dP.double()), Wd.double(), tap, tap_abs)


def conv_ref(X, W, bias, act):
    """float64 act(conv3x3_same(upsample2x_nearest(X), W) + bias) by torch's own interpolate and conv2d, NHWC in and out"""
    import torch.nn.functional as Fn
    y = Fn.conv2d(Fn.interpolate(X.double().permute(0, 3, 1, 2), scale_factor=2, mode='nearest'), W.double().permute(3, 2, 0, 1), bias.double(), padding=1)
    return (Fn.elu(y) if act == ELU else y).permute(0, 2, 3, 1)


def conv_dgrad_ref(dP, W, shape, xelu=None):
    """float64 autograd input gradient of the same graph (without act: dP is the gradient of pre), times elu'(Xelu) when that is given"""
    F, Hi, Wi, Cin, Cout = shape
    x = torch.zeros(F, Hi, Wi, Cin, dtype=F64, requires_grad=True)
    conv_ref(x, W, torch.zeros(Cout, dtype=F64), NONE).backward(dP.double())
    g = x.grad.detach()
    return g * elu_prime(xelu.double()) if xelu is not None else g


# ---------------------------------------------------------------------------------------------------------------------------------------
# dispatch mirrors: stj_upconv_fwd -> upconv_fwd_ws_try -> ws2_launch(_t) | upconv_fwd_ps_try -> fwd_ps_try_t | upconv_fwd_launch,
# stj_upconv_fwd_res -> upconv_fwd_ps_res_try, stj_upconv_dgrad -> upconv_dgrad_ws_try | upconv_dgrad_pf_try | upconv_dgrad_launch.
# Tiles are 8 rows x 16 columns of low-res pixels.
# ---------------------------------------------------------------------------------------------------------------------------------------
def ntiles_of(F, Hi, Wi):
    return F * cdiv(Hi, 8) * cdiv(Wi, 16)


def whole(Hi, Wi):
    return Hi % 8 == 0 and Wi % 16 == 0


def fwd_geometry(dt, F, Hi, Wi, Cin, Cout, act, ws=True):
    """dict(path, ntiles, ct, walkers, grid): what the launcher of the path computes"""
    nt = ntiles_of(F, Hi, Wi)
    if dt in B16 and ws and act == ELU:
        if Cout % 8 == 0 and Cin == 96:
            ct = cdiv(Cout, 48)
            nblk = max(1, min(256 // ct, nt))
            return dict(path='FWS96/E' if whole(Hi, Wi) and Cout % 48 == 0 else 'FWS96/R', ntiles=nt, ct=ct, walkers=nblk, grid=nblk * ct)
        if Cout % 8 == 0 and Cin == 128:
            ct = cdiv(Cout, 32)
            ex = whole(Hi, Wi) and Cout % 32 == 0
            nw = 80
            while nw > 8 and nw - 8 >= nt:
                nw -= 8
            # the straight-line movers need a tile for every walker: whole tiles with nw > ntiles take the 2-D grid
            if ct == 3 and nt >= 8 and (not ex or nw <= nt):
                return dict(path=f"FWS128/{'E' if ex else 'R'}+X3", ntiles=nt, ct=ct, walkers=nw, grid=nw * 3)
            nblk = max(1, min(256 // ct, nt))
            return dict(path=f"FWS128/{'E' if ex else 'R'}", ntiles=nt, ct=ct, walkers=nblk, grid=nblk * ct)
        if Cin % 32 == 0 and Cin > 128 and Cout % 32 == 0:
            th = 16 if Hi % 16 == 0 else 8
            tiles = F * cdiv(Hi, th) * cdiv(Wi, 16)
            return dict(path=f'FPS{th}', ntiles=tiles, ct=Cout // 32, walkers=tiles, grid=tiles * (Cout // 32))
    if Cout % 64 == 0 or Cout > 96:
        return dict(path='FG4', ntiles=nt, ct=cdiv(Cout, 64), walkers=nt, grid=nt * cdiv(Cout, 64))
    return dict(path='FG3', ntiles=nt, ct=cdiv(Cout, 48), walkers=nt, grid=nt * cdiv(Cout, 48))


def expected_fwd_path(dt, F, Hi, Wi, Cin, Cout, act, ws=True):
    return fwd_geometry(dt, F, Hi, Wi, Cin, Cout, act, ws)['path']


def expected_res_path(dt, F, Hi, Wi, Cin, Cout, r1=True, y2=True, r2=True, ws=True):
    """the kernel stj_upconv_fwd_res runs, or None: STJ_EUNSUPPORTED"""
    if dt in B16 and ws and Cin % 32 == 0 and Cin > 128 and Cout % 32 == 0 and r1 and y2 == r2:
        return 'RES/FPS16' if Hi % 16 == 0 else 'RES/FPS8'
    return None


def dgrad_geometry(dt, F, Hi, Wi, Cin, Cout, ws=True):
    nt = ntiles_of(F, Hi, Wi)
    if dt == BF16 and ws and Cin % 8 == 0 and Cout % 8 == 0:
        if Cin == 96 and Cout == 48:
            return dict(path='DWS2/V3' if whole(Hi, Wi) else 'DWS2/G', ntiles=nt, ct=1, walkers=min(nt, 256), grid=min(nt, 256))
        if Cin == 128 and Cout == 96 and F * 4 * Hi * Wi * Cout * 2 < 2 ** 31:          # the halo loader's 32-bit byte offsets
            return dict(path='DWS', ntiles=nt, ct=2, walkers=min(128, nt), grid=min(128, nt) * 2)
    if dt in B16 and ws and whole(Hi, Wi) and Cin % 64 == 0 and Cout % 32 == 0 and Cin > 128:
        ct = Cin // 64
        nblk = min(max(256 // ct // 8 * 8, 8), nt)

        def slots(n):
            return (cdiv(nt, n) + 3) // 4 * 4
        while nblk > 8 and slots(nblk - 8) == slots(nblk):
            nblk -= 8
        nseq8 = cdiv(nblk, 8) * 8
        return dict(path='DPF', ntiles=nt, ct=ct, walkers=nblk, nseq8=nseq8, grid=nseq8 * ct)
    if Cin % 96 == 0 and Cin % 64 != 0:
        return dict(path='DG6', ntiles=nt, ct=Cin // 96, walkers=nt, grid=nt * (Cin // 96))
    return dict(path='DG4', ntiles=nt, ct=cdiv(Cin, 64), walkers=nt, grid=nt * cdiv(Cin, 64))


def expected_dgrad_path(dt, F, Hi, Wi, Cin, Cout, ws=True):
    return dgrad_geometry(dt, F, Hi, Wi, Cin, Cout, ws)['path']


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case tables: the smallest shapes at which each branch can still go wrong
# ---------------------------------------------------------------------------------------------------------------------------------------
def _case(kind, path, shape, dts, **kw):
    d = dict(kind=kind, path=path, shape=shape, dts=tuple(dts), name='x'.join(str(v) for v in shape), act=ELU, sparse=False, skips=None)
    d.update(kw)
    if d['act'] != ELU:
        d['name'] += '-act0'
    if d['skips']:
        d['name'] += '-' + d['skips']
    return d


def _f(path, shape, dts, **kw):
    return _case('fwd', path, shape, dts, **kw)


def _d(path, shape, dts, **kw):
    return _case('dgrad', path, shape, dts, sparse=path.startswith('DWS'), **kw)


FWD_CASES = [
    _f('FG3', (1, 1, 1, 8, 8), ALL),                        # a map that is all halo
    _f('FG3', (2, 5, 19, 24, 40), ALL),
    _f('FG3', (1, 19, 5, 24, 40), (F32,)),                  # its transpose
    _f('FG3', (2, 8, 16, 96, 48), (F32,)),
    _f('FG3', (1, 8, 16, 128, 96), (F32,)),                 # two cout tiles
    _f('FG3', (2, 8, 16, 96, 48), B16, act=NONE),           # the 16-bit generic kernel at a shape the wave-specialised one would take with ELU
    _f('FG4', (1, 3, 17, 72, 136), ALL),
    _f('FG4', (1, 9, 20, 40, 64), ALL),
    _f('FWS96/E', (2, 8, 16, 96, 48), B16),
    _f('FWS96/E', (1, 16, 48, 96, 96), B16, geo=dict(ct=2, ntiles=6, walkers=6)),
    _f('FWS96/E', (5, 40, 96, 96, 96), (BF16,), geo=dict(ntiles=150, ct=2, walkers=128)),      # 150 tiles on 128 walkers
    _f('FWS96/R', (2, 5, 19, 96, 40), B16),                 # ragged rows, columns and cout
    _f('FWS96/R', (1, 12, 40, 96, 48), B16),
    _f('FWS96/R', (1, 8, 16, 96, 56), B16, geo=dict(ct=2)),             # whole tiles with a ragged second cout tile
    _f('FWS96/R', (1, 19, 5, 96, 48), (BF16,)),
    _f('FWS128/E', (1, 8, 16, 128, 96), B16, geo=dict(ct=3, ntiles=1, walkers=1, grid=3)),     # one tile, 2-D grid
    _f('FWS128/E', (1, 8, 16, 128, 64), B16, geo=dict(ct=2)),
    _f('FWS128/E', (1, 8, 16, 128, 32), (BF16,), geo=dict(ct=1)),
    # whole tiles, 12 of them: the walker grid would be 16 wide, and the straight-line movers of walkers 12..15 used to store their stage
    # past the end of Y (found by reading for this table; fixed in ws2_launch_t: the 2-D grid with 12 walkers)
    _f('FWS128/E', (3, 16, 32, 128, 96), B16, geo=dict(ct=3, ntiles=12, walkers=12, grid=36)),
    _f('FWS128/E+X3', (2, 16, 32, 128, 96), B16, geo=dict(ntiles=8, walkers=8, grid=24)),
    _f('FWS128/E+X3', (3, 48, 96, 128, 96), (BF16,), geo=dict(ntiles=108, walkers=80, grid=240)),     # 108 tiles on 80 walkers
    _f('FWS128/R', (1, 8, 16, 128, 40), B16, geo=dict(ct=2)),
    _f('FWS128/R+X3', (2, 12, 40, 128, 96), B16, geo=dict(ntiles=12, walkers=16, grid=48)),    # four walkers without a tile
    _f('FPS8', (1, 8, 16, 160, 32), B16),
    _f('FPS8', (2, 8, 8, 384, 192), B16),                   # half a column tile
    _f('FPS8', (1, 24, 16, 192, 128), B16, geo=dict(ntiles=3)),
    _f('FPS16', (1, 16, 16, 192, 128), B16, geo=dict(ntiles=1)),
    _f('FPS16', (2, 16, 24, 160, 32), B16),                 # ragged columns
    _f('FPS16', (1, 32, 16, 384, 192), (BF16,), geo=dict(ntiles=2)),
]
RES_CASES = [
    _case('res', 'RES/FPS16', (1, 16, 16, 192, 128), B16, skips='r1r2'),
    _case('res', 'RES/FPS8', (2, 8, 8, 384, 192), B16, skips='r1'),
    _case('res', 'RES/FPS8', (1, 24, 40, 160, 32), B16, skips='r1r2'),      # ragged columns
]
DGRAD_CASES = [
    _d('DG4', (1, 1, 1, 8, 8), ALL),
    _d('DG4', (1, 3, 17, 72, 136), ALL),
    _d('DG4', (1, 12, 40, 192, 128), B16),                  # ragged: the pipelined kernel refuses
    _d('DG4', (1, 8, 16, 160, 32), B16),
    _d('DG4', (1, 8, 16, 192, 40), B16),
    _d('DG4', (1, 8, 16, 128, 96), (F32, F16)),             # (bf16: DWS)
    _d('DG6', (2, 8, 16, 96, 48), (F32, F16)),              # (bf16: DWS2/V3)
    _d('DG6', (2, 5, 19, 96, 40), ALL),
    _d('DG6', (1, 3, 17, 288, 24), ALL, geo=dict(ct=3)),
    _d('DWS2/V3', (2, 8, 16, 96, 48), (BF16,)),
    _d('DWS2/V3', (1, 16, 48, 96, 48), (BF16,), geo=dict(ntiles=6)),
    _d('DWS2/V3', (5, 64, 112, 96, 48), (BF16,), geo=dict(ntiles=280, walkers=256)),     # 280 tiles on 256 workgroups: the rolling halo
    _d('DWS2/G', (2, 5, 19, 96, 48), (BF16,)),
    _d('DWS2/G', (1, 12, 40, 96, 48), (BF16,)),
    _d('DWS2/G', (1, 19, 5, 96, 48), (BF16,)),
    _d('DWS', (1, 8, 16, 128, 96), (BF16,)),
    _d('DWS', (2, 5, 19, 128, 96), (BF16,)),
    _d('DWS', (1, 19, 5, 128, 96), (BF16,)),
    _d('DWS', (3, 56, 112, 128, 96), (BF16,), geo=dict(ntiles=147, walkers=128, grid=256)),            # 147 tiles on 128
    _d('DPF', (1, 8, 16, 192, 128), B16, geo=dict(ntiles=1, ct=3, walkers=1, nseq8=8, grid=24)),        # 1 tile, sequences padded to 8
    _d('DPF', (1, 8, 16, 192, 32), B16, geo=dict(walkers=1, nseq8=8)),                                  # one cout chunk
    _d('DPF', (1, 16, 32, 384, 192), B16, geo=dict(ntiles=4, ct=6, walkers=4, nseq8=8, grid=48)),
    # 48 tiles: 40 sequences fit, 16 need the same four tile slots each (conv.hip: slots()), so 16 sequences of 3 tiles run
    _d('DPF', (3, 32, 64, 384, 192), (BF16,), geo=dict(ntiles=48, ct=6, walkers=16, nseq8=16, grid=96)),
]
XELU_MODES = (False, True)
TABLES = {'fwd': FWD_CASES, 'res': RES_CASES, 'dgrad': DGRAD_CASES}


def expected_path(cs, dt):
    if cs['kind'] == 'fwd':
        return expected_fwd_path(dt, *cs['shape'], cs['act'])
    if cs['kind'] == 'res':
        return expected_res_path(dt, *cs['shape'], True, 'r2' in cs['skips'], 'r2' in cs['skips'])
    return expected_dgrad_path(dt, *cs['shape'])


def geometry(cs, dt):
    if cs['kind'] == 'dgrad':
        return dgrad_geometry(dt, *cs['shape'])
    return fwd_geometry(dt, *cs['shape'], cs['act'])


def pixels(cs):
    F, Hi, Wi, _, _ = cs['shape']
    return F * Hi * Wi


def on_device(cs):
    """rows whose statement is evaluated on the device: more than BIG high-res pixels, or more than 2^31 multiply-adds per evaluation"""
    _, _, _, Cin, Cout = cs['shape']
    return 4 * pixels(cs) > BIG or 16 * pixels(cs) * Cin * Cout > MACS_BIG


def rows(kind, pred=lambda cs: True):
    return [(cs, dt) for cs in TABLES[kind] for dt in cs['dts'] if pred(cs)]


def first_of_path(cs, dt):
    """the first (case, dtype) of its path in table order: its random twin also runs stj_upconv_prep on the device, against torch's conv2d"""
    for c, d in rows(cs['kind']):
        if c['path'] == cs['path']:
            return c is cs and d == dt
    return False


# ---------------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seed(cs, dt, exact):
    return (zlib.crc32(f"{cs['kind']}{cs['shape']}{cs['act']}".encode()) & 0xFFFFFF) + 2 * ALL.index(dt) + int(exact)


def _tern(n, gen, p_zero):
    """n values of {-1, 0, 1} (f32), zero with probability p_zero"""
    sgn = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    return (sgn * (torch.rand(n, generator=gen) >= p_zero)).float()


def _rand(n, gen, scale=1.0):
    mag = torch.rand(n, generator=gen) * 0.75 + 0.25
    sgn = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    return mag * sgn * scale


class Ops:
    """operands of one (row, element type, twin) on the CPU: W f32 [3,3,Cin,Cout]; Wf, Wd (T) = prep_ref(W) cast; bias f32; X, R1, R2, dP, Xelu (T)"""


def operands(cs, dt, exact):
    F, Hi, Wi, Cin, Cout = cs['shape']
    g = torch.Generator().manual_seed(_seed(cs, dt, exact))
    o = Ops()
    nX, nY = F * Hi * Wi * Cin, F * 4 * Hi * Wi * Cout
    pw, pp = (2 / 3, 1 / 2) if cs['sparse'] else (1 / 3, 1 / 3)

    def val(n, p=1 / 3):
        return _tern(n, g, p) if exact else _rand(n, g)
    o.W = (_tern(9 * Cin * Cout, g, pw) if exact else _rand(9 * Cin * Cout, g, 0.05)).view(3, 3, Cin, Cout)
    wf, wd = prep_ref(o.W)
    o.Wf, o.Wd = wf.to(dt), wd.to(dt)
    o.bias = val(Cout)
    if cs['kind'] == 'dgrad':
        o.dP = val(nY, pp).to(dt).view(F, 2 * Hi, 2 * Wi, Cout)
        if exact:
            o.Xelu = torch.tensor([-0.5, 0.0, 1.0, 2.0])[torch.randint(0, 4, (nX,), generator=g)].to(dt).view(F, Hi, Wi, Cin)
        else:
            o.Xelu = elu(_rand(nX, g)).to(dt).view(F, Hi, Wi, Cin)
    else:
        o.X = val(nX).to(dt).view(F, Hi, Wi, Cin)
        o.R1 = o.R2 = None
        if cs['kind'] == 'res':
            o.R1 = val(nY).to(dt).view(F, 2 * Hi, 2 * Wi, Cout)
            if 'r2' in cs['skips']:
                o.R2 = val(nY).to(dt).view(F, 2 * Hi, 2 * Wi, Cout)
    return o


class Ref:
    """float64 on the CPU.  fwd / res: pre, S (res: S holds |bias| only; the judgement adds |R1|, |R2|); dgrad: sum, S"""


def reference(cs, o, device='cpu'):
    R = Ref()
    if cs['kind'] == 'dgrad':
        P, Wd = o.dP.to(device).double(), o.Wd.to(device).double()
        R.sum, R.S = dgrad_sum(P, Wd).cpu(), dgrad_sum(P.abs(), Wd.abs()).cpu()
    else:
        X, Wf, b = o.X.to(device).double(), o.Wf.to(device).double(), o.bias.to(device).double()
        R.pre, R.S = fwd_pre(X, Wf, b).cpu(), fwd_pre(X.abs(), Wf.abs(), b.abs()).cpu()
    return R


# ---------------------------------------------------------------------------------------------------------------------------------------
# judgement.  Outputs come as flat buffers [GUARD][values][GUARD] of T with the image they started from.
# ---------------------------------------------------------------------------------------------------------------------------------------
def flat_of(vals, dt):
    """values (any float type) rounded to T between two NaN-pattern guards, and the all-pattern image an output buffer starts from"""
    n = vals.numel()
    init = pattern(GUARD + n + GUARD, dt)
    flat = init.clone()
    flat[GUARD:GUARD + n] = vals.reshape(-1).to(dt)
    return flat, init


def unguard(label, name, flat, init, shape):
    n = init.numel() - 2 * GUARD
    fails = []
    if not (torch.equal(bits(flat[:GUARD]), bits(init[:GUARD])) and torch.equal(bits(flat[GUARD + n:]), bits(init[GUARD + n:]))):
        fails.append(f'{label}: {name}: guard elements changed')
    return flat[GUARD:GUARD + n].reshape(shape), fails


def _equal(label, name, got, want, where=None):
    ne = got.double() != want.double()                 # NaN != anything: an element nobody wrote, or one fed from a guard, differs
    if where is not None:
        ne = ne & where
    if bool(ne.any()):
        ix = tuple(ne.nonzero()[0].tolist())
        return [f'{label}: {name}: {int(ne.sum())} of {ne.numel()} elements differ from the exact result, first {ix}: got {float(got[ix])}, '
                f'want {float(want[ix])}']
    return []


def _within(label, name, got, want, tol, where):
    bad = ~((got.double() - want).abs() <= tol) & where            # ~(NaN <= tol) is True
    if bool(bad.any()):
        ix = tuple(bad.nonzero()[0].tolist())
        return [f'{label}: {name}: {int(bad.sum())} elements off expm1 by more than the rounding of T, first {ix}: got {float(got[ix])}, '
                f'want {float(want[ix])}']
    return []


def _ratio(label, name, got, want, S, g, ratios):
    r = float(torch.nan_to_num((got.double() - want).abs() / (S + 1e-300), nan=float('inf')).max())
    ratios[name] = r
    return [] if r <= g else [f'{label}: {name}: max |err| / sum |terms| = {r:.3e} over the gate {g:.3e}']


def judge_fwd(label, cs, dt, exact, g, o, R, flats, plain=None):
    """flats: {'Y': (flat, init)[, 'Y2': (flat, init)]}; plain (res, random twin): the Y of stj_upconv_fwd on the same operands, to whose sums
    by separate adds in T the skip outputs are held bit for bit.  Returns (failures, {output: ratio})."""
    F, Hi, Wi, Cin, Cout = cs['shape']
    shape = (F, 2 * Hi, 2 * Wi, Cout)
    fails, ratios = [], {}
    Y, f = unguard(label, 'Y', *flats['Y'], shape)
    fails += f
    pos = R.pre > 0
    e = elu(R.pre) if cs['act'] == ELU else R.pre
    u2 = 2 * U_T[dt]
    if cs['kind'] == 'fwd':
        if exact:
            fails += _equal(label, 'Y', Y, R.pre.to(dt), pos if cs['act'] == ELU else None)
            if cs['act'] == ELU:
                fails += _within(label, 'Y', Y, e, u2 * e.abs() + EXP_ABS, ~pos)
        else:
            fails += _ratio(label, 'Y', Y, e, R.S, g, ratios)
        return fails, ratios
    r1 = o.R1.double()
    if exact:
        fails += _equal(label, 'Y', Y, (R.pre.to(dt).double() + r1).to(dt), pos)
        fails += _within(label, 'Y', Y, e + r1, u2 * (e.abs() + (e + r1).abs()) + EXP_ABS, ~pos)
    else:
        fails += _ratio(label, 'Y', Y, e + r1, R.S + r1.abs(), g, ratios)
        if plain is not None:
            fails += _equal(label, 'Y (against the plain forward + R1 in T)', Y, plain + o.R1)
    if o.R2 is not None:
        Y2, f = unguard(label, 'Y2', *flats['Y2'], shape)
        fails += f
        r2 = o.R2.double()
        if exact:
            fails += _equal(label, 'Y2 (against RN_T(Y + R2) of the Y returned)', Y2, (Y.double() + r2).to(dt), ~torch.isnan(Y.double()))
            fails += _equal(label, 'Y2', Y2, ((R.pre.to(dt).double() + r1).to(dt).double() + r2).to(dt), pos)
        else:
            fails += _ratio(label, 'Y2', Y2, e + r1 + r2, R.S + r1.abs() + r2.abs(), g, ratios)
            if plain is not None:
                fails += _equal(label, 'Y2 (against (the plain forward + R1) + R2 in T)', Y2, (plain + o.R1) + o.R2)
    return fails, ratios


def judge_dgrad(label, cs, dt, exact, g, o, R, xelu, flat, init):
    """xelu: whether Xelu was handed in.  Returns (failures, {'dX': ratio})."""
    F, Hi, Wi, Cin, Cout = cs['shape']
    fails, ratios = [], {}
    dX, f = unguard(label, 'dX', flat, init, (F, Hi, Wi, Cin))
    fails += f
    want = R.sum * elu_prime(o.Xelu.double()) if xelu else R.sum
    if exact:
        fails += _equal(label, 'dX', dX, want.to(dt))
    else:
        fails += _ratio(label, 'dX', dX, want, R.S, g, ratios)
    return fails, ratios


def dws_condition(o):
    """the largest, over the elements of dX, sum over the 16 taps of |that tap's partial over co|"""
    return float(dgrad_sum(o.dP, o.Wd, tap_abs=True)[1].max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutated statements: what a subtly wrong kernel would leave in its output buffers.  Each returns flat buffers like the kernel's.
# ---------------------------------------------------------------------------------------------------------------------------------------
FWD_MUTATIONS = ('drop_border_tap', 'halo_hw_swapped', 'right_halo_twice', 'tile_unwritten', 'row_too_far')
RES_MUTATIONS = FWD_MUTATIONS + ('y2_rounded_once',)
DGRAD_MUTATIONS = FWD_MUTATIONS + ('elu_from_own_sign',)


def _finish_fwd(cs, dt, o, pre):
    """(Y, Y2 | None) in T from a float64 pre, by the statement's roundings"""
    y = (elu(pre) if cs['act'] == ELU else pre).to(dt)
    if cs['kind'] == 'fwd':
        return y, None
    y = y + o.R1                                      # torch adds in T: f32 sum, one rounding
    return y, (y + o.R2 if o.R2 is not None else None)


def _spoil(kind, cs, t, out_scale):
    """tile_unwritten / row_too_far on the flat image of one output t [F,H,W,C] (T); out_scale 2 for the high-res outputs"""
    flat, init = flat_of(t, t.dtype)
    F, H, W, C = t.shape
    if kind == 'tile_unwritten':                      # the last tile of the last frame stays NaN pattern
        th, tw = 8 * out_scale, 16 * out_scale
        v = flat[GUARD:GUARD + t.numel()].view(F, H, W, C)
        v[F - 1, (H - 1) // th * th:, (W - 1) // tw * tw:] = pattern(1, t.dtype)[0]
    if kind == 'row_too_far':                         # every frame's last row again, one row further down: into the next frame, or the guard
        for f in range(F):
            end = GUARD + (f + 1) * H * W * C
            n = min(W * C, flat.numel() - end)
            flat[end:end + n] = t[f, H - 1].reshape(-1)[:n]
    return flat, init


def mutated_fwd(kind, cs, dt, o, R):
    """{'Y': (flat, init)[, 'Y2': ...]} of a forward that is wrong in one way (kind None: the statement itself)"""
    F, Hi, Wi, Cin, Cout = cs['shape']
    Xd, Wf, b = o.X.double(), o.Wf.double(), o.bias.double()
    pre = R.pre
    if kind == 'drop_border_tap':                     # low-res column 0, odd output columns: the tap that reads column 0 itself
        def tap(pt, a, b_, r, s, t):
            if b_ == 1 and s == 0:
                t = t.clone()
                t[:, :, 0] = 0
            return t
        pre = fwd_pre(Xd, Wf, b, tap)
    elif kind == 'halo_hw_swapped':                   # the in-map test written gy < Wi && gx < Hi
        Xm = Xd.clone()
        Xm[:, min(Hi, Wi):] = 0
        Xm[:, :, min(Hi, Wi):] = 0
        pre = fwd_pre(Xm, Wf, b)
    elif kind == 'right_halo_twice':                  # frame 0: the zero column right of the map holds the map's last column again
        Xp = pad_ring(Xd)
        Xp[0, 1:Hi + 1, Wi + 1] = Xd[0, :, Wi - 1]
        pre = fwd_pre_from_padded(Xp, Wf, b)
    y, y2 = _finish_fwd(cs, dt, o, pre)
    if kind == 'y2_rounded_once':
        y2 = (elu(pre) + o.R1.double() + o.R2.double()).to(dt)
    spoil = kind if kind in ('tile_unwritten', 'row_too_far') else None
    out = {'Y': _spoil(spoil, cs, y, 2)}
    if y2 is not None:
        out['Y2'] = _spoil(spoil, cs, y2, 2)
    return out


def mutated_dgrad(kind, cs, dt, o, R, xelu):
    """(flat, init) of a dX that is wrong in one way (kind None: the statement itself)"""
    F, Hi, Wi, Cin, Cout = cs['shape']
    Pd, Wd = o.dP.double(), o.Wd.double()
    s = R.sum
    if kind == 'drop_border_tap':                     # the last low-res row: the tap that reads the map's last high-res row
        def tap(u, v, t):
            if u == 1:
                t = t.clone()
                t[:, Hi - 1] = 0
            return t
        s = dgrad_sum(Pd, Wd, tap)
    elif kind == 'halo_hw_swapped':
        Pm = Pd.clone()
        Pm[:, 2 * min(Hi, Wi):] = 0
        Pm[:, :, 2 * min(Hi, Wi):] = 0
        s = dgrad_sum(Pm, Wd)
    elif kind == 'right_halo_twice':
        Pp = pad_ring(Pd)
        Pp[0, 1:2 * Hi + 1, 2 * Wi + 1] = Pd[0, :, 2 * Wi - 1]
        s = dgrad_sum_from_padded(Pp, Wd)
    fac = elu_prime(o.Xelu.double()) if xelu else 1.0
    if kind == 'elu_from_own_sign':
        fac = elu_prime(s)
    return _spoil(kind if kind in ('tile_unwritten', 'row_too_far') else None, cs, (s * fac).to(dt), 1)
