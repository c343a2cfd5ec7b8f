"""Cases, flat-buffer layout, float64 references and the judge shared by test_layernorm_gpu.py (the kernels) and test_layernorm_ref.py
(a plain float32 PyTorch statement through the same judge).  Nothing here needs a GPU or the library.

A case is a dict (lncase / chaincase).  prepare(cs, dt, kind, exact) lays every tensor of one call into a flat CPU allocation filled with
the NaN bit pattern of test_gemm_gpu.PAT -- GUARD elements in front and behind, the gaps between parameter sets (gstride > C) and between
partial copies (part_stride > C) included -- and evaluates the float64 reference and the bounds from those same flat buffers.  judge()
takes the flat buffers as they are after the call: everything that is no output element must be bit-identical (inputs included), and the
output elements meet their bound (or equal the reference in the exact twin).  The derivations of the bounds are in the docstring of
test_layernorm_gpu.py.
"""
import numpy as np
import torch

from test_gemm_gpu import GUARD, bits, draw, pattern
from test_ops_gpu import EPS_ELEM

F32 = torch.float32
EPSF = EPS_ELEM[F32]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
QUAD = [(0, 0), (1, 0), (0, 1), (1, 1)]      # (di, dj) of quadrant q of a merged row: x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)
MAX_ROWS = 4096                               # EPS_ELEM[float32] rests on at most a few thousand rows per parameter sum


def vn_of(dt):
    return 4 if dt == F32 else 8


def cdiv(a, b):
    return -(-a // b)


def lncase(name, rows, C, **kw):
    d = dict(name=name, rows=rows, C=C, eps=1e-5, gres=0, B=0, C0=0, ngroups=1, group_rows=0, gstride=0, res=False, dres=False, nparts=1,
             pstride=0, mis=None, kinds=('fwd', 'bwd'), tail=0)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    assert 0 < d['rows'] <= MAX_ROWS
    return d


def gcase(name, B, gres, C0, **kw):
    return lncase(name, B * (gres // 2) ** 2, 4 * C0, gres=gres, B=B, C0=C0, **kw)


def chaincase(name, rows, C, d2out=True, np2=1, ps2=0, np1=1, ps1=0):
    return dict(name=name, rows=rows, C=C, eps=1e-5, d2out=d2out, np2=np2, ps2=ps2, np1=np1, ps1=ps1, kinds=('chain',))


# ------------------------------------------------------------------------------------------------------------------------------------------
# The dispatcher's rule, restated: used ONLY to choose row counts around a pass, to label the error-ratio table and to know how many
# workgroups share the partial copies (the per-copy check).  No reference and no bound depends on it; a kernel trace of the module
# is the record of what really ran.
# ------------------------------------------------------------------------------------------------------------------------------------------
def v2_shape(C, dt):
    """(LPR, NCHK, U) of the 16-byte-vector kernels for width C, or None when C is no whole number of vectors / more than 192 of them"""
    vn = vn_of(dt)
    if C % vn or C // vn > 192:
        return None
    ch = C // vn
    lpr = 16 if ch <= 16 else (32 if ch <= 32 else 64)
    nchk = 1 if ch <= 64 else (2 if ch <= 128 else 3)
    return lpr, nchk, {1: 4, 2: 2, 3: 1}[nchk]


def pass_rows(C, dt):
    """rows one workgroup of the vector kernels covers per pass: 4 waves x U x 64 / LPR"""
    lpr, _, u = v2_shape(C, dt)
    return 4 * u * (64 // lpr)


def takes_v2(cs, dt, kind):
    if v2_shape(cs['C'], dt) is None or (cs['gres'] and cs['C0'] % vn_of(dt)) or cs['gstride'] % 4:
        return False
    fwd_ptrs, bwd_ptrs = ('x', 'y', 'res', 'gamma'), ('x', 'dy', 'dx', 'dres', 'gamma')
    return cs['mis'] not in (fwd_ptrs if kind == 'fwd' else bwd_ptrs)


def path_of(cs, dt, kind):
    if kind == 'chain':
        return f'chain LPR {v2_shape(cs["C"], dt)[0]}' if chain_takes(cs['C'], dt) else 'chain (refused)'
    if not takes_v2(cs, dt, kind):
        return 'v1 scalar'
    lpr, nchk, _ = v2_shape(cs['C'], dt)
    return f'v2 {lpr}x{nchk}'


def bwd_geometry(cs, dt):
    """(workgroups per parameter group, S sub-runs per run, L rows per sub-run) of stj_layernorm_bwd.
    COUPLING: this and chain_blocks copy the grid arithmetic of ln_launch / ln_chain_launch (rows per pass, the 256-workgroup cap) and feed
    p.copies, the number of partial copies the per-copy share check expects to be written.  Retuning that arithmetic in norm.hip fails the
    share check for a reason that is no error of the kernels: update these two helpers with it."""
    rows, ng = cs['rows'], max(1, cs['ngroups'])
    gr = cs['group_rows'] if (ng > 1 and cs['group_rows'] > 0) else rows
    nr = cdiv(cdiv(rows, gr), ng)
    rpp = pass_rows(cs['C'], dt) if takes_v2(cs, dt, 'bwd') else 64
    nbt = max(1, min(cdiv(rows // ng, rpp), 256 // ng))
    S = max(1, cdiv(nbt, nr))
    return min(nbt, nr * S), S, cdiv(gr, S)


def chain_takes(C, dt):
    return v2_shape(C, dt) is not None and C // vn_of(dt) <= 64


def chain_blocks(cs, dt):
    if not chain_takes(cs['C'], dt):
        return 1
    return min(256, cdiv(cs['rows'], 4 * 2 * (64 // v2_shape(cs['C'], dt)[0])))


# ------------------------------------------------------------------------------------------------------------------------------------------
# The case matrix (per dtype: the vector width, and with it every pass size and path, depends on the storage type)
# ------------------------------------------------------------------------------------------------------------------------------------------
def matrix(dt):
    f32 = dt == F32
    m = {}
    # 1. every LPR x NCHK: rows 1, one short of / equal to / one past a workgroup's pass, three passes and a ragged tail; both eps
    m['v2'] = []
    for C in (8, 48, 96, 128, 192, 384, 768) + (() if f32 else (1032, 1536)):
        P = pass_rows(C, dt)
        for rows in sorted({1, P - 1, P, P + 1, 3 * P + 5} - {0}):
            for eps in (1e-5, 1e-3):
                m['v2'].append(lncase(f'v2_C{C}_r{rows}_eps{eps:g}', rows, C, eps=eps))
    # 2. the scalar kernels, one case per reason that selects them
    v1w = 98 if f32 else 100
    m['v1'] = [lncase(f'v1_C{v1w}', 77, v1w), lncase('v1_C1', 70, 1), lncase('v1_C63', 70, 63, eps=1e-3), lncase('v1_C65', 70, 65)]
    if f32:
        m['v1'] += [lncase('v1_f32_C1000', 37, 1000), lncase('v1_f32_C1536', 21, 1536, eps=1e-3)]
    for ptr in ('x', 'gamma'):
        m['v1'].append(lncase(f'v1_mis_{ptr}', 70, 96, mis=ptr))
    m['v1'] += [lncase('v1_mis_y', 70, 96, mis='y', kinds=('fwd',)), lncase('v1_mis_res', 70, 96, mis='res', res=True, kinds=('fwd',)),
                lncase('v1_mis_dy', 70, 96, mis='dy', kinds=('bwd',)), lncase('v1_mis_dx', 70, 96, mis='dx', kinds=('bwd',)),
                lncase('v1_mis_dres', 70, 96, mis='dres', dres=True, kinds=('bwd',)),
                lncase('v1_gstride_mod4', 150, 96, ngroups=2, group_rows=37, gstride=98),
                gcase('v1_gather_C0_20', 3, 4, 20),            # C0 % VN != 0 in 16 bits only (f32: 20 = 5 vectors, the vector kernels)
                gcase('v1_gather_C0_22', 3, 4, 22)]            # C = 88 a whole number of vectors, C0 = 22 not, in every type
    # 3. PatchMerging gather: C0 24 / 96 vector kernels, 20 scalar
    m['gather'] = [gcase(f'gather_B{B}_res{r}_C0{C0}', B, r, C0, eps=1e-5 if B == 1 else 1e-3) for r in (2, 4, 16) for B in (1, 3) for C0 in (24, 96, 20)]
    # 4. parameter groups: three rounds of runs with the last run cut short by rows; group_rows = 37 is no multiple of any pass; gstride > C
    m['groups'] = []
    for C in (96, v1w):
        for ng in (2, 3, 8):
            rows = 3 * ng * 37 - 11
            for res in (False, True):
                m['groups'].append(lncase(f'groups{ng}_C{C}_{"res" if res else "plain"}', rows, C, ngroups=ng, group_rows=37, gstride=C + 8, res=res, dres=res,
                                          eps=1e-3 if res else 1e-5))
        # S > 1 with L off the pass size (C = 96 in 16 bits: S = 8, L = 63)
        m['groups'].append(lncase(f'groups2_C{C}_subruns', 1000, C, ngroups=2, group_rows=500, gstride=C + 8))
        m['groups'].append(lncase(f'groups2_C{C}_subruns_dres', 1000, C, ngroups=2, group_rows=500, gstride=C + 8, dres=True, kinds=('bwd',)))
        m['groups'].append(lncase(f'groups3_C{C}_parts', 700, C, ngroups=3, group_rows=100, gstride=C + 8, nparts=3, pstride=3 * (C + 8) + 8, kinds=('bwd',)))
    # 5. partial copies: fewer workgroups than copies (70 rows) and more (1000 rows)
    m['parts'] = [lncase(f'parts{n}_C{C}_ps{ps}_r{rows}', rows, C, nparts=n, pstride=ps if n > 1 else 0, kinds=('bwd',))
                  for C in (96, v1w) for n in (1, 3, 8) for ps in (C, C + 24) for rows in (70, 1000) if n > 1 or ps == C]
    # 6. res forward / dres backward without groups
    m['res'] = [lncase(f'res_C{C}', 77, C, res=True, dres=True, eps=1e-3) for C in (96, v1w)]
    # 7. the two-norm backward chain: LPR 16 / 32 / 64, ragged rows, d2out null and not, nparts2 != nparts1
    wide = 256 if f32 else 512
    m['chain'] = [chaincase('chain_C8_r777', 777, 8, np2=3, ps2=8 + 24, np1=2, ps1=8), chaincase('chain_C8_r1_no_d2', 1, 8, d2out=False),
                  chaincase('chain_C96_r203', 203, 96, np2=2, ps2=96, np1=3, ps1=96 + 24), chaincase('chain_C96_r203_no_d2', 203, 96, d2out=False),
                  chaincase('chain_C128_r61', 61, 128, np2=1, ps2=0, np1=2, ps1=128), chaincase('chain_C128_r333_no_d2', 333, 128, d2out=False, np2=8, ps2=152, np1=1),
                  chaincase(f'chain_C{wide}_r16', 16, wide, np2=2, ps2=wide, np1=1), chaincase(f'chain_C{wide}_r203', 203, wide, d2out=False, np2=3, ps2=wide + 24, np1=8, ps1=wide)]
    if not f32:          # 32 vectors: LPR 32 in the 16-bit types (in f32 that is C = 96 / 128 above)
        m['chain'].append(chaincase('chain_C256_r77', 77, 256, np2=2, ps2=256, np1=3, ps1=256 + 24))
    return m


# ------------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def hostile_rows(rows, C, dt, gen, shift=0):
    """[rows, C] of +-U[0.25, 1) with, spread with period 11 (coprime to every run, sub-run and pass length used) and forced onto the last
    rows: rows around +-64 with spread 1 (multiples of 0.5: exact in bf16), constant rows, all-zero rows and one row of magnitude ~1e4.
    shift moves the pattern: the chain's x1 has its constant / zero rows (rstd = eps^-1/2 = 316) where x2 has none: 316^2 |dy| overflows fp16."""
    X = draw(rows * C, F32, gen, False).reshape(rows, C)
    kind = {3: '+', 5: 'c', 7: 'z', 9: '-'}
    kinds = [kind.get((r + shift) % 11, 'n') for r in range(rows)]
    tail = ['c', '+', 'z', 'b']
    if rows >= 6:
        for i in range(4):
            kinds[rows - 1 - i] = tail[(i + (1 if shift else 0)) % 4]
    elif rows >= 2:
        kinds[rows - 1] = 'b'
    for r, k in enumerate(kinds):
        if k in '+-':
            o = 0.5 * torch.randint(-2, 3, (C,), generator=gen).float()
            X[r] = (64.0 + o) * (1.0 if k == '+' else -1.0)
        elif k == 'c':
            X[r] = X[r, 0].item()
        elif k == 'z':
            X[r] = 0.0
        elif k == 'b':
            X[r] = X[r] * 8192.0
    return X.to(dt)


class Buf:
    def __init__(self, n, dt, base, idx, values, out):
        self.init = pattern(GUARD + n + GUARD, dt)
        self.base, self.idx, self.out = GUARD + base, (idx + GUARD + base), out
        if values is not None:
            self.init[self.idx.reshape(-1)] = values.reshape(-1).to(dt)

    def logical(self, flat):
        return flat[self.idx.reshape(-1)].reshape(self.idx.shape)


class Prep:
    pass


def x_index(cs):
    """flat position (relative to x) of logical element [row, c]; gather: row (b, i, j) = the four C0-wide quadrants in QUAD order"""
    rows, C = cs['rows'], cs['C']
    if not cs['gres']:
        return torch.arange(rows * C).reshape(rows, C)
    B, R, C0 = cs['B'], cs['gres'], cs['C0']
    pos = torch.arange(B * R * R * C0).reshape(B, R // 2, 2, R // 2, 2, C0)          # [b, i, di, j, dj, cc]
    return torch.cat([pos[:, :, di, :, dj, :] for di, dj in QUAD], -1).reshape(rows, C)


def row_group(cs):
    r = torch.arange(cs['rows'])
    return (r // cs['group_rows']) % cs['ngroups'] if cs['ngroups'] > 1 else torch.zeros_like(r)


def eps32(cs):
    return float(np.float32(cs['eps']))          # the ABI takes eps as a float


# ---- float64 references, one per entry point ------------------------------------------------------------------------------------------
def ref_forward(X, Gm, Bt, R, eps):
    """X, Gm, Bt (, R): [rows, C] float64 (gamma / beta already picked per row) -> y, mean, rstd and their bounds"""
    mu = X.mean(1, keepdim=True)
    var = ((X - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (X - mu) * rstd * Gm + Bt
    T = (X.abs() + mu.abs()) * rstd * Gm.abs() + Bt.abs()
    if R is not None:
        y, T = y + R, T + R.abs()
    A = X.abs().mean(1, keepdim=True)
    T_rstd = rstd * (1.0 + (var + EPSF * A * A) / (var + eps))
    return dict(y=y, mean=mu[:, 0], rstd=rstd[:, 0]), dict(y=T, mean=A[:, 0], rstd=T_rstd[:, 0])


def ref_backward(DY, X, Gm, mean, rstd, DR, grp, ngroups):
    xh = (X - mean[:, None]) * rstd[:, None]
    gg = DY * Gm
    dx = rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    T = rstd[:, None] * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg.abs() * xh.abs()).mean(1, keepdim=True))
    if DR is not None:
        dx, T = dx + DR, T + DR.abs()
    z = torch.zeros(ngroups, X.shape[1], dtype=torch.float64)
    out = dict(dx=dx, dgamma=z.index_add(0, grp, DY * xh), dbeta=z.index_add(0, grp, DY))
    Ts = dict(dx=T, dgamma=z.index_add(0, grp, DY.abs() * xh.abs()), dbeta=z.index_add(0, grp, DY.abs()))
    return out, Ts


def ref_chain(DY, X2, g2, m2, r2, X1, g1, m1, r1, dt):
    """d2 = dLN2(dy) at x2, rounded once to dt (the documented hand-over); dx1 = dLN1(d2) at x1"""
    z = torch.zeros(DY.shape[0], dtype=torch.long)
    o2, T2 = ref_backward(DY, X2, g2[None, :].expand_as(DY), m2, r2, None, z, 1)
    d2 = o2['dx'].to(dt).double()
    o1, T1 = ref_backward(d2, X1, g1[None, :].expand_as(DY), m1, r1, None, z, 1)
    # a d2 element of the kernel may land on the neighbouring dt value: |delta d2| <= EPS[dt] |d2|, carried through LN1's (linear) backward
    _, Tx = ref_backward(d2.abs(), X1, g1.abs()[None, :].expand_as(DY), m1, r1, None, z, 1)
    out = dict(d2out=d2, dx1=o1['dx'], dgamma2=o2['dgamma'], dbeta2=o2['dbeta'], dgamma1=o1['dgamma'], dbeta1=o1['dbeta'])
    Ts = dict(d2out=T2['dx'], dx1=T1['dx'] + Tx['dx'], dgamma2=T2['dgamma'], dbeta2=T2['dbeta'], dgamma1=T1['dgamma'], dbeta1=T1['dbeta'])
    return out, Ts


# ---- one call: buffers, reference, bounds ---------------------------------------------------------------------------------------------
def _params(p, name, C, ng, gstride, nparts, pstride, vals, out, mis=0):
    idx = (torch.arange(nparts)[:, None, None] * pstride + torch.arange(ng)[None, :, None] * gstride + torch.arange(C)[None, None, :])
    p.bufs[name] = Buf(int(idx.max()) + 1 + mis, F32, mis, idx, vals, out)


def _twin_stats(rows):
    return torch.zeros(rows), torch.where(torch.arange(rows) % 2 == 0, torch.tensor(1.0), torch.tensor(0.5))


def prepare(cs, dt, kind, exact=False, benign=False):
    p = Prep()
    p.cs, p.dt, p.kind, p.exact, p.bufs, p.exact_names = cs, dt, kind, exact, {}, set()
    p.path = path_of(cs, dt, kind)
    rows, C = cs['rows'], cs['C']
    g = torch.Generator().manual_seed(4242 + 7 * rows + C + (100000 if exact else 0))
    if kind == 'chain':
        return _prepare_chain(p, g)
    ng, gs, eps = max(1, cs['ngroups']), cs['gstride'], eps32(cs)
    mis = lambda n: 1 if cs['mis'] == n else 0
    xi, grp = x_index(cs), row_group(cs)
    rc = torch.arange(rows * C).reshape(rows, C)
    X = draw(rows * C, dt, g, True, lim=2).reshape(rows, C) if exact else (draw(rows * C, dt, g, False).reshape(rows, C) if benign else hostile_rows(rows, C, dt, g))
    gam = draw(ng * C, F32, g, exact).reshape(1, ng, C)
    p.bufs['x'] = Buf(xi.numel() + mis('x') + cs['tail'], dt, mis('x'), xi, X, False)
    _params(p, 'gamma', C, ng, gs, 1, 0, gam, False, mis('gamma'))
    X64, Gm = X.double(), gam[0].double()[grp]
    if kind == 'fwd':
        bet = draw(ng * C, F32, g, False).reshape(1, ng, C)
        _params(p, 'beta', C, ng, gs, 1, 0, bet, False)
        R = None
        if cs['res']:
            Rv = draw(rows * C, dt, g, False).reshape(rows, C)
            p.bufs['res'] = Buf(rows * C + mis('res'), dt, mis('res'), rc, Rv, False)
            R = Rv.double()
        p.bufs['y'] = Buf(rows * C + mis('y'), dt, mis('y'), rc, None, True)
        for n in ('mean', 'rstd'):
            p.bufs[n] = Buf(rows, F32, 0, torch.arange(rows), None, True)
        p.ref, p.T = ref_forward(X64, Gm, bet[0].double()[grp], R, eps)
        p.eps_of = dict(y=dt, mean=F32, rstd=F32)
        return p
    DY = draw(rows * C, dt, g, exact).reshape(rows, C)
    p.bufs['dy'] = Buf(rows * C + mis('dy'), dt, mis('dy'), rc, DY, False)
    if exact:
        mean, rstd = _twin_stats(rows)
    else:
        f, _ = ref_forward(X64, Gm, Gm, None, eps)
        mean, rstd = f['mean'].float(), f['rstd'].float()
    p.bufs['mean'] = Buf(rows, F32, 0, torch.arange(rows), mean, False)
    p.bufs['rstd'] = Buf(rows, F32, 0, torch.arange(rows), rstd, False)
    DR = None
    if cs['dres']:
        DRv = draw(rows * C, dt, g, exact, lim=4).reshape(rows, C)
        p.bufs['dres'] = Buf(rows * C + mis('dres'), dt, mis('dres'), rc, DRv, False)
        DR = DRv.double()
    p.bufs['dx'] = Buf(xi.numel() + mis('dx') + cs['tail'], dt, mis('dx'), xi, None, True)
    npt, ps = cs['nparts'], cs['pstride']
    p.init = {}
    for n in ('dgamma', 'dbeta'):
        p.init[n] = draw(npt * ng * C, F32, g, exact, lim=50, scale=4.0).reshape(npt, ng, C)
        _params(p, n, C, ng, gs, npt, ps, p.init[n], True)
    p.ref, p.T = ref_backward(DY.double(), X64, Gm, mean.double(), rstd.double(), DR, grp, ng)
    for n in ('dgamma', 'dbeta'):
        p.ref[n] = p.ref[n] + p.init[n].double().sum(0)
        p.T[n] = p.T[n] + p.init[n].double().abs().sum(0)
    p.eps_of = dict(dx=dt, dgamma=F32, dbeta=F32)
    p.copies = dict(dgamma=min(npt, bwd_geometry(cs, dt)[0]), dbeta=min(npt, bwd_geometry(cs, dt)[0]))
    # exact twin: every dy xh and every partial sum is an integer multiple of 1/2 below 2^24; dx divides by C: exact for a power of two
    p.exact_names = ({'dgamma', 'dbeta'} | ({'dx'} if (C & (C - 1)) == 0 else set())) if exact else set()
    return p


def _prepare_chain(p, g):
    cs, dt, exact = p.cs, p.dt, p.exact
    rows, C, eps = cs['rows'], cs['C'], eps32(cs)
    rc = torch.arange(rows * C).reshape(rows, C)
    X2, X1 = ((draw(rows * C, dt, g, True, lim=2).reshape(rows, C) for _ in range(2)) if exact else (hostile_rows(rows, C, dt, g, sh) for sh in (0, 4)))
    DY = draw(rows * C, dt, g, exact).reshape(rows, C)
    g2, g1 = draw(C, F32, g, exact), draw(C, F32, g, exact)
    st = {}
    for n, X in (('2', X2), ('1', X1)):
        if exact:
            st['mean' + n], st['rstd' + n] = _twin_stats(rows)
        else:
            ones = torch.ones(rows, C, dtype=torch.float64)
            f, _ = ref_forward(X.double(), ones, ones, None, eps)
            st['mean' + n], st['rstd' + n] = f['mean'].float(), f['rstd'].float()
    for n, v in (('dy', DY), ('x2', X2), ('x1', X1)):
        p.bufs[n] = Buf(rows * C, dt, 0, rc, v, False)
    for n, v in (('gamma2', g2), ('gamma1', g1)):
        _params(p, n, C, 1, 0, 1, 0, v.reshape(1, 1, C), False)
    for n, v in st.items():
        p.bufs[n] = Buf(rows, F32, 0, torch.arange(rows), v, False)
    p.bufs['d2out'] = Buf(rows * C, dt, 0, rc, None, True)          # allocated in every case, handed over only when cs['d2out']
    p.bufs['dx1'] = Buf(rows * C, dt, 0, rc, None, True)
    p.init = {}
    for n, npt, ps in (('dgamma2', cs['np2'], cs['ps2']), ('dbeta2', cs['np2'], cs['ps2']), ('dgamma1', cs['np1'], cs['ps1']), ('dbeta1', cs['np1'], cs['ps1'])):
        p.init[n] = draw(npt * C, F32, g, exact, lim=50, scale=4.0).reshape(npt, 1, C)
        _params(p, n, C, 1, 0, npt, ps, p.init[n], True)
    p.ref, p.T = ref_chain(DY.double(), X2.double(), g2.double(), st['mean2'].double(), st['rstd2'].double(), X1.double(), g1.double(),
                           st['mean1'].double(), st['rstd1'].double(), dt)
    p.extra = {}
    for n in p.init:
        p.ref[n] = p.ref[n] + p.init[n].double().sum(0)
        p.T[n] = p.T[n] + p.init[n].double().abs().sum(0)
    # the same neighbouring-value term for the sums LN1 takes over d2: sum_rows EPS[dt] |d2| |xh1| and sum_rows EPS[dt] |d2|
    z = torch.zeros(rows, dtype=torch.long)
    d2a = p.ref['d2out'].abs()
    _, Tn = ref_backward(d2a, X1.double(), torch.ones(rows, C, dtype=torch.float64), st['mean1'].double(), st['rstd1'].double(), None, z, 1)
    p.extra = dict(dgamma1=EPS_ELEM[dt] * Tn['dgamma'], dbeta1=EPS_ELEM[dt] * Tn['dbeta'])
    p.eps_of = dict(d2out=dt, dx1=dt, dgamma2=F32, dbeta2=F32, dgamma1=F32, dbeta1=F32)
    nb = chain_blocks(cs, dt)
    p.copies = dict(dgamma2=min(cs['np2'], nb), dbeta2=min(cs['np2'], nb), dgamma1=min(cs['np1'], nb), dbeta1=min(cs['np1'], nb))
    # exact twin: dgamma2 / dbeta2 always.  d2 is a multiple of 2^-3 / C below 2^6 when C is a power of two: exact in f32 (at most 18 bits),
    # so both sides round the same value to dt.  sum_rows d2 xh1 is then a multiple of 2^-4 / C below 2^7 rows: exact in f32 in any order
    # while 2^11 rows C <= 2^24.  dx1 divides a second time by C (multiples of 2^-7 / C^2 below 2^9): 24 bits only at C = 8.
    p.exact_names = set()
    if exact:
        p.exact_names = {'dgamma2', 'dbeta2'}
        if (C & (C - 1)) == 0:
            p.exact_names |= {'d2out'} | ({'dgamma1', 'dbeta1'} if rows * C <= 8192 else set()) | ({'dx1'} if C <= 8 else set())
    return p


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def judge(p, after, ratios=None, per_copy=False):
    """after: name -> the flat CPU buffer as the call left it.  Raises AssertionError; appends (entry, path, dtype, output, case, ratio, eps)."""
    cs, label = p.cs, p.cs['name'] + f' {p.kind}' + (' (exact twin)' if p.exact else '')
    for name, b in p.bufs.items():
        keep = torch.ones(b.init.numel(), dtype=torch.bool)
        if b.out and not (name == 'd2out' and not cs['d2out']):
            keep[b.idx.reshape(-1)] = False
        bad = (bits(after[name])[keep] != bits(b.init)[keep]).nonzero()
        assert bad.numel() == 0, f'{label}: {bad.numel()} elements of {name} outside the output changed, first at flat index {int(keep.nonzero()[bad[0, 0]])}'
    for name, ref in p.ref.items():
        if name == 'd2out' and not cs['d2out']:
            continue
        b = p.bufs[name]
        got = b.logical(after[name]).double()
        odt = p.eps_of[name]
        is_param = got.dim() == 3
        if is_param:
            if per_copy and p.exact and got.shape[0] > 1:
                for c in range(p.copies[name]):
                    assert bool((got[c] != p.init[name][c].double()).any()), f'{label}: copy {c} of {name} received nothing ({p.copies[name]} workgroups share {got.shape[0]} copies)'
            got = got.sum(0)
        if name in p.exact_names:
            want = ref.to(odt).double()
            ne = got != want          # NaN (an element nobody wrote) differs from everything
            assert not bool(ne.any()), (f'{label}: {int(ne.sum())} of {ne.numel()} elements of {name} differ from the exact result, first '
                                        f'{tuple(ne.nonzero()[0].tolist())}: got {float(got[ne][0])}, want {float(want[ne][0])}')
            continue
        eps = EPS_ELEM[odt]
        T = p.T[name].reshape(ref.shape)
        if name in getattr(p, 'extra', {}):
            T = T + p.extra[name].reshape(ref.shape) / eps
        err = (got.reshape(ref.shape) - ref).abs()
        ok = err <= eps * T           # False for NaN
        ratio = float((err / (T + 1e-300)).nan_to_num(nan=float('inf')).max())
        if ratios is not None:
            ratios.append((p.kind, p.path, str(p.dt), name, cs['name'], ratio, eps))
        assert bool(ok.all()), (f'{label}: {name}: {int((~ok).sum())} of {ok.numel()} elements over the bound, largest |err| / T = {ratio:.3e} '
                                f'(bound {eps:.3e}), first at {tuple((~ok).nonzero()[0].tolist())}')


def report(ratios, title):
    best = {}
    for kind, path, dt, name, case, r, eps in ratios:
        k = (kind, path, dt, name)
        if k not in best or r > best[k][0]:
            best[k] = (r, case, eps)
    print()
    for (kind, path, dt, name), (r, case, eps) in sorted(best.items()):
        print(f'{title} {kind:5s} {path:12s} {dt:15s} {name:8s} largest |err| / T {r:.3e} ({case}), bound {eps:.3e}')
