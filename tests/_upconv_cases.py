"""The up-conv weight-gradient chain (stj_upconv_prep -> stj_upconv_wgrad -> stj_upconv_fold, csrc/conv.hip and csrc/conv_ws.hip): float64
statements from the header formulas, the case table with the kernel each row is meant to reach, a plain Python copy of the dispatch
conditions, the judgement, and the mutated statements the judgement must reject.  No GPU is needed to import or test this module
(test_upconv_wgrad_ref.py); test_upconv_wgrad_abi_gpu.py runs the table through the C ABI.

Layouts (NHWC / row-major, as the entry points take them):
    X [F,Hi,Wi,Cin]   dP [F,2Hi,2Wi,Cout]   dWeff f32 [16,Cout,Cin]   dbias f32 [db_parts,Cout]   W, dW f32 [3,3,Cin,Cout]
    Wf [16,Cout,Cin]   Wd [16,Cin,Cout]
Statements:
    dWeff[a*8+b*4+r*2+s][co][ci] = sum_{f,i,j} dP[f,2i+a,2j+b,co] * X[f,i+a-1+r,j+b-1+s,ci]      (X zero outside the map)
    dbias[co]                    = sum dP[...,co]
    dW[dy][dx][ci][co]           = sum_{a,b} dWeff[a,b,r(a,dy),s(b,dx)][co][ci],  r(0,.) = (0,1,1), r(1,.) = (0,0,1) over dy = 0,1,2
    Wf[pt][co][ci]               = sum_{dy in R(a,r), dx in R(b,s)} W[dy][dx][ci][co] = Wd[(u+1)*4+(v+1)][ci][co], u = 2-a-2r, v = 2-b-2s
    R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}   (tap indices dy + 1; the head comment of conv.hip in offsets)

Judgement (judge_values), per case and element type, on two data sets:
  * exact twin: X, dP and the starting contents of dWeff, dbias and dW are integers in [-3, 3].  Every product and every f32 partial sum is
    exact in any order while 9 * 4 * F Hi Wi < 2^24 (|dWeff| <= 9 P, |dbias| <= 3 * 4 P, a folded tap <= 9 * 4 P; the table test asserts
    it), so dWeff, the sum of the dbias copies and dW after the fold must EQUAL start + reference; every dbias copy is an integer within
    3 * 4 P of its start.
  * random twin: operands +-U[0.25, 1) rounded to the element type; per element |got - ref| <= GATE[path] * sum |terms|, the sum evaluated
    by the same statement on |X|, |dP| (plus |start|).  GATE starts at EPS_ELEM[float32] = 2^-17, the project's bound for f32 outputs of
    exact products, and is four times the largest ratio measured on an MI355X where that is below a quarter of 2^-17 (see GATE below).
A chunk, for the mutations and the launch mirror, is what one barrier pair of the kernel consumes: 128 low-res pixels (4 rows x 32 columns
or 8 rows x 16 columns) on the transpose-read paths, one row segment of up to 32 columns on the generic path.
"""
import zlib

import torch

from test_gemm_gpu import GUARD, bits, draw, pattern        # noqa: F401  (GUARD, bits, pattern: for the two test modules)
from test_ops_gpu import EPS_ELEM

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
ALL = (F32, BF16, F16)
PATHS = ('G36', 'G44', 'TR36/32', 'TR36/16', 'TR44/32', 'TR44/16', 'TR4_36/32', 'TR4_64/32', 'TR4_44/32', 'TR4_36/16', 'TR4_64/16', 'TR4_44/16')
BIG = 100000                    # low-res pixels from which the float64 reference is evaluated on the device
RTAB = ((0, 1, 1), (0, 0, 1))   # r(a, dy): which of phase a's two taps reads 3x3 tap row dy
RSET = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}

# Per-path gate of the random twin.  2^-17 = 7.63e-06 is the bound; two runs on an MI355X measured the ratios below (the largest of a path
# over both runs, its rows, element types, outputs, budgets and dbias modes; profiles/test_upconv_wgrad_ratios.txt is a later run under
# these gates), all below a quarter of the bound, so every path's gate is four times its own largest ratio.  What sets the ratio: exact
# products, f32 accumulation -- the rounding of each partial sum, relative to sum |terms|.  It is largest where one element is one term plus a non-zero start (the one-pixel map: 2^-24 of the
# result, G36) and where one strip sums all 262144 pixels in one accumulator (wg_budget = 1: TR4_36/32; 3.1e-09 at the default budget).
MEASURED = {'G36': 1.100e-07, 'G44': 1.276e-07, 'TR36/32': 1.399e-08, 'TR36/16': 1.648e-08, 'TR44/32': 3.503e-08, 'TR44/16': 2.561e-08,
            'TR4_36/32': 7.584e-08, 'TR4_64/32': 4.490e-09, 'TR4_44/32': 7.608e-09, 'TR4_36/16': 3.420e-09, 'TR4_64/16': 3.859e-09,
            'TR4_44/16': 3.078e-09}
GATE = {p: (4 * MEASURED[p] if 4 * MEASURED[p] < EPS_ELEM[F32] else EPS_ELEM[F32]) for p in PATHS}


def phases():
    for pt in range(16):
        yield pt, pt >> 3, (pt >> 2) & 1, (pt >> 1) & 1, pt & 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tmm(D, Xs):
    """D^T Xs over the pixel axis; on the device in 256 blocks summed afterwards (a [Cout, Cin] result of a 262144-deep product would
    otherwise run on a handful of workgroups)"""
    n = D.shape[0]
    if D.is_cuda and n >= 32768 and n % 256 == 0:
        return (D.view(256, n // 256, -1).transpose(1, 2) @ Xs.view(256, n // 256, -1)).sum(0)
    return D.t() @ Xs


def pad_ring(X):
    F, Hi, Wi, Cin = X.shape
    Xp = X.new_zeros(F, Hi + 2, Wi + 2, Cin)
    Xp[:, 1:Hi + 1, 1:Wi + 1] = X
    return Xp


def dweff_from_padded(Xp, dP):
    F, Hp, Wp, Cin = Xp.shape
    Hi, Wi, Cout = Hp - 2, Wp - 2, dP.shape[3]
    assert tuple(dP.shape) == (F, 2 * Hi, 2 * Wi, Cout), (tuple(Xp.shape), tuple(dP.shape))
    out = Xp.new_empty(16, Cout, Cin)
    for pt, a, b, r, s in phases():
        D = dP[:, a::2, b::2].reshape(-1, Cout)
        Xs = Xp[:, a + r:a + r + Hi, b + s:b + s + Wi].reshape(-1, Cin)      # X row i + a - 1 + r is padded row i + a + r
        out[pt] = _tmm(D, Xs)
    return out


def dweff_ref(X, dP):
    """(dWeff [16,Cout,Cin], dbias [Cout]) in float64 on the device the operands are on"""
    X, dP = X.double(), dP.double()
    return dweff_from_padded(pad_ring(X), dP), dP.sum((0, 1, 2))


def fold_ref(dWeff):
    _, Cout, Cin = dWeff.shape
    g = dWeff.double().reshape(2, 2, 2, 2, Cout, Cin)
    dW = g.new_zeros(3, 3, Cin, Cout)
    for dy in range(3):
        for dx in range(3):
            for a in range(2):
                for b in range(2):
                    dW[dy, dx] += g[a, b, RTAB[a][dy], RTAB[b][dx]].t()
    return dW


def prep_ref(W):
    """(Wf [16,Cout,Cin], Wd [16,Cin,Cout]) in float64"""
    W = W.double()
    _, _, Cin, Cout = W.shape
    Wf, Wd = W.new_zeros(16, Cout, Cin), W.new_zeros(16, Cin, Cout)
    for pt, a, b, r, s in phases():
        acc = W.new_zeros(Cin, Cout)
        for dy in RSET[a, r]:
            for dx in RSET[b, s]:
                acc = acc + W[dy, dx]
        Wf[pt] = acc.t()
        u, v = 2 - a - 2 * r, 2 - b - 2 * s
        Wd[(u + 1) * 4 + (v + 1)] = acc
    return Wf, Wd


def upsample_pad(X):
    """nearest 2x up-sample of X [F,Hi,Wi,C] with a zero ring: [F,2Hi+2,2Wi+2,C]"""
    F, Hi, Wi, C = X.shape
    U = X.new_zeros(F, 2 * Hi + 2, 2 * Wi + 2, C)
    U[:, 1:-1, 1:-1] = X.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return U


def chain_ref(X, dP):
    """(dW [3,3,Cin,Cout], dbias [Cout]): float64 autograd gradient of sum(dP * y), y = conv3x3_same(upsample2x_nearest(X), W) + bias, the
    convolution written as nine shifted matmuls (device-agnostic; test_upconv_wgrad_ref.py holds it to torch's conv2d)."""
    X, dP = X.double(), dP.double()
    F, Hi, Wi, Cin = X.shape
    Cout = dP.shape[3]
    U = upsample_pad(X)
    W = X.new_zeros(3, 3, Cin, Cout, requires_grad=True)
    bias = X.new_zeros(Cout, requires_grad=True)
    G = dP.reshape(-1, Cout)
    for dy in range(3):
        for dx in range(3):
            y = U[:, dy:dy + 2 * Hi, dx:dx + 2 * Wi].reshape(-1, Cin) @ W[dy, dx]
            (y * G).sum().backward()
    (bias.expand_as(G) * G).sum().backward()
    return W.grad.detach(), bias.grad.detach()


# ---------------------------------------------------------------------------------------------------------------------------------------
# dispatch mirror: stj_upconv_wgrad -> upconv_wgrad_tr_try -> wgrad_tr_launch (-> wgrad_tr4_launch) | upconv_wgrad_launch
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tr_geometry(dt, Hi, Wi, Cin, Cout):
    """chunk width of the transpose-read family, or None: bf16, channels % 8 == 0, Wi % 32 == 0 and Hi % 4 == 0 or Wi % 16 == 0 and Hi % 8 == 0"""
    if dt != BF16 or Cin % 8 or Cout % 8:
        return None
    if Wi % 32 == 0 and Hi % 4 == 0:
        return 32
    if Wi % 16 == 0 and Hi % 8 == 0:
        return 16
    return None


def expected_path(dt, F, Hi, Wi, Cin, Cout):
    small = Cout <= 48 and Cin <= 96
    CW = _tr_geometry(dt, Hi, Wi, Cin, Cout)
    if CW is None:
        return 'G36' if small else 'G44'
    CR = 128 // CW
    nchunks = F * (Hi // CR) * (Wi // CW)
    if Hi % (256 // CW) == 0 and nchunks >= 2048:
        if small:
            return f'TR4_36/{CW}'
        if Cout == 96 and Cin % 64 == 0:
            return f'TR4_64/{CW}'
        return f'TR4_44/{CW}'
    return f'TR36/{CW}' if small else f'TR44/{CW}'


def cdiv(a, b):
    return (a + b - 1) // b


def launch_geometry(dt, F, Hi, Wi, Cin, Cout, wg_budget=0):
    """What the launcher of expected_path(...) computes: chunks, channel tiles, strips of cpb chunks (the last one holds `last`), the strips
    the grid is rounded up to (the surplus workgroups return at once) and the workgroup count."""
    path = expected_path(dt, F, Hi, Wi, Cin, Cout)
    t44 = cdiv(Cout, 64) * cdiv(Cin, 64)
    if path[0] == 'G':
        nchunks = F * Hi * cdiv(Wi, 32)
        tiles = 1 if path == 'G36' else t44
        want, per_strip, round8 = max(1, 1024 // (4 * tiles)), 4 * tiles, False
    else:
        CW = int(path.split('/')[1])
        nchunks = F * (Hi // (128 // CW)) * (Wi // CW)
        kind = path.split('/')[0]
        if kind == 'TR36':
            tiles, want, per_strip = 1, 256, 4
        elif kind == 'TR44':
            tiles = t44
            want, per_strip = max(1, 1024 // (4 * tiles)), 4 * tiles
        else:
            tiles = {'TR4_36': 1, 'TR4_64': Cin // 64, 'TR4_44': t44}[kind]
            want, per_strip = max(1, (wg_budget if wg_budget > 0 else 128) // (2 * tiles)), 2 * tiles
        round8 = True
    strips = min(nchunks, want)
    cpb = cdiv(nchunks, strips)
    strips = cdiv(nchunks, cpb)
    grid_strips = cdiv(strips, 8) * 8 if round8 else strips
    return dict(path=path, nchunks=nchunks, tiles=tiles, strips=strips, cpb=cpb, last=nchunks - (strips - 1) * cpb, grid_strips=grid_strips,
                grid=grid_strips * per_strip)


def chunk_index(path, F, Hi, Wi):
    """chunk number of every low-res pixel, [F,Hi,Wi] (raster order of the kernels: frame, row group, column segment)"""
    f, i, j = torch.meshgrid(torch.arange(F), torch.arange(Hi), torch.arange(Wi), indexing='ij')
    if path[0] == 'G':
        return (f * Hi + i) * cdiv(Wi, 32) + j // 32
    CW = int(path.split('/')[1])
    CR = 128 // CW
    return (f * (Hi // CR) + i // CR) * (Wi // CW) + j // CW


# ---------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------
def _case(path, shape, dts=(BF16,), **kw):
    d = dict(path=path, shape=shape, dts=tuple(dts), name='x'.join(str(v) for v in shape), budgets=(0,))
    d.update(kw)
    return d


CASES = [
    # generic kernel, 48 x 96 tile: bf16 lands here because the geometry fits neither transpose-read rule
    _case('G36', (2, 5, 37, 24, 40), ALL),            # a ragged 32-column segment, channels below the tile
    _case('G36', (1, 1, 1, 8, 8), ALL),               # a map that is all halo
    _case('G36', (2, 8, 32, 96, 48), (F32, F16)),     # (bf16: TR36/32, below)
    _case('G44', (1, 3, 33, 72, 136), ALL),           # 3 x 2 ragged channel tiles
    _case('G44', (1, 131, 24, 128, 96), ALL, geo=dict(cpb=3, strips=44, last=2)),
    _case('TR36/32', (2, 8, 32, 96, 48)),
    _case('TR36/32', (3, 4, 64, 40, 24)),             # rectangular, ragged channels
    _case('TR36/32', (9, 32, 128, 96, 48), geo=dict(nchunks=288, strips=144, cpb=2, last=2)),
    _case('TR36/16', (2, 8, 16, 96, 48)),
    _case('TR36/16', (1, 16, 48, 96, 48)),
    _case('TR44/32', (2, 8, 32, 128, 96), budgets=(0, 256)),      # a half-empty second cout tile; wg_budget is not this path's to read
    _case('TR44/32', (1, 4, 32, 384, 192), geo=dict(tiles=18)),
    _case('TR44/32', (1, 4, 32, 72, 136)),            # ragged channels both ways
    _case('TR44/32', (5, 20, 96, 128, 96), geo=dict(nchunks=75, cpb=2, last=1)),
    _case('TR44/16', (2, 8, 16, 192, 128)),
    _case('TR4_36/32', (64, 64, 64, 96, 48), budgets=(0, 256, 140, 4096, 1), geo=dict(nchunks=2048)),
    _case('TR4_36/32', (9, 64, 512, 40, 24), geo=dict(nchunks=2304)),       # rectangular, ragged channels
    _case('TR4_64/32', (64, 64, 64, 64, 96), geo=dict(tiles=1)),
    _case('TR4_64/32', (64, 64, 64, 128, 96), geo=dict(tiles=2)),           # the model's layer
    _case('TR4_44/32', (64, 64, 64, 8, 56)),
    _case('TR4_44/32', (16, 128, 128, 72, 72), geo=dict(tiles=4)),
    _case('TR4_36/16', (1024, 16, 16, 96, 48), geo=dict(nchunks=2048)),
    _case('TR4_64/16', (1024, 16, 16, 64, 96)),
    _case('TR4_44/16', (1024, 16, 16, 8, 56)),
    _case('TR4_36/16', (344, 16, 48, 96, 48), geo=dict(nchunks=2064)),      # three segments per row
]
# the launch mirror at the five budgets of (64,64,64,96,48)
BUDGET_GEO = {0: dict(strips=64, cpb=32, last=32, grid_strips=64, grid=128),
              256: dict(strips=128, cpb=16, last=16, grid_strips=128, grid=256),
              140: dict(strips=69, cpb=30, last=8, grid_strips=72, grid=144),
              4096: dict(strips=2048, cpb=1, last=1, grid_strips=2048, grid=4096),        # no prefetch: every strip is one chunk
              1: dict(strips=1, cpb=2048, last=2048, grid_strips=8, grid=16)}             # one strip walks all chunks
DB_MODES = (1, 7, None)         # db_parts (7: co-prime with every grid of the table); None: dbias == NULL
PREP_SHAPES = [(8, 8), (24, 40), (72, 136), (96, 48), (384, 192)]       # (Cin, Cout); the last one is beyond one pass of the 2048-block grid


def pixels(cs):
    F, Hi, Wi, _, _ = cs['shape']
    return F * Hi * Wi


def rows(pred=lambda cs: True):
    """(case, dtype) pairs of the table"""
    return [(cs, dt) for cs in CASES for dt in cs['dts'] if pred(cs)]


def case_id(v):
    if isinstance(v, dict):
        return v['path'].replace('/', '_') + '-' + v['name']
    return str(v).replace('torch.', '')


def first_of_path(cs, dt):
    """the first (case, dtype) of its path in table order: it starts from zeros in the random twin and runs the chain against autograd"""
    for c, d in rows():
        if c['path'] == cs['path']:
            return c is cs and d == dt
    return False


# ---------------------------------------------------------------------------------------------------------------------------------------
# data and judgement
# ---------------------------------------------------------------------------------------------------------------------------------------
def draw_on(device, n, dt, seed, exact, lim=3, scale=1.0):
    """test_gemm_gpu.draw on the CPU; for a device the same two distributions drawn there (the large cases: ~300 MB of operands)"""
    if torch.device(device).type == 'cpu':
        return draw(n, dt, torch.Generator().manual_seed(seed), exact, lim=lim, scale=scale)
    g = torch.Generator(device=device).manual_seed(seed)
    if exact:
        return torch.randint(-lim, lim + 1, (n,), generator=g, device=device).to(dt)
    mag = torch.rand(n, generator=g, device=device) * 0.75 + 0.25
    sgn = torch.randint(0, 2, (n,), generator=g, device=device) * 2 - 1
    return (mag * sgn * scale).to(dt)


def _seed(cs):
    return zlib.crc32(str(cs['shape']).encode()) & 0xFFFFFF


def operands(cs, dt, exact, device='cpu'):
    """X [F,Hi,Wi,Cin], dP [F,2Hi,2Wi,Cout] of the element type on `device`"""
    F, Hi, Wi, Cin, Cout = cs['shape']
    seed = _seed(cs) + 2 * ALL.index(dt) + int(exact)
    X = draw_on(device, F * Hi * Wi * Cin, dt, seed, exact).view(F, Hi, Wi, Cin)
    dP = draw_on(device, F * 4 * Hi * Wi * Cout, dt, seed + 100003, exact).view(F, 2 * Hi, 2 * Wi, Cout)
    return X, dP


class Ref:
    """float64 on the CPU: dweff, db and the sums of |terms| Tw, Tdb"""


def reference(X, dP):
    R = Ref()
    w, b = dweff_ref(X, dP)
    tw, tb = dweff_ref(X.abs(), dP.abs())
    R.dweff, R.db, R.Tw, R.Tdb = w.cpu(), b.cpu(), tw.cpu(), tb.cpu()
    return R


def starts(cs, dt, exact, parts, zero):
    """starting contents of dWeff [16,Cout,Cin], dbias [parts,Cout] (None with dbias == NULL) and dW [3,3,Cin,Cout], f32 on the CPU"""
    _, _, _, Cin, Cout = cs['shape']
    g = torch.Generator().manual_seed(_seed(cs) + 1000 + 16 * ALL.index(dt) + (parts or 0))

    def one(*shape):
        n = 1
        for v in shape:
            n *= v
        return torch.zeros(shape) if zero else draw(n, F32, g, exact, lim=3, scale=4.0).view(shape)
    return dict(dweff=one(16, Cout, Cin), db=one(parts, Cout) if parts else None, dw=one(3, 3, Cin, Cout))


def judge_values(label, exact, gate, R, start, got, P):
    """got / start: dict(dweff [16,Cout,Cin], db [parts,Cout] | None, dw [3,3,Cin,Cout] | None).  Returns (failures, {output: ratio}); the
    ratios are empty on the exact twin."""
    fails, ratios = [], {}
    want_w = start['dweff'].double() + R.dweff
    T_w = start['dweff'].double().abs() + R.Tw
    items = [('dWeff', got['dweff'].double(), want_w, T_w)]
    if got.get('db') is not None:
        s = start['db'].double()
        items.append(('dbias', got['db'].double().sum(0), s.sum(0) + R.db, s.abs().sum(0) + R.Tdb))
        if exact:
            d = got['db'].double()
            if not bool((d == d.round()).all()):
                fails.append(f'{label}: a dbias copy holds a non-integer')
            elif not bool(((d - s).abs() <= 12 * P).all()):
                fails.append(f'{label}: a dbias copy left its band of 3 * 4 * {P} around its start')
    if got.get('dw') is not None:
        s = start['dw'].double()
        items.append(('dW', got['dw'].double(), s + fold_ref(want_w), s.abs() + fold_ref(T_w)))
    for name, g, want, T in items:
        if exact:
            ne = g != want                       # NaN != anything: an element nobody wrote, or one fed from a guard, differs
            if bool(ne.any()):
                ix = tuple(ne.nonzero()[0].tolist())
                fails.append(f'{label}: {name}: {int(ne.sum())} of {ne.numel()} elements differ from the exact result, first {ix}: got '
                             f'{float(g[ix])}, want {float(want[ix])}')
        else:
            err = (g - want).abs() / (T + 1e-300)
            ratio = float(torch.nan_to_num(err, nan=float('inf')).max())
            ratios[name] = ratio
            if not ratio <= gate:
                fails.append(f'{label}: {name}: max |err| / sum |terms| = {ratio:.3e} over the gate {gate:.3e}')
    return fails, ratios


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutated statements: what a subtly wrong kernel would compute.  Each returns (dWeff, dbias) in float64.
# ---------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('drop_chunk', 'drop_last_strip', 'swap_r_a1', 'halo_hw_swapped', 'right_halo_twice', 'dbias_one_parity')


def _without_pixels(X, dP, keep):
    """the statement with the low-res pixels where keep [F,Hi,Wi] is False left out: their four outputs contribute nothing"""
    m = keep.repeat_interleave(2, 1).repeat_interleave(2, 2).unsqueeze(-1).to(dP.dtype)
    return dweff_ref(X, dP * m)


def mutated(kind, cs, dt, X, dP, R):
    F, Hi, Wi, Cin, Cout = cs['shape']
    geo = launch_geometry(dt, *cs['shape'])
    Xd, Pd = X.double(), dP.double()
    if kind == 'drop_chunk':
        return _without_pixels(Xd, Pd, chunk_index(geo['path'], F, Hi, Wi) != geo['nchunks'] // 2)
    if kind == 'drop_last_strip':
        return _without_pixels(Xd, Pd, chunk_index(geo['path'], F, Hi, Wi) < (geo['strips'] - 1) * geo['cpb'])
    if kind == 'swap_r_a1':
        w = R.dweff.reshape(2, 2, 2, 2, Cout, Cin).clone()
        w[1] = w[1].flip(1)
        return w.reshape(16, Cout, Cin), R.db
    if kind == 'halo_hw_swapped':                  # the in-map test written gy < Wi && gx < Hi: the map beyond the smaller extent reads as zero
        Xm = Xd.clone()
        Xm[:, min(Hi, Wi):] = 0
        Xm[:, :, min(Hi, Wi):] = 0
        return dweff_ref(Xm, Pd)[0], R.db
    if kind == 'right_halo_twice':                 # frame 0: the zero column right of the map holds the map's last column again
        Xp = pad_ring(Xd)
        Xp[0, 1:Hi + 1, Wi + 1] = Xd[0, :, Wi - 1]
        return dweff_from_padded(Xp, Pd), R.db
    if kind == 'dbias_one_parity':
        return R.dweff, Pd[:, :, 0::2].sum((0, 1, 2))
    raise KeyError(kind)
