"""stj_upconv_fwd, stj_upconv_fwd_res and stj_upconv_dgrad through the raw C ABI, per dispatch path, against the float64 statements of
_upconv_fwd_cases.py (which test_upconv_fwd_ref.py tests on the CPU, together with the dispatch mirrors and the judgement's sensitivity).

Every call is ops.call with raw pointers into flat guarded buffers; the kernels are handed Wf / Wd = prep_ref(W) cast to the element type on
the CPU.  Per table row and element type, two data sets (docstring of _upconv_fwd_cases.py): the exact twin, where the outputs must EQUAL the
rounded statement (ELU's negative branch: within the rounding of T of expm1), and the random twin, judged per element against
gate(path, T) * sum |terms|.  The input gradient runs every row with Xelu == NULL and with Xelu given.

  * every test asserts expected_*_path(row) == row.path before it launches; profiles/test_upconv_fwd_kernels.txt lists the kernels one run
    of this module launched, and every template the mirrors name is in it.
  * the first row of every path also runs stj_upconv_prep on the device (random twin) and is held to float64
    elu(conv2d(interpolate(x))) of torch and its autograd input gradient, at gate + the unit round-off of T (the folded weight's rounding).
  * stj_upconv_fwd_res on the random twin is also held bit for bit to stj_upconv_fwd on the same operands followed by torch adds in T.
  * guards: every operand and output lies between 64 NaN-pattern elements; outputs start as NaN pattern; guards and all inputs are compared
    bitwise after the call; all pointers are 16-byte aligned.
  * references: float64 on the CPU; on float64 device tensors for the rows above 100000 high-res pixels or 2^31 multiply-adds, and one
    mid-size row holds the two evaluations equal on the integer twin.
  * refusals return their status with a message and change no byte.

Found: one fault by reading, before the first run.  The wave-specialised forward at Cin = 128, Cout = 96 on whole tiles took the 1-D walker
grid (walkers a multiple of 8) whenever it had 8 tiles or more; with a tile count that is no multiple of 8 below 80 (12 tiles: 16 walkers) the
straight-line movers of the walkers without a tile drained their stage to the coordinates of tiles 12..15, past the end of Y.  No workload
shape has such a count (F is a multiple of 8 there).  ws2_launch_t now gives those shapes the 2-D grid, every walker of which has a tile; the
row (3,16,32,128,96) is in the table for it.  Nothing else was found wrong: all 138 exact twins (rows x element types, both Xelu modes of the
input gradient) report equality on all 18 paths -- rectangular maps, the ragged cout tiles of the wave-specialised forward, fp16 on the
generic and pipelined input gradients, the padded sequences of the pipelined one and the bf16 hand-over of the wave-specialised ones
included -- and stj_upconv_fwd_res equals stj_upconv_fwd + adds in T bit for bit.

Largest |err| / sum |terms| of the random twin per path and element type on an MI355X (MEASURED in _upconv_fwd_cases.py; the gate is four
times that where below EPS_ELEM = 2^-17 / 2^-7 / 2^-10, profiles/test_upconv_fwd_ratios.txt has the gates applied):
    path          bf16       fp16       f32           path       bf16       fp16       f32
    FG3           2.149e-03  2.725e-04  1.824e-07     DG4        7.573e-04  1.251e-04  2.378e-07
    FG4           2.397e-03  2.707e-04  1.973e-07     DG6        7.682e-04  8.903e-05  2.216e-07
    FWS96/E       1.604e-03  1.481e-04                DWS2/V3    1.150e-03
    FWS96/R       1.331e-03  1.509e-04                DWS2/G     9.243e-04
    FWS128/E      1.264e-03  1.324e-04                DWS        7.527e-04
    FWS128/E+X3   1.453e-03  1.242e-04                DPF        6.915e-04  9.971e-05
    FWS128/R      8.361e-04  1.181e-04                RES/FPS8   1.838e-03  2.395e-04
    FWS128/R+X3   9.913e-04  1.429e-04                RES/FPS16  2.187e-03  2.489e-04
    FPS8          8.790e-04  1.101e-04
    FPS16         9.977e-04  1.329e-04
With stj_upconv_prep on the device the first row of every path stays below 8.2e-04 (bf16) and 1.2e-07 (f32) against torch's conv2d.
The pipelined input gradient runs (3,32,64,384,192) on 16 sequences, not 40: its launcher lowers the count while the tile slots per sequence
stay the same (conv.hip, slots()); the mirror and its hand-written value in test_upconv_fwd_ref.py follow the launcher.
"""
import pytest
import torch

import _upconv_fwd_cases as UF
from _upconv_fwd_cases import BF16, ELU, F16, F32, GUARD, bits, pattern

pytestmark = pytest.mark.gpu

_RATIOS = []            # (path, dtype, case, output, ratio, gate)
_EXACT = []             # (path, dtype, case): exact twins that reported equality
U_ROUND = {F32: 2.0 ** -24, BF16: 2.0 ** -8, F16: 2.0 ** -11}      # unit round-off: one more rounding of the folded weight (prep rows)
OK, EINVAL, EUNSUPPORTED = 0, -1, -3


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()
    yield
    best = {}
    for path, dt, name, out, r, g in _RATIOS:
        k = (path, UF.case_id(dt))
        if k not in best or r > best[k][0]:
            best[k] = (r, name, out, g)
    print()
    for (path, dt), (r, name, out, g) in sorted(best.items()):
        print(f'upconv fwd/dgrad {path:12s} {dt:9s} largest |err| / sum |terms| {r:.3e} ({name}, {out}), gate {g:.3e}')
    print(f'upconv fwd/dgrad exact twins reporting equality: {len(_EXACT)} (rows x element types x modes), on {len(set(e[0] for e in _EXACT))} paths')


class Buf:
    """[GUARD pattern][vals][GUARD pattern] on the device, with its CPU image; vals None: an output of n elements, all pattern"""

    def __init__(self, vals=None, n=None, dt=None):
        if vals is not None:
            dt, n = vals.dtype, vals.numel()
        self.init = pattern(GUARD + n + GUARD, dt)
        if vals is not None:
            self.init[GUARD:GUARD + n] = vals.reshape(-1)
        self.dev = self.init.cuda()
        self.n = n

    @property
    def ptr(self):
        from strajnet_amd import ops
        p = ops._poff(self.dev, GUARD)
        assert p.value % 16 == 0
        return p

    def unchanged(self):
        return torch.equal(bits(self.dev.cpu()), bits(self.init))

    def flat(self):
        return self.dev.cpu(), self.init


def _null():
    from strajnet_amd import ops
    return ops._p(None)


def fwd_call(cs, dt, X, Wf, bias, Y, **over):
    from strajnet_amd import ops
    F, Hi, Wi, Cin, Cout = cs['shape']
    v = dict(F=F, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, act=cs['act'], dtype=ops.DTYPE_CODE[dt])
    v.update(over)
    return ('stj_upconv_fwd', X.ptr, Wf.ptr, bias.ptr, Y.ptr, v['F'], v['Hi'], v['Wi'], v['Cin'], v['Cout'], v['act'], v['dtype'], ops._st())


def res_call(cs, dt, X, Wf, bias, Y, R1, Y2, R2, **over):
    from strajnet_amd import ops
    F, Hi, Wi, Cin, Cout = cs['shape']
    v = dict(F=F, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, dtype=ops.DTYPE_CODE[dt])
    v.update(over)
    p = [b.ptr if b is not None else _null() for b in (R1, Y2, R2)]
    return ('stj_upconv_fwd_res', X.ptr, Wf.ptr, bias.ptr, Y.ptr, p[0], p[1], p[2], v['F'], v['Hi'], v['Wi'], v['Cin'], v['Cout'], v['dtype'], ops._st())


def dgrad_call(cs, dt, dP, Wd, dX, Xelu, **over):
    from strajnet_amd import ops
    F, Hi, Wi, Cin, Cout = cs['shape']
    v = dict(F=F, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, dtype=ops.DTYPE_CODE[dt])
    v.update(over)
    return ('stj_upconv_dgrad', dP.ptr, Wd.ptr, dX.ptr, Xelu.ptr if Xelu is not None else _null(), v['F'], v['Hi'], v['Wi'], v['Cin'], v['Cout'],
            v['dtype'], ops._st())


def device_prep(o, dt):
    """stj_upconv_prep of the row's f32 kernel on the device: (Wf, Wd) as guarded buffers (guards checked)"""
    from strajnet_amd import ops
    _, _, Cin, Cout = o.W.shape
    Wb = Buf(o.W)
    fb, db = Buf(n=16 * Cin * Cout, dt=dt), Buf(n=16 * Cin * Cout, dt=dt)
    ops.call('stj_upconv_prep', Wb.ptr, fb.ptr, db.ptr, Cin, Cout, ops.DTYPE_CODE[dt], ops._st())
    torch.cuda.synchronize()
    for b in (fb, db):
        got = b.dev.cpu()
        assert torch.equal(bits(got[:GUARD]), bits(b.init[:GUARD])) and torch.equal(bits(got[GUARD + b.n:]), bits(b.init[GUARD + b.n:]))
        b.init = got                                   # the image the later comparison holds it to
    assert Wb.unchanged()
    return fb, db


def _record(label, path, dt, name, ratios, g, failed, fails):
    failed += fails
    for out, r in ratios.items():
        print(f'{label:100s} {out:4s} |err| / sum |terms| = {r:.3e}  (gate {g:.3e})')
        _RATIOS.append((path, dt, name, out, r, g))


def _dev(cs):
    return 'cuda' if UF.on_device(cs) else 'cpu'


def run_fwd_row(cs, dt):
    """one forward or skip-sum row in one element type: both twins; the first row of a path also from the device's own prep"""
    from strajnet_amd import ops
    path = UF.expected_path(cs, dt)
    assert path == cs['path']
    F, Hi, Wi, Cin, Cout = cs['shape']
    n = F * 4 * Hi * Wi * Cout
    g = UF.gate(path, dt)
    failed = []
    for exact in (False, True):
        o = UF.operands(cs, dt, exact)
        R = UF.reference(cs, o, _dev(cs))
        ins = dict(X=Buf(o.X), Wf=Buf(o.Wf), bias=Buf(o.bias))
        if cs['kind'] == 'res':
            ins['R1'] = Buf(o.R1)
            if o.R2 is not None:
                ins['R2'] = Buf(o.R2)
        label = f"{cs['kind']} {cs['name']} [{UF.case_id(dt)}] {'exact' if exact else 'random'} twin"
        Y = Buf(n=n, dt=dt)
        flats, plain = {}, None
        if cs['kind'] == 'fwd':
            ops.call(*fwd_call(cs, dt, ins['X'], ins['Wf'], ins['bias'], Y))
        else:
            Y2 = Buf(n=n, dt=dt) if o.R2 is not None else None
            ops.call(*res_call(cs, dt, ins['X'], ins['Wf'], ins['bias'], Y, ins['R1'], Y2, ins.get('R2')))
            if Y2 is not None:
                torch.cuda.synchronize()
                flats['Y2'] = Y2.flat()
            if not exact:
                P = Buf(n=n, dt=dt)
                ops.call(*fwd_call(cs, dt, ins['X'], ins['Wf'], ins['bias'], P))
                torch.cuda.synchronize()
                plain = P.dev.cpu()[GUARD:GUARD + n].view(F, 2 * Hi, 2 * Wi, Cout)
        torch.cuda.synchronize()
        flats['Y'] = Y.flat()
        fails, ratios = UF.judge_fwd(label, cs, dt, exact, g, o, R, flats, plain)
        _record(label, path, dt, cs['name'], ratios, g, failed, fails)
        if not exact and cs['kind'] == 'fwd' and UF.first_of_path(cs, dt):
            # the chain from the f32 kernel: the device's own fold, against torch's float64 up-sample and convolution
            fb, _ = device_prep(o, dt)
            C = Buf(n=n, dt=dt)
            ops.call(*fwd_call(cs, dt, ins['X'], fb, ins['bias'], C))
            torch.cuda.synchronize()
            got, f = UF.unguard(label, 'Y (prep on the device)', *C.flat(), (F, 2 * Hi, 2 * Wi, Cout))
            failed += f
            want = UF.conv_ref(o.X, o.W, o.bias, cs['act'])
            S = UF.fwd_pre(o.X.abs(), UF.prep_ref(o.W.abs())[0], o.bias.abs())
            r = float(torch.nan_to_num((got.double() - want).abs() / (S + 1e-300), nan=float('inf')).max())
            gc = g + U_ROUND[dt]
            print(f'{label:100s} Y vs conv2d, prep on the device: |err| / sum |terms| = {r:.3e}  (gate {gc:.3e})')
            if not r <= gc:
                failed.append(f'{label}: Y with the device prep against conv2d: {r:.3e} over {gc:.3e}')
            if not fb.unchanged():
                failed.append(f'{label}: the entry point wrote Wf')
        for k, b in ins.items():
            if not b.unchanged():
                failed.append(f'{label}: the entry point wrote {k} (or its guards)')
        if exact and not failed:
            _EXACT.append((path, dt, cs['name']))
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


def run_dgrad_row(cs, dt):
    """one input-gradient row in one element type: both twins, Xelu == NULL and Xelu given"""
    from strajnet_amd import ops
    path = UF.expected_path(cs, dt)
    assert path == cs['path']
    F, Hi, Wi, Cin, Cout = cs['shape']
    n = F * Hi * Wi * Cin
    g = UF.gate(path, dt)
    failed = []
    for exact in (False, True):
        o = UF.operands(cs, dt, exact)
        R = UF.reference(cs, o, _dev(cs))
        ins = dict(dP=Buf(o.dP), Wd=Buf(o.Wd), Xelu=Buf(o.Xelu))
        chain = not exact and UF.first_of_path(cs, dt)
        db = device_prep(o, dt)[1] if chain else None
        for xelu in UF.XELU_MODES:
            label = f"dgrad {cs['name']} [{UF.case_id(dt)}] {'exact' if exact else 'random'} twin, Xelu {'given' if xelu else 'NULL'}"
            dX = Buf(n=n, dt=dt)
            ops.call(*dgrad_call(cs, dt, ins['dP'], ins['Wd'], dX, ins['Xelu'] if xelu else None))
            torch.cuda.synchronize()
            fails, ratios = UF.judge_dgrad(label, cs, dt, exact, g, o, R, xelu, *dX.flat())
            _record(label, path, dt, cs['name'], ratios, g, failed, fails)
            if exact and not fails:
                _EXACT.append((path, dt, cs['name'] + ('+Xelu' if xelu else '')))
            if chain:
                C = Buf(n=n, dt=dt)
                ops.call(*dgrad_call(cs, dt, ins['dP'], db, C, ins['Xelu'] if xelu else None))
                torch.cuda.synchronize()
                got, f = UF.unguard(label, 'dX (prep on the device)', *C.flat(), (F, Hi, Wi, Cin))
                failed += f
                want = UF.conv_dgrad_ref(o.dP, o.W, cs['shape'], o.Xelu if xelu else None)
                S = UF.dgrad_sum(o.dP.abs(), UF.prep_ref(o.W.abs())[1])
                r = float(torch.nan_to_num((got.double() - want).abs() / (S + 1e-300), nan=float('inf')).max())
                gc = g + U_ROUND[dt]
                print(f'{label:100s} dX vs autograd, prep on the device: |err| / sum |terms| = {r:.3e}  (gate {gc:.3e})')
                if not r <= gc:
                    failed.append(f'{label}: dX with the device prep against autograd: {r:.3e} over {gc:.3e}')
        if db is not None and not db.unchanged():
            failed.append(f"dgrad {cs['name']} [{dt}]: the entry point wrote Wd")
        for k, b in ins.items():
            if not b.unchanged():
                failed.append(f"dgrad {cs['name']} [{dt}] {'exact' if exact else 'random'} twin: the entry point wrote {k} (or its guards)")
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


@pytest.mark.parametrize('cs,dt', UF.rows('fwd'), ids=UF.case_id)
def test_fwd(cs, dt):
    run_fwd_row(cs, dt)


@pytest.mark.parametrize('cs,dt', UF.rows('res'), ids=UF.case_id)
def test_fwd_res(cs, dt):
    run_fwd_row(cs, dt)


@pytest.mark.parametrize('cs,dt', UF.rows('dgrad'), ids=UF.case_id)
def test_dgrad(cs, dt):
    run_dgrad_row(cs, dt)


def test_reference_on_device_equals_reference_on_cpu():
    """the integer twins of (5,40,96,96,96) forward and (3,56,112,128,96) dgrad: the float64 statements evaluated on the device and on the
    CPU agree exactly"""
    for kind, shape in (('fwd', (5, 40, 96, 96, 96)), ('dgrad', (3, 56, 112, 128, 96))):
        cs = next(c for c in UF.TABLES[kind] if c['shape'] == shape)
        o = UF.operands(cs, BF16, True)
        Rc, Rd = UF.reference(cs, o, 'cpu'), UF.reference(cs, o, 'cuda')
        if kind == 'fwd':
            assert torch.equal(Rc.pre, Rd.pre) and torch.equal(Rc.S, Rd.S)
        else:
            assert torch.equal(Rc.sum, Rd.sum) and torch.equal(Rc.S, Rd.S)


def _refused(name, status, args, bufs, what):
    from strajnet_amd import ops
    from strajnet_amd._lib import StjError
    with pytest.raises(StjError) as ei:
        ops.call(*args)
    msg = str(ei.value)
    assert f'{name} failed ({status}):' in msg and len(msg.split(':', 1)[1].strip()) > 0, (what, msg)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.unchanged(), (what, k)


def test_refusals_change_nothing():
    """stj_upconv_fwd and stj_upconv_dgrad: STJ_EINVAL for F = 0, Cin = 12 in bf16, Cout = 6 in f32 and dtype = 7; stj_upconv_fwd_res:
    STJ_EUNSUPPORTED for f32, Cin = 128, Cout = 40, R1 == NULL and Y2 without R2 -- each with a message, every buffer bit for bit as before"""
    from strajnet_amd import ops
    f32 = ops.DTYPE_CODE[F32]
    bad = [('F = 0', dict(F=0)), ('Cin = 12 in bf16', dict(Cin=12)), ('Cout = 6 in f32', dict(Cout=6, dtype=f32)), ('dtype = 7', dict(dtype=7))]
    cs = next(c for c in UF.FWD_CASES if c['shape'] == (2, 8, 16, 96, 48) and BF16 in c['dts'] and c['act'] == ELU)
    o = UF.operands(cs, BF16, False)
    n = o.X.numel() // 96 * 4 * 48
    b = dict(X=Buf(o.X), Wf=Buf(o.Wf), bias=Buf(o.bias), Y=Buf(n=n, dt=BF16))
    for what, over in bad:
        _refused('stj_upconv_fwd', EINVAL, fwd_call(cs, BF16, b['X'], b['Wf'], b['bias'], b['Y'], **over), b, what)
    ops.call(*fwd_call(cs, BF16, b['X'], b['Wf'], b['bias'], b['Y']))             # the unmodified arguments are legal
    torch.cuda.synchronize()
    assert not b['Y'].unchanged()

    cd = next(c for c in UF.DGRAD_CASES if c['shape'] == (2, 8, 16, 96, 48) and BF16 in c['dts'])
    o = UF.operands(cd, BF16, False)
    d = dict(dP=Buf(o.dP), Wd=Buf(o.Wd), Xelu=Buf(o.Xelu), dX=Buf(n=o.Xelu.numel(), dt=BF16))
    for what, over in bad:
        _refused('stj_upconv_dgrad', EINVAL, dgrad_call(cd, BF16, d['dP'], d['Wd'], d['dX'], d['Xelu'], **over), d, what)
    ops.call(*dgrad_call(cd, BF16, d['dP'], d['Wd'], d['dX'], d['Xelu']))
    torch.cuda.synchronize()
    assert not d['dX'].unchanged()

    cr = next(c for c in UF.RES_CASES if c['shape'] == (1, 16, 16, 192, 128))
    o = UF.operands(cr, BF16, False)
    n = o.R1.numel()
    r = dict(X=Buf(o.X), Wf=Buf(o.Wf), bias=Buf(o.bias), R1=Buf(o.R1), R2=Buf(o.R2), Y=Buf(n=n, dt=BF16), Y2=Buf(n=n, dt=BF16))

    def rc(R1='R1', Y2='Y2', R2='R2', **over):
        return res_call(cr, BF16, r['X'], r['Wf'], r['bias'], r['Y'], r.get(R1), r.get(Y2), r.get(R2), **over)
    for what, args in (('f32', rc(dtype=f32)), ('Cin = 128', rc(Cin=128)), ('Cout = 40', rc(Cout=40)), ('R1 == NULL', rc(R1=None)),
                       ('Y2 without R2', rc(R2=None))):
        _refused('stj_upconv_fwd_res', EUNSUPPORTED, args, r, what)
    ops.call(*rc())
    torch.cuda.synchronize()
    assert not r['Y'].unchanged() and not r['Y2'].unchanged()
