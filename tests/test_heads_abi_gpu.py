"""stj_outconv_fwd, stj_outconv_pair_fwd, stj_outconv_bwd, stj_upconv_fwd_head, stj_outconv_pair_gather and stj_outconv_pair_gather_q through the
raw C ABI, per dispatch path, against the float64 statements of _heads_cases.py (which test_heads_ref.py tests on the CPU, together with the
dispatch mirrors and the judgement's sensitivity).

Every call is ops.call with raw pointers into flat guarded buffers.  Per table row and element type, two data sets (docstring of
_heads_cases.py): the exact twin, where the outputs must EQUAL the statement, and the random twin, judged per element against
gate(path, T) * sum |terms|.  The backward runs every row with elu_in 0 and 1; the MFMA rows run with the head at channel offset 0 and 2 of
the interleaved [B,H,W,32] tensor, whose 30 other channels must keep their NaN pattern.

  * every test asserts the mirror's path for the row before it launches.
  * dW and db start from non-zero values (the "+="), ws from NaN pattern; inputs and all guards are compared bitwise after the call.
  * the first MFMA row is also handed an unrounded f32 W (random twin), bound gate + the unit round-off of T.
  * stj_outconv_pair_gather_q must equal, byte for byte, stj_quantize_waypoints of the gather's own Y; the row with NaN pattern in channels
    18, 19 of Z must give the Y and the Q of its twin without them, bit for bit.
  * references: float64 on the CPU; on float64 device tensors above 100000 output pixels, and one mid-size row holds the two equal.
  * refusals return their status with a message and change no byte; the unmodified call that follows is legal.

Found by reading, before the first run: stj_outconv_fwd and stj_outconv_bwd took any F and Tn (F % Tn != 0: frame indices past F in the MFMA
kernels' decode and a batch index the caller's Y does not have in the generic ones; Tn < 1: a division by zero; F < 1: an empty grid and
STJ_ELAUNCH) -- now STJ_EINVAL before any launch (outconv_check in conv.hip).  An odd y_bstride or y_tstride reached the MFMA kernels'
float2 accesses at 4-byte alignment: both *_mfma_try conditions now send any odd stride to the generic kernels.
Found by the run: nothing else.  All 117 exact twins (rows x element types x head offsets x elu_in modes) report equality on all 7 paths --
the single-head MFMA forward, which nothing ran before, nt = 4, the rectangular and t-major rows, the persistent rows (832 tiles on 768
workgroups forward and backward, 513 spatial tiles on 257 paired workgroups, 273 tiles on 256 in the head epilogue, 2050 on 2048 in the
gather, 1088 on 1024 in the generic backward) included; Q equals stj_quantize_waypoints of the gather's own Y on every row, and NaN pattern
in channels 18, 19 of Z changes no bit of Y or Q.  Every refusal holds against the fixed launchers.  profiles/test_heads_kernels.txt
lists the kernels one run of this module launched.

Largest |err| / sum |terms| of the random twin per path and element type on an MI355X (MEASURED in _heads_cases.py; the gate is four times
that where below the bound -- EPS_ELEM[T] = 2^-7 / 2^-10 / 2^-17, 2^-17 for the f32 outputs --, profiles/test_heads_ratios.txt has the
gates applied):
    path      bf16       fp16       f32            path      bf16       fp16       f32
    FM        1.311e-08  4.369e-08                 BM/dX     3.800e-03
    FG        1.287e-08  1.377e-07  2.111e-07      BM/dW     1.124e-08
    PAIR      1.542e-08  4.507e-08                 BG/dX     3.291e-03  4.455e-04  1.698e-07
    GATHER    7.447e-08  7.388e-08                 BG/dW     9.441e-09  1.194e-07  1.343e-07
    HEAD      2.100e-04  2.666e-05
dX is one rounding of the stored element, up to the unit round-off of T where an element is a single term: its gates stay at EPS_ELEM.
With an unrounded f32 W the MFMA forward stays at 3.2e-04 (bf16) / 4.0e-05 (fp16) of sum |terms|, bound gate + 2^-8 / 2^-11.
"""
import pytest
import torch

import _heads_cases as HC
from _heads_cases import BF16, EINVAL, EUNSUPPORTED, F16, F32, GUARD, bits, pattern
from test_upconv_fwd_abi_gpu import Buf, _refused

pytestmark = pytest.mark.gpu

_RATIOS = []            # (path, dtype, case, ratio, gate)
_EXACT = []             # (path, dtype, case): exact twins that reported equality


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()
    yield
    best = {}
    for path, dt, name, r, g in _RATIOS:
        k = (path, HC.case_id(dt))
        if k not in best or r > best[k][0]:
            best[k] = (r, name, g)
    print()
    for (path, dt), (r, name, g) in sorted(best.items()):
        print(f'heads {path:8s} {dt:9s} largest |err| / sum |terms| {r:.3e} ({name}), gate {g:.3e}')
    print(f'heads exact twins reporting equality: {len(_EXACT)} (rows x element types x modes), on {len(set(e[0] for e in _EXACT))} paths')


class DevBuf(Buf):
    """a Buf whose values were drawn on the device (the large rows); the image it is compared with stays there too"""

    def __init__(self, vals=None, n=None, dt=None):
        if vals is not None:
            dt, n = vals.dtype, vals.numel()
        self.dev = pattern(GUARD + n + GUARD, dt).cuda()
        if vals is not None:
            self.dev[GUARD:GUARD + n] = vals.reshape(-1)
        self.init = self.dev.clone()
        self.n = n

    def unchanged(self):
        return torch.equal(bits(self.dev), bits(self.init))

    def flat(self):
        return self.dev, self.init


def mk(vals=None, n=None, dt=None, dev='cpu'):
    big = vals.is_cuda if vals is not None else dev == 'cuda'
    return (DevBuf if big else Buf)(vals, n, dt)


def guards_ok(b):
    """a scratch buffer: only its guards are held to their first bits"""
    got = bits(b.dev[:GUARD]), bits(b.dev[GUARD + b.n:])
    return torch.equal(got[0].cpu(), bits(b.init[:GUARD]).cpu()) and torch.equal(got[1].cpu(), bits(b.init[GUARD + b.n:]).cpu())


def _dev(cs):
    return 'cuda' if HC.on_device(cs) else 'cpu'


def _label(kind, cs, dt, exact, extra=''):
    return f"{kind} {cs['name']} [{HC.case_id(dt)}] {'exact' if exact else 'random'} twin{extra}"


def _record(label, path, dt, name, ratios, g):
    for out, r in ratios.items():
        p = f'{path}/{"dX" if out == "dX" else "dW"}' if path in ('BM', 'BG') else path
        print(f'{label:96s} {out:3s} |err| / sum |terms| = {r:.3e}  (gate {g[out]:.3e})')
        _RATIOS.append((p, dt, name, r, g[out]))


def _ypos(buf, cs, off):
    from strajnet_amd import ops
    return ops._poff(buf.dev, GUARD + cs['mis'] + off)


def oc_fwd_call(cs, dt, X, W, bias, Y, off=0, **over):
    from strajnet_amd import ops
    F, H, Wd, C, Tn = cs['shape']
    (ybs, yts, yps), _ = HC.strides(cs)
    v = dict(F=F, H=H, W=Wd, C=C, Tn=Tn, dtype=ops.DTYPE_CODE[dt])
    v.update(over)
    return ('stj_outconv_fwd', X.ptr, W.ptr, bias.ptr, _ypos(Y, cs, off), v['F'], v['H'], v['W'], v['C'], v['Tn'], ybs, yts, yps, v['dtype'], ops._st())


def oc_bwd_call(cs, dt, X, W, dY, dX, dW, db, ws, elu_in, off=0, **over):
    from strajnet_amd import ops
    F, H, Wd, C, Tn = cs['shape']
    (ybs, yts, yps), _ = HC.strides(cs)
    v = dict(F=F, H=H, W=Wd, C=C, Tn=Tn, dtype=ops.DTYPE_CODE[dt], dWp=dW.ptr, dbp=db.ptr)
    v.update(over)
    wsp, wsb = (ws.ptr, HC.OCB_WS_BYTES - (1 if cs['ws'] == 'short' else 0)) if cs['ws'] != 'null' else (ops._p(None), 0)
    return ('stj_outconv_bwd', X.ptr, W.ptr, _ypos(dY, cs, off), dX.ptr, v['dWp'], v['dbp'], v['F'], v['H'], v['W'], v['C'], v['Tn'], ybs, yts, yps,
            elu_in, wsp, wsb, v['dtype'], ops._st())


def _inputs_unchanged(label, ins, failed):
    for k, b in ins.items():
        if not b.unchanged():
            failed.append(f'{label}: the entry point wrote {k} (or its guards)')


@pytest.mark.parametrize('cs,dt', HC.oc_rows('fwd'), ids=HC.case_id)
def test_outconv_fwd(cs, dt):
    from strajnet_amd import ops
    path, dev, failed = cs['fwd'][dt], _dev(cs), []
    g = HC.gate(path, dt)
    for off in cs['offs']:
        geo = HC.oc_geometry(cs, dt, 'fwd', off)
        assert geo['status'] == HC.OK and geo['path'] == path, geo
    for exact in (False, True):
        o = HC.oc_operands(cs, dt, exact, 'fwd', device=dev)
        R = HC.oc_reference(o, 'fwd')
        ins = dict(X=mk(o.X), W=mk(o.W), bias=mk(o.bias))
        for off in cs['offs']:
            label = _label('outconv_fwd', cs, dt, exact, f', head at {off}')
            Y = mk(n=HC.y_numel(cs), dt=F32, dev=dev)
            ops.call(*oc_fwd_call(cs, dt, ins['X'], ins['W'], ins['bias'], Y, off))
            torch.cuda.synchronize()
            ratios = {}
            fails = HC.judge(label, 'Y', *Y.flat(), HC.y_index(cs, off, dev), R.Y, R.S, exact, g, ratios)
            _record(label, path, dt, cs['name'], ratios, {'Y': g})
            failed += fails
            if exact and not fails:
                _EXACT.append((path, dt, cs['name'] + f'@{off}'))
        if cs['raw_w'] and not exact:              # the kernel's own rounding of W: one more unit round-off of T
            label = _label('outconv_fwd', cs, dt, exact, ', unrounded W')
            Wb, Y = mk(o.Wraw), mk(n=HC.y_numel(cs), dt=F32, dev=dev)
            ops.call(*oc_fwd_call(cs, dt, ins['X'], Wb, ins['bias'], Y, 0))
            torch.cuda.synchronize()
            Rr, ratios = HC.oc_reference(o, 'fwd', W=o.Wraw), {}
            failed += HC.judge(label, 'Y', *Y.flat(), HC.y_index(cs, 0, dev), Rr.Y, Rr.S, False, g + HC.U_ROUND[dt], ratios)
            print(f"{label:96s} Y   |err| / sum |terms| = {ratios['Y']:.3e}  (gate {g + HC.U_ROUND[dt]:.3e})")
            assert bool((o.Wraw != o.W).any()) and Wb.unchanged()
        _inputs_unchanged(_label('outconv_fwd', cs, dt, exact), ins, failed)
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


@pytest.mark.parametrize('cs,dt', HC.oc_rows('bwd'), ids=HC.case_id)
def test_outconv_bwd(cs, dt):
    from strajnet_amd import ops
    path, dev, failed = cs['bwd'][dt], _dev(cs), []
    F, H, Wd, C, Tn = cs['shape']
    from strajnet_amd._lib import lib
    assert int(lib().stj_outconv_bwd_workspace_bytes()) == HC.OCB_WS_BYTES
    gx, gw = HC.gate(path + '/dX', dt), HC.gate(path + '/dW', dt)
    for off in cs['offs']:
        geo = HC.oc_geometry(cs, dt, 'bwd', off)
        assert geo['status'] == HC.OK and geo['path'] == path, geo
    for exact in (False, True):
        for elu_in in HC.ELU_MODES:
            o = HC.oc_operands(cs, dt, exact, 'bwd', elu_in, device=dev)
            R = HC.oc_reference(o, 'bwd', elu_in)
            ins = dict(X=mk(o.X), W=mk(o.W))
            for off in cs['offs']:
                label = _label('outconv_bwd', cs, dt, exact, f', elu_in {elu_in}, head at {off}')
                dYv = pattern(HC.y_numel(cs), F32).to(o.G.device)
                dYv[HC.y_index(cs, off, dev).reshape(-1)] = o.G.reshape(-1)          # every element of dY that is not the head's is NaN pattern
                ins['dY'] = mk(dYv)
                dX, dW, db = mk(n=o.X.numel(), dt=dt, dev=dev), mk(o.dW0.cpu()), mk(o.db0.cpu())
                ws = mk(n=HC.OCB_WS_BYTES // 4, dt=F32, dev='cuda')
                ops.call(*oc_bwd_call(cs, dt, ins['X'], ins['W'], ins['dY'], dX, dW, db, ws, elu_in, off))
                torch.cuda.synchronize()
                ratios = {}
                n = o.X.numel()
                fails = HC.judge(label, 'dX', *dX.flat(), HC.whole(n, dev), R.dX, R.SdX, exact, gx, ratios, rn=dt)
                fails += HC.judge(label, 'dW', *dW.flat(), HC.whole(18 * C), R.dW.cpu(), R.SdW.cpu(), exact, gw, ratios)
                fails += HC.judge(label, 'db', *db.flat(), HC.whole(2), R.db.cpu(), R.Sdb.cpu(), exact, gw, ratios)
                if not guards_ok(ws):
                    fails.append(f'{label}: the guards of ws changed')
                _record(label, path, dt, cs['name'], ratios, {'dX': gx, 'dW': gw, 'db': gw})
                failed += fails
                if exact and not fails:
                    _EXACT.append((path, dt, cs['name'] + f'@{off}+elu{elu_in}'))
                _inputs_unchanged(label, ins, failed)
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


@pytest.mark.parametrize('cs,dt', HC.rows(HC.PAIR_CASES), ids=HC.case_id)
def test_outconv_pair_fwd(cs, dt):
    from strajnet_amd import ops
    B, H, Wd, tm = cs['shape']
    dev, failed = _dev(cs), []
    g = HC.gate('PAIR', dt)
    assert HC.geometry(cs, dt)['path'] == 'PAIR'
    for exact in (False, True):
        label = _label('outconv_pair_fwd', cs, dt, exact)
        o = HC.pair_operands(cs, dt, exact, dev)
        R = HC.pair_reference(cs, o)
        ins = dict(X0=mk(o.X[0]), X1=mk(o.X[1]), W0=mk(o.W[0]), W1=mk(o.W[1]), b0=mk(o.bias[0]), b1=mk(o.bias[1]))
        n = B * H * Wd * 32
        Y = mk(n=n, dt=F32, dev=dev)
        ops.call('stj_outconv_pair_fwd', *(ins[k].ptr for k in ('X0', 'X1', 'W0', 'W1', 'b0', 'b1')), Y.ptr, B, 8, H, Wd, 48, tm, ops.DTYPE_CODE[dt], ops._st())
        torch.cuda.synchronize()
        ratios = {}
        fails = HC.judge(label, 'Y', *Y.flat(), HC.whole(n, dev), R.Y, R.S, exact, g, ratios)
        _record(label, 'PAIR', dt, cs['name'], ratios, {'Y': g})
        failed += fails
        if exact and not fails:
            _EXACT.append(('PAIR', dt, cs['name']))
        _inputs_unchanged(label, ins, failed)
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


@pytest.mark.parametrize('cs,dt', HC.rows(HC.HEAD_CASES), ids=HC.case_id)
def test_upconv_fwd_head(cs, dt):
    from strajnet_amd import ops
    F, Hi, Wi = cs['shape']
    dev, failed = _dev(cs), []
    g = HC.gate('HEAD', dt)
    assert HC.geometry(cs, dt)['path'] == 'HEAD'
    shape = (F, 2 * Hi, 2 * Wi, 20)
    n = F * 4 * Hi * Wi * 20
    for exact in (False, True):
        label = _label('upconv_fwd_head', cs, dt, exact)
        o = HC.head_operands(cs, dt, exact, dev)
        R = HC.head_reference(o, dt)
        ins = dict(X=mk(o.X), Wf=mk(o.Wf), bias=mk(o.bias), Wh=mk(o.Wh))
        Z = mk(n=n, dt=dt, dev=dev)
        ops.call('stj_upconv_fwd_head', ins['X'].ptr, ins['Wf'].ptr, ins['bias'].ptr, ins['Wh'].ptr, Z.ptr, F, Hi, Wi, 96, 48, ops.DTYPE_CODE[dt], ops._st())
        torch.cuda.synchronize()
        ratios = {}
        fails = HC.judge(label, 'Z', *Z.flat(), HC.whole(n, dev), R.Z, R.S, exact, g, ratios, rn=dt, bitwise=(HC.z_zero_index(shape, dev), 0))
        if not exact:
            neg = float((R.pre <= 0).double().mean())
            print(f'{label:96s} share of pre <= 0 (the ELU branch): {neg:.3f}')
            assert 0.05 < neg < 0.95
        _record(label, 'HEAD', dt, cs['name'], ratios, {'Z': g})
        failed += fails
        if exact and not fails:
            _EXACT.append(('HEAD', dt, cs['name']))
        _inputs_unchanged(label, ins, failed)
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


def _qbuf(n):
    return torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')


@pytest.mark.parametrize('cs,dt', HC.rows(HC.GATHER_CASES), ids=HC.case_id)
def test_outconv_pair_gather_and_q(cs, dt):
    from strajnet_amd import ops
    B, H, Wd, tm = cs['shape']
    dev, failed = _dev(cs), []
    g = HC.gate('GATHER', dt)
    assert HC.geometry(cs, dt)['path'] == 'GATHER'
    n = B * H * Wd * 32
    code = ops.DTYPE_CODE[dt]

    def run(o):
        ins = dict(Z0=mk(o.Z[0]), Z1=mk(o.Z[1]), b0=mk(o.bias[0]), b1=mk(o.bias[1]))
        Y, Q, Q2 = mk(n=n, dt=F32, dev=dev), _qbuf(n), _qbuf(n)
        a = [ins[k].ptr for k in ('Z0', 'Z1', 'b0', 'b1')]
        ops.call('stj_outconv_pair_gather', *a, Y.ptr, B, 8, H, Wd, tm, code, ops._st())
        ops.call('stj_outconv_pair_gather_q', *a, ops._poff(Q, GUARD), B, 8, H, Wd, tm, code, ops._st())
        ops.call('stj_quantize_waypoints', Y.ptr, ops._poff(Q2, GUARD), B, 8, H, Wd, ops._st())
        torch.cuda.synchronize()
        return ins, Y, Q, Q2

    for exact in (False, True):
        label = _label('outconv_pair_gather', cs, dt, exact)
        o = HC.gather_operands(cs, dt, exact, dev)
        R = HC.gather_reference(cs, o)
        ins, Y, Q, Q2 = run(o)
        ratios = {}
        fails = HC.judge(label, 'Y', *Y.flat(), HC.whole(n, dev), R.Y, R.S, exact, g, ratios)
        if not torch.equal(Q, Q2):
            fails.append(f'{label}: Q differs from stj_quantize_waypoints of the gather\'s own Y in {int((Q != Q2).sum())} bytes (guards included)')
        if not (bool((Q2[:GUARD] == 0xA5).all()) and bool((Q2[GUARD + n:] == 0xA5).all()) and len(torch.unique(Q[GUARD:GUARD + n])) > 2):
            fails.append(f'{label}: Q: guards changed, or the bytes do not vary')
        if cs['nan']:                               # channels 18, 19 of Z are never read: the twin without the NaN pattern gives the same bits
            c2 = dict(cs, nan=False)
            _, Y0, Q0, _ = run(HC.gather_operands(c2, dt, exact, dev))
            if not (torch.equal(bits(Y.dev), bits(Y0.dev)) and torch.equal(Q, Q0)):
                fails.append(f'{label}: NaN pattern in channels 18, 19 of Z changed Y or Q')
        _record(label, 'GATHER', dt, cs['name'], ratios, {'Y': g})
        failed += fails
        if exact and not fails:
            _EXACT.append(('GATHER', dt, cs['name']))
        _inputs_unchanged(label, ins, failed)
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


def test_reference_on_device_equals_reference_on_cpu():
    """the integer twin of (16,32,48,48,8), forward and backward: the float64 statements evaluated on the device and on the CPU agree exactly"""
    cs = HC.OC_CASES[1]
    o = HC.oc_operands(cs, BF16, True, 'fwd')
    od = HC.Ops()                               # the same operands on the device (a draw there differs)
    for t in ('X', 'W', 'bias'):
        setattr(od, t, getattr(o, t).cuda())
    Rc, Rd = HC.oc_reference(o, 'fwd'), HC.oc_reference(od, 'fwd')
    assert torch.equal(Rc.Y, Rd.Y.cpu()) and torch.equal(Rc.S, Rd.S.cpu())
    o = HC.oc_operands(cs, BF16, True, 'bwd', 1)
    od = HC.Ops()
    for t in ('X', 'W', 'G', 'dW0', 'db0'):
        setattr(od, t, getattr(o, t).cuda())
    Rc, Rd = HC.oc_reference(o, 'bwd', 1), HC.oc_reference(od, 'bwd', 1)
    for t in ('dX', 'SdX', 'dW', 'SdW', 'db', 'Sdb'):
        assert torch.equal(getattr(Rc, t), getattr(Rd, t).cpu()), t


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_outconv_refusals_change_nothing():
    """stj_outconv_fwd / stj_outconv_bwd: STJ_EINVAL for H = 24, C = 12, dtype = 7, F = 0, Tn = 0 and F % Tn != 0 (bwd: dW or db NULL too),
    STJ_EUNSUPPORTED for C = 120 -- each with a message, every buffer bit for bit as before, then the unmodified call"""
    from strajnet_amd import ops
    cs = HC.OC_CASES[0]
    bad = [('H = 24', EINVAL, dict(H=24)), ('C = 12', EINVAL, dict(C=12)), ('dtype = 7', EINVAL, dict(dtype=7)), ('F = 0', EINVAL, dict(F=0)),
           ('Tn = 0', EINVAL, dict(Tn=0)), ('F % Tn != 0', EINVAL, dict(F=12)), ('F < Tn', EINVAL, dict(F=4)), ('C = 120', EUNSUPPORTED, dict(C=120))]
    o = HC.oc_operands(cs, BF16, False, 'fwd')
    b = dict(X=Buf(o.X), W=Buf(o.W), bias=Buf(o.bias), Y=Buf(n=HC.y_numel(cs), dt=F32))
    for what, st, over in bad:
        _refused('stj_outconv_fwd', st, oc_fwd_call(cs, BF16, b['X'], b['W'], b['bias'], b['Y'], **over), b, what)
    ops.call(*oc_fwd_call(cs, BF16, b['X'], b['W'], b['bias'], b['Y']))
    torch.cuda.synchronize()
    assert not b['Y'].unchanged()

    o = HC.oc_operands(cs, BF16, False, 'bwd', 1)
    dYv = pattern(HC.y_numel(cs), F32)
    dYv[HC.y_index(cs, 0).reshape(-1)] = o.G.reshape(-1)
    d = dict(X=Buf(o.X), W=Buf(o.W), dY=Buf(dYv), dX=Buf(n=o.X.numel(), dt=BF16), dW=Buf(o.dW0), db=Buf(o.db0), ws=Buf(n=HC.OCB_WS_BYTES // 4, dt=F32))

    def bc(**over):
        return oc_bwd_call(cs, BF16, d['X'], d['W'], d['dY'], d['dX'], d['dW'], d['db'], d['ws'], 1, **over)
    for what, st, over in bad + [('dW == NULL', EINVAL, dict(dWp=ops._p(None))), ('db == NULL', EINVAL, dict(dbp=ops._p(None)))]:
        _refused('stj_outconv_bwd', st, bc(**over), d, what)
    ops.call(*bc())
    torch.cuda.synchronize()
    assert not d['dX'].unchanged() and not d['dW'].unchanged() and not d['db'].unchanged()


def test_pair_head_gather_refusals_change_nothing():
    """stj_outconv_pair_fwd: STJ_EUNSUPPORTED for f32, C = 40, Tn = 4, H = 24, STJ_EINVAL for B = 0; stj_upconv_fwd_head: STJ_EUNSUPPORTED for
    f32, Cin = 128, Hi = 12, Wi = 8; stj_outconv_pair_gather and _q: STJ_EUNSUPPORTED for f32, Tn = 4, W = 24 and a Y 4 bytes off,
    STJ_EINVAL for B = 0"""
    from strajnet_amd import ops
    bf, f32 = ops.DTYPE_CODE[BF16], ops.DTYPE_CODE[F32]
    cs = HC.PAIR_CASES[0]
    B, H, Wd, tm = cs['shape']
    o = HC.pair_operands(cs, BF16, False)
    p = dict(X0=Buf(o.X[0]), X1=Buf(o.X[1]), W0=Buf(o.W[0]), W1=Buf(o.W[1]), b0=Buf(o.bias[0]), b1=Buf(o.bias[1]), Y=Buf(n=B * H * Wd * 32, dt=F32))

    def pc(**over):
        v = dict(B=B, Tn=8, H=H, C=48, dtype=bf)
        v.update(over)
        return ('stj_outconv_pair_fwd', *(p[k].ptr for k in ('X0', 'X1', 'W0', 'W1', 'b0', 'b1', 'Y')), v['B'], v['Tn'], v['H'], Wd, v['C'], tm, v['dtype'], ops._st())
    for what, st, over in (('f32', EUNSUPPORTED, dict(dtype=f32)), ('C = 40', EUNSUPPORTED, dict(C=40)), ('Tn = 4', EUNSUPPORTED, dict(Tn=4)),
                           ('H = 24', EUNSUPPORTED, dict(H=24)), ('B = 0', EINVAL, dict(B=0))):
        _refused('stj_outconv_pair_fwd', st, pc(**over), p, what)
    ops.call(*pc())
    torch.cuda.synchronize()
    assert not p['Y'].unchanged()

    cs = HC.HEAD_CASES[0]
    F, Hi, Wi = cs['shape']
    o = HC.head_operands(cs, BF16, False)
    h = dict(X=Buf(o.X), Wf=Buf(o.Wf), bias=Buf(o.bias), Wh=Buf(o.Wh), Z=Buf(n=F * 4 * Hi * Wi * 20, dt=BF16))

    def hc(**over):
        v = dict(Hi=Hi, Wi=Wi, Cin=96, dtype=bf)
        v.update(over)
        return ('stj_upconv_fwd_head', *(h[k].ptr for k in ('X', 'Wf', 'bias', 'Wh', 'Z')), F, v['Hi'], v['Wi'], v['Cin'], 48, v['dtype'], ops._st())
    for what, over in (('f32', dict(dtype=f32)), ('Cin = 128', dict(Cin=128)), ('Hi = 12', dict(Hi=12)), ('Wi = 8', dict(Wi=8))):
        _refused('stj_upconv_fwd_head', EUNSUPPORTED, hc(**over), h, what)
    ops.call(*hc())
    torch.cuda.synchronize()
    assert not h['Z'].unchanged()

    cs = HC.GATHER_CASES[0]
    B, H, Wd, tm = cs['shape']
    o = HC.gather_operands(cs, BF16, False)
    n = B * H * Wd * 32
    for name, out in (('stj_outconv_pair_gather', Buf(n=n + 4, dt=F32)), ('stj_outconv_pair_gather_q', Buf(n=n // 4 + 4, dt=F32))):
        q = dict(Z0=Buf(o.Z[0]), Z1=Buf(o.Z[1]), b0=Buf(o.bias[0]), b1=Buf(o.bias[1]), out=out)

        def gc(off=0, **over):
            v = dict(B=B, Tn=8, W=Wd, dtype=bf)
            v.update(over)
            return (name, *(q[k].ptr for k in ('Z0', 'Z1', 'b0', 'b1')), ops._poff(out.dev, GUARD + off), v['B'], v['Tn'], H, v['W'], tm, v['dtype'], ops._st())
        for what, st, args in (('f32', EUNSUPPORTED, gc(dtype=f32)), ('Tn = 4', EUNSUPPORTED, gc(Tn=4)), ('W = 24', EUNSUPPORTED, gc(W=24)),
                               ('output 4 bytes off', EUNSUPPORTED, gc(off=1)), ('B = 0', EINVAL, gc(B=0))):
            _refused(name, st, args, q, what)
        ops.call(*gc())
        torch.cuda.synchronize()
        assert not out.unchanged()
