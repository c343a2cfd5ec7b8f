"""stj_upconv_prep, stj_upconv_wgrad and stj_upconv_fold through the raw C ABI, per dispatch path, against the float64 statements of
_upconv_cases.py (which test_upconv_wgrad_ref.py tests on the CPU, together with the dispatch mirror and the judgement's sensitivity).

Every call is ops.call with raw pointers into flat guarded buffers.  Per table row and element type, two data sets (docstring of
_upconv_cases.py): the exact integer twin, where dWeff, the sum of the dbias copies and dW after the fold must EQUAL start + reference --
f32 atomics, split strips and the MFMA ones-vector bias sum included -- and the random twin, judged per element against
GATE[path] * sum |terms|.  The gates: 2^-17 = 7.63e-06 (EPS_ELEM[float32]) is the bound.  Two runs on an MI355X measured, as the largest
ratio of each path over both (MEASURED in _upconv_cases.py; per path and element type in profiles/test_upconv_wgrad_ratios.txt), and the gate is four
times that, every one being below a quarter of the bound:
    path       measured   gate          path        measured   gate
    G36        1.100e-07  4.400e-07     TR4_36/32   7.584e-08  3.034e-07   (wg_budget = 1; 3.1e-09 at the default budget)
    G44        1.276e-07  5.104e-07     TR4_64/32   4.490e-09  1.796e-08
    TR36/32    1.399e-08  5.596e-08     TR4_44/32   7.608e-09  3.043e-08
    TR36/16    1.648e-08  6.592e-08     TR4_36/16   3.420e-09  1.368e-08
    TR44/32    3.503e-08  1.401e-07     TR4_64/16   3.859e-09  1.544e-08
    TR44/16    2.561e-08  1.024e-07     TR4_44/16   3.078e-09  1.231e-08
Nothing was found wrong: every exact twin reports equality on all twelve paths, the CW = 16 instantiations of the 512-thread kernel included.

  * "+=": dWeff, dbias and dW start from non-zero contents in the exact twin and in the random twin, except for the first row of every path,
    whose random twin starts from zeros and is also held, after the fold, to the float64 autograd gradient of the up-sample-then-conv
    statement (kernel and bias).
  * db_parts = 1, 7 (co-prime with every grid: all copies are used; every copy stays an integer inside its band on the exact twin, the sum
    over copies is judged) and dbias == NULL.  The copies are contiguous by the ABI (copy i at dbias + i * Cout), so the NaN-pattern guards
    lie in front of the first and behind the last copy, not between them.
  * wg_budget = 0, 256, 140, 4096 and 1 on (64,64,64,96,48): split strips with a partial last one and idle workgroups, one chunk per
    strip (no prefetch), one strip walking all 2048 chunks; 0 and 256 on one TR44/32 row (that launcher does not read it).
  * guards: dWeff, the dbias copies and dW sit between 64 floats of NaN pattern, compared bitwise after the call; X and dP sit between 64
    NaN-pattern elements (a halo over-read would surface as NaN in an output) and are compared bitwise with their copies; all pointers
    are 16-byte aligned.
  * references: float64 on the CPU below 100000 low-res pixels, the same functions on float64 device tensors above (operands drawn on the
    device there); one mid-size row holds the two evaluations equal.
  * refusals return STJ_EINVAL and change no byte.
The three CW = 16 rows of upconv_wgrad_tr4_kernel, which no workload shape dispatches, run in the last test function of the file.
profiles/test_upconv_wgrad_kernels.txt lists the kernels one run of this module launched.
"""
import pytest
import torch

import _upconv_cases as UC
from _upconv_cases import BF16, F16, F32, GUARD, bits, draw, pattern

pytestmark = pytest.mark.gpu

_RATIOS = []            # (path, dtype, case, output, ratio, gate)
_EXACT = []             # (path, dtype, case): exact twins that reported equality
U_T = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()
    yield
    best = {}
    for path, dt, name, out, r, gate in _RATIOS:
        k = (path, UC.case_id(dt))
        if k not in best or r > best[k][0]:
            best[k] = (r, name, out, gate)
    print()
    for (path, dt), (r, name, out, gate) in sorted(best.items()):
        print(f'upconv wgrad {path:10s} {dt:9s} largest |err| / sum |terms| {r:.3e} ({name}, {out}), gate {gate:.3e}')
    print(f'upconv wgrad exact twins reporting equality: {len(_EXACT)} (rows x element types), on {len(set(e[0] for e in _EXACT))} paths')


def guarded(vals):
    """[GUARD pattern][vals][GUARD pattern] on the device of vals"""
    g = pattern(GUARD, vals.dtype).to(vals.device)
    return torch.cat([g, vals.reshape(-1), g])


def out_buffer(start):
    """an f32 output between two guards, on the device, with its CPU image"""
    init = pattern(GUARD + start.numel() + GUARD, F32)
    init[GUARD:GUARD + start.numel()] = start.reshape(-1)
    return init.cuda(), init


def read_back(dev, init, shape, what):
    got = dev.cpu()
    n = init.numel() - 2 * GUARD
    assert torch.equal(bits(got[:GUARD]), bits(init[:GUARD])) and torch.equal(bits(got[GUARD + n:]), bits(init[GUARD + n:])), \
        f'{what}: guard elements changed'
    return got[GUARD:GUARD + n].reshape(shape)


def wgrad_args(cs, dt, Xb, Pb, wd, dbd, parts, budget, **over):
    from strajnet_amd import ops
    F, Hi, Wi, Cin, Cout = cs['shape']
    v = dict(X=ops._poff(Xb, GUARD), dP=ops._poff(Pb, GUARD), dWeff=ops._poff(wd, GUARD), dbias=ops._poff(dbd, GUARD) if dbd is not None else None,
             db_parts=parts or 1, F=F, Hi=Hi, Wi=Wi, Cin=Cin, Cout=Cout, wg_budget=budget, dtype=ops.DTYPE_CODE[dt])
    v.update(over)
    for k in ('X', 'dP', 'dWeff', 'dbias'):
        assert v[k] is None or v[k].value % 16 == 0
    return ('stj_upconv_wgrad', ops._p(v['X']), ops._p(v['dP']), ops._p(v['dWeff']), ops._p(v['dbias']), v['db_parts'], v['F'], v['Hi'], v['Wi'],
            v['Cin'], v['Cout'], v['wg_budget'], v['dtype'], ops._st())


def run_chain(cs, dt, Xb, Pb, start, parts, budget):
    """stj_upconv_wgrad then stj_upconv_fold from the given starting contents; guards checked; the three outputs on the CPU"""
    from strajnet_amd import ops
    _, _, _, Cin, Cout = cs['shape']
    wd, w0 = out_buffer(start['dweff'])
    dbd, db0 = out_buffer(start['db']) if parts else (None, None)
    dwd, dw0 = out_buffer(start['dw'])
    ops.call(*wgrad_args(cs, dt, Xb, Pb, wd, dbd, parts, budget))
    ops.call('stj_upconv_fold', ops._poff(wd, GUARD), ops._poff(dwd, GUARD), Cin, Cout, ops._st())
    torch.cuda.synchronize()
    return dict(dweff=read_back(wd, w0, (16, Cout, Cin), 'dWeff'), db=read_back(dbd, db0, (parts, Cout), 'dbias') if parts else None,
                dw=read_back(dwd, dw0, (3, 3, Cin, Cout), 'dW'))


def run_row(cs, dt):
    """one row of the table in one element type: both twins, every budget of the row, the three dbias modes"""
    P = UC.pixels(cs)
    path = UC.expected_path(dt, *cs['shape'])
    assert path == cs['path']
    gate = UC.GATE[path]
    first = UC.first_of_path(cs, dt)
    dev = 'cuda' if P >= UC.BIG else 'cpu'
    failed = []
    for exact in (False, True):
        X, dP = UC.operands(cs, dt, exact, dev)
        R = UC.reference(X, dP)
        Xb, Pb = guarded(X.cuda()), guarded(dP.cuda())
        X0, P0 = Xb.clone(), Pb.clone()
        zero_run = None
        for bi, budget in enumerate(cs['budgets']):
            for parts in (UC.DB_MODES if bi == 0 else (7,)):
                zero = first and not exact and bi == 0 and parts == 1
                start = UC.starts(cs, dt, exact, parts, zero)
                label = f"{cs['name']} [{UC.case_id(dt)}] {'exact' if exact else 'random'} twin, wg_budget {budget}, db_parts {parts}"
                try:
                    got = run_chain(cs, dt, Xb, Pb, start, parts, budget)
                except AssertionError as e:
                    failed.append(f'{label}: {e}')
                    continue
                fails, ratios = UC.judge_values(label, exact, gate, R, start, got, P)
                failed += fails
                for out, r in ratios.items():
                    print(f'{label:100s} {out:6s} |err| / sum |terms| = {r:.3e}  (gate {gate:.3e})')
                    _RATIOS.append((path, dt, cs['name'], out, r, gate))
                if zero:
                    zero_run = got
        if not (torch.equal(bits(Xb), bits(X0)) and torch.equal(bits(Pb), bits(P0))):
            failed.append(f"{cs['name']} [{dt}]: the entry point wrote X or dP (or their guards)")
        if zero_run is not None:
            # the chain from zeros against autograd of the up-sample-then-conv statement
            cW, cb = (t.cpu() for t in UC.chain_ref(X, dP))
            for name, g, want, T in (('dW', zero_run['dw'].double(), cW, UC.fold_ref(R.Tw)), ('dbias', zero_run['db'].double().sum(0), cb, R.Tdb)):
                r = float(torch.nan_to_num((g - want).abs() / (T + 1e-300), nan=float('inf')).max())
                print(f"{cs['name']} [{UC.case_id(dt)}] chain vs autograd {name:6s} |err| / sum |terms| = {r:.3e}  (gate {gate:.3e})")
                _RATIOS.append((path, dt, cs['name'], name + ' (autograd)', r, gate))
                if not r <= gate:
                    failed.append(f"{cs['name']} [{dt}]: chain vs autograd, {name}: {r:.3e} over the gate {gate:.3e}")
        if exact and not failed:
            _EXACT.append((path, dt, cs['name']))
        del X, dP, Xb, Pb, X0, P0, R
    assert not failed, f'{len(failed)} judgements failed:\n' + '\n'.join(failed)


def _cw16_tr4(cs):
    return cs['path'].startswith('TR4_') and cs['path'].endswith('/16')


@pytest.mark.parametrize('cs,dt', UC.rows(lambda c: UC.pixels(c) < UC.BIG), ids=UC.case_id)
def test_wgrad_generic_and_256_thread_paths(cs, dt):
    run_row(cs, dt)


@pytest.mark.parametrize('cs,dt', UC.rows(lambda c: UC.pixels(c) >= UC.BIG and not _cw16_tr4(c)), ids=UC.case_id)
def test_wgrad_tr4_cw32(cs, dt):
    run_row(cs, dt)


def test_reference_on_device_equals_reference_on_cpu():
    """the integer twin of (9,32,128,96,48): the float64 statement evaluated on the device (the blocked pixel sum of the large rows) and on
    the CPU agree exactly"""
    cs = next(c for c in UC.CASES if c['shape'] == (9, 32, 128, 96, 48))
    X, dP = UC.operands(cs, BF16, True)
    w, b = UC.dweff_ref(X, dP)
    wd, bd = UC.dweff_ref(X.cuda(), dP.cuda())
    assert torch.equal(wd.cpu(), w) and torch.equal(bd.cpu(), b)
    tw, _ = UC.dweff_ref(X.abs(), dP.abs())
    twd, _ = UC.dweff_ref(X.cuda().abs(), dP.cuda().abs())
    assert torch.equal(twd.cpu(), tw)


@pytest.mark.parametrize('dt', UC.ALL, ids=UC.case_id)
def test_prep(dt):
    """Wf and Wd: EQUAL to prep_ref on integer weights; on random ones within (u_T + 3 * 2^-24) * sum |W| over the at most four taps summed
    (one rounding to T of an f32 sum of four terms); all 16 slots of Wd written over a NaN pattern; guards and W untouched."""
    from strajnet_amd import ops
    failed = []
    for Cin, Cout in UC.PREP_SHAPES:
        for exact in (False, True):
            g = torch.Generator().manual_seed(Cin * 1000 + Cout + int(exact))
            W = draw(9 * Cin * Cout, F32, g, exact).view(3, 3, Cin, Cout)
            n = 16 * Cin * Cout
            Wb = guarded(W.cuda())
            W0 = Wb.clone()
            f0, d0 = pattern(GUARD + n + GUARD, dt), pattern(GUARD + n + GUARD, dt)
            fd, dd = f0.cuda(), d0.cuda()
            ops.call('stj_upconv_prep', ops._poff(Wb, GUARD), ops._poff(fd, GUARD), ops._poff(dd, GUARD), Cin, Cout, ops.DTYPE_CODE[dt], ops._st())
            torch.cuda.synchronize()
            assert torch.equal(bits(Wb), bits(W0))
            rf, rd = UC.prep_ref(W)
            af, ad = UC.prep_ref(W.abs())
            for name, dev, init, ref, A, shape in (('Wf', fd, f0, rf, af, (16, Cout, Cin)), ('Wd', dd, d0, rd, ad, (16, Cin, Cout))):
                got = dev.cpu()
                if not (torch.equal(bits(got[:GUARD]), bits(init[:GUARD])) and torch.equal(bits(got[GUARD + n:]), bits(init[GUARD + n:]))):
                    failed.append(f'{name} {Cin}->{Cout}: guard elements changed')
                y = got[GUARD:GUARD + n].reshape(shape).double()
                if bool(torch.isnan(y).any()):
                    failed.append(f'{name} {Cin}->{Cout}: {int(torch.isnan(y).sum())} elements were not written')
                elif exact:
                    if not torch.equal(y, ref):
                        failed.append(f'{name} {Cin}->{Cout}: differs from the exact result')
                else:
                    r = float(((y - ref).abs() / A).max())
                    bound = U_T[dt] + 3 * 2.0 ** -24
                    print(f'prep {name} {Cin}->{Cout} {UC.case_id(dt)}: |err| / sum |W| = {r:.3e} (bound {bound:.3e})')
                    if not r <= bound:
                        failed.append(f'{name} {Cin}->{Cout}: |err| / sum |W| = {r:.3e} over {bound:.3e}')
    assert not failed, '\n'.join(failed)


def test_refusals_change_nothing():
    """db_parts = 0 with a dbias, wg_budget = -1 and 4097, Cin = 12 in bf16, Cin = 6 in f32, F = 0 and a dtype code outside the enum:
    STJ_EINVAL (-1) with a message, and every buffer bit for bit as before"""
    from strajnet_amd import ops
    from strajnet_amd._lib import StjError
    cs = next(c for c in UC.CASES if c['shape'] == (2, 8, 32, 96, 48) and BF16 in c['dts'])
    X, dP = UC.operands(cs, BF16, False)
    Xb, Pb = guarded(X.cuda()), guarded(dP.cuda())
    start = UC.starts(cs, BF16, False, 2, False)
    wd, w0 = out_buffer(start['dweff'])
    dbd, db0 = out_buffer(start['db'])
    X0, P0 = Xb.clone(), Pb.clone()
    bad = [('db_parts = 0 with a dbias', dict(db_parts=0)), ('wg_budget = -1', dict(wg_budget=-1)), ('wg_budget = 4097', dict(wg_budget=4097)),
           ('Cin = 12 in bf16', dict(Cin=12)), ('Cin = 6 in f32', dict(Cin=6, dtype=ops.DTYPE_CODE[F32])), ('F = 0', dict(F=0)),
           ('dtype outside the enum', dict(dtype=7))]
    for what, over in bad:
        with pytest.raises(StjError) as ei:
            ops.call(*wgrad_args(cs, BF16, Xb, Pb, wd, dbd, 2, 0, **over))
        msg = str(ei.value)
        assert 'stj_upconv_wgrad failed (-1):' in msg and len(msg.split(':', 1)[1].strip()) > 0, (what, msg)
        torch.cuda.synchronize()
        assert torch.equal(bits(wd.cpu()), bits(w0)) and torch.equal(bits(dbd.cpu()), bits(db0)), what
        assert torch.equal(bits(Xb), bits(X0)) and torch.equal(bits(Pb), bits(P0)), what
    ops.call(*wgrad_args(cs, BF16, Xb, Pb, wd, dbd, 2, 0))          # the unmodified arguments are legal
    torch.cuda.synchronize()
    assert not torch.equal(bits(wd.cpu()), bits(w0))


@pytest.mark.parametrize('cs,dt', UC.rows(_cw16_tr4), ids=UC.case_id)
def test_wgrad_tr4_cw16_runs_last(cs, dt):
    """upconv_wgrad_tr4_kernel with 8 x 16 chunks: no workload shape has ever dispatched these three instantiations.  (Read before the first
    run: a k-step is two chunk rows of 16; the dP image is [8][32][LDO], + 32 columns is the next row; the X image is [9][18][LDI], k-step
    rr reads rows 2 rr + r and 2 rr + r + 1 <= 8 and columns <= 15 + b + s <= 17: the staged extents YW = 32, XW = 18 and XHI = XW * LDI hold
    them.)"""
    run_row(cs, dt)
