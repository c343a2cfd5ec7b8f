"""The FG-MSA entry points through the raw C ABI, per dispatch path, for float32, bf16 and fp16, against the float64 statement of _fg_cases.py:
stj_fg_attn_fwd / _bwd (csrc/fgattn.hip), stj_fg_bias_fwd / _bwd and stj_fg_offset_fwd / _bwd (csrc/attn.hip), stj_fgoff_pack / _fwd / _bwd
(csrc/fgoff_fused.hip).

Every call takes raw pointers into flat guarded buffers (ops.call; lib() where a status other than STJ_OK is expected).  Cases (with the table
of the kernel each one selects), layout, references, rounding twin and the judge are in _fg_cases.py and are themselves tested on the CPU by
test_fg_ref.py; this module builds no model.  What is judged, per output tensor and per ROW, and what must hold exactly (the offset gradient
on the integer lattice and beyond the table, the far group's column of dtable, the saturated tanh): see the docstring of _fg_cases.py.
The contracts no caller in ops exercises are exercised here: doff handed in with the NaN pattern where the backward has one query tile / one
query slice and with non-zero values where it adds; dtable and the offset head's parameter gradients start non-zero; dkp / dvp hold the
pattern in one run and zeros in the next; lse == NULL; every NULL mode of the offset head.

profiles/test_fg_abi_ratios.txt is the record of one run of this module (test_zz_report), profiles/test_fg_abi_kernels.txt the distinct
fgattn_* / fgoff_* / fg_bias_* / fg_offset_* kernels one run of it launched.
"""
import pytest
import torch

import _fg_cases as FC
from _fg_cases import F32, GUARD, judge, prepare
from test_gemm_gpu import bits

pytestmark = pytest.mark.gpu

_RATIOS = []
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
ORDER = {
    ('attn', 'fwd'): ('stj_fg_attn_fwd', ('q', 'k', 'v', 'off', 'table', 'a', 'lse', 'B', 'G', 'Hh', 'Ww', 'scale', 'dtype', 'stream')),
    ('attn', 'bwd'): ('stj_fg_attn_bwd', ('q', 'k', 'v', 'off', 'table', 'a', 'lse', 'da', 'dq', 'dk', 'dv', 'dkp', 'dvp', 'dtable', 'doff', 'B', 'G', 'Hh', 'Ww',
                                          'scale', 'dtype', 'stream')),
    ('bias', 'fwd'): ('stj_fg_bias_fwd', ('off', 'table', 'bias', 'B', 'G', 'Hh', 'Ww', 'dtype', 'stream')),
    ('bias', 'bwd'): ('stj_fg_bias_bwd', ('off', 'table', 'dbias', 'dtable', 'doff', 'B', 'G', 'Hh', 'Ww', 'dtype', 'stream')),
    ('offset', 'fwd'): ('stj_fg_offset_fwd', ('o', 'W1', 'W2', 'b2', 'qres', 'off', 'fh', 'B', 'HW', 'G', 'gc', 'C2', 'scale', 'zmajor', 'dtype', 'stream')),
    ('offset', 'bwd'): ('stj_fg_offset_bwd', ('o', 'off', 'W1', 'W2', 'doff', 'dfh', 'dO', 'dq', 'doff_out', 'dW1', 'dW2', 'db2', 'B', 'HW', 'G', 'gc', 'C2', 'scale',
                                              'zmajor', 'dtype', 'stream')),
}
SCALARS = ('B', 'G', 'Hh', 'Ww', 'HW', 'gc', 'C2', 'scale')


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


def upload(p):
    return {k: b.init.cuda() for k, b in p.bufs.items()}


def download(dev):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def nulls(p):
    """the pointers the call's mode hands in as NULL"""
    if p.cs['fam'] == 'attn':
        return () if p.with_saves else ('lse',)
    if p.cs['fam'] != 'offset':
        return ()
    if p.kind == 'fwd':
        m = FC.FMODES[p.mode]
        return tuple(n for n in ('fh', 'qres', 'b2', 'o') if not m[n])
    m = FC.BMODES[p.mode]
    return tuple(n for n in ('doff', 'dfh', 'dO', 'dq', 'db2') if not m[n]) + (('doff_out',) if m['dO'] else ())


def arguments(p, dev):
    from strajnet_amd import ops
    cs = p.cs
    null = nulls(p)
    v = {k: (None if k in null else ops._poff(t, GUARD)) for k, t in dev.items()}
    v.update({k: cs[k] for k in SCALARS if k in cs})
    v.update(dtype=ops.DTYPE_CODE[p.dt], stream=ops._st())
    if p.mode is not None:
        v['zmajor'] = (FC.FMODES if p.kind == 'fwd' else FC.BMODES)[p.mode]['zmajor']
    return v


def launch(p, v, raw=False):
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    name, order = ORDER[p.cs['fam'], p.kind]
    args = [ops._p(v[k]) if (v[k] is None or isinstance(v[k], ops.vp)) else v[k] for k in order]
    if raw:
        return getattr(lib(), name)(*args)
    ops.call(name, *args)


def run(p, edit=None, **over):
    """upload, call, download.  edit(dev): changes to the uploaded buffers; over: arguments replaced"""
    dev = upload(p)
    if edit is not None:
        edit(dev)
    launch(p, dict(arguments(p, dev), **over))
    return download(dev)


# ---- stj_fg_attn_* ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dt', FC.family('attn'), ids=FC.case_id)
def test_attn_forward(name, dt):
    """a per (b, token, group) and lse per (b, g) against float64; with lse == NULL the same a bit for bit and lse untouched"""
    cs = FC.case(name)
    p = prepare(cs, dt, 'fwd')
    after = run(p)
    judge(p, after, _RATIOS)
    q = prepare(cs, dt, 'fwd', with_lse=False)
    bare = run(q)
    judge(q, bare, _RATIOS)
    assert torch.equal(bits(bare['a']), bits(after['a'])), 'a of the inference form differs from the training form'


def _zero_scratch(dev):
    for n in ('dkp', 'dvp'):
        dev[n][GUARD:-GUARD] = 0


@pytest.mark.parametrize('name,dt', FC.family('attn'), ids=FC.case_id)
def test_attn_backward_on_reference_saves(name, dt):
    """the backward alone, handed a and lse of R64 (a rounded to dt): every gradient per row; doff carries the pattern at 8 x 8 and non-zero
    values at 16 x 16, dtable starts non-zero; the workspaces need no zeroing: pattern-filled and zero-filled dkp / dvp give the same bits"""
    from strajnet_amd._lib import lib
    cs = FC.case(name)
    assert lib().stj_fg_attn_bwd_workspace_bytes(cs['B'], cs['G'], cs['Hh'], cs['Ww']) == 4 * FC.ws_elems(cs)
    p = prepare(cs, dt, 'bwd')
    after = run(p)
    judge(p, after, _RATIOS)
    again = run(p, _zero_scratch)
    for n in ('dq', 'dk', 'dv'):
        assert torch.equal(bits(after[n]), bits(again[n])), f'{name}: {n} depends on what dkp / dvp held before the call'


@pytest.mark.parametrize('name,dt', FC.family('attn'), ids=FC.case_id)
def test_attn_forward_into_backward(name, dt):
    """the backward kernel on what the forward kernel wrote, against the end-to-end twin (16 bit: under _fg_cases.E2E_TOL)"""
    cs = FC.case(name)
    p = prepare(cs, dt, 'fwd')
    after = run(p)
    judge(p, after)
    q = prepare(cs, dt, 'bwd', saves_from=(FC.value(p, after, 'a'), FC.value(p, after, 'lse')))
    judge(q, run(q), _RATIOS, label=' (behind the forward kernel)')


def test_attn_status_codes():
    """6 x 6, 8 x 16 and 32 x 32 maps are STJ_EUNSUPPORTED, an unknown dtype STJ_EINVAL, B = 0 STJ_OK; none of them writes anything"""
    from strajnet_amd._lib import lib
    for dt in FC.ALL3:
        for kind in ('fwd', 'bwd'):
            p = prepare(FC.case('a16_2'), dt, kind)           # the largest buffers: any of the refused geometries would fit
            dev = upload(p)
            v = arguments(p, dev)
            for over, want in ((dict(Hh=6, Ww=6), EUNSUPPORTED), (dict(Hh=8, Ww=16), EUNSUPPORTED), (dict(Hh=32, Ww=32, B=1, G=1), EUNSUPPORTED),
                               (dict(dtype=7), EINVAL), (dict(B=0), OK)):
                rc = launch(p, dict(v, **over), raw=True)
                assert rc == want, (dt, kind, over, rc, want)
                if want != OK:
                    assert lib().stj_last_error(), (kind, over)
                after = download(dev)
                for n, b in p.bufs.items():
                    assert torch.equal(bits(after[n]), bits(b.init)), (dt, kind, over, n)
            assert launch(p, v, raw=True) == OK
            judge(p, download(dev))


# ---- stj_fg_bias_* ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('fwd', 'bwd'))
@pytest.mark.parametrize('name,dt', FC.family('bias'), ids=FC.case_id)
def test_bias(name, dt, kind):
    """square and 8 x 16 maps; the backward at QS = 8, 7 (ragged query slices; doff and dtable start non-zero) and 1 (doff written over the pattern)"""
    cs = FC.case(name)
    assert cs['QS'] == {1: 8, 9: 7, 33: 1}[cs['B']]
    p = prepare(cs, dt, kind)
    judge(p, run(p), _RATIOS)


# ---- stj_fg_offset_* ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('fwd', 'bwd'))
@pytest.mark.parametrize('name,dt', FC.family('offset'), ids=FC.case_id)
def test_offset_modes(name, dt, kind):
    """every mode of the offset head alone: the tensors a mode hands in as NULL stay bit-identical, dW1 / dW2 / db2 start non-zero"""
    cs = FC.case(name)
    for mode in FC.modes(cs, kind):
        p = prepare(cs, dt, kind, mode)
        judge(p, run(p), _RATIOS)


@pytest.mark.parametrize('dt', FC.ALL3, ids=FC.case_id)
def test_offset_forward_into_backward(dt):
    cs = FC.case('o8_48_384_64')
    p = prepare(cs, dt, 'fwd', 'fh')
    after = run(p)
    judge(p, after)
    q = prepare(cs, dt, 'bwd', 'both', saves_from=FC.value(p, after, 'off'))
    judge(q, run(q), _RATIOS, label=' (behind the forward kernel)')


def test_offset_status_codes():
    """HW = 24 and a misaligned fh / dfh are STJ_EINVAL and write nothing"""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    for dt in FC.ALL3:
        for kind, mode, big in (('fwd', 'fh', 'fh'), ('bwd', 'both', 'dfh')):
            p = prepare(FC.case('o8_48_384_64'), dt, kind, mode)
            dev = upload(p)
            v = arguments(p, dev)
            for over in (dict(HW=24), {big: ops._poff(dev[big], GUARD + 1)}, dict(dtype=7)):
                rc = launch(p, dict(v, **over), raw=True)
                assert rc == EINVAL and lib().stj_last_error(), (dt, kind, over, rc)
                after = download(dev)
                for n, b in p.bufs.items():
                    assert torch.equal(bits(after[n]), bits(b.init)), (dt, kind, over, n)
            assert launch(p, v, raw=True) == OK
            judge(p, download(dev))


# ---- stj_fgoff_* --------------------------------------------------------------------------------------------------------------------------
FGOFF_PTRS = {'fwd': ('q', 'bias', 'gamma', 'beta', 'w1', 'off', 'cols', 'c', 'mean', 'rstd'),
              'bwd': ('gamma', 'beta', 'w1', 'off', 'c', 'mean', 'rstd', 'doff', 'dc', 'dq', 'd_w1', 'd_gamma', 'd_beta', 'd_bias')}
_PACKS = {}


def fgoff_pack(p):
    """the device copy of the case's packed conv kernel in p.dt, between guards (made once per case and dtype)"""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    key = (p.cs['name'], p.dt)
    if key not in _PACKS:
        code = ops.DTYPE_CODE[p.dt]
        out = FC.Buf(int(lib().stj_fgoff_pack_workspace_bytes(code)) // torch.empty(0, dtype=p.dt).element_size(), p.dt).init.cuda()
        w = p.I['w'].contiguous().cuda()
        ops.call('stj_fgoff_pack', ops._p(w), ops._poff(out, GUARD), code, ops._st())
        torch.cuda.synchronize()
        _PACKS[key] = out
    return _PACKS[key]


def fgoff_call(p, dev, null=(), raw=False, **over):
    import ctypes
    from strajnet_amd import ops
    from strajnet_amd._lib import FgOffArgs, lib
    cs = p.cs
    at = lambda t: t.data_ptr() + GUARD * t.element_size()
    f = dict(B=cs['B'], H=cs['H'], W=cs['W'], dtype=ops.DTYPE_CODE[p.dt], scale=cs['scale'], eps=cs['eps'], pack=at(fgoff_pack(p)))
    f.update({n: (None if n in null else at(dev[n])) for n in FGOFF_PTRS[p.kind]})
    f.update(over)
    a = FgOffArgs(**f)
    name = 'stj_fgoff_' + p.kind
    if raw:
        return getattr(lib(), name)(ctypes.byref(a), ops._st())
    ops.call(name, ctypes.byref(a), ops._st())


def fgoff_run(p, null=()):
    dev = upload(p)
    fgoff_call(p, dev, null)
    return download(dev)


SAVED = ('cols', 'c', 'mean', 'rstd')


@pytest.mark.parametrize('name,dt', FC.family('fgoff'), ids=FC.case_id)
def test_fgoff_forward(name, dt):
    """training: off, c, mean and rstd each against float64, cols bit for bit the im2col matrix of q; inference (the four saved pointers NULL):
    off bit-identical and nothing else written"""
    cs = FC.case(name)
    p = prepare(cs, dt, 'fwd')
    after = fgoff_run(p)
    judge(p, after, _RATIOS)
    q = prepare(cs, dt, 'fwd', with_lse=False)
    bare = fgoff_run(q, SAVED)
    judge(q, bare, _RATIOS)
    assert torch.equal(bits(bare['off']), bits(after['off'])), 'off of the inference form differs from the training form'


@pytest.mark.parametrize('name,dt', FC.family('fgoff'), ids=FC.case_id)
def test_fgoff_backward(name, dt):
    """the backward on the reference's saves (c, off rounded to dt), then behind the forward kernel; dq and dc written, the four parameter
    gradients added to non-zero starts"""
    cs = FC.case(name)
    p = prepare(cs, dt, 'bwd')
    judge(p, fgoff_run(p), _RATIOS)
    f = prepare(cs, dt, 'fwd')
    after = fgoff_run(f)
    judge(f, after)
    q = prepare(cs, dt, 'bwd', saves_from=tuple(FC.value(f, after, n) for n in ('c', 'mean', 'rstd', 'off')))
    judge(q, fgoff_run(q), _RATIOS, label=' (behind the forward kernel)')


def test_fgoff_status_codes():
    """W = 24, odd H at W = 8 and f32 at W = 32 are STJ_EUNSUPPORTED; three of the four saved pointers STJ_EINVAL; B = 0 STJ_OK: nothing written"""
    from strajnet_amd._lib import lib
    for dt in FC.ALL3:
        for kind in ('fwd', 'bwd'):
            p = prepare(FC.case('f2_5_16'), dt, kind)          # 160 pixels: H = 3, W = 24 / 32 and H = 5, W = 8 would fit
            dev = upload(p)
            refused = [(dict(W=24, H=3), (), EUNSUPPORTED), (dict(W=8), (), EUNSUPPORTED), (dict(dtype=7), (), EUNSUPPORTED), (dict(scale=0.0), (), EINVAL),
                       (dict(B=0), (), OK)]
            if dt == F32:
                refused.append((dict(W=32, H=2), (), EUNSUPPORTED))
            if kind == 'fwd':
                refused += [({}, tuple(n for n in SAVED if n != skip), EINVAL) for skip in SAVED]
            else:
                refused += [({}, (n,), EINVAL) for n in ('c', 'mean', 'doff', 'dc', 'dq', 'd_w1', 'd_bias')]
            for over, null, want in refused:
                rc = fgoff_call(p, dev, null, raw=True, **over)
                assert rc == want, (dt, kind, over, null, rc, want)
                if want != OK:
                    assert lib().stj_last_error(), (kind, over, null)
                after = download(dev)
                for n, b in p.bufs.items():
                    assert torch.equal(bits(after[n]), bits(b.init)), (dt, kind, over, null, n)
            assert fgoff_call(p, dev, raw=True) == OK
            judge(p, download(dev))


# ---- stj_fgoff_pack / stj_fgoff_supported -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', FC.ALL3, ids=FC.case_id)
def test_fgoff_pack_fills_exactly_its_workspace(dt):
    """stj_fgoff_pack writes exactly stj_fgoff_pack_workspace_bytes(dtype) bytes between intact guards: each direction's half holds every
    weight of the [3, 3, 48, 384] kernel once, rounded to dt, and zeros for the k-steps' padding; a misaligned out is STJ_EINVAL"""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    code = ops.DTYPE_CODE[dt]
    n = int(lib().stj_fgoff_pack_workspace_bytes(code)) // torch.empty(0, dtype=dt).element_size()
    assert n > 0 and n % 2 == 0 and lib().stj_fgoff_pack_workspace_bytes(7) == 0
    g = torch.Generator().manual_seed(11)
    w = FC.Buf(9 * 48 * 384, F32, FC.draw(9 * 48 * 384, F32, g, False))
    out = FC.Buf(n, dt)
    dw, do = w.init.cuda(), out.init.cuda()
    rc = lib().stj_fgoff_pack(ops._poff(dw, GUARD), ops._poff(do, GUARD + 1), code, ops._st())
    torch.cuda.synchronize()
    assert rc == EINVAL and torch.equal(bits(do.cpu()), bits(out.init))
    ops.call('stj_fgoff_pack', ops._poff(dw, GUARD), ops._poff(do, GUARD), code, ops._st())
    torch.cuda.synchronize()
    got = do.cpu()
    assert torch.equal(bits(dw.cpu()), bits(w.init))
    for guard in (slice(0, GUARD), slice(GUARD + n, None)):
        assert torch.equal(bits(got[guard]), bits(out.init[guard])), 'a guard of the pack changed'
    want = w.init[GUARD:-GUARD].to(dt).float().sort().values
    for half in got[GUARD:GUARD + n].float().reshape(2, n // 2):
        assert not bool(half.isnan().any()), 'an element of the pack was not written'
        live = half[half != 0]
        assert live.numel() == want.numel() and torch.equal(live.sort().values, want)


def test_fgoff_supported_geometries():
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    ok = lambda H, W, dt, C=384, G=8: lib().stj_fgoff_supported(H, W, C, G, ops.DTYPE_CODE[dt])
    for dt in FC.ALL3:
        assert ok(2, 8, dt) and ok(6, 8, dt) and ok(1, 16, dt) and ok(5, 16, dt) and ok(4, 16, dt)
        assert not ok(4, 24, dt) and not ok(3, 8, dt) and not ok(0, 16, dt) and not ok(4, 16, dt, C=192) and not ok(4, 16, dt, G=4)
        assert bool(ok(3, 32, dt)) == (dt != F32) and bool(ok(32, 32, dt)) == (dt != F32)
    assert not lib().stj_fgoff_supported(4, 16, 384, 8, 7)


def test_zz_report():
    """(runs last in this file) the largest ||err|| / bound per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(FC.report_lines(_RATIOS, 'fg abi')))
