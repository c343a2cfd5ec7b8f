"""The references, bounds and layout of _layernorm_cases.py, checked without a GPU: for every case of the matrix of test_layernorm_gpu.py
(refusals excepted) a plain PyTorch-CPU statement of the same call goes through the same judge and must pass.

The plain statement works in float32 on the inputs as stored (rounded to dt) and rounds its outputs once to dt.  Forward: F.layer_norm,
mean and var of torch.  Parameter groups by slicing run after run in a Python loop; the PatchMerging gather by torch.cat of the four
strided views (as test_ops_gpu.test_layernorm_merge_gather) and its inverse by strided assignment; the chain as two backward passes with
the intermediate rounded to dt.  It reads and writes the flat buffers by base address and stride, never through the judge's index maps.
Backward: the entry points take mean and rstd as INPUTS, so their statement is the closed form
    dx = rstd (gg - mean_c gg - xh mean_c(gg xh)),  gg = dy gamma,  xh = (x - mean) rstd,  dgamma = sum_rows dy xh,  dbeta = sum_rows dy
in float32 tensor operations on the handed-in statistics.  (Autograd through F.layer_norm recomputes the statistics in float32: on the rows
around +-64 torch's row moments carry |mu| / sigma 2^-24 ~ EPS_ELEM[float32] of relative error in rstd, and on constant rows one ulp of
the mean becomes 316 ulp of xh where the handed-in mean gives 0 -- a different function from the one the ABI defines, and measured here
at 0.9 to 6 times the bound.  The exact twins hand in mean = 0 and a power-of-two rstd that no x has and cannot be stated by autograd at all.)
The exact twins must come out exactly equal here too.

What this shows: the index-arithmetic reference agrees with an independent formulation of groups, gather, res and dres, and every bound is
met by an honest float32 implementation on the hostile rows (large common offset, constant, all-zero, magnitude 1e4).
"""
import pytest
import torch
import torch.nn.functional as F

import _layernorm_cases as LC
from _layernorm_cases import DTYPES, F32, cdiv, judge, matrix, prepare

_RATIOS = []


def _nat(p, name, n):
    b = p.bufs[name]
    return b.init[b.base:b.base + n].float()


def _put(p, after, name, val):
    b = p.bufs[name]
    after[name][b.base:b.base + val.numel()] = val.reshape(-1).to(b.init.dtype)


def _param(p, name, g, part=0, pstride=0):
    cs, b = p.cs, p.bufs[name]
    o = b.base + part * pstride + g * cs.get('gstride', 0)
    return b.init[o:o + cs['C']].clone()


def _merged(cs, xn):
    """logical [rows, C] view of the natural x (gather: the four strided views, concatenated)"""
    if not cs['gres']:
        return xn.reshape(cs['rows'], cs['C'])
    xx = xn.reshape(cs['B'], cs['gres'], cs['gres'], cs['C0'])
    return torch.cat([xx[:, 0::2, 0::2], xx[:, 1::2, 0::2], xx[:, 0::2, 1::2], xx[:, 1::2, 1::2]], -1).reshape(cs['rows'], cs['C'])


def _unmerge(cs, d):
    if not cs['gres']:
        return d
    C0 = cs['C0']
    out = torch.zeros(cs['B'], cs['gres'], cs['gres'], C0)
    dd = d.reshape(cs['B'], cs['gres'] // 2, cs['gres'] // 2, 4 * C0)
    out[:, 0::2, 0::2], out[:, 1::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 1::2] = dd[..., :C0], dd[..., C0:2 * C0], dd[..., 2 * C0:3 * C0], dd[..., 3 * C0:]
    return out


def _runs(cs):
    """(row slice, parameter set) run after run"""
    rows, ng = cs['rows'], max(1, cs.get('ngroups', 1))
    gr = cs['group_rows'] if ng > 1 else rows
    return [(slice(r * gr, min(rows, (r + 1) * gr)), r % ng) for r in range(cdiv(rows, gr))]


def _closed_form(dy, xs, gam, mean, rstd):
    xh = (xs - mean[:, None]) * rstd[:, None]
    gg = dy * gam
    return rstd[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)), dy * xh


def plain_forward(p, after):
    cs = p.cs
    rows, C, ng = cs['rows'], cs['C'], max(1, cs['ngroups'])
    xs = _merged(cs, _nat(p, 'x', rows * C))
    y = torch.empty(rows, C)
    for sl, g in _runs(cs):
        y[sl] = F.layer_norm(xs[sl], (C,), _param(p, 'gamma', g), _param(p, 'beta', g), cs['eps'])
    if cs['res']:
        y = y + _nat(p, 'res', rows * C).reshape(rows, C)
    _put(p, after, 'y', y)
    _put(p, after, 'mean', xs.mean(1))
    _put(p, after, 'rstd', torch.rsqrt(xs.var(1, unbiased=False) + cs['eps']))


def _ln_backward(cs, xn, dy, gammas, mean, rstd):
    """-> dx in x's natural layout, [dgamma per set], [dbeta per set] in float32"""
    rows, C = cs['rows'], cs['C']
    runs = _runs(cs)
    xs = _merged(cs, xn)
    dxs, dgs, dbs = torch.empty(rows, C), [torch.zeros(C) for _ in gammas], [torch.zeros(C) for _ in gammas]
    for sl, g in runs:
        dxs[sl], t = _closed_form(dy[sl], xs[sl], gammas[g], mean[sl], rstd[sl])
        dgs[g] += t.sum(0)
        dbs[g] += dy[sl].sum(0)
    return _unmerge(cs, dxs).reshape(-1), dgs, dbs


def _put_param_grads(p, after, name, sums, pstride):
    for g, s in enumerate(sums):          # the whole sum into copy 0; the other copies keep their starting values
        b = p.bufs[name]
        o = b.base + g * p.cs.get('gstride', 0)
        after[name][o:o + s.numel()] = _param(p, name, g) + s


def plain_backward(p, after):
    cs = p.cs
    rows, C, ng = cs['rows'], cs['C'], max(1, cs['ngroups'])
    dy = _nat(p, 'dy', rows * C).reshape(rows, C)
    dx, dgs, dbs = _ln_backward(cs, _nat(p, 'x', rows * C), dy, [_param(p, 'gamma', g) for g in range(ng)], _nat(p, 'mean', rows), _nat(p, 'rstd', rows))
    if cs['dres']:
        dx = dx + _nat(p, 'dres', rows * C)
    _put(p, after, 'dx', dx)
    _put_param_grads(p, after, 'dgamma', dgs, cs['pstride'])
    _put_param_grads(p, after, 'dbeta', dbs, cs['pstride'])


def plain_chain(p, after):
    cs = p.cs
    rows, C = cs['rows'], cs['C']
    dy = _nat(p, 'dy', rows * C).reshape(rows, C)
    d2, dg2, db2 = _ln_backward(cs | dict(gres=0), _nat(p, 'x2', rows * C), dy, [_param(p, 'gamma2', 0)], _nat(p, 'mean2', rows), _nat(p, 'rstd2', rows))
    d2 = d2.to(p.dt)
    dx1, dg1, db1 = _ln_backward(cs | dict(gres=0), _nat(p, 'x1', rows * C), d2.float().reshape(rows, C), [_param(p, 'gamma1', 0)], _nat(p, 'mean1', rows),
                                 _nat(p, 'rstd1', rows))
    if cs['d2out']:
        _put(p, after, 'd2out', d2)
    _put(p, after, 'dx1', dx1)
    for n, s in (('dgamma2', dg2), ('dbeta2', db2), ('dgamma1', dg1), ('dbeta1', db1)):
        _put_param_grads(p, after, n, s, 0)


PLAIN = dict(fwd=plain_forward, bwd=plain_backward, chain=plain_chain)


def run_plain(cs, dt):
    for kind in cs['kinds']:
        for exact in ((False,) if kind == 'fwd' else (False, True)):
            p = prepare(cs, dt, kind, exact)
            after = {k: b.init.clone() for k, b in p.bufs.items()}
            PLAIN[kind](p, after)
            judge(p, after, _RATIOS)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
@pytest.mark.parametrize('family', ['v2', 'v1', 'gather', 'groups', 'parts', 'res', 'chain'])
def test_plain_float32_statement_passes_the_judge(family, dt):
    failed = []
    cases = matrix(dt)[family]
    for cs in cases:
        try:
            run_plain(cs, dt)
        except AssertionError as e:
            failed.append(f"{cs['name']} [{dt}]: {e}")
    assert not failed, f'{len(failed)} of {len(cases)} cases failed:\n' + '\n'.join(failed)


def test_judge_notices_single_element_faults():
    """The judge itself: one guard element, one unwritten output element, one row of dx missed, one group's gamma taken from its neighbour,
    one row counted twice in the twin's dbeta -- each must fail."""
    dt = torch.bfloat16
    cs = LC.lncase('judge', 150, 96, ngroups=2, group_rows=37, gstride=104, dres=True)

    def run(kind, exact, spoil):
        p = prepare(cs, dt, kind, exact)
        after = {k: b.init.clone() for k, b in p.bufs.items()}
        PLAIN[kind](p, after)
        judge(p, after)
        spoil(p, after)
        with pytest.raises(AssertionError):
            judge(p, after)

    def guard(p, after):
        after['y'][p.bufs['y'].base - 1] = 1.0

    def unwritten(p, after):
        after['y'][p.bufs['y'].base + 5] = p.bufs['y'].init[0]

    def row_missed(p, after):
        b = p.bufs['dx']
        after['dx'][b.base + 36 * 96:b.base + 37 * 96] = _nat(p, 'dres', 150 * 96)[36 * 96:37 * 96].to(dt)     # dres only, no LayerNorm term

    def neighbours_gamma(p, after):          # row 37 is the first row of run 1 (parameter set 1): give it set 0's parameters
        xs = _nat(p, 'x', 150 * 96).reshape(150, 96)
        b = p.bufs['y']
        after['y'][b.base + 37 * 96:b.base + 38 * 96] = F.layer_norm(xs[37], (96,), _param(p, 'gamma', 0), _param(p, 'beta', 0), cs['eps']).to(dt)

    def twice(p, after):
        b = p.bufs['dbeta']
        after['dbeta'][b.base:b.base + 96] += _nat(p, 'dy', 150 * 96)[:96]

    run('fwd', False, guard)
    run('fwd', False, unwritten)
    run('bwd', False, row_missed)
    run('fwd', False, neighbours_gamma)
    run('bwd', True, twice)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_closed_form_agrees_with_autograd_on_benign_rows(dt):
    """The closed form above against an independent derivation: F.layer_norm and autograd in float32 through the same judge, on rows of
    +-U[0.25, 1) only (where the statistics autograd recomputes agree with the handed-in ones to float32 rounding): plain, res / dres,
    parameter groups with a short last run, and the gather."""
    cases = [LC.lncase('auto_plain', 77, 96), LC.lncase('auto_v1', 77, 100, dres=True), LC.gcase('auto_gather', 3, 4, 24),
             LC.lncase('auto_groups', 3 * 3 * 37 - 11, 96, ngroups=3, group_rows=37, gstride=104, dres=True)]
    for cs in cases:
        rows, C, ng = cs['rows'], cs['C'], cs['ngroups']
        p = prepare(cs, dt, 'bwd', False, benign=True)
        after = {k: b.init.clone() for k, b in p.bufs.items()}
        xn = _nat(p, 'x', rows * C).requires_grad_(True)
        gam = [_param(p, 'gamma', g).requires_grad_(True) for g in range(ng)]
        bet = [torch.zeros(C, requires_grad=True) for _ in range(ng)]
        xs = _merged(cs, xn)
        y = torch.cat([F.layer_norm(xs[sl], (C,), gam[g], bet[g], cs['eps']) for sl, g in _runs(cs)], 0)
        y.backward(_nat(p, 'dy', rows * C).reshape(rows, C))
        dx = xn.grad.reshape(-1)
        _put(p, after, 'dx', dx + _nat(p, 'dres', rows * C) if cs['dres'] else dx)
        _put_param_grads(p, after, 'dgamma', [t.grad for t in gam], 0)
        _put_param_grads(p, after, 'dbeta', [t.grad for t in bet], 0)
        judge(p, after)


def test_restated_launch_geometry():
    """the sub-run example of the case matrix: C = 96 in 16 bits, two groups of 500 rows -> S = 8 sub-runs of L = 63 rows, off the 64-row pass"""
    cs = LC.lncase('g', 1000, 96, ngroups=2, group_rows=500, gstride=104)
    assert LC.bwd_geometry(cs, torch.bfloat16) == (8, 8, 63) and LC.pass_rows(96, torch.bfloat16) == 64
    for dt in DTYPES:
        for fam, cases in matrix(dt).items():
            for c in cases:
                for kind in c['kinds']:
                    if c['name'] == 'v1_gather_C0_20' and dt == F32:
                        continue                  # C0 = 20 is a whole number of 4-element vectors: scalar kernels in 16 bits only
                    assert LC.path_of(c, dt, kind).startswith({'v2': 'v2', 'v1': 'v1', 'chain': 'chain'}.get(fam, ''))
    assert {(str(dt), LC.path_of(c, dt, 'chain')) for dt in DTYPES for c in matrix(dt)['chain']} == {(str(dt), f'chain LPR {l}') for dt in DTYPES for l in (16, 32, 64)}
    shapes = {(str(dt), LC.v2_shape(c['C'], dt)[:2]) for dt in DTYPES for c in matrix(dt)['v2']}
    assert shapes == {(str(dt), s) for dt in DTYPES for s in ((16, 1), (32, 1), (64, 1), (64, 2), (64, 3))}


def test_zz_report_plain_statement_ratios():
    """(runs last in this file) the largest |err| / T of the float32 statement per (entry point, path, dtype, output), under pytest -s"""
    LC.report(_RATIOS, 'plain f32')
