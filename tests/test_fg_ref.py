"""The references, bounds and judge of _fg_cases.py, checked without a GPU.

  1. The twin with the identity for a rounding -- its forward walking the keys as the kernel does, its backward on its own forward and on
     the reference's saves -- reproduces R64 on every case.
  2. R64's hand-written backward equals autograd through the oracle's restatement of sample (oracle.torch_ref._sample = grid_sample) away
     from the lattice: the attention core on an 8 x 8 map (some keys far outside the table) and the bias alone on the non-square 8 x 16 map;
     the fused offset head's equals autograd through F.conv2d / F.layer_norm / F.gelu(tanh), and cols^T dc is the conv kernel's gradient.
  3. On the lattice the tie rule holds as derived in _fg_cases.py: an alpha receives a gradient iff 0 < a <= 1; in the LATTICE group of the
     marked cases R64's offset gradient is exactly zero wherever no query passes one although the one-sided slopes are not, the keys whose
     sample point reaches alpha == 1 carry one, and the FAR group has none at all and no table gradient.
  4. A CPU float32 statement of R64 (the same text evaluated in torch.float32, the 16-bit rows with the twin's roundings) passes the judge
     on every case, mode and dtype, and at ratio <= 0.5 wherever the bound is the float32 one: TOL_FWD / TOL_BWD of _xattn_cases are kept.
     Largest float32 ratio measured: see RATIO_F32_MAX below.  The forward-into-backward form of test_fg_abi_gpu.py (the backward on the
     saves of the statement's own forward, against the end-to-end twin) is at ratio <= 0.5 in every dtype under _fg_cases.E2E_TOL.
     profiles/test_fg_ref_ratios.txt is the record of one run (test_zz_report_float32_ratios).
  5. The judge is sensitive, in float32 and bf16: one (b, g) block of a scaled by 1.02; one key slice's contribution dropped; doff added
     twice; a "+=" output overwritten (both, and a block of dq scaled by 1.02, again under the end-to-end bound with E2E_TOL); one halo row
     of the fused offset head's conv taken from the neighbouring sample; an offset gradient of 1e-6 where the rule says zero; the far
     group's dtable column touched; one guard element changed; one output element left at the pattern.
"""
import pytest
import torch

import _fg_cases as FC
from _fg_cases import BF16, F32, F64, GUARD, judge, pack, prepare

RATIO_F32_MAX = 0.5          # the float32 statement must stay at or under this on every case (measured, profiles/test_fg_ref_ratios.txt: 0.24 -- fh of o8_256_1024_16; a 0.21, doff 0.12 of a16_*)
_RATIOS = []


def _calls():
    out = []
    # (the float32 statement is judged on every case, the 16-bit-only geometries included: prepare() does not look at a case's dts)
    for name, dt in FC.CASE_DT + [(c['name'], F32) for c in FC.cases() if F32 not in c['dts']]:
        for kind in ('fwd', 'bwd'):
            out += [(name, dt, kind, m) for m in FC.modes(FC.case(name), kind)]
    return out


def _statement(p, dtype, rd, **kw):
    """the outputs of the call p describes by _fg_cases' statement in `dtype`, the backward on the saves the call is handed"""
    cs, fam = p.cs, p.cs['fam']
    saves = None
    if p.kind == 'bwd' and fam == 'attn':
        saves = tuple(p.bufs[n].init[GUARD:-GUARD].to(dtype) for n in ('a', 'lse'))
    if p.kind == 'bwd' and fam == 'fgoff':
        saves = tuple(p.bufs[n].init[GUARD:-GUARD].to(dtype) for n in ('c', 'mean', 'rstd', 'off'))
    if p.kind == 'bwd' and fam == 'offset':
        saves = p.bufs['off'].init[GUARD:-GUARD].to(dtype).reshape(cs['B'], cs['G'], cs['HW'], 2)
    T = FC.STATEMENT[fam](cs, p.I, dtype=dtype, rd=rd, saves=saves, **kw)
    return T[f'{p.kind}:{p.mode}'] if fam == 'offset' else T


# ---- 1. the twin --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in FC.cases()])
def test_twin_without_rounding_is_r64(name):
    cs = FC.case(name)
    I, R, _ = FC.references(cs, F32)
    kw = dict(stepwise=True) if cs['fam'] == 'attn' else {}
    sv = dict(attn=lambda: (R['a'], R['lse']), bias=lambda: None, offset=lambda: R['fwd:off_only']['off'],
              fgoff=lambda: (R['c'], R['mean'], R['rstd'], R['off']))[cs['fam']]()
    for saves in (None, sv):
        T = FC.STATEMENT[cs['fam']](cs, I, rd=lambda t: t, saves=saves, **kw)
        pairs = [(T[k], R[k], k) for k in R if not k.startswith('_')] if cs['fam'] != 'offset' else \
                [(T[m][k], R[m][k], m + k) for m in R if not m.startswith('_') for k in R[m]]
        for t, r, k in pairs:
            assert float((t - r).abs().max()) <= 1e-10 * max(float(r.abs().max()), 1e-30), k


# ---- 2. the hand-written backward against autograd ----------------------------------------------------------------------------------------
def _autograd_bias(cs, off, table):
    """bias [B, G, HW, HW] through the oracle's sample; off, table float64 leaves"""
    from oracle.torch_ref import _sample
    B, G, HW, Hh, Ww = cs['B'], cs['G'], cs['HW'], cs['Hh'], cs['Ww']
    n = torch.arange(HW)
    i, j = (n // Ww).double(), (n % Ww).double()
    x = (i[:, None] - i[None, :])[None, None] - off[..., 1][:, :, None, :]
    y = (j[:, None] - j[None, :])[None, None] - off[..., 0][:, :, None, :]
    tab = table.permute(2, 0, 1)[None].expand(B, -1, -1, -1).reshape(B * G, 2 * Hh - 1, 2 * Ww - 1, 1)
    return _sample(tab, torch.stack((x, y), -1).reshape(B * G, HW, HW, 2)).reshape(B, G, HW, HW)


@pytest.mark.parametrize('cs', [FC.acase('tiny_a', 2, 8, G=2), FC.bcase('tiny_b', 2, 8, 16, G=3)], ids=lambda c: c['name'])
def test_r64_backward_agrees_with_autograd_off_the_lattice(cs):
    assert not cs['marked']
    I = FC.make_inputs(cs, F32)
    I['off'][0, 0, :4] = FC.FAR_OFF
    I['off'][1, 1, 5:9] = -FC.FAR_OFF
    R = FC.STATEMENT[cs['fam']](cs, I)
    off, table = (I[n].double().clone().requires_grad_(True) for n in ('off', 'table'))
    bias = _autograd_bias(cs, off, table)
    assert float((bias.detach() - R.get('bias', bias.detach())).abs().max()) <= 1e-12
    if cs['fam'] == 'bias':
        bias.backward(I['dbias'].double())
        got = dict(doff=off.grad, dtable=table.grad)
    else:
        q, k, v = (FC._heads(I[n].double(), cs).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
        logit = cs['scale'] * (q @ k.transpose(-1, -2)) + bias
        a = torch.softmax(logit, -1) @ v
        a.backward(FC._heads(I['da'].double(), cs))
        got = dict(a=FC._tokens(a.detach(), cs), lse=torch.logsumexp(logit.detach(), -1), dq=FC._tokens(q.grad, cs), dk=FC._tokens(k.grad, cs),
                   dv=FC._tokens(v.grad, cs), doff=off.grad, dtable=table.grad)
    for n, g in got.items():
        assert float((g - R[n]).abs().max()) <= 1e-10 * float(R[n].abs().max()), n
    assert float(R['doff'].abs().max()) > 0 and float(R['dtable'].abs().max()) > 0


def test_fused_offset_head_backward_agrees_with_autograd():
    import torch.nn.functional as F
    cs = FC.fcase('tiny_f', 2, 2, 8)
    I = FC.make_inputs(cs, F32)
    R = FC.fgoff_statement(cs, I)
    q, w, bias, gamma, beta, w1 = (I[n].double().clone().requires_grad_(True) for n in ('q', 'w', 'bias', 'gamma', 'beta', 'w1'))
    c = (F.conv2d(q.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1, groups=8).permute(0, 2, 3, 1) + bias)
    c.retain_grad()
    o = F.gelu(F.layer_norm(c, (FC.FC_C,), gamma, beta, cs['eps']), approximate='tanh')
    off = torch.tanh(torch.einsum('bngc,co->bgno', o.reshape(cs['B'], cs['HW'], 8, FC.D), w1)) * cs['scale']
    off.backward(I['doff'].double())
    got = dict(off=off.detach(), c=c.detach(), dc=c.grad, dq=q.grad, d_w1=w1.grad, d_gamma=gamma.grad, d_beta=beta.grad, d_bias=bias.grad)
    for n, g in got.items():
        assert float((g - R[n]).abs().max()) <= 1e-10 * float(R[n].abs().max()), n
    # the caller's weight gradient is cols^T dc: the saved im2col matrix and dc reproduce autograd's
    dw = torch.einsum('mgk,mgn->gkn', FC.im2col(I['q']).double(), R['dc'].reshape(-1, 8, FC.D)).reshape(8, 3, 3, FC.D, FC.D).permute(1, 2, 3, 0, 4)
    assert float((dw.reshape(3, 3, FC.D, FC.FC_C) - w.grad).abs().max()) <= 1e-10 * float(w.grad.abs().max())


# ---- 3. the lattice -----------------------------------------------------------------------------------------------------------------------
def test_an_alpha_passes_a_gradient_iff_it_lies_in_0_1():
    size_p = 17
    #                      interior integer, interior, below the pad (a < 0), a == 1 at size - 1, beyond (a > 1), exactly 0, just inside
    coord = torch.tensor([5.0, 5.5, -0.5, size_p - 1.0, size_p - 0.5, 0.0, 0.125], dtype=F64)
    f, a, g = FC._axis(coord, size_p)
    assert f.tolist() == [5, 5, 0, size_p - 2, size_p - 2, 0, 0]
    assert a.tolist() == [0.0, 0.5, 0.0, 1.0, 1.0, 0.0, 0.125]
    assert g.tolist() == [False, True, False, True, False, False, True]


@pytest.mark.parametrize('name', ['a8_1', 'a16_1', 'b8x8_9', 'b8x16_9'])
def test_lattice_and_far_groups_of_r64(name):
    cs = FC.case(name)
    I, R, _ = FC.references(cs, F32)
    dead, doff = ~R['_passes'], R['doff']
    assert not bool((doff[dead] != 0).any())
    assert bool(dead[:, FC.FAR].all()) and not bool((R['dtable'][:, :, FC.FAR] != 0).any())
    lat = dead[:, FC.LATTICE]
    if cs['Hh'] == cs['Ww']:         # (on the 8 x 16 map column differences reach the last padded row of the 15-row table: alpha == 1 there too)
        assert bool(lat[:, 4:].all()), 'an integer offset within +-Hh/2 passes a gradient'
    assert int(lat[:, 4:].sum()) > lat[:, 4:].numel() // 2
    alive = ~lat[:, :4]
    # (where both alphas are 1 the x slope is taken in the pad row and is zero: most, not all, of the passing components carry a value)
    assert bool(alive.any()) and 2 * int((doff[:, FC.LATTICE, :4][alive] != 0).sum()) > int(alive.sum()), 'alpha == 1 passes the slope towards the pad'
    # the value is not flat there: autograd through grid_sample (a one-sided slope) finds a gradient where TF's rule has none
    off, table = (I[n].double().clone().requires_grad_(True) for n in ('off', 'table'))
    go = R['_P'] if cs['fam'] == 'attn' else I['dbias'].double()
    (_autograd_bias(cs, off, table) * go).sum().backward()
    assert float(off.grad[:, FC.LATTICE, 4:].abs().max()) > 1e-3


# ---- 4. the float32 statement through the judge -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dt,kind,mode', _calls(), ids=FC.case_id)
def test_float32_statement_passes_the_judge(name, dt, kind, mode):
    p = prepare(FC.case(name), dt, kind, mode)
    rd = (lambda t: t) if dt == F32 else (lambda t: t.to(dt).float())
    kw = dict(stepwise=True) if p.cs['fam'] == 'attn' else {}
    r = []
    judge(p, pack(p, _statement(p, F32, rd, **kw)), r)
    _RATIOS.extend(r)
    # (the constants under test are the float32 ones; a 16-bit row only has to pass: float32 arithmetic flips some of the twin's roundings)
    assert dt != F32 or max(x[4] for x in r) <= RATIO_F32_MAX, r


def _forward_into_backward(cs, dt, dtype=F32):
    """(the backward call behind a forward that `dtype` arithmetic with the twin's roundings computed, that statement's outputs)"""
    fam = cs['fam']
    rd = (lambda t: t) if dt == F32 else (lambda t: t.to(dt).to(dtype))
    I = FC.references(cs, dt)[0]
    T = FC.STATEMENT[fam](cs, I, dtype=dtype, rd=rd, **(dict(stepwise=True) if fam == 'attn' else {}))
    if fam == 'attn':
        return prepare(cs, dt, 'bwd', saves_from=(T['a'].to(dt), T['lse'].float())), T
    if fam == 'fgoff':
        return prepare(cs, dt, 'bwd', saves_from=(T['c'].to(dt), T['mean'].float(), T['rstd'].float(), T['off'].to(dt))), T
    return prepare(cs, dt, 'bwd', 'both', saves_from=T['fwd:fh']['off'].to(dt)), T['bwd:both']


E2E = [(n, dt) for n, dt in FC.CASE_DT if FC.case(n)['fam'] in ('attn', 'fgoff') or n == 'o8_48_384_64']


@pytest.mark.parametrize('name,dt', E2E, ids=FC.case_id)
def test_float32_statement_forward_into_backward(name, dt):
    """the form test_fg_abi_gpu.py judges behind the forward kernel: the backward on the saves of the statement's OWN forward, in float32
    with the twin's roundings, against the end-to-end twin -- at ratio <= 0.5 for every output, under E2E_TOL where an output needed it"""
    p, T = _forward_into_backward(FC.case(name), dt)
    r = []
    judge(p, pack(p, T), r, label=' (behind the forward)')
    _RATIOS.extend(r)
    assert max(x[4] for x in r) <= RATIO_F32_MAX, r


def test_zz_report_float32_ratios():
    """(runs last in this file) the largest ratio of the float32 statement per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(FC.report_lines(_RATIOS, 'fg f32 statement')))


# ---- 5. the judge rejects planted faults --------------------------------------------------------------------------------------------------
def _good(p):
    """a passing result: R64 in float32, the twin in the 16-bit types"""
    return {n: (p.R if p.dt == F32 else p.tw)[n].clone() for n in p.outs}


def _rejects(p, after, what):
    with pytest.raises(AssertionError, match=what):
        judge(p, after)


@pytest.mark.parametrize('dt', [F32, BF16], ids=FC.case_id)
def test_judge_rejects_planted_faults(dt):
    cs = FC.case('a16_2')
    f, b = prepare(cs, dt, 'fwd'), prepare(cs, dt, 'bwd')
    judge(f, pack(f, _good(f)))
    judge(b, pack(b, _good(b)))
    # one (b, g) block of a scaled by 1.02
    v = _good(f)
    v['a'].reshape(cs['B'], cs['HW'], cs['G'], FC.D)[1, :, 5] *= 1.02
    _rejects(f, pack(f, v), 'a: 256 of 4096 rows over their bound')
    # one key slice's share of one (b, g) dropped from the sum and the row sum
    rd = (lambda t: t) if dt == F32 else (lambda t: t.to(dt).double())
    v = FC.attn_statement(cs, f.I, rd=rd, fault='slice_dropped')
    _rejects(f, pack(f, v), 'a: ')
    # doff added twice; dtable written instead of added
    v = _good(b)
    v['doff'] = 2 * v['doff']
    _rejects(b, pack(b, v), 'doff: ')
    after = pack(b, _good(b))
    after['dtable'][GUARD:-GUARD] = b.R['dtable'].reshape(-1).float()
    _rejects(b, after, 'dtable: ')
    # the same two, and a block of dq scaled by 1.02, under the end-to-end bound of the forward-into-backward form (E2E_TOL)
    e, T = _forward_into_backward(cs, dt, F64)
    good = lambda: {n: T[n].clone() for n in e.outs}
    judge(e, pack(e, good()))
    v = good()
    v['doff'] = 2 * v['doff']
    _rejects(e, pack(e, v), 'doff: ')
    after = pack(e, good())
    after['dtable'][GUARD:-GUARD] = e.R['dtable'].reshape(-1).float()
    _rejects(e, after, 'dtable: ')
    after = pack(e, good())
    after['doff'][GUARD:-GUARD] = e.R['doff'].reshape(-1).float()
    _rejects(e, after, 'doff')
    v = good()
    v['dq'].reshape(cs['B'], cs['HW'], cs['G'], FC.D)[1, :, 5] *= 1.02
    _rejects(e, pack(e, v), 'dq: ')
    # an offset gradient where the rule says zero, far below any bound
    after = pack(b, _good(b))
    FC.value(b, after, 'doff')[0, FC.LATTICE, 7, 0] += 1e-6
    _rejects(b, after, 'doff moved at 1 ')
    after = pack(b, _good(b))
    FC.value(b, after, 'dtable')[3, 3, FC.FAR] += 1e-6
    _rejects(b, after, 'far group changed')
    # bytes that are no output; an output element never written
    after = pack(b, _good(b))
    after['dq'][GUARD - 1] = 0
    _rejects(b, after, 'outside the outputs changed')
    after = pack(b, _good(b))
    after['q'][GUARD + 5] = 1.0
    _rejects(b, after, 'of q outside the outputs changed')
    after = pack(b, _good(b))
    after['dk'][GUARD + 77] = b.bufs['dk'].init[0]
    _rejects(b, after, 'still hold the fill pattern')
    # one halo row of the fused offset head's conv taken from the neighbouring sample
    cf = FC.case('f3_6_8')
    h = prepare(cf, dt, 'fwd', with_lse=False)
    rd = (lambda t: t) if dt == F32 else (lambda t: t.to(dt).double())
    judge(h, pack(h, FC.fgoff_statement(cf, h.I, rd=rd)))
    _rejects(h, pack(h, FC.fgoff_statement(cf, h.I, rd=rd, fault='halo')), 'off: ')
    # the same two contracts at the bias kernel's ragged query slices
    cb = FC.case('b8x8_9')
    q = prepare(cb, dt, 'bwd')
    judge(q, pack(q, _good(q)))
    v = _good(q)
    v['doff'] = 2 * v['doff']
    _rejects(q, pack(q, v), 'doff: ')
    after = pack(q, _good(q))
    after['doff'][GUARD:-GUARD] = q.R['doff'].reshape(-1).float()
    _rejects(q, after, 'doff')
