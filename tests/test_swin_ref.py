"""The references, bounds and judge of _swin_cases.py, checked without a GPU (the cases below 32768 rows; the larger ones share the code).

  1. R64 is autograd-consistent: on a tiny case per half (MLP: two samples with DropPath; attention: one 8 x 8 map shifted by 3, where a
     single window holds all the mask regions) the directional derivatives of sum(y dy) by central differences in float64 agree with
     autograd for every leaf; and the hand-written backward of the twin, with the identity for a rounding, reproduces R64 and its autograd
     gradients on every case, on its own forward and on the reference's saves.
  2. A plain layer-by-layer statement passes the judge: torch float32, F.layer_norm / F.gelu(tanh) / F.softmax and autograd; the windows
     are gathered through the token index ((row + shift) mod res) and the mask comes from region labels computed by comparison, not from
     roll + reshape + a label image; in the 16-bit rows every layer's output is stored in dt (ln, the fc1 pre-activation, h, the fc2
     output, qkv, P, the attention output, the projection, y), i.e. it rounds at other places than the twin, and its gradients stay
     float32 until they are outputs.  Every case and dtype, forward and backward, the ratios printed.
     Largest float32 ratio measured: see RATIO_F32_MAX below -- under the 0.5 that keeps _xattn_cases' TOL_FWD / TOL_BWD.
  3. The judge is sensitive: single faults of a passing result, each must fail -- in float32 all sixteen, in bf16 all but the erf-form GELU
     (it differs from the tanh form by at most 5e-4, below the bf16 resolution of h and y: honest bf16 bounds cannot see it).
"""
import pytest
import torch
import torch.nn.functional as F

import _swin_cases as SC
from _swin_cases import BF16, EPS, F32, GUARD, OUTS, SCALE, judge, prepare
from test_gemm_gpu import pattern

_RATIOS = []
RATIO_F32_MAX = 0.5          # the float32 statement must stay at or under this on every case (measured: 0.13 -- ln of m384_8176, qkv of a384_2_16_4, h of m192_8192)
SMALL = [(n, dt) for n, dt in SC.CASE_DT if SC.small(SC.case(n))]


# ---- 1. the references --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cs', [SC.mcase('tiny_m', 32, 32, rps=16, p=0.3), SC.acase('tiny_a', 64, 1, 8, 3), SC.acase('tiny_b', 32, 2, 16, 5, p=0.3)],
                         ids=lambda c: c['name'])
def test_r64_gradients_agree_with_finite_differences(cs):
    I = SC.make_inputs(cs, F32)
    dp = SC.dp_rows(cs, SC.cpu_keep(cs))
    D = SC._f64(I)
    leaves = [n for n in SC.INPUTS[cs['half'], 'fwd']]
    for n in leaves:
        D[n] = D[n].clone().requires_grad_(True)
    f = lambda E: ((SC.mlp_graph(E, dp) if cs['half'] == 'mlp' else SC.attn_graph(cs, E, dp))['y'] * E['dy']).sum()
    f(D).backward()
    g = torch.Generator().manual_seed(5)
    h = 1e-6
    for n in leaves:
        d = torch.randn(D[n].shape, generator=g, dtype=torch.float64)
        val = []
        for s in (h, -h):
            E = {k: v.detach() for k, v in D.items()}
            E[n] = E[n] + s * d
            val.append(float(f(E)))
        num, ana = (val[0] - val[1]) / (2 * h), float((D[n].grad * d).sum())
        assert abs(num - ana) <= 1e-6 * max(abs(ana), 1.0), (n, num, ana)


@pytest.mark.parametrize('name', [c['name'] for c in SC.cases() if SC.small(c)])
def test_twin_without_rounding_is_r64(name):
    cs = SC.case(name)
    I, R, _ = SC.references(cs, F32, SC.cpu_keep(cs), 'cpu')
    names = OUTS[cs['half'], 'fwd'] + OUTS[cs['half'], 'bwd']
    for saves in (None,) + (({k: R[k] for k in ('qkv', 'mean', 'rstd')},) if cs['half'] == 'attn' else ()):
        T = SC.twin(cs, I, SC.cpu_keep(cs), lambda t: t, saves)
        for n in names:
            assert float((T[n].reshape(R[n].shape) - R[n]).abs().max()) <= 1e-10 * float(R[n].abs().max()), n


# ---- 2. a plain statement through the judge -----------------------------------------------------------------------------------------------
class _Store(torch.autograd.Function):
    """a layer boundary of a 16-bit chain: the layer's output is stored in dt (gradients pass in f32 and are rounded once, as outputs)"""
    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).float()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _swap(x, saved):
    """the saved value in place of x, x's place in the graph (x - x.detach() is exactly zero)"""
    return saved + (x - x.detach())


def plain(p):
    """name -> output of the call p describes ("+=" outputs without start values), by the layer-by-layer float32 statement"""
    cs, dt, I = p.cs, p.dt, p.I
    C, M, B = cs['C'], cs['M'], cs['B']
    st = (lambda t: t) if dt == F32 else (lambda t: _Store.apply(t, dt))
    x, gamma, beta = (I[n].float().clone().requires_grad_(True) for n in ('x', 'gamma', 'beta'))
    dp = torch.ones(M, 1) if p.keep is None else (p.keep.float() / (1.0 - cs['p'])).repeat_interleave(cs['rps'])[:, None]
    ln = st(F.layer_norm(x, (C,), gamma, beta, EPS))
    if cs['half'] == 'mlp':
        pre = st(ln @ I['w1'].float() + I['b1'])
        pre.retain_grad()
        h = st(F.gelu(pre, approximate='tanh'))
        t = st(h @ I['w2'].float() + I['b2'])
        t.retain_grad()
        y = st(x + dp * t)
        y.backward(I['dy'].float())
        out = dict(y=y, ln=ln, h=h, dpre=pre.grad, dys=t.grad, dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
        return {k: v.detach() for k, v in out.items()}
    res, shift, H, nw = cs['res'], cs['shift'], C // 32, cs['res'] // 8
    table = I['table'].clone().requires_grad_(True)
    wy, wx, ty, tx = torch.meshgrid(torch.arange(nw), torch.arange(nw), torch.arange(8), torch.arange(8), indexing='ij')
    ry, rx = (wy * 8 + ty).reshape(-1, 64), (wx * 8 + tx).reshape(-1, 64)
    tok = (((ry + shift) % res) * res + (rx + shift) % res).reshape(-1)          # token at window slot
    region = lambda r: (r >= res - 8).long() + (r >= res - shift).long()
    lab = region(ry) * 3 + region(rx)
    qi = torch.arange(64)
    bidx = (qi[:, None] // 8 - qi[None, :] // 8 + 7) * 15 + (qi[:, None] % 8 - qi[None, :] % 8 + 7)
    qkv = st(ln @ I['wqkv'].float() + I['bqkv'])
    if p.kind == 'bwd':
        qkv = _swap(qkv, p.bufs['qkv'].init[GUARD:-GUARD].float().reshape(M, 3 * C))
    qkv.retain_grad()
    gq = qkv.reshape(B, res * res, 3 * C)[:, tok].reshape(B, nw * nw, 64, 3, H, 32)
    q, k, v = (gq[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * SCALE + table[bidx.reshape(-1)].reshape(64, 64, H).permute(2, 0, 1)
    if shift > 0:
        s = s + torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)[None, :, None]
    o = st(st(F.softmax(s, -1)) @ v).permute(0, 1, 3, 2, 4).reshape(B, nw * nw * 64, C)
    inv = torch.empty_like(tok)
    inv[tok] = torch.arange(tok.numel())
    a = o[:, inv].reshape(M, C)
    t = st(a @ I['wproj'].float() + I['bproj'])
    t.retain_grad()
    y = st(x + dp * t)
    y.backward(I['dy'].float())
    xd = x.detach()
    mean = xd.mean(-1, keepdim=True)
    out = dict(y=y, qkv=qkv, a=a, ln=ln, mean=mean, rstd=1.0 / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + EPS), dx=x.grad, dqkv=qkv.grad,
               dys=t.grad, dtable=table.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return {k: v.detach() for k, v in out.items()}


def fill(p, values):
    """the flat buffers as a call that produced `values` would leave them; a "+=" output's value is spread evenly over its copies"""
    after = {k: b.init.clone() for k, b in p.bufs.items()}
    for n, (bname, offs, rows, width) in p.outs.items():
        for c, o in enumerate(offs):
            v = values[n].reshape(-1).double()
            if n in SC.ADDED:
                v = p.start[n][c].reshape(-1) + v / len(offs)
            after[bname][GUARD + o:GUARD + o + rows * width] = v.to(after[bname].dtype)
    return after


@pytest.mark.parametrize('name,dt', SMALL, ids=SC.case_id)
def test_plain_statement_passes_the_judge(name, dt):
    cs = SC.case(name)
    for kind in ('fwd', 'bwd'):
        p = prepare(cs, dt, kind)
        mine = []
        judge(p, fill(p, plain(p)), mine)
        _RATIOS.extend(mine)
        if dt == F32:
            worst = max(mine, key=lambda r: r[4])
            assert worst[4] <= RATIO_F32_MAX, f'the float32 statement reaches {worst[4]:.3f} of the bound ({worst[2]}): the f32 tolerances are too tight'


# ---- 3. the judge -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [F32, BF16], ids=SC.case_id)
def test_judge_notices_single_faults(dt):
    noticed = []

    def fails(p, after, what):
        with pytest.raises(AssertionError):
            judge(p, after)
            print(f'not noticed: {what}')
        noticed.append(what)

    def setup(name):
        cs = SC.case(name)
        pf, pb = prepare(cs, dt, 'fwd'), prepare(cs, dt, 'bwd')
        base = {'fwd': plain(pf), 'bwd': plain(pb)}
        judge(pf, fill(pf, base['fwd']))
        judge(pb, fill(pb, base['bwd']))
        return cs, pf, pb, base

    def faulted(p, base, fault=None, dp=None, only=None):
        """the passing result with the outputs of this call replaced by R64 evaluated with one fault"""
        R2 = SC.r64(p.cs, p.I, p.keep, fault, dp)
        v = dict(base[p.kind])
        v.update({n: R2[n] for n in (only or p.outs)})
        return fill(p, v)

    # ---- attention: shifted by 3 on a 16 x 16 map, three copies of the bias-table gradient
    cs, pf, pb, base = setup('a96_2_16_3')
    fails(pf, faulted(pf, base, 'swap_qk'), 'relative-position index with q and k swapped (forward)')
    fails(pb, faulted(pb, base, 'swap_qk', only=('dtable',)), 'relative-position index with q and k swapped (dtable)')
    fails(pf, faulted(pf, base, 'label', only=('y',)), 'one mask region mislabelled in the last window row')
    fails(pf, faulted(pf, base, 'roll_back', only=('y', 'a')), 'roll in the wrong direction on the way back')
    fails(pf, faulted(pf, base, 'head_dropped', only=('y',)), "one head slice's partial sum dropped")
    fails(pf, faulted(pf, base, 'eps', only=('rstd',)), 'eps left out of rstd (the save)')
    fails(pf, faulted(pf, base, 'eps', only=('y', 'ln')), 'eps left out of rstd (ln, y)')
    after = fill(pb, base['bwd'])
    _, offs, rows, width = pb.outs['dtable']
    after['dtable'][GUARD + offs[1]:GUARD + offs[1] + rows * width] = pb.start['dtable'][1].reshape(-1).float()
    fails(pb, after, 'one tparts copy lost')
    # ---- MLP: three samples of 80 rows, the sample boundaries inside 64-row blocks
    cs, pf, pb, base = setup('m96_3x80_p')
    fails(pf, faulted(pf, base, 'hidden_twice'), 'one hidden slice counted twice')
    rows = torch.arange(cs['M'])
    dp = SC.dp_rows(cs, pf.keep)
    dp_block = dp[(rows // 64 * 64)]                      # every row takes the factor of its 64-row block's first row
    assert not torch.equal(dp, dp_block)
    fails(pf, faulted(pf, base, dp=dp_block), 'DropPath keep of the neighbouring sample on a straddling block (y)')
    fails(pb, faulted(pb, base, dp=dp_block, only=('dx', 'dys')), 'DropPath keep of the neighbouring sample on a straddling block (dx, dys)')
    fails(pb, faulted(pb, base, 'eps', only=('ln',)), 'eps left out of rstd (MLP ln)')
    if dt == F32:
        fails(pb, faulted(pb, base, 'erf', only=('h',)), 'erf-form instead of tanh-form GELU')
    after = fill(pf, base['fwd'])
    after['y'][GUARD + (cs['M'] - 1) * cs['C']:GUARD + cs['M'] * cs['C']] = pattern(cs['C'], dt)
    fails(pf, after, 'last tail row unwritten')
    v = dict(base['bwd'])
    after = fill(pb, v)
    after['dgamma'][GUARD:GUARD + cs['C']] -= pb.start['dgamma'][0].reshape(-1).float()
    fails(pb, after, 'dgamma written instead of added')
    after = fill(pb, v)
    after['dbeta'][GUARD + cs['C'] + 5] = 0.0                  # the gap between two copies
    fails(pb, after, 'gap between the copies')
    assert len(noticed) >= (16 if dt == F32 else 15)


def test_layout_and_matrix():
    """16-byte alignment of every tensor, and the case matrix selects what the docstring table says (the thresholds of mlp_dispatch /
    attn_dispatch restated: a case that drifts off its path fails here, not silently)"""
    assert GUARD * 2 % 16 == 0
    for cs in SC.cases():
        assert cs['rps'] % 16 == 0 and (cs['C'] + SC.PSTRIDE_EXTRA) % 4 == 0
    M = {c['name']: c['M'] for c in SC.cases()}
    blocks = lambda n: (M[n] + 63) // 64
    assert blocks('m384_2048') == 32 and blocks('m384_2064') == 33 and blocks('m384_4096') == 64 and blocks('m384_4112') == 65
    assert M['m384_8176'] < 8192 <= M['m384_8272'] and M['m384_8272'] % 128 and M['m96_32848'] >= 32768 and M['m96_32848'] % 128
    assert M['m96_131072'] >= 4 * 32768 and M['m192_8192'] < 32768 <= M['m192_32848']
    U = {c['name']: c['units'] for c in SC.cases()}
    assert (U['a384_48w'], U['a384_49w'], U['a384_52w_p'], U['a192_255w'], U['a192_256w']) == (48, 49, 52, 255, 256)


def test_zz_report_plain_statement_ratios():
    """(runs last in this file) the largest ||err|| / bound of the plain statement per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(SC.report_lines(_RATIOS, 'swin plain')))
