"""The references, bounds and judge of _xattn_cases.py, checked without a GPU.

  1. R64 is autograd-consistent: on a cut-down block (Z = 1, two scenes of 4 tokens, one of them ALL masked) the directional derivatives of
     sum(y dy) by central differences in float64 agree with autograd for every leaf, the masked-logit construction included; and the
     hand-written backward of the twin, with the identity for a rounding, reproduces R64 and its autograd gradients on every case.
  2. A plain layer-by-layer statement passes the judge: torch float32, one weight set and one head at a time, F.softmax / F.layer_norm /
     F.elu and autograd; in the 16-bit rows every layer's output is stored in dt (q, the dropped-out P, O, v1, n1, the FFN1
     pre-activation, hd, the FFN2 output, u2, y) and the gradients stay float32 until they are outputs, i.e. it rounds at other places
     than the twin (which keeps v1, the pre-activation and u2 in f32 and rounds du2, dpre, dv1, dO, dS and dq on the way back).  Every case and dtype, forward and backward, with the ratios printed: the
     inputs and the factor 2 of the 16-bit bound are attainable by honest arithmetic.
  3. The judge is sensitive: nine single faults of a passing result, each must fail.
"""
import pytest
import torch
import torch.nn.functional as F

import _xattn_cases as XC
from _xattn_cases import CB, DTYPES, F1, F32, GRADS, HP, HS, NH, NKEY, O1, SCALE, judge, prepare

_RATIOS = []


# ---- 1. the references --------------------------------------------------------------------------------------------------------------------
def _small_inputs():
    cs = dict(name='small', Z=1, B=2, HW=4, zstride=XC.TIGHT, kvalid=('random', 'none'), p=0.25, rng=True)
    I = XC.make_inputs(cs, F32)
    return cs, I, XC._factors(cs, XC.cpu_masks(cs))


def test_r64_gradients_agree_with_finite_differences():
    cs, I, fac = _small_inputs()
    assert not bool(I['valid'][1].any()) and bool(I['valid'][0].any())
    D = XC._f64(I)
    for n in XC.LEAVES:
        D[n] = D[n].clone().requires_grad_(True)
    T = XC.forward_graph(D, fac)
    (T['y'] * D['dy']).sum().backward()
    frozen = T['logits'].detach()
    g = torch.Generator().manual_seed(5)
    h = 1e-6
    for n in XC.LEAVES:
        d = torch.randn(D[n].shape, generator=g, dtype=torch.float64)
        val = []
        for s in (h, -h):
            E = {k: v.detach() for k, v in D.items()}
            E[n] = E[n] + s * d
            val.append(float((XC.forward_graph(E, fac, linearised_at=frozen)['y'] * E['dy']).sum()))
        num, ana = (val[0] - val[1]) / (2 * h), float((D[n].grad * d).sum())
        # 1e-4: the -1e10 of the masked logits carries float64 rounding of 2e-6 into P; the differences themselves are good to ~1e-9
        assert abs(num - ana) <= 1e-4 * max(abs(ana), 1.0), (n, num, ana)
    # the all-masked scene does take part: its keys receive a gradient
    assert float(D['k'].grad[:, 1].abs().max()) > 0


@pytest.mark.parametrize('cs', XC.cases(), ids=lambda c: c['name'])
def test_twin_without_rounding_is_r64(cs):
    I, fac, R, _ = XC.references(cs, F32, XC.cpu_masks(cs), 'cpu')
    for saves in (None, {k: R[k] for k in ('sq', 'sv1', 'su2')}):
        T = XC.twin(I, fac, lambda t: t, saves)
        for n in XC.FWD_OUT + XC.BWD_OUT:
            assert float((T[n] - R[n]).abs().max()) <= 1e-11 * float(R[n].abs().max()), n


# ---- 2. a plain statement through the judge -----------------------------------------------------------------------------------------------
class _Store(torch.autograd.Function):
    """a layer boundary of a 16-bit chain: the layer's output is stored in dt (gradients pass in f32 and are rounded once, as outputs)"""
    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).float()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _swap(x, saved):
    """the saved value in place of x, x's place in the graph (x - x.detach() is exactly zero)"""
    return saved + (x - x.detach())


def plain(p):
    """name -> output of the call p describes, by the layer-by-layer float32 statement (backward: on the saves the call is handed)"""
    cs, dt, I = p.cs, p.dt, p.I
    Z, B, HW = cs['Z'], cs['B'], cs['HW']
    st = (lambda t: t) if dt == F32 else (lambda t: _Store.apply(t, dt))
    bwd = p.kind == 'bwd'
    sc = 1.0 / (1.0 - cs['p'])
    keep = None
    if p.fac is not None:
        keep = {k: (v != 0).float() for k, v in p.fac.items()}
    saved = {n: p.bufs[n].init[XC.GUARD:-XC.GUARD].float().reshape(Z, B, HW, -1) for n in ('sq', 'sv1', 'su2')} if bwd else None
    addend = torch.where(I['valid'], torch.tensor(0.0), torch.tensor(-10e9))[:, None, :]          # f32: logit + -1e10 is -1e10, the add's gradient 1
    names = XC.FWD_OUT + XC.BWD_OUT
    out = {n: [] for n in names}
    for z in range(Z):
        x, k, v = (I[n][z].float().requires_grad_(True) for n in ('query', 'k', 'v'))
        wq, wo, w1, w2 = (I[n][z].to(dt).float() for n in ('wq', 'wo', 'w1', 'w2'))          # the weights in the compute type
        bo, g1, be1, b1, b2, g2, be2 = (I[n][z].clone().requires_grad_(True) for n in ('bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2'))
        qs, os_ = [], []
        for h in range(NH):
            q = st(x @ wq[h])
            if bwd:
                q = _swap(q, saved['sq'][z, :, :, HP * h:HP * h + HS])
            q.retain_grad()
            kh, vh = k[:, :, HS * h:HS * (h + 1)], v[:, :, HS * h:HS * (h + 1)]
            P = F.softmax((q * SCALE) @ kh.transpose(1, 2) + addend, -1)
            if keep is not None:
                P = P * keep['a'][z, :, h] * sc
            P = st(P)
            qs.append(q)
            os_.append(st(P @ vh))
        v1 = st(torch.cat(os_, -1) @ wo.reshape(NH * HS, O1) + bo)
        if bwd:
            v1 = _swap(v1, saved['sv1'][z])
        v1.retain_grad()
        n1 = st(F.layer_norm(v1, (O1,), g1, be1, XC.LN_EPS))
        pre = st(n1 @ w1 + b1)
        pre.retain_grad()
        hd = F.elu(pre)
        if keep is not None:
            hd = hd * keep['1'][z].reshape(B, HW, F1) * sc
        hd = st(hd)
        t2 = st(hd @ w2 + b2)
        t2.retain_grad()
        u2 = st(t2 * keep['2'][z].reshape(B, HW, CB) * sc) if keep is not None else t2
        if bwd:
            u2 = _swap(u2, saved['su2'][z])
        y = st(F.layer_norm(u2, (CB,), g2, be2, XC.LN_EPS) + x)
        y.backward(I['dy'][z].float())
        pad = lambda ts: torch.cat([F.pad(t, (0, HP - HS)) for t in ts], -1)
        vals = dict(y=y, sq=pad(qs), so=pad(os_), sv1=v1, su2=u2, dquery=x.grad, dk=k.grad, dv=v.grad, hd=hd, dpre=pre.grad, du2=t2.grad, n1=n1,
                    dv1=v1.grad, dq=pad([q.grad for q in qs]), dg1=g1.grad, dbe1=be1.grad, dbo=bo.grad, dg2=g2.grad, dbe2=be2.grad)
        for n in names:
            out[n].append(vals[n].detach() + (I['start_' + n][z] if n in GRADS else 0.0))
    return {n: torch.stack(t) for n, t in out.items()}


def fill(p, values):
    """the flat buffers as a call that produced `values` (name -> tensor, any float type) would leave them"""
    after = {k: b.init.clone() for k, b in p.bufs.items()}
    for n, (bname, idx) in p.outs.items():
        after[bname][XC.GUARD + idx.reshape(-1)] = values[n].reshape(-1).to(after[bname].dtype)
    return after


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_plain_statement_passes_the_judge(dt):
    failed = []
    for cs in XC.cases():
        for kind in ('fwd', 'bwd'):
            p = prepare(cs, dt, kind)
            try:
                judge(p, fill(p, plain(p)), _RATIOS)
            except AssertionError as e:
                failed.append(f"{cs['name']} [{dt}]: {e}")
    assert not failed, f'{len(failed)} failed:\n' + '\n'.join(failed)


# ---- 3. the judge -------------------------------------------------------------------------------------------------------------------------
def _with(p, masks=None, **over):
    """R64 of p's call with some inputs replaced (a mutated computation)"""
    I = dict(p.I, **over)
    return XC.r64(I, XC._factors(p.cs, masks) if masks is not None else p.fac)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=str)
def test_judge_notices_single_faults(dt):
    cs = XC.case('z3_t3_p0.1')
    Z, B, HW = cs['Z'], cs['B'], cs['HW']
    masks = XC.cpu_masks(cs)
    pf, pb = prepare(cs, dt, 'fwd'), prepare(cs, dt, 'bwd')
    base = {'fwd': plain(pf), 'bwd': plain(pb)}
    judge(pf, fill(pf, base['fwd']))
    judge(pb, fill(pb, base['bwd']))
    valid = pf.I['valid']

    def fails(p, after, what):
        with pytest.raises(AssertionError):
            judge(p, after)
            print(f'not noticed: {what}')

    def mutated(p, **values):
        v = dict(base[p.kind])
        v.update(values)
        return fill(p, v)

    # two neighbouring token rows of y swapped
    y = base['fwd']['y'].clone()
    y[1, 2, [100, 101]] = y[1, 2, [101, 100]]
    fails(pf, mutated(pf, y=y), 'rows swapped')
    # one weight set's y computed with the previous set's g2
    g2 = pf.I['g2'].clone()
    g2[1] = g2[0]
    y = base['fwd']['y'].clone()
    y[1] = _with(pf, g2=g2)['y'][1]
    fails(pf, mutated(pf, y=y), "the neighbouring set's g2")
    # one masked key of scene 0 treated as valid
    v2 = valid.clone()
    dead = int((~valid[0]).nonzero()[0])
    v2[0, dead] = True
    R2 = _with(pf, valid=v2)
    fails(pf, mutated(pf, **{n: R2[n] for n in XC.FWD_OUT}), 'a masked key taken for valid (forward)')
    fails(pb, mutated(pb, **{n: _with(pb, valid=v2)[n] for n in ('dk', 'dv')}), 'a masked key taken for valid (dk, dv)')
    # the attention-dropout mask shifted by one draw
    m2 = dict(masks, a=masks['a'].reshape(-1).roll(1).reshape(masks['a'].shape))
    R2 = _with(pf, masks=m2)
    fails(pf, mutated(pf, **{n: R2[n] for n in XC.FWD_OUT}), 'mask shifted by one draw')
    # the mask laid out [Z,B,HW,3,64]
    m2 = dict(masks, a=masks['a'].reshape(Z, B, HW, NH, NKEY).permute(0, 1, 3, 2, 4).contiguous())
    R2 = _with(pf, masks=m2)
    fails(pf, mutated(pf, **{n: R2[n] for n in XC.FWD_OUT}), 'mask layout [Z,B,HW,3,64]')
    # one tile's share missing from dk (y's rows depend on k token by token: the share of a tile is dk of dy zeroed elsewhere)
    dy = torch.zeros_like(pb.I['dy'])
    dy[2, 0, 64:128] = pb.I['dy'][2, 0, 64:128]
    dk = base['bwd']['dk'].clone()
    dk[2, 0] -= _with(pb, dy=dy)['dk'][2, 0]
    fails(pb, mutated(pb, dk=dk), "a tile's share of dk")
    # one pad column of sq set to 1e-3
    sq = base['fwd']['sq'].clone()
    sq[0, 1, 7, HP + HS + 2] = 1e-3
    fails(pf, mutated(pf, sq=sq), 'pad column')
    # one guard element overwritten
    after = mutated(pf)
    after['su2'][XC.GUARD + pf.bufs['su2'].n] = 0.0
    fails(pf, after, 'guard behind su2')
    after = mutated(pb)
    after['grads'][XC.GUARD + XC.TIGHT + 3] = 0.0          # the gap between set 0 and set 1
    fails(pb, after, 'gap between sets')
    # one "+=" output missing its start value
    dg1 = base['bwd']['dg1'].clone()
    dg1[2] -= pb.I['start_dg1'][2]
    fails(pb, mutated(pb, dg1=dg1), 'start value of dg1')


def test_layout_is_aligned_and_cases_stay_small():
    for cs in XC.cases():
        assert cs['zstride'] % 4 == 0 and cs['zstride'] >= XC.TIGHT and cs['Z'] * cs['B'] * cs['HW'] <= 1728
    assert all(off % 4 == 0 for off, _ in XC.SETLAY.values()) and XC.GUARD % 4 == 0


def test_zz_report_plain_statement_ratios():
    """(runs last in this file) the largest ||err|| / bound of the plain statement per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(XC.report_lines(_RATIOS, 'xattn plain')))
