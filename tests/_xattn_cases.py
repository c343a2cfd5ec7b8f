"""Cases, flat-buffer layout, float64 references and the judge shared by test_xattn_abi_gpu.py (the kernels of csrc/xattn_fused.hip through
the C ABI) and test_xattn_ref.py (the references and the judge themselves, on the CPU).  Nothing here needs a GPU or the library.

A case is a dict (xcase).  prepare(cs, dt, kind) lays every tensor of one stj_xattn_fwd ('fwd') or stj_xattn_bwd ('bwd') call into flat CPU
allocations filled with the NaN pattern of test_gemm_gpu.PAT, GUARD elements in front and behind.  The f32 parameters of the Z weight sets
lie in ONE allocation as in the model's flat buffer (set z at + z * zstride, the gap behind a set where zstride exceeds the tight size
keeps the pattern), their gradients in a second one of the same layout in which only dg1, dbe1, dbo, dg2, dbe2 hold (non-zero) start
values.  Every f32 vector starts at a multiple of 4 elements of a 16-byte aligned base and zstride % 4 == 0: the kernels read them as float4.

R64 (reference): the block in float64 torch, gradients by autograd -- the expected value of every output.
Rdt (twin): the same block with a hand-written backward, rounding to dt where the kernels do.  With the identity for a rounding it must
    reproduce R64 and its autograd gradients (test_xattn_ref.py); with dt it only MEASURES how far honest 16-bit arithmetic lands from R64.
judge(): per output tensor and per row (a token, a key, one weight set's vector)  ||got[r] - R64[r]|| <= bound[r];
    f32     bound[r] = tol (max(||R64[r]||, rms_r ||R64[r]||) + ||start[r]||), tol 2e-5 forward / 2e-4 backward (test_xattn_gpu.py's f32 figures)
    16 bit  bound[r] = 2 max(e_twin[r], rms_r e_twin[r]) + the f32 bound,  e_twin[r] = ||Rdt[r] - R64[r]||
    (kernel and twin round at the same places but each may land on a neighbouring value: the triangle inequality), and everything that is
    no output element is bit-identical, no output element keeps the pattern, the 42..47 pad columns of sq / so / dq are exactly zero and
    so are the dk / dv rows of masked keys in scenes that have a valid key.
"""
import math

import torch
import torch.nn.functional as F

from test_gemm_gpu import GUARD, bits, draw, pattern
from test_ops_gpu import EPS_ELEM

F32 = torch.float32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CB, NH, HS, HP, O1, F1, NKEY, TOK = 384, 3, 42, 48, 128, 512, 64, 64
QS = NH * HP
SCALE = 42.0 ** -0.5
LN_EPS = 1e-3
TOL_FWD, TOL_BWD = 2e-5, 2e-4            # the project's f32 figures (test_xattn_gpu.py: tol_y, tol_g)
assert EPS_ELEM[F32] < TOL_FWD           # the f32 tolerances sit above the storage resolution the other ABI tests use

# one weight set in the flat parameter buffer: name -> (offset, shape); every offset is a multiple of 4 elements
_ORDER = (('wq', (NH, CB, HS)), ('wo', (NH, HS, O1)), ('bo', (O1,)), ('g1', (O1,)), ('be1', (O1,)), ('w1', (O1, F1)), ('b1', (F1,)),
          ('w2', (F1, CB)), ('b2', (CB,)), ('g2', (CB,)), ('be2', (CB,)))
SETLAY, TIGHT = {}, 0
for _n, _s in _ORDER:
    SETLAY[_n] = (TIGHT, _s)
    TIGHT += math.prod(_s)
    assert TIGHT % 4 == 0
GRADS = {'dg1': 'g1', 'dbe1': 'be1', 'dbo': 'bo', 'dg2': 'g2', 'dbe2': 'be2'}          # "+=" output -> its slot in the gradient buffer
FWD_OUT = ('y', 'sq', 'so', 'sv1', 'su2')
BWD_OUT = ('dquery', 'dk', 'dv', 'hd', 'dpre', 'du2', 'n1', 'dv1', 'dq') + tuple(GRADS)
WIDTH = dict(y=CB, sq=QS, so=QS, sv1=O1, su2=CB, dquery=CB, hd=F1, dpre=F1, du2=CB, n1=O1, dv1=O1, dq=QS, query=CB, dy=CB)


def xcase(name, Z, B, HW, zextra, kvalid, p, rng=True):
    """kvalid: None (NULL pointer) or one entry per scene: 'random' (key 0 valid), 'random0' (key 0 as drawn), 'none', 'one'"""
    assert HW % TOK == 0 and Z * B * HW <= 1728 and (kvalid is None or len(kvalid) == B)
    return dict(name=name, Z=Z, B=B, HW=HW, zstride=(TIGHT + 3) // 4 * 4 + zextra, kvalid=kvalid, p=p, rng=rng)


def cases():
    out = []
    for p in (0.0, 0.1):
        out.append(xcase(f'z8_p{p:g}', 8, 2, 64, 0, ('random', 'random'), p, rng=p > 0))
        out.append(xcase(f'z3_t3_p{p:g}', 3, 3, 192, 40, ('random', 'none', 'one'), p, rng=p > 0))
    out.append(xcase('z1_t5', 1, 1, 320, 0, None, 0.5))
    out.append(xcase('z5_p0', 5, 1, 64, 4, ('random0',), 0.0, rng=True))
    return out


def case(name):
    return {c['name']: c for c in cases()}[name]


def draw_shapes(cs):
    Z, B, HW = cs['Z'], cs['B'], cs['HW']
    return {'a': (Z, B, NH, HW, NKEY), '1': (Z, B * HW, F1), '2': (Z, B * HW, CB)}


def cpu_masks(cs, seed=99):
    """any fixed Bernoulli keep masks (the GPU tests hand in the ones stj_dropout_mask states)"""
    if not cs['p'] > 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(s, generator=g) >= cs['p']).to(torch.uint8) for k, s in draw_shapes(cs).items()}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(cs, dt):
    """name -> CPU tensor as stored: activations in dt, parameters and start values f32, valid bool [B,64].  Scales: every product's
    output has a spread of about 1 (softmax neither uniform nor one-hot, FFN1 pre-activations of both signs: asserted by prepare)."""
    Z, B, HW = cs['Z'], cs['B'], cs['HW']
    g = torch.Generator().manual_seed(1000 + 131 * Z + 17 * B + HW)
    d = lambda shape, scale=1.0, t=F32: draw(math.prod(shape), t, g, False, scale=scale).reshape(shape)
    I = dict(query=d((Z, B, HW, CB), t=dt), k=d((Z, B, NKEY, NH * HS), 3.0, dt), v=d((Z, B, NKEY, NH * HS), t=dt), dy=d((Z, B, HW, CB), t=dt))
    I.update(wq=d((Z, NH, CB, HS), 0.116), wo=d((Z, NH, HS, O1), 0.4), w1=d((Z, O1, F1), 0.12), w2=d((Z, F1, CB), 0.09))
    for n, w in (('bo', O1), ('be1', O1), ('b1', F1), ('b2', CB), ('be2', CB)):
        I[n] = d((Z, w), 0.5)
    for n, w in (('g1', O1), ('g2', CB)):
        I[n] = 1.0 + d((Z, w), 0.3)
    for n, src in GRADS.items():
        I['start_' + n] = d((Z, SETLAY[src][1][0]))
    valid = torch.ones(B, NKEY, dtype=torch.bool)
    for b, how in enumerate(cs['kvalid'] or ()):
        if how in ('random', 'random0'):
            valid[b] = torch.rand(NKEY, generator=g) < 0.7
            if how == 'random':
                valid[b, 0] = True
        elif how == 'none':
            valid[b] = False
        elif how == 'one':
            valid[b] = False
            valid[b, 37] = True
    I['valid'] = valid
    return I


def _factors(cs, masks):
    if masks is None:
        return None
    sc = 1.0 / (1.0 - cs['p'])
    return {k: masks[k].reshape(s).double() * sc for k, s in draw_shapes(cs).items()}


def _f64(I):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in I.items()}


def _ln_stats(x):
    m = x.mean(-1, keepdim=True)
    var = ((x - m) ** 2).mean(-1, keepdim=True)
    return m, 1.0 / torch.sqrt(var + LN_EPS)


def _heads(t):
    """[Z,B,N,3*42] -> [Z,B,3,N,42]"""
    Z, B, N, _ = t.shape
    return t.reshape(Z, B, N, NH, HS).permute(0, 1, 3, 2, 4)


def _pad144(t):
    """[Z,B,3,N,42] -> [Z,B,N,144] (head h at columns 48 h .. 48 h + 41, pads zero)"""
    Z, B, _, N, _ = t.shape
    return F.pad(t.permute(0, 1, 3, 2, 4), (0, HP - HS)).reshape(Z, B, N, QS)


def _unpad144(t):
    Z, B, N, _ = t.shape
    return t.reshape(Z, B, N, NH, HP)[..., :HS].permute(0, 1, 3, 2, 4)


def _v(t):
    """a per-set vector [Z, n] against [Z, B, N, n]"""
    return t[:, None, None, :]


# ------------------------------------------------------------------------------------------------------------------------------------------
# R64: the block in float64, gradients by autograd (header of include/strajnet_hip.h; trajNet.py:189-234,305-317)
# ------------------------------------------------------------------------------------------------------------------------------------------
def forward_graph(D, fac, linearised_at=None):
    """D: float64 tensors (leaves may require grad), fac: None or keep / (1 - p) factors in the draw shapes.  Returns every intermediate.
    linearised_at (finite-difference check only): logits frozen at the point of evaluation; an all-masked scene then takes
    softmax(logits - frozen) -- the function whose derivative `the gradient of the ADD stays 1` states (softmax ignores the common -1e10,
    and float64 cannot resolve a finite-difference step next to 1e10)."""
    T = {}
    T['q'] = torch.einsum('zbni,zhio->zbhno', D['query'], D['wq'])                       # unscaled q (what sq saves)
    kh, vh = _heads(D['k']), _heads(D['v'])
    logits = torch.einsum('zbhno,zbhmo->zbhnm', T['q'] * SCALE, kh)
    ok = D['valid'][None, :, None, None, :]
    # tfa: logits += -10e9 (1 - mask): the value is -1e10, the gradient of the ADD stays 1 (an all-masked scene has a uniform softmax and a non-zero dS)
    T['logits'] = logits
    if linearised_at is None:
        logits = logits + torch.where(ok, torch.zeros_like(logits), (-10e9 - logits).detach())
    else:
        none = ~D['valid'].any(1)[None, :, None, None, None]
        logits = torch.where(none, logits - linearised_at, logits + torch.where(ok, torch.zeros_like(logits), (-10e9 - logits).detach()))
    T['P'] = torch.softmax(logits, -1)
    Pd = T['P'] * fac['a'] if fac else T['P']
    T['o'] = torch.einsum('zbhnm,zbhmo->zbhno', Pd, vh)
    T['v1'] = torch.einsum('zbhno,zhoc->zbnc', T['o'], D['wo']) + _v(D['bo'])
    m, r = _ln_stats(T['v1'])
    T['n1'] = (T['v1'] - m) * r * _v(D['g1']) + _v(D['be1'])
    T['pre'] = torch.einsum('zbnc,zcf->zbnf', T['n1'], D['w1']) + _v(D['b1'])
    h = F.elu(T['pre'])
    T['hd'] = h * fac['1'].reshape(h.shape) if fac else h
    T['t2'] = torch.einsum('zbnf,zfc->zbnc', T['hd'], D['w2']) + _v(D['b2'])             # FFN2 output + b2 (du2 is its gradient)
    T['u2'] = T['t2'] * fac['2'].reshape(T['t2'].shape) if fac else T['t2']
    m, r = _ln_stats(T['u2'])
    T['y'] = (T['u2'] - m) * r * _v(D['g2']) + _v(D['be2']) + D['query']
    return T


LEAVES = ('query', 'k', 'v', 'wq', 'wo', 'w1', 'w2', 'bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2')


def r64(I, fac):
    """name -> float64 value of every output of both entry points (the five "+=" outputs include their start values)"""
    D = _f64(I)
    for n in LEAVES:
        D[n] = D[n].clone().requires_grad_(True)
    T = forward_graph(D, fac)
    for n in ('q', 'v1', 'pre', 't2'):
        T[n].retain_grad()
    (T['y'] * D['dy']).sum().backward()
    out = dict(y=T['y'], sq=_pad144(T['q']), so=_pad144(T['o']), sv1=T['v1'], su2=T['u2'], hd=T['hd'], n1=T['n1'], dquery=D['query'].grad,
               dk=D['k'].grad, dv=D['v'].grad, dq=_pad144(T['q'].grad), dv1=T['v1'].grad, dpre=T['pre'].grad, du2=T['t2'].grad)
    for n, src in GRADS.items():
        out[n] = D[src].grad + D['start_' + n]
    out = {k: v.detach() for k, v in out.items()}
    out['_P'], out['_pre'] = T['P'].detach(), T['pre'].detach()
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# Rdt: the same block with the kernels' rounding points and a hand-written backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def twin(I, fac, rd, saves=None):
    """The block as xattn_fwd_kernel / xattn_bwd_kernel evaluate it, in float64 with rd() applied once wherever the kernels turn an f32
    accumulator into the next product's operand (from_acc, frag_pack) or store it (st4, stf).  rd = identity gives R64 (checked on the CPU).
    Rounding points, forward:
      the packed weights Wq, Wo, W1, W2 (stj_xattn_pack; the f32 vectors bo .. be2 are read as they are);
      q, unscaled, before q k^T (the 42^-1/2 multiplies the f32 logits) and as the save sq;
      the dropped-out P before P v;  O before O Wo and as the save so;
      n1 = LN1(v1) before FFN1 (v1 itself stays f32 in the forward; the save sv1 is rounded);
      hd = dropout(elu(.)) before FFN2;  the save su2 (LN2 takes the f32 value);  y.
    Backward (reads the saves sq, sv1, su2 as stored -- `saves`, or this function's own forward when None):
      du2 (frag_pack: the stored tensor IS the operand of W2 du2);  n1 recomputed from the stored v1 (frag_pack);  hd (store only);
      dpre (from_acc, and the store);  dv1 (from_acc, and the store; dbo sums the f32 value);
      dO before dO v^T (HeadOp::from_acc) and in the dO tile of dv = Pd^T dO;
      Pd and dS in their LDS tiles (dk = dS^T q, dv = Pd^T dO) and dS before dq = dS k (from_acc);
      dq (from_acc before Wq dq, and the store);  dquery, dk, dv (the f32 per-tile partial sums are not rounded).
    The five LayerNorm / bias gradient sums stay f32 throughout."""
    D = _f64(I)
    wq, wo, w1, w2 = rd(D['wq']), rd(D['wo']), rd(D['w1']), rd(D['w2'])
    kh, vh = _heads(D['k']), _heads(D['v'])
    ok = D['valid'][None, :, None, None, :]
    fa = fac['a'] if fac else 1.0

    def softmax_of(q):
        logits = torch.einsum('zbhno,zbhmo->zbhnm', q, kh) * SCALE
        return torch.softmax(torch.where(ok, logits, torch.full_like(logits, -10e9)), -1)

    # forward
    q = rd(torch.einsum('zbni,zhio->zbhno', D['query'], wq))
    o = rd(torch.einsum('zbhnm,zbhmo->zbhno', rd(softmax_of(q) * fa), vh))
    v1 = torch.einsum('zbhno,zhoc->zbnc', o, wo) + _v(D['bo'])
    f1 = fac['1'].reshape(v1.shape[:3] + (F1,)) if fac else 1.0
    f2 = fac['2'].reshape(v1.shape[:3] + (CB,)) if fac else 1.0
    m, r = _ln_stats(v1)
    n1f = rd((v1 - m) * r * _v(D['g1']) + _v(D['be1']))
    hdf = rd(F.elu(torch.einsum('zbnc,zcf->zbnf', n1f, w1) + _v(D['b1'])) * f1)
    u2 = (torch.einsum('zbnf,zfc->zbnc', hdf, w2) + _v(D['b2'])) * f2
    m, r = _ln_stats(u2)
    out = dict(y=rd((u2 - m) * r * _v(D['g2']) + _v(D['be2']) + D['query']), sq=_pad144(q), so=_pad144(o), sv1=rd(v1), su2=rd(u2))
    # backward
    S = {k: out[k] for k in ('sq', 'sv1', 'su2')} if saves is None else {k: v.double() for k, v in saves.items()}
    dy = D['dy']
    m, r = _ln_stats(S['su2'])
    xh = (S['su2'] - m) * r
    a = dy * _v(D['g2'])
    du2 = rd(r * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True)) * f2)
    out.update(du2=du2, dg2=(dy * xh).sum((1, 2)), dbe2=dy.sum((1, 2)))
    m1, r1 = _ln_stats(S['sv1'])
    xh1 = (S['sv1'] - m1) * r1
    n1 = rd(xh1 * _v(D['g1']) + _v(D['be1']))
    pre = torch.einsum('zbnc,zcf->zbnf', n1, w1) + _v(D['b1'])
    h = F.elu(pre)
    dhd = torch.einsum('zbnc,zfc->zbnf', du2, w2)
    dpre = rd(dhd * f1 * torch.where(pre > 0, torch.ones_like(h), h + 1.0))
    out.update(n1=n1, hd=rd(h * f1), dpre=dpre)
    dn1 = torch.einsum('zbnf,zcf->zbnc', dpre, w1)
    a = dn1 * _v(D['g1'])
    dv1f = r1 * (a - a.mean(-1, keepdim=True) - xh1 * (a * xh1).mean(-1, keepdim=True))
    dv1 = rd(dv1f)
    out.update(dg1=(dn1 * xh1).sum((1, 2)), dbe1=dn1.sum((1, 2)), dbo=dv1f.sum((1, 2)), dv1=dv1)
    dO = rd(torch.einsum('zbnc,zhoc->zbhno', dv1, wo))
    qs = _unpad144(S['sq'])
    P = softmax_of(qs)
    dP = torch.einsum('zbhno,zbhmo->zbhnm', dO, vh) * fa
    dS = rd(P * (dP - (P * dP).sum(-1, keepdim=True)) * SCALE)
    Pd = rd(P * fa)
    dq = rd(torch.einsum('zbhnm,zbhmo->zbhno', dS, kh))
    unheads = lambda t: t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], NKEY, NH * HS)
    out.update(dq=_pad144(dq), dk=rd(unheads(torch.einsum('zbhnm,zbhno->zbhmo', dS, qs))), dv=rd(unheads(torch.einsum('zbhnm,zbhno->zbhmo', Pd, dO))),
               dquery=rd(dy + torch.einsum('zbhno,zhio->zbni', dq, wq)))
    for n in GRADS:
        out[n] = out[n] + D['start_' + n]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# One call: buffers, reference, bounds
# ------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """one flat allocation: pattern everywhere, `values` at flat positions `idx` (relative to base = GUARD)"""
    def __init__(self, n, dt, scratch=False):
        self.init, self.base, self.n, self.scratch = pattern(GUARD + n + GUARD, dt), GUARD, n, scratch
        self.out = torch.zeros(GUARD + n + GUARD, dtype=torch.bool)          # elements this call may write

    def put(self, idx, values):
        self.init[GUARD + idx.reshape(-1)] = values.reshape(-1).to(self.init.dtype)


class Prep:
    pass


def set_index(cs, name):
    """flat positions [Z, numel] of parameter `name` of every set in the parameter (or gradient) allocation"""
    off, shape = SETLAY[name]
    return torch.arange(cs['Z'])[:, None] * cs['zstride'] + off + torch.arange(math.prod(shape))[None, :]


_REF = {}


def references(cs, dt, masks, tag):
    """(inputs, R64, Rdt on the reference's saves) of one case and dtype, computed once per process and left unchanged"""
    key = (cs['name'], dt, tag)
    if key not in _REF:
        I = make_inputs(cs, dt)
        fac = _factors(cs, masks)
        R = r64(I, fac)
        # the inputs exercise the block: a softmax that is neither uniform nor one-hot, ELU on both branches
        many = I['valid'].sum(1) > 1
        if bool(many.any()):
            peak = float(R['_P'][:, many].max(-1).values.mean())
            assert 0.1 <= peak <= 0.7, f'{cs["name"]}: mean max_key P = {peak:.3f}: the attention is uniform or one-hot'
        pos = float((R['_pre'] > 0).double().mean())
        assert 0.2 <= pos <= 0.8, f'{cs["name"]}: {pos:.2f} of the FFN1 pre-activations are positive'
        tw = None
        if dt != F32:
            rd = lambda t: t.to(dt).double()
            tw = twin(I, fac, rd, {k: R[k].to(dt) for k in ('sq', 'sv1', 'su2')})
        _REF[key] = (I, fac, R, tw)
    return _REF[key]


def _rows(t):
    """the judge's row view: a token, a key, or one weight set's vector"""
    return t.reshape(-1, t.shape[-1])


def _row_bound(ref, tol, start=None):
    n = _rows(ref).norm(dim=1)
    b = torch.maximum(n, (n ** 2).mean().sqrt())
    if start is not None:
        b = b + start.norm(dim=1)
    return tol * b


def prepare(cs, dt, kind, masks=None, tag='cpu', with_saves=True, saves_from=None):
    """kind 'fwd' / 'bwd'.  masks: the keep masks of the three sites (draw shapes) when cs['p'] > 0; default: cpu_masks(cs).
    with_saves False: the inference form of the forward (sq .. su2 NULL).  saves_from: dict sq, sv1, su2 (dt tensors) the backward is
    handed instead of the reference's (forward into backward); the twin is then evaluated end to end."""
    assert kind in ('fwd', 'bwd')
    if cs['p'] > 0 and masks is None:
        masks, tag = cpu_masks(cs), 'cpu'
    I, fac, R, tw = references(cs, dt, masks if cs['p'] > 0 else None, tag)
    Z, B, HW = cs['Z'], cs['B'], cs['HW']
    rows = Z * B * HW
    p = Prep()
    p.cs, p.dt, p.kind, p.I, p.fac, p.R, p.bufs, p.outs, p.with_saves = cs, dt, kind, I, fac, R, {}, {}, with_saves
    if dt != F32 and saves_from is not None:
        key = (cs['name'], dt, tag, 'e2e')
        if key not in _REF:
            _REF[key] = twin(I, fac, lambda t: t.to(dt).double())
        tw = _REF[key]
    p.tw = tw

    def tensor(name, shape, t, values=None, out=False, scratch=False):
        n = math.prod(shape)
        b = p.bufs[name] = Buf(n, t, scratch)
        if values is not None:
            b.put(torch.arange(n), values)
        if out:
            b.out[GUARD:GUARD + n] = True
            p.outs[name] = (name, torch.arange(n).reshape(-1, shape[-1]))

    for n in ('query', 'k', 'v'):
        tensor(n, I[n].shape, dt, I[n])
    if cs['kvalid'] is not None:
        tensor('kvalid', (B, NKEY), torch.int32, I['valid'].to(torch.int32))
    par = p.bufs['params'] = Buf((Z - 1) * cs['zstride'] + TIGHT, F32)
    for n in SETLAY:
        par.put(set_index(cs, n), I[n])
    if kind == 'fwd':
        for n in FWD_OUT if with_saves else ('y',):
            tensor(n, (Z, B, HW, WIDTH[n]), dt, out=True)
    else:
        S = saves_from if saves_from is not None else {k: R[k].to(dt) for k in ('sq', 'sv1', 'su2')}
        tensor('dy', I['dy'].shape, dt, I['dy'])
        for n in ('sq', 'sv1', 'su2'):
            tensor(n, (Z, B, HW, WIDTH[n]), dt, S[n])
        for n in ('dquery', 'hd', 'dpre', 'du2', 'n1', 'dv1', 'dq'):
            tensor(n, (Z, B, HW, WIDTH[n]), dt, out=True)
        for n in ('dk', 'dv'):
            tensor(n, (Z, B, NKEY, NH * HS), dt, out=True)
        for n in ('dkp', 'dvp'):
            tensor(n, (Z * B * (HW // TOK) * NKEY * QS,), F32, scratch=True)
        gr = p.bufs['grads'] = Buf((Z - 1) * cs['zstride'] + TIGHT, F32)
        for n, src in GRADS.items():
            idx = set_index(cs, src)
            gr.put(idx, I['start_' + n])
            gr.out[GUARD + idx.reshape(-1)] = True
            p.outs[n] = ('grads', idx)
    # bounds
    p.bound = {}
    for n in p.outs:
        f32b = _row_bound(R[n], TOL_FWD if kind == 'fwd' else TOL_BWD, I['start_' + n].double() if n in GRADS else None)
        if dt == F32:
            p.bound[n] = f32b
        else:
            e = _rows(tw[n] - R[n]).norm(dim=1)
            p.bound[n] = 2.0 * torch.maximum(e, (e ** 2).mean().sqrt()) + f32b
    return p


def logical(p, after, name):
    bname, idx = p.outs[name]
    return after[bname][GUARD + idx.reshape(-1)].reshape(idx.shape)


def judge(p, after, ratios=None, label=''):
    """after: name -> the flat CPU buffer as the call left it.  Raises AssertionError; appends (kind, dtype, output, case, largest e / bound)."""
    cs = p.cs
    label = f"{cs['name']} {p.kind}{'' if p.with_saves else ' (no saves)'}{label}"
    for name, b in p.bufs.items():
        keep = ~b.out
        if b.scratch:
            keep[GUARD:GUARD + b.n] = False
        bad = (bits(after[name])[keep] != bits(b.init)[keep]).nonzero()
        assert bad.numel() == 0, f'{label}: {bad.numel()} elements of {name} outside the outputs changed, first at flat index {int(keep.nonzero()[bad[0, 0]]) - GUARD}'
    pat = int(bits(pattern(1, p.dt))[0])
    for name in p.outs:
        raw = logical(p, after, name)
        left = bits(raw) == (pat if raw.dtype == p.dt else int(bits(pattern(1, F32))[0]))
        assert not bool(left.any()), f'{label}: {int(left.sum())} elements of {name} still hold the fill pattern, first at {tuple(left.nonzero()[0].tolist())}'
        got, ref = raw.double(), _rows(p.R[name])
        err = (got - ref).norm(dim=1)
        ok = err <= p.bound[name]            # False for NaN
        ratio = float((err / (p.bound[name] + 1e-300)).nan_to_num(nan=float('inf')).max())
        if ratios is not None:
            ratios.append((p.kind, str(p.dt), name, cs['name'], ratio))
        assert bool(ok.all()), (f'{label}: {name}: {int((~ok).sum())} of {ok.numel()} rows over their bound, largest ||err|| / bound = {ratio:.3e}, '
                                f'first row {int((~ok).nonzero()[0])}')
        if name in ('sq', 'so', 'dq'):
            pads = got.reshape(-1, NH, HP)[:, :, HS:]
            assert not bool((pads != 0).any()), f'{label}: {int((pads != 0).sum())} pad elements (columns 42..47 of a head) of {name} are not zero'
        if name in ('dk', 'dv'):
            valid = p.I['valid']
            dead = (~valid & (valid.sum(1, keepdim=True) > 0))[None].expand(cs['Z'], -1, -1).reshape(-1)
            nz = (got[dead] != 0).any(1)
            assert not bool(nz.any()), f'{label}: {int(nz.sum())} rows of {name} that belong to masked keys are not zero'


def report_lines(ratios, title):
    best = {}
    for kind, dt, name, cname, r in ratios:
        k = (kind, dt, name)
        if k not in best or r > best[k][0]:
            best[k] = (r, cname)
    return [f'{title} {kind:3s} {dt:15s} {name:7s} largest ||err|| / bound {r:.3e} ({cname})' for (kind, dt, name), (r, cname) in sorted(best.items())]
