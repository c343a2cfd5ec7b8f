"""Cases, flat-buffer layout, float64 references and the judge shared by test_agent_abi_gpu.py (the kernels of csrc/agent_fused.hip through
the C ABI) and test_agent_ref.py (the references and the judge themselves, on the CPU).  Nothing here needs a GPU or the library.

Two blocks: the TrajEncoder ('enc': stj_agent_enc_fwd / _bwd, trajNet.py:29-48) and the interaction block ('int': stj_agent_int_fwd / _bwd,
trajNet.py:65-87,125-187).  prepare(cs, dt, kind) lays every tensor of one call ('enc_fwd', 'enc_bwd', 'int_fwd', 'int_bwd') into flat CPU
allocations filled with the NaN pattern of test_gemm_gpu.PAT, GUARD elements in front and behind.  The f32 masters of all 28 parameters lie
in ONE allocation ('params'), each at a multiple of 4 elements of a 16-byte aligned base; the "+=" outputs lie in a second one of the same
layout ('grads') and start from non-zero values.  The natural-layout kernels the backward reads lie in 'wnat' (dt), same offsets.

R64 (reference): every stage in float64 torch, gradients by autograd.  The max-pool takes the maximum; its tie set is
    {t : out[t] >= max - 1e-9 max|out|} (immune to BLAS noise), or the tie set handed in, and its gradient is dy / |tie set| on the tie set
    (the rule of tf.reduce_max).  Masked logits are -1e10 with the gradient of the ADD kept (oracle/torch_ref._mha).  Keep masks are inputs.
Rdt (twin): the same stages with a hand-written backward, rounding to dt where the kernels do (enc_forward / int_forward: every rd(); the
    backward reads the saves as stored).  With the identity for rd it reproduces R64 (test_agent_ref.py); with dt it MEASURES how far honest
    16-bit arithmetic lands from R64.
judge(): per output tensor and per row (a token, an agent, a step, a parameter row)  ||got[r] - R64[r]|| <= bound[r];
    f32     bound[r] = tol (max(||R64[r]||, rms_r ||R64[r]||) + ||start[r]||), tol 2e-5 forward / 3e-4 backward (test_agent_fused_gpu.py's figures)
    16 bit  bound[r] = 2 max(e_twin[r], rms_r e_twin[r]) + the f32 bound,  e_twin[r] = ||Rdt[r] - R64[r]||
    slab workspaces (ws_v1, ws_u2, ws_dn1, d_enc) are judged as the sum of their slabs; cmi is judged exactly; every element that is no
    output is bit-identical and no output element keeps the pattern.
    s_pmask: no bit >= 11, at least one bit, and the R64 pre-pool value of every set step lies within
    2 (largest |twin - R64| of that agent's pre-pool block; f32: 0) + 2e-5 |R64 maximum| of the R64 maximum; where float64 has a tie (two and
    more steps: rows that are bitwise equal in any arithmetic) its steps are marked all or none, and in f32 the word equals float64's tie set.
"""
import math

import torch
import torch.nn.functional as F

from test_gemm_gpu import GUARD, bits, draw, pattern

F32, F64 = torch.float32, torch.float64
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT16 = [torch.bfloat16, torch.float16]
TN, NF, EH, ED, EO, CB, IH, IDH, FF, NA = 11, 64, 4, 64, 320, 384, 6, 64, 1536, 64
LN_EPS = 1e-3
TOL_FWD, TOL_BWD = 2e-5, 3e-4            # the project's f32 figures for this branch (test_agent_fused_gpu.py: tol_y, tol_g)
TIE_REL = 1e-9

# the parameters: name -> (shape, draw scale, 'w' | 'g' (1 + draw) ); every product's output has a spread of about 1
_PORDER = (('wn', (5, NF), .25, 'w'), ('bn', (NF,), .3, 'w'), ('wv3', (3, NF), .5, 'w'), ('e_wq', (EH, NF, ED), .3, 'w'), ('e_wk', (EH, NF, ED), .3, 'w'),
           ('e_wv', (EH, NF, ED), .2, 'w'), ('e_wo', (EH, ED, EO), .15, 'w'), ('e_bo', (EO,), .3, 'w'), ('e_ws', (CB, CB), .06, 'w'), ('e_bs', (CB,), .3, 'w'),
           ('seg', (2, CB), .5, 'w'), ('i_wq', (IH, CB, IDH), .12, 'w'), ('i_wk', (IH, CB, IDH), .12, 'w'), ('i_wv', (IH, CB, IDH), .06, 'w'),
           ('i_wo', (IH, IDH, CB), .3, 'w'), ('i_bo', (CB,), .3, 'w'), ('g1', (CB,), .3, 'g'), ('be1', (CB,), .3, 'w'), ('i_w1', (CB, FF), .08, 'w'),
           ('b1', (FF,), .3, 'w'), ('i_w2', (FF, CB), .06, 'w'), ('b2', (CB,), .3, 'w'), ('g2', (CB,), .3, 'g'), ('be2', (CB,), .3, 'w'),
           ('g_obs', (CB,), .3, 'g'), ('b_obs', (CB,), .3, 'w'), ('g_occ', (CB,), .3, 'g'), ('b_occ', (CB,), .3, 'w'))
LAY, PTOTAL = {}, 0
for _n, _s, _, _ in _PORDER:
    LAY[_n] = (PTOTAL, _s)
    PTOTAL += math.prod(_s)
    assert PTOTAL % 4 == 0                # every f32 vector 16-byte aligned: the kernels read bo, bs, b1 as float4
PACK_KEYS = ('e_wq', 'e_wk', 'e_wv', 'e_wo', 'e_ws', 'i_wq', 'i_wk', 'i_wv', 'i_wo', 'i_w1', 'i_w2')       # the order of stj_agent_weights
ENC_GRADS = {'dwn': 'wn', 'dbn': 'bn', 'dwv3': 'wv3'}                                                     # "+=" output -> its slot
INT_GRADS = {'dseg': 'seg', 'dg1': 'g1', 'dbe1': 'be1', 'dg2': 'g2', 'dbe2': 'be2', 'dg_obs': 'g_obs', 'db_obs': 'b_obs', 'dg_occ': 'g_occ', 'db_occ': 'b_occ'}
ENC_SAVES = ('s_nodes', 's_qkv', 's_att', 's_pmask', 's_cat')
INT_SAVES = ('s_concat', 's_qin', 's_q', 's_k', 's_v', 's_att', 's_v1', 's_n1', 's_h', 's_u2', 's_out')
INT_DY = ('dq', 'dk', 'dv', 'dv1', 'dpre1', 'dz2')
SLABS = {'ws_v1': IH, 'ws_u2': FF // CB, 'ws_dn1': FF // CB, 'd_enc': 1 + IH}
# name in oracle/torch_ref._traj's parameter dict
TRAJ_NAMES = dict(wn='traj_net/traj_encoder/node_feature/kernel', bn='traj_net/traj_encoder/node_feature/bias', wv3='traj_net/traj_encoder/vector_feature/kernel',
                  e_wq='traj_net/traj_encoder/node_attention/query_kernel', e_wk='traj_net/traj_encoder/node_attention/key_kernel',
                  e_wv='traj_net/traj_encoder/node_attention/value_kernel', e_wo='traj_net/traj_encoder/node_attention/projection_kernel',
                  e_bo='traj_net/traj_encoder/node_attention/projection_bias', e_ws='traj_net/traj_encoder/sublayer/kernel', e_bs='traj_net/traj_encoder/sublayer/bias',
                  seg='traj_net/seg_embed/kernel', i_wq='traj_net/cross_attention/mha/query_kernel', i_wk='traj_net/cross_attention/mha/key_kernel',
                  i_wv='traj_net/cross_attention/mha/value_kernel', i_wo='traj_net/cross_attention/mha/projection_kernel',
                  i_bo='traj_net/cross_attention/mha/projection_bias', g1='traj_net/cross_attention/norm1/gamma', be1='traj_net/cross_attention/norm1/beta',
                  i_w1='traj_net/cross_attention/FFN1/kernel', b1='traj_net/cross_attention/FFN1/bias', i_w2='traj_net/cross_attention/FFN2/kernel',
                  b2='traj_net/cross_attention/FFN2/bias', g2='traj_net/cross_attention/norm2/gamma', be2='traj_net/cross_attention/norm2/beta',
                  g_obs='traj_net/obs_norm/gamma', b_obs='traj_net/obs_norm/beta', g_occ='traj_net/occ_norm/gamma', b_occ='traj_net/occ_norm/beta')

# kinds of track: fully valid; one / two / three invalid steps (x == 0; two and more: the invalid query rows attend uniformly and tie in front
# of the max-pool); an all-zero padded agent (all 11 steps tie); step 0 invalid with its type one-hot in place; one x = -0.0 (invalid);
# one x = 2^-26 (valid: the RAW float32 value counts, although it rounds to 0 in fp16); x = 2^-26 as the ONLY valid step (cmi = 1)
KINDS = ('valid', 'one', 'two', 'pad', 'step0', 'negzero', 'tiny', 'three', 'tinyonly')
TIE_FREE = ('valid', 'one', 'step0', 'negzero', 'tiny')


def ecase(name, B, n_obs, n_occ, p, shift=0, empty0=False, kinds=KINDS):
    assert (n_obs + n_occ) % 2 == 0 and B <= 3
    return dict(name=name, block='enc', B=B, n_obs=n_obs, n_occ=n_occ, A=n_obs + n_occ, p=p, shift=shift, empty0=empty0, kinds=kinds)


def icase(name, B, n_obs, p, cm, A=NA):
    """cm: one entry per scene: 'random' (70 % of the agents valid), 'all', 'none', 'one' (a single valid agent)"""
    assert len(cm) == B and B <= 3
    return dict(name=name, block='int', B=B, n_obs=n_obs, n_occ=A - n_obs, A=A, p=p, cm=cm)


def enc_cases():
    return [ecase('e1_1_1', 1, 1, 1, 0.0, shift=6),                       # one 16-bit workgroup holds an obs and an occ track
            ecase('e2_3_5_p0', 2, 3, 5, 0.0), ecase('e2_3_5_p0.1', 2, 3, 5, 0.1),      # odd n_obs: tiles straddle the segment boundary
            ecase('e1_0_2', 1, 0, 2, 0.0, shift=3), ecase('e1_2_0', 1, 2, 0, 0.1, shift=1),      # an empty side
            ecase('e3_48_16_p0', 3, 48, 16, 0.0, empty0=True), ecase('e3_48_16_p0.1', 3, 48, 16, 0.1, empty0=True)]


def int_cases():
    return [icase('i48_p0', 1, 48, 0.0, ('random',)), icase('i37_p0', 3, 37, 0.0, ('random', 'none', 'one')),
            icase('i37_p0.1', 3, 37, 0.1, ('random', 'none', 'one')), icase('i0_p0.1', 1, 0, 0.1, ('random',)), icase('i64_p0', 1, 64, 0.0, ('all',))]


def tie_free_cases():
    """whole-branch cases without max-pool ties, for the cross-check against oracle.torch_ref._traj"""
    return [ecase('tf2_3_5', 2, 3, 5, 0.1, kinds=TIE_FREE), ecase('tf1_37_27', 1, 37, 27, 0.1, kinds=TIE_FREE)]


def case(name):
    return {c['name']: c for c in enc_cases() + int_cases() + tie_free_cases()}[name]


def draw_shapes(cs):
    N = cs['B'] * cs['A']
    if cs['block'] == 'enc':
        return {'e': (N, EH, TN, TN)}
    return {'a': (cs['B'], IH, cs['A'], cs['A']), '1': (N, FF), '2': (N, CB)}


def cpu_masks(cs, seed=99, block=None):
    """any fixed Bernoulli keep masks (the GPU tests hand in the ones stj_dropout_mask states)"""
    if not cs['p'] > 0:
        return None
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(s, generator=g) >= cs['p']).to(torch.uint8) for k, s in draw_shapes(dict(cs, block=block or cs['block'])).items()}


def _factors(cs, masks):
    if masks is None:
        return None
    return {k: masks[k].double() / (1.0 - cs['p']) for k in masks}


# ------------------------------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------------------------------
_PARAMS = []


def params():
    """name -> f32 master, the same for every case"""
    if not _PARAMS:
        g = torch.Generator().manual_seed(4242)
        P = {}
        for n, s, sc, how in _PORDER:
            t = draw(math.prod(s), F32, g, False, scale=sc).reshape(s)
            P[n] = 1.0 + t if how == 'g' else t
        for n in list(ENC_GRADS) + list(INT_GRADS):
            src = {**ENC_GRADS, **INT_GRADS}[n]
            P['start_' + n] = draw(math.prod(LAY[src][1]), F32, g, False).reshape(LAY[src][1])
        _PARAMS.append(P)
    return _PARAMS[0]


def make_tracks(cs):
    """obs [B,n_obs,11,8], occ [B,n_occ,11,8] f32 and the kind of every agent [B][A]"""
    B, A = cs['B'], cs['A']
    g = torch.Generator().manual_seed(77 + 1000 * B + 10 * cs['n_obs'] + cs['n_occ'] + cs['shift'])
    a = torch.zeros(B, A, TN, 8)
    a[..., 0:2] = (torch.rand((B, A, TN, 2), generator=g) * 3.5 + 0.5) * (torch.randint(0, 2, (B, A, TN, 2), generator=g) * 2 - 1)
    a[..., 2:4] = torch.randn((B, A, TN, 2), generator=g)
    a[..., 4] = torch.rand((B, A, TN), generator=g) * 6.283 - 3.1416
    ty = torch.randint(0, 3, (B, A), generator=g)
    for k in range(3):
        a[..., 5 + k] = (ty == k).float()[..., None]
    kinds = [[cs['kinds'][(b * A + i + cs['shift']) % len(cs['kinds'])] for i in range(A)] for b in range(B)]
    for b in range(B):
        for i in range(A):
            kd = kinds[b][i]
            steps = torch.randperm(TN, generator=g).tolist()
            if kd in ('one', 'two', 'three'):
                for t in steps[:{'one': 1, 'two': 2, 'three': 3}[kd]]:
                    a[b, i, t, 0] = 0.0
            elif kd == 'pad':
                a[b, i] = 0.0
            elif kd == 'step0':
                a[b, i, 0, 0] = 0.0
            elif kd == 'negzero':
                a[b, i, steps[0], 0] = -0.0
            elif kd == 'tiny':
                a[b, i, steps[0], 0] = 2.0 ** -26
            elif kd == 'tinyonly':
                a[b, i, :, 0] = 0.0
                a[b, i, steps[0], 0] = 2.0 ** -26
    if cs['empty0']:
        a[0] = 0.0
        kinds[0] = ['pad'] * A
    return a[:, :cs['n_obs']].contiguous(), a[:, cs['n_obs']:].contiguous(), kinds


def make_inputs(cs, dt):
    """name -> CPU tensor as stored.  enc block: obs, occ (f32), d_enc (dt) and seven f32 slabs whose sum is another gradient of enc.
    int block: enc (dt), cmi (int32), dkey (dt).  Parameters: params()."""
    B, A = cs['B'], cs['A']
    N = B * A
    g = torch.Generator().manual_seed(500 + 31 * B + 7 * cs['n_obs'] + (1 if cs['block'] == 'int' else 0))
    d = lambda shape, scale=1.0, t=F32: draw(math.prod(shape), t, g, False, scale=scale).reshape(shape)
    I = {}
    if cs['block'] == 'enc':
        I['obs'], I['occ'], I['kinds'] = make_tracks(cs)
        I['d_enc'] = d((N, CB), t=dt)
        I['d_enc_slabs'] = d((7, N, CB), 0.4)
    else:
        I['enc'] = d((B, A, CB), t=dt)
        cm = torch.zeros(B, A, dtype=torch.bool)
        for b, how in enumerate(cs['cm']):
            if how == 'random':
                cm[b] = torch.rand(A, generator=g) < 0.7
                cm[b, 0], cm[b, A - 1] = True, False
            elif how == 'all':
                cm[b] = True
            elif how == 'one':
                cm[b, 41 % A] = True
        I['cm'] = cm
        I['dkey'] = d((B, A, CB), t=dt)
    return I


def _f64(D):
    return {k: v.double() for k, v in D.items() if torch.is_tensor(v) and v.is_floating_point()}


def ident(t):
    return t


def rounder(dt):
    return lambda t: t.to(dt).double()


def _ln_stats(x):
    m = x.mean(-1, keepdim=True)
    return m, 1.0 / torch.sqrt(((x - m) ** 2).mean(-1, keepdim=True) + LN_EPS)


def _ln_bwd(xh, t, rs):
    return rs * (t - t.mean(-1, keepdim=True) - xh * (t * xh).mean(-1, keepdim=True))


def _masked(lg, ok):
    """tfa: logits += -10e9 (1 - mask) in f32: the value is exactly -1e10, the gradient of the ADD stays 1 (an all-masked row has a uniform
    softmax and a non-zero dS)"""
    return torch.where(ok, lg, lg - lg.detach() - 10e9)


# ------------------------------------------------------------------------------------------------------------------------------------------
# TrajEncoder
# ------------------------------------------------------------------------------------------------------------------------------------------
def tracks_of(I):
    """[N,11,8] float64, agents in the kernels' order (scene by scene, obs first)"""
    x = torch.cat([I['obs'], I['occ']], 1).double()
    return x.reshape(-1, TN, 8)


def enc_forward(D, X, fe, rd, tie=None, tie_rel=TIE_REL):
    """agent_enc_fwd_kernel stage by stage.  D: float64 parameters, X: raw tracks [N,11,8], fe: None or keep / (1 - p) [N,4,11,11].
    rd(): once wherever the kernel stores to a dt tile or turns an accumulator into the next product's operand:
      the track and the three small kernels Wn, Wv3 (read as f32 masters, rounded in the loop), the packed kernels;
      nodes;  q | k | v;  the probabilities, and once more after the dropout factor (Ch::from_acc);  att;  out = att Wo + bo BEFORE the pool;
      vector;  enc.  bn, bo, bs are added in f32.  Step validity is the RAW x != 0.
    tie: bool [N,11,320] handed in, else {t: out[t] >= max - tie_rel max|out|}."""
    N = X.shape[0]
    valid = X[..., 0] != 0
    x = rd(X)
    T = {}
    T['nodes'] = rd(F.elu(x[..., :5] @ rd(D['wn']) + D['bn']))
    W = torch.stack([rd(D['e_wq']), rd(D['e_wk']), rd(D['e_wv'])])                               # [3,4,64 in,64 out]
    T['qkv'] = rd(torch.einsum('nti,mhio->ntmho', T['nodes'], W))                                  # [N,11,3,4,64]: column (m, h, o) of s_qkv
    q, k, v = T['qkv'][:, :, 0], T['qkv'][:, :, 1], T['qkv'][:, :, 2]
    ok = valid[:, None, :, None] & valid[:, None, None, :]
    T['P'] = rd(torch.softmax(_masked(torch.einsum('nihd,njhd->nhij', q, k) * 0.125, ok), -1))
    Pd = rd(T['P'] * fe) if fe is not None else T['P']
    T['att'] = rd(torch.einsum('nhij,njhd->nihd', Pd, v)).reshape(N, TN, EH * ED)
    T['out'] = rd(T['att'] @ rd(D['e_wo']).reshape(EH * ED, EO) + D['e_bo'])
    mx = T['out'].max(1).values
    if tie is None:
        tie = T['out'].detach() >= mx.detach()[:, None] - tie_rel * float(T['out'].detach().abs().max())
    T['tie'] = tie
    w = tie.double() / tie.sum(1, keepdim=True)
    pooled = mx.detach() + ((T['out'] - T['out'].detach()) * w).sum(1)                              # value: the maximum; gradient: dy / |tie set| on the tie set
    vec = rd(x[:, 0, 5:8] @ rd(D['wv3']))
    T['cat'] = torch.cat([pooled, vec], -1)
    T['pre_s'] = T['cat'] @ rd(D['e_ws']) + D['e_bs']
    T['enc'] = rd(F.elu(T['pre_s']))
    T['cmi'] = valid.any(1)
    return T


ENC_LEAVES = ('wn', 'bn', 'wv3', 'e_wq', 'e_wk', 'e_wv', 'e_wo', 'e_bo', 'e_ws', 'e_bs')


def pmask_bits(tie):
    """bool [N,11,320] -> the uint16 words of s_pmask [N,320] (as int32)"""
    return (tie.to(torch.int32) * (1 << torch.arange(TN, dtype=torch.int32))[None, :, None]).sum(1)


def pmask_tie(words):
    """the inverse: int [N,320] -> bool [N,11,320] (bits >= 11 ignored)"""
    return ((words.to(torch.int32)[:, None, :] >> torch.arange(TN, dtype=torch.int32)[None, :, None]) & 1).bool()


def enc_outputs(T):
    N = T['enc'].shape[0]
    return dict(enc=T['enc'], cmi=T['cmi'].to(torch.int32), s_nodes=T['nodes'], s_qkv=T['qkv'].reshape(N, TN, 3 * EH * ED), s_att=T['att'],
                s_cat=T['cat'], s_pmask=pmask_bits(T['tie']), _out=T['out'], _P=T['P'], _tie=T['tie'])


def enc_r64(P, X, fe, d_enc, tie=None):
    """float64, gradients by autograd: every output of both encoder entry points (the three "+=" outputs without their start values)"""
    D = {k: v.clone().requires_grad_(True) for k, v in _f64(P).items() if k in ENC_LEAVES}
    T = enc_forward(D, X, fe, ident, tie)
    for n in ('pre_s', 'out', 'qkv'):
        T[n].retain_grad()
    (T['enc'] * d_enc).sum().backward()
    N = X.shape[0]
    out = enc_outputs(T)
    out.update(dpre_s=T['pre_s'].grad, dout=T['out'].grad, dqkv=T['qkv'].grad.reshape(N, TN, 3 * EH * ED), dwn=D['wn'].grad, dbn=D['bn'].grad[None],
               dwv3=D['wv3'].grad)
    out['_grads'] = {k: D[k].grad for k in ENC_LEAVES}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def enc_backward_twin(P, X, fe, d_enc, S, rd):
    """agent_enc_bwd_kernel stage by stage, hand-written.  S: enc, s_nodes, s_qkv (float64 values as stored) and tie (bool).  rd():
      dpre_s = d_enc ELU'(enc);  dcat = dpre_s Ws^T;  dout = dcat / |tie set|;  datt = dout Wo^T;  dS and Pd in their LDS tiles;  dq | dk | dv
      (the tile the next product reads IS the stored dqkv).  d(pre-activation of the nodes) and the three small gradient sums stay f32."""
    D = _f64(P)
    N = X.shape[0]
    valid = X[..., 0] != 0
    x = rd(X)
    y = S['enc']
    o = {}
    o['dpre_s'] = rd(d_enc * torch.where(y > 0, torch.ones_like(y), y + 1.0))
    dcat = rd(o['dpre_s'] @ rd(D['e_ws']).t())
    tie = S['tie']
    o['dout'] = rd(dcat[:, None, :EO] * (tie.double() / tie.sum(1, keepdim=True)))
    o['dwv3'] = torch.einsum('nk,nc->kc', x[:, 0, 5:8], dcat[:, EO:])
    datt = rd(o['dout'] @ rd(D['e_wo']).reshape(EH * ED, EO).t()).reshape(N, TN, EH, ED)
    qkv = S['s_qkv'].reshape(N, TN, 3, EH, ED)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    ok = valid[:, None, :, None] & valid[:, None, None, :]
    Pr = rd(torch.softmax(_masked(torch.einsum('nihd,njhd->nhij', q, k) * 0.125, ok), -1))
    fa = fe if fe is not None else 1.0
    dP = torch.einsum('nihd,njhd->nhij', datt, v) * fa
    dS = rd(Pr * (dP - (Pr * dP).sum(-1, keepdim=True)) * 0.125)
    Pd = rd(Pr * fa)
    dq = rd(torch.einsum('nhij,njhd->nihd', dS, k))
    dk = rd(torch.einsum('nhij,nihd->njhd', dS, q))
    dv = rd(torch.einsum('nhij,nihd->njhd', Pd, datt))
    dqkv = torch.stack([dq, dk, dv], 2)
    o['dqkv'] = dqkv.reshape(N, TN, 3 * EH * ED)
    W = torch.stack([rd(D['e_wq']), rd(D['e_wk']), rd(D['e_wv'])])
    nodes = S['s_nodes']
    dnf = torch.einsum('ntmho,mhio->nti', dqkv, W) * torch.where(nodes > 0, torch.ones_like(nodes), nodes + 1.0)
    o['dwn'] = torch.einsum('ntk,ntc->kc', x[..., :5], dnf)
    o['dbn'] = dnf.sum((0, 1))[None]
    return o


# ------------------------------------------------------------------------------------------------------------------------------------------
# interaction block
# ------------------------------------------------------------------------------------------------------------------------------------------
def _seg_ln(x, n_obs, go, bo, gc, bc):
    m, r = _ln_stats(x)
    xh = (x - m) * r
    ob = (torch.arange(x.shape[1]) < n_obs)[None, :, None]
    return xh * torch.where(ob, go, gc) + torch.where(ob, bo, bc)


def int_forward(D, enc, cm, n_obs, fac, rd):
    """the three forward kernels stage by stage.  enc [B,A,384], cm bool [B,A], D['seg'] as stored (the kernels read it in dt).  rd():
      the packed kernels;  qin = concat + embed (a save only);  q = concat Wq + embed Wq -- the embedding product is added in f32 -- , k, v;
      the probabilities, and once more after the dropout factor;  att;  v1 = sum of the head slabs + bo;  n1;  elu(.), and once more after the
      dropout factor (s_h);  FFN2 + b2, and once more after the dropout factor (s_u2);  value;  enc + value;  + embed (s_out);  key."""
    B, A, _ = enc.shape
    sg = (torch.arange(A) >= n_obs).long()
    emb = D['seg'][sg]
    T = {}
    T['concat'] = enc * cm[..., None].double()
    T['qin'] = rd(T['concat'] + emb)
    Wq, Wk, Wv = rd(D['i_wq']), rd(D['i_wk']), rd(D['i_wv'])
    T['q'] = rd(torch.einsum('bni,hio->bnho', T['concat'], Wq) + torch.einsum('si,hio->sho', D['seg'], Wq)[sg])
    T['k'] = rd(torch.einsum('bni,hio->bnho', T['concat'], Wk))
    T['v'] = rd(torch.einsum('bni,hio->bnho', T['concat'], Wv))
    ok = cm[:, None, :, None] & cm[:, None, None, :]
    T['P'] = rd(torch.softmax(_masked(torch.einsum('bihd,bjhd->bhij', T['q'], T['k']) * 0.125, ok), -1))
    Pd = rd(T['P'] * fac['a']) if fac else T['P']
    T['att'] = rd(torch.einsum('bhij,bjhd->bihd', Pd, T['v'])).reshape(B, A, CB)
    T['v1lin'] = T['att'] @ rd(D['i_wo']).reshape(CB, CB)
    T['v1'] = rd(T['v1lin'] + D['i_bo'])
    m, r = _ln_stats(T['v1'])
    T['n1'] = rd((T['v1'] - m) * r * D['g1'] + D['be1'])
    T['pre1'] = T['n1'] @ rd(D['i_w1']) + D['b1']
    h = rd(F.elu(T['pre1']))
    T['h'] = rd(h * fac['1'].reshape(h.shape)) if fac else h
    T['t2lin'] = T['h'] @ rd(D['i_w2'])
    T['t2'] = T['t2lin'] + D['b2']
    u2 = rd(T['t2'])
    T['u2'] = rd(u2 * fac['2'].reshape(u2.shape)) if fac else u2
    m, r = _ln_stats(T['u2'])
    val = rd((T['u2'] - m) * r * D['g2'] + D['be2'])
    T['out'] = rd(rd(enc + val) + emb)
    T['key'] = rd(_seg_ln(T['out'], n_obs, D['g_obs'], D['b_obs'], D['g_occ'], D['b_occ']))
    return T


INT_LEAVES = ('seg', 'i_wq', 'i_wk', 'i_wv', 'i_wo', 'i_bo', 'g1', 'be1', 'i_w1', 'b1', 'i_w2', 'b2', 'g2', 'be2', 'g_obs', 'b_obs', 'g_occ', 'b_occ')


def int_outputs(T):
    B, A, _ = T['key'].shape
    f = lambda t: t.reshape(B, A, -1)
    return dict(key=T['key'], s_concat=T['concat'], s_qin=T['qin'], s_q=f(T['q']), s_k=f(T['k']), s_v=f(T['v']), s_att=T['att'], s_v1=T['v1'], s_n1=T['n1'],
                s_h=T['h'], s_u2=T['u2'], s_out=T['out'], ws_v1=T['v1lin'], ws_u2=T['t2lin'], _P=T['P'], _pre1=T['pre1'])


def int_r64(P, enc, cm, n_obs, fac, dkey):
    """float64, gradients by autograd: every output of both interaction entry points (the nine "+=" outputs without their start values; the
    slab workspaces as the sum of their slabs)"""
    D = {k: v.clone().requires_grad_(True) for k, v in _f64(P).items() if k in INT_LEAVES}
    enc = enc.clone().requires_grad_(True)
    T = int_forward(D, enc, cm, n_obs, fac, ident)
    for n in ('q', 'k', 'v', 'v1', 'n1', 'pre1', 't2'):
        T[n].retain_grad()
    (T['key'] * dkey).sum().backward()
    B, A, _ = enc.shape
    f = lambda t: t.reshape(B, A, -1)
    out = int_outputs(T)
    out.update(dq=f(T['q'].grad), dk=f(T['k'].grad), dv=f(T['v'].grad), dv1=T['v1'].grad, dpre1=T['pre1'].grad, dz2=T['t2'].grad, ws_dn1=T['n1'].grad,
               d_enc=enc.grad, dseg=D['seg'].grad)
    for n, src in INT_GRADS.items():
        if n != 'dseg':
            out[n] = D[src].grad[None]
    out['_grads'] = {k: D[k].grad for k in INT_LEAVES}
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def int_backward_twin(P, cs, cm, fac, dkey, S, rd, seg=None):
    """the three backward kernels stage by stage, hand-written.  S: s_q, s_k, s_v, s_v1, s_h, s_u2, s_out (float64 values as stored).  rd():
      d(out) (it is the residual's slab of d_enc, the operand of LayerNorm2's backward and the summand of d_embed);  dz2;  dpre1;  dv1;
      datt of a head;  dS (both its LDS tile and the chained fragment) and Pd;  dq | dk | dv.  The slabs, the LayerNorm gradient sums and the
      shares of d(qin) / d(concat) stay f32."""
    D = _f64(P)
    if seg is not None:
        D['seg'] = seg
    B, A, n_obs, p = cs['B'], cs['A'], cs['n_obs'], cs['p']
    ob = (torch.arange(A) < n_obs)
    o = {}
    m, r = _ln_stats(S['s_out'])
    xh = (S['s_out'] - m) * r
    gm = torch.where(ob[None, :, None], D['g_obs'], D['g_occ'])
    o['dg_obs'], o['db_obs'] = (dkey * xh)[:, ob].sum((0, 1))[None], dkey[:, ob].sum((0, 1))[None]
    o['dg_occ'], o['db_occ'] = (dkey * xh)[:, ~ob].sum((0, 1))[None], dkey[:, ~ob].sum((0, 1))[None]
    d = rd(_ln_bwd(xh, dkey * gm, r))
    m, r = _ln_stats(S['s_u2'])
    xh = (S['s_u2'] - m) * r
    o['dg2'], o['dbe2'] = (d * xh).sum((0, 1))[None], d.sum((0, 1))[None]
    du = _ln_bwd(xh, d * D['g2'], r)
    o['dz2'] = rd(du * fac['2'].reshape(du.shape)) if fac else rd(du)
    y = S['s_h'] * (1.0 - p) if fac else S['s_h']
    dh = o['dz2'] @ rd(D['i_w2']).t()
    if fac:
        dh = dh * fac['1'].reshape(dh.shape)
    o['dpre1'] = rd(dh * torch.where(y > 0, torch.ones_like(y), y + 1.0))
    o['ws_dn1'] = o['dpre1'] @ rd(D['i_w1']).t()
    m, r = _ln_stats(S['s_v1'])
    xh = (S['s_v1'] - m) * r
    o['dg1'], o['dbe1'] = (o['ws_dn1'] * xh).sum((0, 1))[None], o['ws_dn1'].sum((0, 1))[None]
    o['dv1'] = rd(_ln_bwd(xh, o['ws_dn1'] * D['g1'], r))
    datt = rd(torch.einsum('bnc,hoc->bnho', o['dv1'], rd(D['i_wo'])))
    hs = lambda t: t.reshape(B, A, IH, IDH)
    q, k, v = hs(S['s_q']), hs(S['s_k']), hs(S['s_v'])
    ok = cm[:, None, :, None] & cm[:, None, None, :]
    Pr = rd(torch.softmax(_masked(torch.einsum('bihd,bjhd->bhij', q, k) * 0.125, ok), -1))
    fa = fac['a'] if fac else 1.0
    dP = torch.einsum('bihd,bjhd->bhij', datt, v) * fa
    dS = rd(Pr * (dP - (Pr * dP).sum(-1, keepdim=True)) * 0.125)
    Pd = rd(Pr * fa)
    dq = rd(torch.einsum('bhij,bjhd->bihd', dS, k))
    dk = rd(torch.einsum('bhij,bihd->bjhd', dS, q))
    dv = rd(torch.einsum('bhij,bihd->bjhd', Pd, datt))
    o['dq'], o['dk'], o['dv'] = dq.reshape(B, A, CB), dk.reshape(B, A, CB), dv.reshape(B, A, CB)
    dqi = torch.einsum('bnho,hio->bni', dq, rd(D['i_wq']))
    dco = torch.einsum('bnho,hio->bni', dk, rd(D['i_wk'])) + torch.einsum('bnho,hio->bni', dv, rd(D['i_wv']))
    o['d_enc'] = d + cm[..., None].double() * (dqi + dco)
    tot = d + dqi
    o['dseg'] = torch.stack([tot[:, ob].sum((0, 1)), tot[:, ~ob].sum((0, 1))])
    return o


# ------------------------------------------------------------------------------------------------------------------------------------------
# the pack
# ------------------------------------------------------------------------------------------------------------------------------------------
def pack_image(P, dt):
    """stj_agent_pack's output as the header and P_EQKV .. P_TOTAL of csrc/agent_fused.hip state it: the transposed copies [N][K], K contiguous,
    one after the other: node_attention q | k | v [3 x 256][64] (row (h, o)), its projection [320][256], sublayer [384][384], cross_attention q | k | v
    [3 x 384][384] (row (h, o)), its projection [384][384], FFN1 [1536][384], FFN2 [384][1536].
    COUPLING: this restates the element offsets P_EQKV .. P_TOTAL.  Reordering the pack fails test_pack for a reason that is no error of
    the kernels: update pack_image with it."""
    tfa = lambda w: w.permute(0, 2, 1).reshape(-1, w.shape[1])            # [H][K][hs] -> [(h, o)][K]
    parts = [tfa(P['e_wq']), tfa(P['e_wk']), tfa(P['e_wv']), P['e_wo'].reshape(EH * ED, EO).t(), P['e_ws'].t(), tfa(P['i_wq']), tfa(P['i_wk']), tfa(P['i_wv']),
             P['i_wo'].reshape(CB, CB).t(), P['i_w1'].t(), P['i_w2'].t()]
    return torch.cat([t.reshape(-1) for t in parts]).to(dt)


PACK_ELEMS = 3 * EH * ED * NF + EO * EH * ED + CB * CB + 3 * CB * CB + CB * CB + 2 * FF * CB


# ------------------------------------------------------------------------------------------------------------------------------------------
# One call: buffers, reference, bounds
# ------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """one flat allocation: pattern everywhere, `values` at flat positions `idx` (relative to base = GUARD)"""
    def __init__(self, n, dt):
        self.init, self.base, self.n = pattern(GUARD + n + GUARD, dt), GUARD, n
        self.out = torch.zeros(GUARD + n + GUARD, dtype=torch.bool)          # elements this call may write

    def put(self, idx, values):
        self.init[GUARD + idx.reshape(-1)] = values.reshape(-1).to(self.init.dtype)


class Prep:
    pass


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def _row_bound(ref, tol, start=None):
    n = _rows(ref).norm(dim=1)
    b = torch.maximum(n, (n ** 2).mean().sqrt())
    if start is not None:
        b = b + _rows(start).norm(dim=1)
    return tol * b


_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def enc_reference(cs, dt, masks, tag, d_enc_mode, tie=None, tie_tag=None):
    """(I, fe, R64, twin) of one encoder case, dtype and gradient form; computed once per process and left unchanged.
    d_enc_mode 0: d_enc in dt; 1 / 7: that many f32 slabs.  tie: the tie sets the backward is handed (default: R64's own); the twin's
    backward then reads R64's saves rounded to dt, or, with tie handed in (behind the forward kernel), its own forward's."""
    def make():
        I = make_inputs(cs, dt)
        X = tracks_of(I)
        fe = _factors(cs, masks)['e'] if masks else None
        d_enc = I['d_enc'].double() if d_enc_mode == 0 else I['d_enc_slabs'][:d_enc_mode].double().sum(0)
        R = enc_r64(params(), X, fe, d_enc, tie)
        tw = None
        if dt != F32:
            rd = rounder(dt)
            tw = enc_outputs(enc_forward(_f64(params()), X, fe, rd, tie, tie_rel=0.0))
            if tie is None:
                S = dict(enc=rd(R['enc']), s_nodes=rd(R['s_nodes']), s_qkv=rd(R['s_qkv']), tie=R['_tie'])
            else:
                S = dict(enc=tw['enc'], s_nodes=tw['s_nodes'], s_qkv=tw['s_qkv'], tie=tie)
            tw.update(enc_backward_twin(params(), X, fe, d_enc, S, rd))
        return I, fe, R, tw
    return _cached((cs['name'], dt, tag, d_enc_mode, tie_tag), make)


def int_reference(cs, dt, masks, tag, e2e=False):
    def make():
        I = make_inputs(cs, dt)
        fac = _factors(cs, masks)
        P = dict(params())
        rd = rounder(dt)
        P['seg'] = rd(P['seg'].double())                              # the kernels read seg_embed in dt: that IS the input
        R = int_r64(P, I['enc'].double(), I['cm'], cs['n_obs'], fac, I['dkey'].double())
        tw = int_outputs(int_forward(_f64(P), I['enc'].double(), I['cm'], cs['n_obs'], fac, rd))
        src = tw if e2e else {k: rd(R[k]) for k in INT_SAVES}
        tw.update(int_backward_twin(P, cs, I['cm'], fac, I['dkey'].double(), {k: src[k] for k in INT_SAVES}, rd, seg=P['seg']))
        return I, fac, R, tw, P
    return _cached((cs['name'], dt, tag, 'int', e2e), make)


ROWS11 = ('s_nodes', 's_qkv', 's_att', 'dout', 'dqkv')
ENC_W = dict(enc=CB, s_nodes=NF, s_qkv=3 * EH * ED, s_att=EH * ED, s_cat=CB, dpre_s=CB, dout=EO, dqkv=3 * EH * ED, d_enc=CB)
INT_W = dict(s_h=FF, dpre1=FF)


def _param_bufs(p, grads):
    P = params()
    par = p.bufs['params'] = Buf(PTOTAL, F32)
    wn = p.bufs['wnat'] = Buf(PTOTAL, p.dt)
    for n, (off, shape) in LAY.items():
        idx = off + torch.arange(math.prod(shape))
        par.put(idx, P[n])
        wn.put(idx, P[n])
    if grads:
        gr = p.bufs['grads'] = Buf(PTOTAL, F32)
        for n, src in grads.items():
            off, shape = LAY[src]
            idx = off + torch.arange(math.prod(shape))
            gr.put(idx, P['start_' + n])
            gr.out[GUARD + idx] = True
            p.outs[n] = ('grads', idx.reshape(-1, shape[-1]), 'rows')


def prepare(cs, dt, kind, masks=None, tag='cpu', with_saves=True, d_enc_mode=0, saves_from=None, tie=None, tie_tag=None):
    """kind 'enc_fwd' / 'enc_bwd' / 'int_fwd' / 'int_bwd'.  masks: the keep masks (draw_shapes) when cs['p'] > 0; default cpu_masks(cs).
    with_saves False: the inference form of a forward.  d_enc_mode: enc_bwd's gradient form (0: dt, 1 / 7: f32 slabs).
    saves_from (+ tie for the encoder): what a forward kernel wrote, for the backward behind it."""
    assert kind in ('enc_fwd', 'enc_bwd', 'int_fwd', 'int_bwd') and kind.startswith(cs['block'])
    if cs['p'] > 0 and masks is None:
        masks, tag = cpu_masks(cs), 'cpu'
    if not cs['p'] > 0:
        masks = None
    B, A = cs['B'], cs['A']
    N = B * A
    p = Prep()
    p.cs, p.dt, p.kind, p.bufs, p.outs, p.with_saves, p.d_enc_mode, p.extra = cs, dt, kind, {}, {}, with_saves, d_enc_mode, {}
    fwd = kind.endswith('fwd')

    def tensor(name, shape, t, values=None, out=None):
        n = math.prod(shape)
        b = p.bufs[name] = Buf(n, t)
        if values is not None:
            b.put(torch.arange(n), values)
        if out:
            b.out[GUARD:GUARD + n] = True
            p.outs[name] = (name, torch.arange(n).reshape(-1, shape[-1]), out)

    if cs['block'] == 'enc':
        I, fe, R, tw = enc_reference(cs, dt, masks, tag, d_enc_mode if not fwd else 0, tie, tie_tag)
        p.I, p.fac, p.R, p.tw = I, fe, R, tw
        tensor('obs', I['obs'].shape, F32, I['obs'])
        tensor('occ', I['occ'].shape, F32, I['occ'])
        _param_bufs(p, None if fwd else ENC_GRADS)
        if fwd:
            tensor('enc', (N, CB), dt, out='rows')
            tensor('cmi', (N, 1), torch.int32, out='exact')
            if with_saves:
                for n in ('s_nodes', 's_qkv', 's_att'):
                    tensor(n, (N * TN, ENC_W[n]), dt, out='rows')
                tensor('s_pmask', (N, EO), torch.int16, out='pmask')
                tensor('s_cat', (N, CB), dt, out='rows')
        else:
            S = saves_from if saves_from is not None else dict(enc=R['enc'], cmi=R['cmi'], s_nodes=R['s_nodes'], s_qkv=R['s_qkv'], s_att=R['s_att'],
                                                               s_cat=R['s_cat'], s_pmask=R['s_pmask'])
            tensor('enc', (N, CB), dt, S['enc'])
            tensor('cmi', (N, 1), torch.int32, S['cmi'])
            for n in ('s_nodes', 's_qkv', 's_att'):
                tensor(n, (N * TN, ENC_W[n]), dt, S[n])
            tensor('s_pmask', (N, EO), torch.int16, S['s_pmask'])
            tensor('s_cat', (N, CB), dt, S['s_cat'])
            if d_enc_mode == 0:
                tensor('d_enc', (N, CB), dt, I['d_enc'])
            else:
                tensor('d_enc', (d_enc_mode, N, CB), F32, I['d_enc_slabs'][:d_enc_mode])
            tensor('dpre_s', (N, CB), dt, out='rows')
            tensor('dout', (N * TN, EO), dt, out='rows')
            tensor('dqkv', (N * TN, 3 * EH * ED), dt, out='rows')
    else:
        I, fac, R, tw, P = int_reference(cs, dt, masks, tag, e2e=saves_from is not None)
        p.I, p.fac, p.R, p.tw = I, fac, R, tw
        tensor('enc', (N, CB), dt, I['enc'])
        tensor('cmi', (N, 1), torch.int32, I['cm'].to(torch.int32))
        tensor('seg', (2, CB), dt, P['seg'])
        _param_bufs(p, None if fwd else INT_GRADS)
        if fwd:
            tensor('key', (N, CB), dt, out='rows')
            tensor('ws_v1', (SLABS['ws_v1'], N, CB), F32, out='slabs')
            tensor('ws_u2', (SLABS['ws_u2'], N, CB), F32, out='slabs')
            if with_saves:
                for n in INT_SAVES:
                    tensor(n, (N, INT_W.get(n, CB)), dt, out='rows')
        else:
            S = saves_from if saves_from is not None else {k: R[k] for k in INT_SAVES}
            for n in INT_SAVES:
                tensor(n, (N, INT_W.get(n, CB)), dt, S[n])
            tensor('dkey', (N, CB), dt, I['dkey'])
            for n in INT_DY:
                tensor(n, (N, INT_W.get(n, CB)), dt, out='rows')
            tensor('ws_dn1', (SLABS['ws_dn1'], N, CB), F32, out='slabs')
            tensor('d_enc', (SLABS['d_enc'], N, CB), F32, out='slabs')
    # bounds
    tol = TOL_FWD if fwd else TOL_BWD
    grads = {**ENC_GRADS, **INT_GRADS}
    p.bound = {}
    for n, (_, _, how) in p.outs.items():
        if how not in ('rows', 'slabs'):
            continue
        start = params()['start_' + n].double() if n in grads else None
        f32b = _row_bound(p.R[n], tol, start)
        if dt == F32:
            p.bound[n] = f32b
        else:
            e = _rows(p.tw[n] - p.R[n]).norm(dim=1)
            p.bound[n] = 2.0 * torch.maximum(e, (e ** 2).mean().sqrt()) + f32b
    return p


def expected(p, name):
    """R64's value of an output as the judge compares it ("+=" outputs with their start values), rows"""
    ref = _rows(p.R[name].double())
    if name in ENC_GRADS or name in INT_GRADS:
        ref = ref + _rows(params()['start_' + name].double())
    return ref


def logical(p, after, name):
    bname, idx, _ = p.outs[name]
    return after[bname][GUARD + idx.reshape(-1)].reshape(idx.shape)


def pmask_slack(p):
    """per agent: 2 (largest |twin - R64| of the agent's pre-pool block) + 2e-5 of the largest |R64 maximum| of the agent"""
    o64 = p.R['_out']
    e = (p.tw['_out'] - o64).abs().amax((1, 2)) if p.tw is not None else torch.zeros(o64.shape[0], dtype=F64)
    return 2.0 * e + TOL_FWD * o64.max(1).values.abs().amax(1)


def judge(p, after, ratios=None, label=''):
    """after: name -> the flat CPU buffer as the call left it.  Raises AssertionError; appends (kind, dtype, output, case, largest e / bound)."""
    cs = p.cs
    label = f"{cs['name']} {p.kind}{'' if p.with_saves else ' (no saves)'}{label}"
    for name, b in p.bufs.items():
        keep = ~b.out
        bad = (bits(after[name])[keep] != bits(b.init)[keep]).nonzero()
        assert bad.numel() == 0, f'{label}: {bad.numel()} elements of {name} outside the outputs changed, first at flat index {int(keep.nonzero()[bad[0, 0]]) - GUARD}'
    for name, (bname, idx, how) in p.outs.items():
        raw = logical(p, after, name)
        if raw.numel() == 0:
            continue
        left = bits(raw) == int(bits(pattern(1, raw.dtype))[0])
        if how == 'pmask':
            left = left.all(1)                                       # (0x7FA5 has bits >= 11 set: caught below as well)
        assert not bool(left.any()), f'{label}: {int(left.sum())} elements of {name} still hold the fill pattern, first at {tuple(left.nonzero()[0].tolist())}'
        if how == 'exact':
            ne = raw.reshape(-1).long() != p.R[name].reshape(-1).long()
            assert not bool(ne.any()), f'{label}: {name}: {int(ne.sum())} values differ, first at {int(ne.nonzero()[0])}'
            continue
        if how == 'pmask':
            words = raw.to(torch.int32) & 0xffff
            assert not bool((words >> TN).any()), f'{label}: s_pmask: {int((words >> TN != 0).sum())} words have a bit >= 11 set'
            assert bool((words != 0).all()), f'{label}: s_pmask: {int((words == 0).sum())} words are empty'
            # admissible: no marked step lies further below the float64 maximum than honest arithmetic in dt can put it
            o64, marked = p.R['_out'], pmask_tie(words)
            short = (o64.max(1, keepdim=True).values - o64) / (pmask_slack(p)[:, None, None] + 1e-300)
            bad = marked & (short > 1.0)
            ratio = float((short * marked).max())
            if ratios is not None:
                ratios.append((p.kind, str(p.dt), name, cs['name'], ratio))
            assert not bool(bad.any()), (f'{label}: s_pmask: {int(bad.sum())} steps are marked as holding the maximum whose float64 value is too far below it, '
                                         f'largest distance / slack = {ratio:.3e}, first (agent, step, column) {tuple(bad.nonzero()[0].tolist())}')
            # the ties of float64 are rows that are bitwise equal in front of the pool in ANY arithmetic (invalid steps attend uniformly): the
            # steps of such a tie set are marked all or none (16 bit: another step may round above them), and in f32 the word is float64's
            t64 = p.R['_tie']
            tied = (t64.sum(1) > 1)
            some = (t64 & marked).any(1) & (t64 & ~marked).any(1) & tied
            assert not bool(some.any()), f'{label}: s_pmask: {int(some.sum())} tie sets of float64 are marked in part, first (agent, column) {tuple(some.nonzero()[0].tolist())}'
            if p.dt == F32:
                ne = (words != p.R['s_pmask']) & (p.R['_tie'].sum(1) > 1)
                assert not bool(ne.any()), f'{label}: s_pmask: {int(ne.sum())} words differ from the tie sets of float64, first at {tuple(ne.nonzero()[0].tolist())}'
            continue
        got = raw.double()
        if how == 'slabs':
            got = got.reshape(SLABS[name], -1, CB).sum(0)
        ref = expected(p, name)
        err = (got - ref).norm(dim=1)
        ok = err <= p.bound[name]            # False for NaN
        ratio = float((err / (p.bound[name] + 1e-300)).nan_to_num(nan=float('inf')).max())
        if ratios is not None:
            ratios.append((p.kind, str(p.dt), name, cs['name'], ratio))
        assert bool(ok.all()), (f'{label}: {name}: {int((~ok).sum())} of {ok.numel()} rows over their bound, largest ||err|| / bound = {ratio:.3e}, '
                                f'first row {int((~ok).nonzero()[0])}')


def stage(p, values=None, source=None):
    """`after` buffers as a call that wrote `values` (name -> logical tensor; default: R64's, "+=" outputs with their start values, rounded
    to the storage type, the sum of a slab workspace spread evenly over its slabs) would have left them -- the judge's own test bench"""
    after = {k: b.init.clone() for k, b in p.bufs.items()}
    for name, (bname, idx, how) in p.outs.items():
        if values is not None and name in values:
            v = values[name]
        elif how in ('rows', 'slabs'):
            v = expected(p, name) if source is None else _rows(source[name].double())
        else:
            v = (p.R if source is None else source)[name]
        if how == 'slabs':
            v = (v.reshape(1, -1, CB) / SLABS[name]).expand(SLABS[name], -1, -1)
        after[bname][GUARD + idx.reshape(-1)] = v.reshape(-1).to(after[bname].dtype)
    return after


def report_lines(ratios, title):
    best = {}
    for kind, dt, name, cname, r in ratios:
        k = (kind, dt, name)
        if k not in best or r > best[k][0]:
            best[k] = (r, cname)
    return [f'{title} {kind:7s} {dt:15s} {name:8s} largest ||err|| / bound {r:.3e} ({cname})' for (kind, dt, name), (r, cname) in sorted(best.items())]
