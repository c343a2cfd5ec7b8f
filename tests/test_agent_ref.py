"""The references and the judge of _agent_cases.py themselves, on the CPU (test_agent_abi_gpu.py judges the kernels of csrc/agent_fused.hip
with them):
  R64 against the project's independent float64 statement of the branch, oracle.torch_ref._traj, on the tie-free cases: key, cm and every
      traj_net/* parameter gradient rebuilt as X^T dY from R64's operands (the products the caller of the kernels queues);
  the hand-written backward of the twin, with the identity for a rounding, against R64's autograd gradients, ties included (the forward
      stages are ONE function for both, enc_forward / int_forward: there the identity holds by construction);
  the judge: it accepts float64 rounded to the storage type and the twin, and rejects each planted error;
  the inputs: they exercise the block (softmax neither uniform nor one-hot, FFN pre-activations of both signs, ties present, the twin at a
      non-zero distance in all but a few rows)."""
import pytest
import torch

import _agent_cases as AC
from _agent_cases import CB, DT16, EO, F32, GUARD, IH, IDH, TN, bits, case, judge, params, prepare, stage

BF16, F16 = torch.bfloat16, torch.float16


def _close(a, b, tol, what):
    e = float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))
    assert e <= tol, f'{what}: {e:.3e} of the largest element, allowed {tol:.1e}'


# ---- R64 against oracle.torch_ref._traj ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in AC.tie_free_cases()])
def test_r64_matches_the_oracle_on_tie_free_tracks(name):
    """Tolerance 2e-5 of a tensor's largest element: _mha builds a masked logit as x + (-1e10 - x), which float64 resolves to -1e10 +- 2e-6
    (ulp(1e10) = 1.9e-6), so the `uniform` attention of an invalid step carries 2e-6 relative noise there; R64 states exactly -1e10 as the
    f32 reference arithmetic does.  Everything else agrees to 1e-12."""
    from oracle import torch_ref
    cs = case(name)
    B, A, n_obs = cs['B'], cs['A'], cs['n_obs']
    I = AC.make_inputs(cs, F32)
    X = AC.tracks_of(I)
    me, mi = AC.cpu_masks(cs), AC.cpu_masks(cs, seed=5, block='int')
    P = params()
    G = torch.randn((B, A, CB), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    W = {AC.TRAJ_NAMES[k]: P[k].double().clone() for k in AC.TRAJ_NAMES}
    W[AC.TRAJ_NAMES['wn']] = W[AC.TRAJ_NAMES['wn']][None]
    for w in W.values():
        w.requires_grad_(True)
    pre = 'traj_net/cross_attention'
    torch_ref._MASKS = {'traj_net/traj_encoder/node_attention/dropout': me['e'], pre + '/mha/dropout': mi['a'], pre + '/dropout1': mi['1'], pre + '/dropout2': mi['2']}
    try:
        key, cm = torch_ref._traj(W, I['obs'].double(), I['occ'].double())
    finally:
        torch_ref._MASKS = None
    (key * G).sum().backward()
    fe, fi = AC._factors(cs, me)['e'], AC._factors(cs, mi)
    E0 = AC.enc_r64(P, X, fe, torch.zeros(B * A, CB, dtype=torch.float64))
    assert bool((E0['_tie'].sum(1) == 1).all()), 'the tie-free case has a max-pool tie'
    assert torch.equal(E0['cmi'].bool().reshape(B, A), cm)
    Ri = AC.int_r64(P, E0['enc'].reshape(B, A, CB), cm, n_obs, fi, G)
    Re = AC.enc_r64(P, X, fe, Ri['d_enc'].reshape(B * A, CB))
    tol = 2e-5
    _close(Ri['key'], key.detach(), tol, 'key')
    N = B * A
    r2 = lambda t: t.reshape(-1, t.shape[-1])
    dqkv = Re['dqkv'].reshape(N, TN, 3, AC.EH, AC.ED)
    hd = lambda t: t.reshape(B, A, IH, IDH)
    rebuilt = dict(e_ws=Re['s_cat'].t() @ Re['dpre_s'], e_bs=Re['dpre_s'].sum(0), e_wo=(r2(Re['s_att']).t() @ r2(Re['dout'])).reshape(AC.EH, AC.ED, EO),
                   e_bo=r2(Re['dout']).sum(0), wn=Re['dwn'][None], bn=Re['dbn'][0], wv3=Re['dwv3'], seg=Ri['dseg'],
                   i_wq=torch.einsum('bni,bnho->hio', Ri['s_qin'], hd(Ri['dq'])), i_wk=torch.einsum('bni,bnho->hio', Ri['s_concat'], hd(Ri['dk'])),
                   i_wv=torch.einsum('bni,bnho->hio', Ri['s_concat'], hd(Ri['dv'])), i_wo=(r2(Ri['s_att']).t() @ r2(Ri['dv1'])).reshape(IH, IDH, CB),
                   i_bo=r2(Ri['dv1']).sum(0), i_w1=r2(Ri['s_n1']).t() @ r2(Ri['dpre1']), b1=r2(Ri['dpre1']).sum(0), i_w2=r2(Ri['s_h']).t() @ r2(Ri['dz2']),
                   b2=r2(Ri['dz2']).sum(0))
    for m, k in enumerate(('e_wq', 'e_wk', 'e_wv')):
        rebuilt[k] = torch.einsum('nti,ntho->hio', Re['s_nodes'], dqkv[:, :, m])
    for n, src in AC.INT_GRADS.items():
        if n != 'dseg':
            rebuilt[src] = Ri[n][0]
    assert set(rebuilt) == set(AC.TRAJ_NAMES)
    for k, g in rebuilt.items():
        _close(g, W[AC.TRAJ_NAMES[k]].grad.reshape(g.shape), tol, f'gradient of {AC.TRAJ_NAMES[k]}')


# ---- the twin's hand-written backward with the identity for a rounding --------------------------------------------------------------------
@pytest.mark.parametrize('name', ['e2_3_5_p0', 'e2_3_5_p0.1', 'e1_1_1'])
def test_encoder_twin_with_identity_rounding_is_r64(name):
    cs = case(name)
    p = prepare(cs, F32, 'enc_bwd')
    X = AC.tracks_of(p.I)
    R = p.R
    if cs['p'] == 0:
        assert bool((R['_tie'].sum(1) > 1).any()), 'no tie in a case that is meant to have one'
    S = dict(enc=R['enc'], s_nodes=R['s_nodes'], s_qkv=R['s_qkv'], tie=R['_tie'])
    o = AC.enc_backward_twin(params(), X, p.fac, p.I['d_enc'].double(), S, AC.ident)
    for n in ('dpre_s', 'dout', 'dqkv', 'dwn', 'dbn', 'dwv3'):
        _close(o[n], R[n], 1e-10, f'{name} {n}')


@pytest.mark.parametrize('name', ['i37_p0', 'i37_p0.1', 'i0_p0.1'])
def test_interaction_twin_with_identity_rounding_is_r64(name):
    cs = case(name)
    I = AC.make_inputs(cs, F32)
    fac = AC._factors(cs, AC.cpu_masks(cs))
    R = AC.int_r64(params(), I['enc'].double(), I['cm'], cs['n_obs'], fac, I['dkey'].double())
    o = AC.int_backward_twin(params(), cs, I['cm'], fac, I['dkey'].double(), {k: R[k] for k in AC.INT_SAVES}, AC.ident)
    for n in AC.INT_DY + ('ws_dn1', 'd_enc') + tuple(AC.INT_GRADS):
        _close(o[n], R[n], 1e-10, f'{name} {n}')


# ---- the judge ------------------------------------------------------------------------------------------------------------------------------
def _rejects(p, after, word):
    with pytest.raises(AssertionError, match=word):
        judge(p, after)


@pytest.mark.parametrize('dt', AC.DTYPES, ids=str)
def test_judge_accepts_the_references(dt):
    for name, kinds in (('e2_3_5_p0', ('enc_fwd', 'enc_bwd')), ('i37_p0.1', ('int_fwd', 'int_bwd'))):
        if dt == F32 and name.startswith('i'):
            continue
        for kind in kinds:
            p = prepare(case(name), dt, kind)
            judge(p, stage(p))
            if dt != F32:
                tw = dict(p.tw)
                tw['cmi'] = p.R['cmi'] if 'cmi' in p.R else None
                for n in {**AC.ENC_GRADS, **AC.INT_GRADS}:
                    if n in tw:
                        tw[n] = tw[n] + params()['start_' + n].double().reshape(tw[n].shape)
                judge(p, stage(p, source=tw))


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_judge_rejects_planted_errors_of_the_interaction_block(dt):
    cs = case('i37_p0.1')
    p = prepare(cs, dt, 'int_fwd')
    I, fac = p.I, p.fac
    P = {k: v.double() for k, v in params().items()}
    P['seg'] = AC.rounder(dt)(P['seg'])
    # one head dropped: head 2 contributes nothing to the output projection
    Q = dict(P)
    Q['i_wo'] = P['i_wo'].clone()
    Q['i_wo'][2] = 0
    T = AC.int_outputs(AC.int_forward(Q, I['enc'].double(), I['cm'], cs['n_obs'], fac, AC.ident))
    _rejects(p, stage(p, {n: T[n] for n in ('key', 'ws_v1')}), 'ws_v1|key')
    _rejects(p, stage(p, {'key': T['key']}), 'key')
    # the wrong segment row for one token: token 37 takes the obs row
    T = AC.int_outputs(AC.int_forward(P, I['enc'].double(), I['cm'], 38, fac, AC.ident))
    for n in ('key', 's_qin', 's_q', 's_out'):
        _rejects(p, stage(p, {n: T[n]}), n)
    # backward: one slab omitted, one row of dpre1 scaled by 1.02
    q = prepare(cs, dt, 'int_bwd')
    good = stage(q)
    judge(q, good)
    for n in ('d_enc', 'ws_dn1'):
        bad = {k: v.clone() for k, v in good.items()}
        N = cs['B'] * cs['A']
        bad[n][GUARD + 2 * N * CB:GUARD + 3 * N * CB] = 0
        _rejects(q, bad, n)
    v = AC.expected(q, 'dpre1').clone()
    v[77] *= 1.02
    _rejects(q, stage(q, {'dpre1': v}), 'dpre1')
    # a guard byte touched, an output row left as it was
    bad = {k: v.clone() for k, v in good.items()}
    bits(bad['dq'])[GUARD - 1] ^= 1
    _rejects(q, bad, 'outside the outputs')
    bad = {k: v.clone() for k, v in good.items()}
    bad['dz2'][GUARD + 5 * CB:GUARD + 6 * CB] = q.bufs['dz2'].init[GUARD + 5 * CB:GUARD + 6 * CB]
    _rejects(q, bad, 'fill pattern')


@pytest.mark.parametrize('dt', AC.DTYPES, ids=str)
def test_judge_rejects_planted_errors_of_the_encoder(dt):
    cs = case('e2_3_5_p0')
    p = prepare(cs, dt, 'enc_bwd')
    R = p.R
    tie = R['_tie']
    assert bool((tie.sum(1) > 1).any())
    good = stage(p)
    judge(p, good)
    # a tie gradient not split: every step of a tie set takes the whole gradient
    _rejects(p, stage(p, {'dout': R['dout'] * tie.sum(1, keepdim=True)}), 'dout')
    bad = {k: v.clone() for k, v in good.items()}
    bits(bad['params'])[GUARD + AC.PTOTAL] ^= 1
    _rejects(p, bad, 'outside the outputs')
    bad = {k: v.clone() for k, v in good.items()}
    bad['dqkv'][GUARD + 3 * 768:GUARD + 4 * 768] = p.bufs['dqkv'].init[GUARD + 3 * 768:GUARD + 4 * 768]
    _rejects(p, bad, 'fill pattern')
    # forward: a wrong agent mask; a step marked as a maximum that is none
    f = prepare(cs, dt, 'enc_fwd')
    cmi = f.R['cmi'].clone()
    cmi[3] ^= 1
    _rejects(f, stage(f, {'cmi': cmi}), 'cmi')
    o64 = f.R['_out']
    worst = o64.argmin(1)                                            # [N,320]: the step furthest below the maximum
    words = f.R['s_pmask'].clone()
    words[1, 7] |= 1 << int(worst[1, 7])
    _rejects(f, stage(f, {'s_pmask': words}), 's_pmask')
    words = f.R['s_pmask'].clone()
    words[0, 0] |= 1 << 12
    _rejects(f, stage(f, {'s_pmask': words}), 'bit >= 11')
    words = f.R['s_pmask'].clone()
    words[2, 5] = 0
    _rejects(f, stage(f, {'s_pmask': words}), 'empty')


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------------
def _zero_share(p, names, only=None):
    """share of the rows, among those that are not identically zero in float64 (and, for the names in `only`, lie in its row mask), at which
    the twin does not differ from float64"""
    worst = (0.0, None)
    for n in names:
        ref = p.R[n].double().reshape(-1, p.R[n].shape[-1])
        live = ref.norm(dim=1) > 0
        if only and n in only:
            live = live & only[n]
        e = (p.tw[n].double().reshape(ref.shape) - ref).norm(dim=1)
        s = float((e[live] == 0).double().mean()) if bool(live.any()) else 0.0
        if s > worst[0]:
            worst = (s, n)
    return worst


def test_the_cases_contain_what_they_are_meant_to():
    kinds = set()
    for cs in AC.enc_cases():
        I = AC.make_inputs(cs, F32)
        kinds |= {k for row in I['kinds'] for k in row}
        x = AC.tracks_of(I)[..., 0]
        if cs['name'].startswith('e3_48_16'):
            assert not bool(x[:64].any()), 'scene 0 has an agent'
    assert kinds == set(AC.KINDS)
    x = AC.tracks_of(AC.make_inputs(case('e2_3_5_p0'), F32))
    assert bool((x[..., 0] == 2.0 ** -26).any()) and float(torch.tensor(2.0 ** -26).to(F16)) == 0.0
    neg = (x[..., 0] == 0) & torch.signbit(x[..., 0])
    assert bool(neg.any())
    step0 = (x[:, 0, 0] == 0) & (x[:, 0, 5:8].sum(-1) == 1) & (x[:, 1:, 0] != 0).all(1)
    assert bool(step0.any())
    for n, (off, _) in AC.LAY.items():
        assert off % 4 == 0, n
    assert AC.pack_image(params(), BF16).numel() == AC.PACK_ELEMS


@pytest.mark.parametrize('name', [c['name'] for c in AC.enc_cases()])
def test_encoder_inputs_exercise_the_block(name):
    cs = case(name)
    for dt in DT16:
        p = prepare(cs, dt, 'enc_bwd')
        R = p.R
        valid = AC.tracks_of(p.I)[..., 0] != 0
        rows = valid[:, None, :, None].expand(-1, AC.EH, -1, -1) & (valid.sum(1) > 2)[:, None, None, None]          # unmasked query rows with 3 or more keys
        if bool(rows.any()):
            peak = float(R['_P'].max(-1, keepdim=True).values[rows].mean())
            assert 0.15 <= peak <= 0.85, f'{name}: mean max_key P = {peak:.3f}: the attention is uniform or one-hot'
        if cs['B'] * cs['A'] >= 16:
            ties = R['_tie'].sum(1)
            assert cs['p'] > 0 or bool(((ties > 1) & (ties < TN)).any()), 'no partial tie'
            assert bool((ties == TN).any()) or cs['p'] > 0, 'no padded agent whose 11 steps tie'
        f = prepare(cs, dt, 'enc_fwd')
        share, which = max(_zero_share(p, ('dpre_s', 'dout', 'dqkv')), _zero_share(f, ('enc', 's_nodes', 's_qkv', 's_att', 's_cat')))
        assert share <= 0.05, f'{name} {dt}: the twin equals float64 in {share:.3f} of the rows of {which}'


@pytest.mark.parametrize('name', [c['name'] for c in AC.int_cases()])
def test_interaction_inputs_exercise_the_block(name):
    cs = case(name)
    for dt in DT16:
        p = prepare(cs, dt, 'int_bwd')
        R, cm = p.R, p.I['cm']
        rows = cm[:, None, :, None].expand(-1, IH, -1, -1) & (cm.sum(1) > 2)[:, None, None, None]
        if bool(rows.any()):
            peak = float(R['_P'].max(-1, keepdim=True).values[rows].mean())
            assert 0.05 <= peak <= 0.7, f'{name}: mean max_key P = {peak:.3f}: the attention is uniform or one-hot'
        pos = float((R['_pre1'] > 0).double().mean())
        assert 0.2 <= pos <= 0.8, f'{name}: {pos:.2f} of the FFN1 pre-activations are positive'
        f = prepare(cs, dt, 'int_fwd')
        # s_concat is a masked COPY of enc, and s_qin of a masked agent a copy of its seg_embed row: the twin is exact there by construction,
        # and so is the judge's bound (the f32 term alone)
        share, which = max(_zero_share(p, AC.INT_DY + ('ws_dn1', 'd_enc')),
                           _zero_share(f, ('key', 'ws_v1', 'ws_u2') + tuple(n for n in AC.INT_SAVES if n != 's_concat'), {'s_qin': cm.reshape(-1)}))
        assert share <= 0.05, f'{name} {dt}: the twin equals float64 in {share:.3f} of the rows of {which}'
