"""The fused Swin entry points (csrc/swin_fused.hip: stj_swin_mlp_fwd / _bwd, stj_swin_attn_fwd / _bwd and their finishing launches) through
the raw C ABI, per dispatch path, for float32, bf16 and fp16, against the float64 statement of _swin_cases.py.

Every call takes raw pointers into flat buffers (ops.call; lib() where a status other than STJ_OK is expected).  Cases (with the table of the
template instantiation each one selects), layout, references and the judge are in _swin_cases.py and are themselves tested on the CPU by
test_swin_ref.py; this module builds no model.  What is judged, per output tensor and per ROW: see the docstring of _swin_cases.py.
The DropPath keep flags are the ones stj_dropout_mask(ndraw = B) states at the same (state, site); the site of a case is the first one at
which a sample is kept and one dropped.  The split workspace of a (M, C) is allocated with exactly stj_swin_split_workspace_bytes bytes
between guards, zeroed ONCE and then reused by every call of the module at that (M, C); after every call its last 16384 bytes (the
arrival counters) are zero again and its guards untouched.
The attention backward is judged on the reference's saves (qkv rounded to dt, mean / rstd in f32) and once more behind the forward kernel,
then with the other of nparts / tparts in {1, 3}; the MLP backward reads no saves and runs a second time with the other nparts.

profiles/test_swin_abi_ratios.txt is the record of one run of this module (test_zz_report_swin_error_ratios), profiles/test_swin_abi_kernels.txt
the distinct swin_* kernels one run of it launched.
"""
import pytest
import torch

import _swin_cases as SC
from _swin_cases import ADDED, F32, GUARD, judge, prepare
from test_gemm_gpu import bits, pattern

pytestmark = pytest.mark.gpu

_RATIOS = []
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
SEED_STEP = (20240611, 7)
FIX_CNT_BYTES = 16384
ORDER = {
    ('mlp', 'fwd'): ('stj_swin_mlp_fwd', ('x', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2', 'y', 'M', 'C', 'eps', 'rng', 'site', 'p_drop', 'rps', 'dtype', 'ws', 'stream')),
    ('mlp', 'bwd'): ('stj_swin_mlp_bwd', ('x', 'dy', 'gamma', 'beta', 'w1', 'b1', 'w2', 'dx', 'h', 'dpre', 'ln', 'dys', 'dgamma', 'dbeta', 'nparts', 'pstride', 'M', 'C',
                                          'eps', 'rng', 'site', 'p_drop', 'rps', 'dtype', 'ws', 'stream')),
    ('attn', 'fwd'): ('stj_swin_attn_fwd', ('x', 'gamma', 'beta', 'wqkv', 'bqkv', 'table', 'wproj', 'bproj', 'y', 'qkv', 'a', 'ln', 'mean', 'rstd', 'B', 'res', 'C', 'shift',
                                            'eps', 'rng', 'site', 'p_drop', 'dtype', 'ws', 'stream')),
    ('attn', 'bwd'): ('stj_swin_attn_bwd', ('x', 'dy', 'qkv', 'mean', 'rstd', 'gamma', 'wqkv', 'wproj', 'table', 'dx', 'dqkv', 'dys', 'dtable', 'tparts', 'dgamma', 'dbeta',
                                            'nparts', 'pstride', 'B', 'res', 'C', 'shift', 'rng', 'site', 'p_drop', 'dtype', 'ws', 'stream')),
}
POINTERS = ('x', 'dy', 'gamma', 'beta', 'w1', 'b1', 'w2', 'b2', 'wqkv', 'bqkv', 'table', 'wproj', 'bproj', 'y', 'qkv', 'a', 'ln', 'mean', 'rstd', 'dx', 'h', 'dpre',
            'dys', 'dqkv', 'dtable', 'dgamma', 'dbeta')


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


_STATE, _KEEP, _WS = [], {}, {}


def rng_state():
    if not _STATE:
        _STATE.append(torch.tensor(SEED_STEP, dtype=torch.int64, device='cuda'))
    return _STATE[0]


def gpu_keep(cs):
    """(keep flags [B] as stj_dropout_mask states them, site): the first site that keeps one sample and drops one; (None, 1) without DropPath"""
    from strajnet_amd import ops
    if not cs['p'] > 0:
        return None, 1
    if cs['name'] not in _KEEP:
        for site in range(1, 64):
            t = torch.empty(cs['B'], dtype=torch.uint8, device='cuda')
            ops.call('stj_dropout_mask', ops._p(t), cs['B'], float(cs['p']), ops._p(rng_state()), site, ops._st())
            k = t.cpu()
            if 0 < int(k.sum()) < cs['B']:
                _KEEP[cs['name']] = (k, site)
                break
    return _KEEP[cs['name']]


def workspace(cs):
    """the device workspace of the case's (M, C): GUARD | exactly stj_swin_split_workspace_bytes | GUARD floats, zeroed when first made; or None"""
    from strajnet_amd._lib import lib
    nbytes = int(lib().stj_swin_split_workspace_bytes(cs['M'], cs['C']))
    if not cs['ws'] or nbytes == 0:
        return None
    key = (cs['M'], cs['C'])
    if key not in _WS:
        assert nbytes % 16 == 0 and nbytes > FIX_CNT_BYTES
        t = pattern(GUARD + nbytes // 4 + GUARD, F32)
        t[GUARD:-GUARD] = 0
        _WS[key] = t.cuda()
    return _WS[key]


def check_workspace(ws, label):
    if ws is None:
        return
    torch.cuda.synchronize()
    cnt = ws[-GUARD - FIX_CNT_BYTES // 4:-GUARD].cpu()
    assert not bool((bits(cnt) != 0).any()), f'{label}: {int((bits(cnt) != 0).sum())} arrival counters are not zero after the call'
    for g in (ws[:GUARD].cpu(), ws[-GUARD:].cpu()):
        assert torch.equal(bits(g), bits(pattern(GUARD, F32))), f'{label}: a guard of the workspace changed'


def upload(p):
    return {k: b.init.cuda() for k, b in p.bufs.items()}


def download(dev):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def arguments(p, dev, ws, site):
    from strajnet_amd import ops
    cs = p.cs
    v = {k: (ops._poff(dev[k], GUARD) if k in dev else None) for k in POINTERS}
    v.update(M=cs['M'], C=cs['C'], eps=SC.EPS, rng=ops._p(rng_state()), site=site, p_drop=float(cs['p']), rps=cs['rps'], dtype=ops.DTYPE_CODE[p.dt],
             ws=ops._poff(ws, GUARD) if ws is not None else None, stream=ops._st(), nparts=p.nparts, tparts=p.tparts, pstride=p.pstride, B=cs['B'],
             res=cs.get('res'), shift=cs.get('shift'))
    return v


def launch(p, v, raw=False):
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    name, order = ORDER[p.cs['half'], p.kind]
    args = [ops._p(v[k]) if (v[k] is None or isinstance(v[k], ops.vp)) else v[k] for k in order]
    if raw:
        return getattr(lib(), name)(*args)
    ops.call(name, *args)


def run(p, edit=None, **over):
    """upload, call, download; the workspace contract is checked behind every call.  edit(dev): changes to the uploaded buffers;
    over: arguments replaced"""
    _, site = gpu_keep(p.cs)
    dev, ws = upload(p), workspace(p.cs)
    if edit is not None:
        edit(dev)
    state = rng_state().clone()
    launch(p, dict(arguments(p, dev, ws, site), **over))
    after = download(dev)
    assert torch.equal(state, rng_state()), 'the call changed the random state'
    check_workspace(ws, f"{p.cs['name']} {p.kind}")
    return after


def same_activations(p, a, b, what):
    """every written (not "+=") output bit-identical in two results"""
    for n in p.outs:
        if n not in ADDED:
            assert torch.equal(bits(a[n]), bits(b[n])), f"{p.cs['name']} {p.kind}: {n} differs {what}"


def other(n):
    return 4 - n          # 1 <-> 3


# ---- the case families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dt', SC.CASE_DT, ids=SC.case_id)
def test_forward(name, dt):
    """every output row against float64; the same call again on the un-rezeroed workspace is bit-identical; the attention's inference form
    (no saves) gives the same y bit for bit"""
    cs = SC.case(name)
    keep, _ = gpu_keep(cs)
    p = prepare(cs, dt, 'fwd', keep, 'gpu')
    after = run(p)
    judge(p, after, _RATIOS)
    same_activations(p, after, run(p), 'between two calls on one workspace')
    if cs['half'] == 'attn':
        q = prepare(cs, dt, 'fwd', keep, 'gpu', with_saves=False)
        bare = run(q)
        judge(q, bare, _RATIOS)
        assert torch.equal(bits(bare['y']), bits(after['y'])), 'y of the inference form differs from the training form'


@pytest.mark.parametrize('name,dt', SC.CASE_DT, ids=SC.case_id)
def test_backward_on_reference_saves(name, dt):
    cs = SC.case(name)
    keep, _ = gpu_keep(cs)
    p = prepare(cs, dt, 'bwd', keep, 'gpu')
    after = run(p)
    judge(p, after, _RATIOS)
    same_activations(p, after, run(p), 'between two calls on one workspace')


@pytest.mark.parametrize('name,dt', [(n, dt) for n, dt in SC.CASE_DT if SC.small(SC.case(n))], ids=SC.case_id)
def test_forward_into_backward(name, dt):
    """attention: the backward kernel on what the forward kernel saved, against the end-to-end twin; both halves: the other nparts / tparts"""
    cs = SC.case(name)
    keep, _ = gpu_keep(cs)
    saves = None
    if cs['half'] == 'attn':
        p = prepare(cs, dt, 'fwd', keep, 'gpu')
        after = run(p)
        judge(p, after)
        saves = {n: SC.copies(p, after, n)[0] for n in ('qkv', 'mean', 'rstd')}
    q = prepare(cs, dt, 'bwd', keep, 'gpu', saves_from=saves, nparts=other(cs['nparts']), tparts=other(cs['tparts']))
    judge(q, run(q), _RATIOS, label=' (behind the forward kernel)' if saves else ' (other nparts)')


BLOCKS = [(SC.acase('blk384_a', 384, 2, 16, 4, nparts=3, tparts=3), SC.mcase('blk384_m', 384, 512, rps=256, nparts=3)),
          (SC.acase('blk192_a', 192, 2, 32, 4, nparts=3, tparts=3), SC.mcase('blk192_m', 192, 2048, rps=1024, nparts=3))]


@pytest.mark.parametrize('dt', SC.ALL3, ids=SC.case_id)
@pytest.mark.parametrize('pair', BLOCKS, ids=lambda b: b[0]['name'])
def test_block_shares_one_workspace(pair, dt):
    """one block's four calls -- attention forward, MLP forward, MLP backward, attention backward -- on ONE workspace in stream order with no
    host synchronisation in between, each judged"""
    ca, cm = pair
    assert ca['M'] == cm['M'] and ca['C'] == cm['C']
    ws = workspace(ca)
    assert ws is not None and ws is workspace(cm)
    calls = [prepare(ca, dt, 'fwd'), prepare(cm, dt, 'fwd'), prepare(cm, dt, 'bwd'), prepare(ca, dt, 'bwd')]
    devs = [upload(p) for p in calls]
    torch.cuda.synchronize()
    for p, dev in zip(calls, devs):
        launch(p, arguments(p, dev, ws, 1))
    for p, dev in zip(calls, devs):
        judge(p, download(dev), _RATIOS)
    check_workspace(ws, ca['name'])


@pytest.mark.parametrize('name,dt', [(n, dt) for n in ('m96_3x80_p', 'm192_3x80_p', 'm384_3x80_p', 'a96_3_16_4_p', 'a192_2_16_4', 'a384_52w_p', 'a384_2_16_4')
                                     for dt in SC.case(n)['dts']], ids=SC.case_id)
def test_samples_are_independent(name, dt):
    """other values in sample 1's x leave sample 0's rows of every written output bit-identical (in the 3 x 80-row MLP cases the two samples
    share a 64-row block)"""
    cs = SC.case(name)
    keep, _ = gpu_keep(cs)
    lo, hi = GUARD + cs['rps'] * cs['C'], GUARD + 2 * cs['rps'] * cs['C']

    def edit(dev):
        dev['x'][lo:hi] = (dev['x'][lo:hi].float() * 0.5 + 1.0).to(dev['x'].dtype)

    for kind in ('fwd', 'bwd'):
        p = prepare(cs, dt, kind, keep, 'gpu')
        a, b = run(p), run(p, edit)
        assert not torch.equal(bits(a['x']), bits(b['x']))
        for n in p.outs:
            if n not in ADDED:
                w = p.outs[n][3]
                s0 = slice(GUARD, GUARD + cs['rps'] * w)
                assert torch.equal(bits(a[n][s0]), bits(b[n][s0])), f'{name} {kind}: sample 0 of {n} depends on sample 1 of x'


@pytest.mark.parametrize('name,dt', [(n, dt) for n in ('m96_80', 'm192_80', 'm384_80', 'a96_1_8_4', 'a192_2_16_4', 'a384_1_8_4') for dt in SC.case(n)['dts']],
                         ids=SC.case_id)
def test_dys_may_be_null_without_droppath(name, dt):
    """the header: dys may be NULL when there is no DropPath -- every other output is bit-identical to the call that writes dys"""
    cs = SC.case(name)
    p = prepare(cs, dt, 'bwd')
    a, b = run(p), run(p, dys=None)
    assert torch.equal(bits(b['dys']), bits(p.bufs['dys'].init)), 'dys = NULL, yet the buffer changed'
    for n in p.outs:
        if n not in ADDED and n != 'dys':
            assert torch.equal(bits(a[n]), bits(b[n])), f'{name}: {n} depends on whether dys is written'


def test_status_codes():
    """Every refusal comes from the host checks in front of the launch, leaves every buffer bit-identical and a message in stj_last_error();
    M <= 0 and B <= 0 are STJ_OK and write nothing."""
    from strajnet_amd._lib import lib
    L = lib()
    for M, C, want in ((80, 96, 0), (32768, 192, 0), (80, 192, 2 * 128 * 192 * 4 + FIX_CNT_BYTES), (8272, 384, 8 * 8320 * 384 * 4 + FIX_CNT_BYTES)):
        assert L.stj_swin_split_workspace_bytes(M, C) == want, (M, C)
    for name, dt in (('m96_80', F32), ('m192_80', torch.bfloat16), ('m384_80', torch.float16), ('a96_1_8_0', F32), ('a192_2_16_4', torch.bfloat16),
                     ('a384_1_8_4', torch.float16), ('a384_1_8_4', F32)):
        cs = SC.case(name)
        for kind in ('fwd', 'bwd'):
            p = prepare(cs, dt, kind)
            dev, ws = upload(p), workspace(cs)
            ws0 = ws.cpu() if ws is not None else None
            v = arguments(p, dev, ws, 1)
            refused = [(dict(C=128), EUNSUPPORTED), (dict(dtype=7), EINVAL), (dict(p_drop=1.0), EINVAL), (dict(p_drop=-0.1), EINVAL)]
            if cs['half'] == 'mlp':
                refused += [(dict(rps=cs['M'] + 8), EINVAL), (dict(rps=0), EINVAL)]
            else:
                refused += [(dict(shift=8), EINVAL), (dict(shift=-1), EINVAL), (dict(res=cs['res'] + 4), EINVAL)]
                if kind == 'fwd':
                    refused += [({n: None}, EINVAL) for n in ('qkv', 'a', 'ln', 'mean', 'rstd')]
                else:
                    refused += [(dict(tparts=0), EINVAL)]
            if kind == 'bwd':
                refused += [(dict(nparts=0), EINVAL), (dict(nparts=-2), EINVAL)]
            if cs['C'] == 384:
                refused += [(dict(ws=None), EINVAL)]
            nothing = [dict(M=0), dict(M=-5)] if cs['half'] == 'mlp' else [dict(B=0), dict(B=-1)]
            for over, want in refused + [(o, OK) for o in nothing]:
                rc = launch(p, dict(v, **over), raw=True)
                assert rc == want, (name, kind, dt, over, rc, want)
                if want != OK:
                    assert L.stj_last_error(), (name, kind, over)
                after = download(dev)
                for n, b in p.bufs.items():
                    assert torch.equal(bits(after[n]), bits(b.init)), (name, kind, dt, over, n)
                if ws is not None:
                    assert torch.equal(bits(ws.cpu()), bits(ws0)), (name, kind, dt, over, 'workspace')
            # the unmodified argument list is legal
            assert launch(p, v, raw=True) == OK
            judge(p, download(dev))
            check_workspace(ws, name)


def test_zz_report_swin_error_ratios():
    """(runs last in this file) the largest ||err|| / bound per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(SC.report_lines(_RATIOS, 'swin abi')))
