"""The fused agent-branch entry points (csrc/agent_fused.hip: stj_agent_pack, stj_agent_enc_fwd / _bwd, stj_agent_int_fwd / _bwd) through the
raw C ABI against the float64 statement of _agent_cases.py: float32, bf16 and fp16 for the pack and the encoder, bf16 and fp16 for the
interaction block (it has no f32 form).

Every call takes raw pointers into flat buffers (ops.call; lib() where a status other than STJ_OK is expected).  Cases, layout, references
and the judge are in _agent_cases.py and are themselves tested on the CPU by test_agent_ref.py; this module builds no model.
What is judged, per output tensor and per ROW: see the docstring of _agent_cases.py.  In short: f32 rows within 2e-5 (forward) / 3e-4
(backward) of float64; 16-bit rows within twice the distance of the rounding twin from float64 plus that; every byte that is no output
bit-identical (inputs, guards, parameters); no output element left unwritten -- the slab workspaces included, which enter every call filled
with the NaN pattern; cmi exact; the tie bits s_pmask admissible (16 bit) or equal to float64's tie sets (f32).
The keep masks are the ones stj_dropout_mask states for the draw shapes [agents][4][11][11], [B][6][64][64], [B 64][1536], [B 64][384].
Each backward is judged on its own (handed the saves -- and, for the encoder, the tie sets -- of the float64 reference, rounded to dt), and
once more behind its forward kernel (the encoder then against float64 evaluated with the tie sets that kernel reported).

profiles/test_agent_abi_ratios.txt is the record of one run of this module: the largest ||err|| / bound per (entry point, dtype, output)
as test_zz_report prints it.
"""
import ctypes

import pytest
import torch

import _agent_cases as AC
from _agent_cases import CB, DT16, DTYPES, ENC_GRADS, ENC_SAVES, F32, GUARD, INT_DY, INT_GRADS, INT_SAVES, LAY, TN, judge, prepare
from test_gemm_gpu import bits, pattern

pytestmark = pytest.mark.gpu

_RATIOS = []
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
SITE_E, SITES = 2, (3, 5, 11)          # site ids of the encoder's attention dropout and of the interaction block's three
SEED_STEP = (20240611, 7)


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


_STATE, _MASKS = [], {}


def rng_state():
    if not _STATE:
        _STATE.append(torch.tensor(SEED_STEP, dtype=torch.int64, device='cuda'))
    return _STATE[0]


def gpu_masks(cs):
    """the keep masks the header names as the statement of the draw: stj_dropout_mask over the draw shapes"""
    from strajnet_amd import ops
    if not cs['p'] > 0:
        return None
    if cs['name'] not in _MASKS:
        m = {}
        sites = (SITE_E,) if cs['block'] == 'enc' else SITES
        for (key, shape), site in zip(AC.draw_shapes(cs).items(), sites):
            n = 1
            for d in shape:
                n *= d
            t = torch.empty(n, dtype=torch.uint8, device='cuda')
            ops.call('stj_dropout_mask', ops._p(t), n, float(cs['p']), ops._p(rng_state()), site, ops._st())
            m[key] = t.cpu().reshape(shape)
            assert 0.5 * cs['p'] < 1.0 - float(m[key].float().mean()) < 1.5 * cs['p'], (cs['name'], key)
        _MASKS[cs['name']] = m
    return _MASKS[cs['name']]


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def upload(p):
    return {k: b.init.cuda() for k, b in p.bufs.items()}


def download(dev):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def addr(t, elems=0):
    """device address `elems` elements past the guard of a flat buffer"""
    return t.data_ptr() + (GUARD + elems) * t.element_size()


def make_pack(dev, dt):
    """stj_agent_pack of the masters in dev['params'] into GUARD | pack | GUARD (elements of dt); returns the device buffer"""
    from strajnet_amd import ops
    from strajnet_amd._lib import AgentWeights
    buf = pattern(GUARD + AC.PACK_ELEMS + GUARD, dt).cuda()
    aw = AgentWeights(*[addr(dev['params'], LAY[k][0]) for k in AC.PACK_KEYS])
    ops.call('stj_agent_pack', ctypes.byref(aw), ops.vp(addr(buf)), ops.DTYPE_CODE[dt], ops._st())
    return buf


def fields(p, dev, pack):
    """field name -> value of the argument block of the call a Prep describes (device addresses as int, None for a NULL pointer)"""
    from strajnet_amd import ops
    cs = p.cs
    par = lambda n: addr(dev['params'], LAY[n][0])
    nat = lambda n: addr(dev['wnat'], LAY[n][0])
    grd = lambda n: addr(dev['grads'], LAY[n][0]) if 'grads' in dev else None
    own = lambda n: addr(dev[n]) if n in dev else None
    v = dict(n_obs=cs['n_obs'], n_occ=cs['n_occ'], B=cs['B'], dtype=ops.DTYPE_CODE[p.dt], pack=addr(pack), rng_state=rng_state().data_ptr() if cs['p'] > 0 else None,
             p_drop=float(cs['p']), enc=own('enc'), cmi=own('cmi'))
    if cs['block'] == 'enc':
        v.update(obs=own('obs'), occ=own('occ'), wn=par('wn'), bn=par('bn'), wv3=par('wv3'), bo=par('e_bo'), bs=par('e_bs'), site=SITE_E)
        v.update({n: own(n) for n in ENC_SAVES})
        if p.kind == 'enc_bwd':
            v.update(d_enc=own('d_enc'), d_enc_f32=p.d_enc_mode, wq=nat('e_wq'), wk=nat('e_wk'), wv=nat('e_wv'), wo=nat('e_wo'), ws=nat('e_ws'),
                     dpre_s=own('dpre_s'), dout=own('dout'), dqkv=own('dqkv'), dwn=grd('wn'), dbn=grd('bn'), dwv3=grd('wv3'))
    else:
        v.update(seg=own('seg'), bo=par('i_bo'), site_a=SITES[0], site_1=SITES[1], site_2=SITES[2], key=own('key'), ws_v1=own('ws_v1'), ws_u2=own('ws_u2'))
        v.update({n: par(n) for n in ('g1', 'be1', 'b1', 'b2', 'g2', 'be2', 'g_obs', 'b_obs', 'g_occ', 'b_occ')})
        v.update({n: own(n) for n in INT_SAVES})
        if p.kind == 'int_bwd':
            v.update(dkey=own('dkey'), wq=nat('i_wq'), wk=nat('i_wk'), wv=nat('i_wv'), wo=nat('i_wo'), w1=nat('i_w1'), w2=nat('i_w2'), d_enc=own('d_enc'),
                     ws_dn1=own('ws_dn1'))
            v.update({n: own(n) for n in INT_DY})
            v.update({n: grd(src) for n, src in INT_GRADS.items()})
    return v


ENTRY = dict(enc_fwd='stj_agent_enc_fwd', enc_bwd='stj_agent_enc_bwd', int_fwd='stj_agent_int_fwd', int_bwd='stj_agent_int_bwd')


def launch(p, v, raw=False, null_block=False):
    from strajnet_amd import ops
    from strajnet_amd._lib import AgentEncArgs, AgentIntArgs, lib
    a = (AgentEncArgs if p.cs['block'] == 'enc' else AgentIntArgs)(**v)
    ref = None if null_block else ctypes.byref(a)
    if raw:
        return getattr(lib(), ENTRY[p.kind])(ref, ops._st())
    ops.call(ENTRY[p.kind], ref, ops._st())


def run(p):
    """upload, pack, call; returns the flat buffers as the call left them"""
    dev = upload(p)
    pack = make_pack(dev, p.dt)
    state = rng_state().clone()
    launch(p, fields(p, dev, pack))
    after = download(dev)
    assert torch.equal(state, rng_state()), 'the call changed the random state'
    return after


def run_cases(dt, cases, body):
    failed = []
    for cs in cases:
        try:
            body(cs, dt)
        except AssertionError as e:
            failed.append(f"{cs['name']} [{dt}]: {e}")
    assert not failed, f'{len(failed)} of {len(cases)} cases failed:\n' + '\n'.join(failed)


# ---- stj_agent_pack -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_pack(dt):
    """the eleven transposed copies, rounded to dt, at the stated offsets and nothing else; the stated size; masters and guards untouched"""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    es = torch.empty(0, dtype=dt).element_size()
    assert int(lib().stj_agent_pack_workspace_bytes(ops.DTYPE_CODE[dt])) == AC.PACK_ELEMS * es
    p = prepare(AC.case('e1_1_1'), dt, 'enc_fwd')
    dev = upload(p)
    got = make_pack(dev, dt)
    torch.cuda.synchronize()
    want = pattern(got.numel(), dt)
    want[GUARD:GUARD + AC.PACK_ELEMS] = AC.pack_image(AC.params(), dt)
    ne = (bits(got.cpu()) != bits(want)).nonzero()
    assert ne.numel() == 0, f'{ne.numel()} elements of the pack buffer differ from the stated layout, first at {int(ne[0]) - GUARD}'
    assert torch.equal(bits(dev['params'].cpu()), bits(p.bufs['params'].init))


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_enc_forward(dt):
    """training form (the five saves) and inference form (none, and nothing else written): every output row against float64, cmi exactly
    (the x = 2^-26 step of the `tiny` tracks is a valid step in every dtype), the tie bits; enc is bit-equal in both forms.
    (With step validity taken from the ROUNDED x, as the kernels had it, fp16 fails five of the seven cases here: enc rows of the `tiny`
    and `tinyonly` agents land 1e2 .. 9e2 bounds away; f32 and bf16 hold 2^-26 and pass either way.)"""
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'enc_fwd', m, 'gpu')
        after = run(p)
        judge(p, after, _RATIOS)
        q = prepare(cs, dt, 'enc_fwd', m, 'gpu', with_saves=False)
        bare = run(q)
        judge(q, bare, _RATIOS)
        assert torch.equal(bits(bare['enc']), bits(after['enc'])), 'enc of the inference form differs from the training form'
    run_cases(dt, AC.enc_cases(), body)


@pytest.mark.parametrize('mode', [0, 1, 7])
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_enc_backward_on_reference_saves(dt, mode):
    """stj_agent_enc_bwd alone: saves and tie sets of float64 (rounded to dt); d_enc in dt (mode 0) or as 1 / 7 f32 slabs"""
    def body(cs, dt):
        p = prepare(cs, dt, 'enc_bwd', gpu_masks(cs), 'gpu', d_enc_mode=mode)
        judge(p, run(p), _RATIOS, label=f' (d_enc_f32 = {mode})')
    run_cases(dt, AC.enc_cases(), body)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_enc_forward_into_backward(dt):
    """the backward kernel on what the forward kernel saved; float64 takes the tie sets that kernel reported (found admissible first)"""
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'enc_fwd', m, 'gpu')
        after = run(p)
        judge(p, after)
        saves = {n: AC.logical(p, after, n) for n in ('enc', 'cmi') + ENC_SAVES}
        tie = AC.pmask_tie(saves['s_pmask'].to(torch.int32) & 0xffff)
        q = prepare(cs, dt, 'enc_bwd', m, 'gpu', d_enc_mode=7, saves_from=saves, tie=tie, tie_tag='kernel')
        judge(q, run(q), _RATIOS, label=' (behind the forward kernel)')
    run_cases(dt, [AC.case(n) for n in ('e2_3_5_p0', 'e2_3_5_p0.1', 'e3_48_16_p0')], body)


# ---- the interaction block ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DT16, ids=str)
def test_int_forward(dt):
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'int_fwd', m, 'gpu')
        after = run(p)
        judge(p, after, _RATIOS)
        q = prepare(cs, dt, 'int_fwd', m, 'gpu', with_saves=False)
        bare = run(q)
        judge(q, bare, _RATIOS)
        assert torch.equal(bits(bare['key']), bits(after['key'])), 'key of the inference form differs from the training form'
    run_cases(dt, AC.int_cases(), body)


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_int_backward_on_reference_saves(dt):
    def body(cs, dt):
        p = prepare(cs, dt, 'int_bwd', gpu_masks(cs), 'gpu')
        judge(p, run(p), _RATIOS)
    run_cases(dt, AC.int_cases(), body)


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_int_forward_into_backward(dt):
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'int_fwd', m, 'gpu')
        after = run(p)
        judge(p, after)
        saves = {n: AC.logical(p, after, n) for n in INT_SAVES}
        q = prepare(cs, dt, 'int_bwd', m, 'gpu', saves_from=saves)
        judge(q, run(q), _RATIOS, label=' (behind the forward kernels)')
    run_cases(dt, [AC.case(n) for n in ('i37_p0', 'i37_p0.1')], body)


# ---- properties -------------------------------------------------------------------------------------------------------------------------------
WRITTEN = dict(enc_fwd=('enc', 'cmi') + ENC_SAVES, enc_bwd=('dpre_s', 'dout', 'dqkv'), int_fwd=('key', 'ws_v1', 'ws_u2') + INT_SAVES,
               int_bwd=INT_DY + ('ws_dn1',))


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_repeatable(dt):
    """two identical calls: everything the kernels WRITE is bit-identical (no atomics on activations) -- key, every save, every dY, and the
    gradient of enc as the fixed-order f32 sum of its seven slabs; the small gradients accumulated with atomics are not compared"""
    for cs, kind, mode in ((AC.case('e2_3_5_p0.1'), 'enc_fwd', 0), (AC.case('e2_3_5_p0.1'), 'enc_bwd', 7), (AC.case('i37_p0.1'), 'int_fwd', 0),
                           (AC.case('i37_p0.1'), 'int_bwd', 0)):
        if cs['block'] == 'int' and dt == F32:
            continue
        p = prepare(cs, dt, kind, gpu_masks(cs), 'gpu', d_enc_mode=mode)
        a, b = run(p), run(p)
        for n in WRITTEN[kind]:
            assert torch.equal(bits(a[n]), bits(b[n])), f'{kind}: {n} differs between two identical calls'
        if kind == 'int_bwd':
            N = cs['B'] * cs['A']
            total = lambda t: sum(t[GUARD:GUARD + 7 * N * CB].reshape(7, N * CB)[i] for i in range(7))
            assert torch.equal(bits(total(a['d_enc'])), bits(total(b['d_enc']))), 'int_bwd: the sum of the d_enc slabs differs between two identical calls'


def test_status_codes():
    """Every refusal comes from the host checks in front of the launch, leaves every buffer bit-identical and a message in stj_last_error();
    B = 0 is STJ_OK and writes nothing."""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    L = lib()
    F32C = ops.DTYPE_CODE[F32]
    table = {
        'enc_fwd': [(dict(n_obs=4), EUNSUPPORTED), (dict(n_obs=0, n_occ=0), EUNSUPPORTED), (dict(dtype=7), EUNSUPPORTED), (dict(p_drop=1.0), EINVAL),
                    (dict(p_drop=-0.5), EINVAL), (dict(s_att=None), EINVAL), (dict(s_pmask=None, s_cat=None), EINVAL), (dict(obs=None), EINVAL), (dict(occ=None), EINVAL),
                    (dict(enc=None), EINVAL), (dict(cmi=None), EINVAL), (dict(pack=None), EINVAL), (dict(bo=None), EINVAL), (dict(bs=None), EINVAL), (dict(B=0), OK)],
        'enc_bwd': [(dict(n_occ=4), EUNSUPPORTED), (dict(p_drop=1.0), EINVAL), (dict(d_enc=None), EINVAL), (dict(s_pmask=None), EINVAL), (dict(s_qkv=None), EINVAL),
                    (dict(ws=None), EINVAL), (dict(dout=None), EINVAL), (dict(dwv3=None), EINVAL), (dict(B=0), OK), (dict(B=-1), OK)],
        'int_fwd': [(dict(n_obs=36), EUNSUPPORTED), (dict(n_occ=28), EUNSUPPORTED), (dict(dtype=F32C), EUNSUPPORTED), (dict(p_drop=1.0), EINVAL), (dict(s_h=None), EINVAL),
                    (dict(s_concat=None, s_out=None), EINVAL), (dict(enc=None), EINVAL), (dict(cmi=None), EINVAL), (dict(seg=None), EINVAL), (dict(key=None), EINVAL),
                    (dict(pack=None), EINVAL), (dict(ws_v1=None), EINVAL), (dict(ws_u2=None), EINVAL), (dict(b1=None), EINVAL), (dict(B=0), OK)],
        'int_bwd': [(dict(n_obs=38), EUNSUPPORTED), (dict(dtype=F32C), EUNSUPPORTED), (dict(p_drop=2.0), EINVAL), (dict(s_n1=None), EINVAL), (dict(dkey=None), EINVAL),
                    (dict(d_enc=None), EINVAL), (dict(ws_dn1=None), EINVAL), (dict(dpre1=None), EINVAL), (dict(dseg=None), EINVAL), (dict(w2=None), EINVAL), (dict(B=0), OK)],
    }
    for kind, rows in table.items():
        cs = AC.case('e2_3_5_p0.1' if kind.startswith('enc') else 'i37_p0.1')
        p = prepare(cs, torch.bfloat16, kind, gpu_masks(cs), 'gpu', d_enc_mode=7 if kind == 'enc_bwd' else 0)
        dev = upload(p)
        pack = make_pack(dev, p.dt)
        torch.cuda.synchronize()
        pack0 = pack.cpu()
        v = fields(p, dev, pack)
        for over, want in rows:
            rc = launch(p, dict(v, **over), raw=True)
            assert rc == want, (kind, over, rc, want)
            if want != OK:
                assert L.stj_last_error(), (kind, over)
            after = download(dev)
            for n, b in p.bufs.items():
                assert torch.equal(bits(after[n]), bits(b.init)), (kind, over, n)
            assert torch.equal(bits(pack.cpu()), bits(pack0)), (kind, over, 'pack')
        assert launch(p, v, raw=True, null_block=True) == EINVAL
        # the unmodified argument block is legal
        assert launch(p, v, raw=True) == OK
        judge(p, download(dev))
    # stj_agent_pack: NULL block, NULL output, a NULL weight, a bad dtype
    from strajnet_amd._lib import AgentWeights
    ptrs = [addr(dev['params'], LAY[k][0]) for k in AC.PACK_KEYS]
    code = ops.DTYPE_CODE[torch.bfloat16]
    aw = AgentWeights(*ptrs)
    assert L.stj_agent_pack(None, ops.vp(addr(pack)), code, ops._st()) == EINVAL
    assert L.stj_agent_pack(ctypes.byref(aw), None, code, ops._st()) == EINVAL
    assert L.stj_agent_pack(ctypes.byref(aw), ops.vp(addr(pack)), 7, ops._st()) == EINVAL
    for i in (0, 4, 10):
        bad = AgentWeights(*[None if j == i else q for j, q in enumerate(ptrs)])
        assert L.stj_agent_pack(ctypes.byref(bad), ops.vp(addr(pack)), code, ops._st()) == EINVAL and L.stj_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(pack.cpu()), bits(pack0))
    for a, b, t, want in ((3, 5, TN, 1), (3, 4, TN, 0), (0, 0, TN, 0), (3, 5, 10, 0), (0, 2, TN, 1)):
        assert L.stj_agent_enc_supported(a, b, t, code) == want
    for a, b, c, want in ((37, 27, code, 1), (0, 64, code, 1), (32, 31, code, 0), (48, 16, F32C, 0)):
        assert L.stj_agent_int_supported(a, b, c) == want


def test_zz_report_agent_error_ratios():
    """(runs last in this file) the largest ||err|| / bound per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(AC.report_lines(_RATIOS, 'agent abi')))
