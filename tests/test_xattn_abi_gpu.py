"""The fused Cross_AttentionT entry points (csrc/xattn_fused.hip: stj_xattn_pack, stj_xattn_fwd, stj_xattn_bwd with its dk / dv tile
reduction) through the raw C ABI, for float32, bf16 and fp16, against the float64 statement of _xattn_cases.py.

Every call takes raw pointers into flat buffers (ops.call; lib() where a status other than STJ_OK is expected).  Cases, layout, references
and the judge are in _xattn_cases.py and are themselves tested on the CPU by test_xattn_ref.py; this module builds no model.
What is judged, per output tensor and per ROW (a token, a key, one weight set's vector): see the docstring of _xattn_cases.py.  In short:
f32 rows within 2e-5 (forward) / 2e-4 (backward) of float64; 16-bit rows within twice the distance of the rounding twin from float64 plus
that; every byte that is no output bit-identical (inputs, guards, the gaps between weight sets); no output element left unwritten; the pad
columns 42..47 of sq / so / dq and the dk / dv rows of masked keys exactly zero.
The keep masks of the three dropout sites are the ones stj_dropout_mask states for the draw shapes [Z,B,3,HW,64], [Z,B*HW,512],
[Z,B*HW,384]; the weight stream is made by stj_xattn_pack into a guarded buffer of Z streams plus the tail.
Backward is judged on its own (it is handed sq, sv1, su2 of the float64 reference, rounded to dt), and once more behind the forward kernel.

profiles/test_xattn_abi_ratios.txt is the record of one run of this module: the largest ||err|| / bound per (entry point, dtype, output)
as test_zz_report prints it.

COUPLING: pack_image() restates the stream layout of xat::Geo<T> (chunk sizes and padded row strides).  Retuning that layout fails
test_pack_tail_content_is_not_consumed for a reason that is no error of the kernels: update pack_image with it.
"""
import ctypes

import pytest
import torch

import _xattn_cases as XC
from _xattn_cases import CB, DTYPES, F1, F32, GRADS, GUARD, HP, HS, NH, NKEY, O1, QS, SETLAY, TOK, judge, prepare
from test_gemm_gpu import bits, pattern

pytestmark = pytest.mark.gpu

_RATIOS = []
OK, EINVAL = 0, -1
SITES = (3, 5, 11)                     # site ids of the attention, FFN1 and FFN2 dropout
SEED_STEP = (20240611, 7)
FWD_ORDER = ('query', 'k', 'v', 'kvalid', 'pack', 'bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2', 'zstride', 'y', 'sq', 'so', 'sv1', 'su2', 'Z', 'B', 'HW', 'rng',
             'site_a', 'site_1', 'site_2', 'p_drop', 'dtype', 'stream')
BWD_ORDER = ('dy', 'query', 'k', 'v', 'kvalid', 'pack', 'g1', 'be1', 'b1', 'g2', 'zstride', 'sq', 'sv1', 'su2', 'dquery', 'dk', 'dv', 'dkp', 'dvp', 'hd', 'dpre',
             'du2', 'n1', 'dv1', 'dq', 'dg1', 'dbe1', 'dbo', 'dg2', 'dbe2', 'Z', 'B', 'HW', 'rng', 'site_a', 'site_1', 'site_2', 'p_drop', 'dtype', 'stream')
WRITTEN = ('dquery', 'dk', 'dv', 'hd', 'dpre', 'du2', 'n1', 'dv1', 'dq')          # backward outputs that are written, not added to


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


def es_of(dt):
    return torch.empty(0, dtype=dt).element_size()


def adv(ptr, nbytes):
    return ctypes.c_void_p(ptr.value + nbytes)


_STATE, _MASKS = [], {}


def rng_state():
    if not _STATE:
        _STATE.append(torch.tensor(SEED_STEP, dtype=torch.int64, device='cuda'))
    return _STATE[0]


def gpu_masks(cs):
    """the keep masks the header names as the statement of the draw: stj_dropout_mask over the three draw shapes"""
    from strajnet_amd import ops
    if not cs['p'] > 0:
        return None
    if cs['name'] not in _MASKS:
        m = {}
        for (key, shape), site in zip(XC.draw_shapes(cs).items(), SITES):
            n = 1
            for d in shape:
                n *= d
            t = torch.empty(n, dtype=torch.uint8, device='cuda')
            ops.call('stj_dropout_mask', ops._p(t), n, float(cs['p']), ops._p(rng_state()), site, ops._st())
            m[key] = t.cpu().reshape(shape)
            assert 0.5 * cs['p'] < 1.0 - float(m[key].float().mean()) < 1.5 * cs['p'], (cs['name'], key)
        _MASKS[cs['name']] = m
    return _MASKS[cs['name']]


# ---- the weight stream ------------------------------------------------------------------------------------------------------------------
def pack_geometry(dt):
    f32 = dt == F32
    kstep = 16 if f32 else 32
    g = dict(LDQ=HP + 4, KQ=96 if f32 else 192, LDO=O1 + (4 if f32 else 16), HC=kstep, LD1=kstep + 4, LD2=CB + (4 if f32 else 16))
    g['NQC'], g['NFC'] = CB // g['KQ'], F1 // kstep
    g['QCH'], g['OCH'], g['FCH'] = g['KQ'] * g['LDQ'], HP * g['LDO'], O1 * g['LD1'] + kstep * g['LD2']
    g['STREAM'] = NH * g['NQC'] * g['QCH'] + NH * g['OCH'] + g['NFC'] * g['FCH']
    return g


def pack_image(I, z, dt):
    """one set's stream as the header describes it: the LDS images of the Wq (head, k-part), Wo (head) and FFN-slice chunks, pads zero"""
    g = pack_geometry(dt)
    q = torch.zeros(NH, g['NQC'], g['KQ'], g['LDQ'])
    q[..., :HS] = I['wq'][z].reshape(NH, g['NQC'], g['KQ'], HS)
    o = torch.zeros(NH, HP, g['LDO'])
    o[:, :HS, :O1] = I['wo'][z]
    a = torch.zeros(g['NFC'], O1, g['LD1'])
    a[:, :, :g['HC']] = I['w1'][z].reshape(O1, g['NFC'], g['HC']).permute(1, 0, 2)
    c = torch.zeros(g['NFC'], g['HC'], g['LD2'])
    c[:, :, :CB] = I['w2'][z].reshape(g['NFC'], g['HC'], CB)
    f = torch.cat([a.reshape(g['NFC'], -1), c.reshape(g['NFC'], -1)], 1)
    return torch.cat([q.reshape(-1), o.reshape(-1), f.reshape(-1)]).to(dt)


def pack_sizes(dt):
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    code, es = ops.DTYPE_CODE[dt], es_of(dt)
    ws, tail = int(lib().stj_xattn_pack_workspace_bytes(code)), int(lib().stj_xattn_pack_tail_workspace_bytes(code))
    assert ws % 16 == 0 and tail % es == 0 and ws == pack_geometry(dt)['STREAM'] * es
    return ws // es, tail // es


def make_pack(p, dev, tail='zero'):
    """stj_xattn_pack of the case's Z sets into GUARD | Z streams | tail | GUARD (elements of dt); returns the device buffer"""
    from strajnet_amd import ops
    ws, tl = pack_sizes(p.dt)
    Z = p.cs['Z']
    buf = pattern(GUARD + Z * ws + tl + GUARD, p.dt)
    if tail == 'zero':
        buf[GUARD + Z * ws:GUARD + Z * ws + tl] = 0
    buf = buf.cuda()
    w = [ops._poff(dev['params'], GUARD + SETLAY[n][0]) for n in ('wq', 'wo', 'w1', 'w2')]
    ops.call('stj_xattn_pack', *w, p.cs['zstride'], Z, ops._poff(buf, GUARD), ops.DTYPE_CODE[p.dt], ops._st())
    return buf


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def upload(p):
    return {k: b.init.cuda() for k, b in p.bufs.items()}


def download(dev):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def arguments(p, dev, pack):
    """name -> argument of the call a Prep describes (pointers as c_void_p, None for a NULL pointer)"""
    from strajnet_amd import ops
    cs = p.cs
    v = {k: ops._poff(dev[k], GUARD) for k in p.bufs if k not in ('params', 'grads')}
    for n in ('bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2'):
        v[n] = ops._poff(dev['params'], GUARD + SETLAY[n][0])
    for n, src in GRADS.items():
        v[n] = ops._poff(dev['grads'], GUARD + SETLAY[src][0]) if 'grads' in dev else None
    v.update(pack=ops._poff(pack, GUARD), zstride=cs['zstride'], Z=cs['Z'], B=cs['B'], HW=cs['HW'], rng=ops._p(rng_state()) if cs['rng'] else None,
             site_a=SITES[0], site_1=SITES[1], site_2=SITES[2], p_drop=float(cs['p']), dtype=ops.DTYPE_CODE[p.dt], stream=ops._st())
    for n in ('kvalid', 'sq', 'so', 'sv1', 'su2'):
        v.setdefault(n, None)
    return v


def launch(p, v, raw=False):
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    name, order = ('stj_xattn_fwd', FWD_ORDER) if p.kind == 'fwd' else ('stj_xattn_bwd', BWD_ORDER)
    args = [ops._p(v[k]) if (v[k] is None or isinstance(v[k], ops.vp)) else v[k] for k in order]
    if raw:
        return getattr(lib(), name)(*args)
    ops.call(name, *args)


def run(p, tail='zero'):
    """upload, pack, call; returns the flat buffers as the call left them"""
    dev = upload(p)
    pack = make_pack(p, dev, tail)
    state = rng_state().clone()
    launch(p, arguments(p, dev, pack))
    after = download(dev)
    assert torch.equal(state, rng_state()), 'the call changed the random state'
    return after


def run_cases(dt, names, body):
    failed = []
    for name in names:
        try:
            body(XC.case(name), dt)
        except AssertionError as e:
            failed.append(f'{name} [{dt}]: {e}')
    assert not failed, f'{len(failed)} of {len(names)} cases failed:\n' + '\n'.join(failed)


ALL = [c['name'] for c in XC.cases()]


# ---- the case families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_forward(dt):
    """training form (all four saves) and inference form (none): every output row against float64; without dropout y is bit-equal in both"""
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'fwd', m, 'gpu')
        after = run(p)
        judge(p, after, _RATIOS)
        q = prepare(cs, dt, 'fwd', m, 'gpu', with_saves=False)
        bare = run(q)
        judge(q, bare, _RATIOS)
        if not cs['p'] > 0:
            assert torch.equal(bits(bare['y']), bits(after['y'])), 'y of the inference form differs from the training form at p = 0'
    run_cases(dt, ALL, body)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_backward_on_reference_saves(dt):
    def body(cs, dt):
        p = prepare(cs, dt, 'bwd', gpu_masks(cs), 'gpu')
        judge(p, run(p), _RATIOS)
    run_cases(dt, ALL, body)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_forward_into_backward(dt):
    """z3_t3 end to end: the backward kernel on what the forward kernel saved, through the same judge"""
    def body(cs, dt):
        m = gpu_masks(cs)
        p = prepare(cs, dt, 'fwd', m, 'gpu')
        after = run(p)
        judge(p, after)
        saves = {n: XC.logical(p, after, n).reshape(cs['Z'], cs['B'], cs['HW'], -1) for n in ('sq', 'sv1', 'su2')}
        q = prepare(cs, dt, 'bwd', m, 'gpu', saves_from=saves)
        judge(q, run(q), _RATIOS, label=' (behind the forward kernel)')
    run_cases(dt, ['z3_t3_p0', 'z3_t3_p0.1'], body)


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_pack_tail_content_is_not_consumed(dt):
    """The forward stages fixed 4 KB pieces and reads past the last chunk into the tail: what lies there must not reach any output.  And
    stj_xattn_pack writes all of its Z streams (weights rounded to dt at their places, every pad position zero) and nothing else."""
    cs = XC.case('z3_t3_p0.1')
    p = prepare(cs, dt, 'fwd', gpu_masks(cs), 'gpu')
    zero, pat = run(p, 'zero'), run(p, 'pattern')
    for n in p.bufs:
        assert torch.equal(bits(zero[n]), bits(pat[n])), f'{n} depends on the content of the pack tail'
    judge(p, pat)
    dev = upload(p)
    ws, tl = pack_sizes(dt)
    for tail in ('zero', 'pattern'):
        buf = make_pack(p, dev, tail)
        torch.cuda.synchronize()
        got = buf.cpu()
        want = pattern(got.numel(), dt)
        for z in range(cs['Z']):
            want[GUARD + z * ws:GUARD + (z + 1) * ws] = pack_image(p.I, z, dt)
        if tail == 'zero':
            want[GUARD + cs['Z'] * ws:GUARD + cs['Z'] * ws + tl] = 0
        ne = (bits(got) != bits(want)).nonzero()
        assert ne.numel() == 0, f'{ne.numel()} elements of the pack buffer differ from the stated stream, first at {int(ne[0]) - GUARD} (stream {ws}, tail {tl} elements)'


def _sub_call(p, v, names, over):
    """the call of p with some arguments replaced; `names` outputs go to fresh pattern-filled tensors [rows, width] (returned, on the CPU).
    The "+=" pointers stay those of the full call (set z at + z * zstride needs the whole gradient allocation): they are not compared."""
    from strajnet_amd import ops
    v = dict(v)
    v.update(over)
    fresh = {}
    for n, shape in names.items():
        fresh[n] = pattern(GUARD + shape[0] * shape[1] + GUARD, F32 if n in ('dkp', 'dvp') else p.dt).cuda()
        v[n] = ops._poff(fresh[n], GUARD)
    launch(p, v)
    torch.cuda.synchronize()
    return {n: t.cpu()[GUARD:-GUARD].reshape(names[n]) for n, t in fresh.items()}


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_scenes_and_sets_are_independent(dt):
    """Without dropout: scene b of a Z x B call is bit-equal to a B = 1 call on that scene alone, and set z to a Z = 1 call whose query,
    k, v, parameter and pack pointers are advanced to set z.  Forward outputs and the written (not the "+=") backward outputs."""
    from strajnet_amd import ops
    cs = XC.case('z3_t3_p0')
    Z, B, HW, es = cs['Z'], cs['B'], cs['HW'], es_of(dt)
    ws, _ = pack_sizes(dt)
    for kind, outs in (('fwd', XC.FWD_OUT), ('bwd', WRITTEN)):
        p = prepare(cs, dt, kind, None, 'gpu')
        dev = upload(p)
        pack = make_pack(p, dev)
        v = arguments(p, dev, pack)
        launch(p, v)
        full = download(dev)
        width = {n: (NH * HS if n in ('dk', 'dv') else XC.WIDTH[n]) for n in outs}
        nrow = {n: (NKEY if n in ('dk', 'dv') else HW) for n in outs}
        whole = {n: XC.logical(p, full, n).reshape(Z, B, nrow[n], width[n]) for n in outs}
        ins = ('query', 'k', 'v') + (('dy', 'sq', 'sv1', 'su2') if kind == 'bwd' else ())
        scratch = {n: (B * (HW // TOK) * NKEY, QS) for n in ('dkp', 'dvp')} if kind == 'bwd' else {}
        # one set alone: every per-set pointer advanced to set z
        for z in range(Z):
            over = {n: adv(v[n], z * B * p.bufs[n].n // (Z * B) * es) for n in ins}
            over.update({n: adv(v[n], z * cs['zstride'] * 4) for n in ('bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2')})
            over.update(pack=adv(v['pack'], z * ws * es), Z=1)
            got = _sub_call(p, v, dict({n: (B * nrow[n], width[n]) for n in outs}, **scratch), over)
            for n in outs:
                assert torch.equal(bits(got[n].reshape(B, nrow[n], width[n])), bits(whole[n][z])), f'{kind} {n}: set {z} alone differs from set {z} of the Z = {Z} call'
        # one scene alone: its slices of every [Z, B, ..] input in tensors of their own
        for b in range(B):
            over, hold = {}, []
            for n in ins + ('kvalid',):
                bf = p.bufs[n]
                t = bf.init[GUARD:-GUARD]
                t = t.reshape(1, B, -1) if n == 'kvalid' else t.reshape(Z, B, -1)
                hold.append(t[:, b].contiguous().cuda())
                over[n] = ops._p(hold[-1])
            over.update(B=1)
            scr = {n: (Z * (HW // TOK) * NKEY, QS) for n in scratch}
            got = _sub_call(p, v, dict({n: (Z * nrow[n], width[n]) for n in outs}, **scr), over)
            for n in outs:
                assert torch.equal(bits(got[n].reshape(Z, nrow[n], width[n])), bits(whole[n][:, b])), f'{kind} {n}: scene {b} alone differs from scene {b} of the B = {B} call'


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_repeatable(dt):
    """two identical calls: bit-identical forward outputs (the forward has no atomics) and bit-identical written backward outputs"""
    cs = XC.case('z3_t3_p0.1')
    m = gpu_masks(cs)
    p = prepare(cs, dt, 'fwd', m, 'gpu')
    a, b = run(p), run(p)
    for n in p.bufs:
        assert torch.equal(bits(a[n]), bits(b[n])), f'forward: {n} differs between two identical calls'
    p = prepare(cs, dt, 'bwd', m, 'gpu')
    a, b = run(p), run(p)
    for n in WRITTEN:
        assert torch.equal(bits(a[n]), bits(b[n])), f'backward: {n} differs between two identical calls'


def test_status_codes():
    """Every refusal comes from the host checks in front of the launch (csrc/xattn_fused.hip, the extern "C" entry points), leaves every
    buffer bit-identical and a message in stj_last_error(); Z = 0 and B = 0 are STJ_OK and write nothing."""
    from strajnet_amd._lib import lib
    L = lib()
    for Z, B, HW in ((8, 2, 64), (3, 3, 192), (1, 1, 320), (5, 1, 64), (2, 7, 4096)):
        assert L.stj_xattn_bwd_workspace_bytes(Z, B, HW) == Z * B * (HW // 64) * 64 * 144 * 4
    cs = XC.case('z5_p0')
    for dt in (F32, torch.bfloat16):
        for kind in ('fwd', 'bwd'):
            p = prepare(cs, dt, kind, None, 'gpu')
            dev = upload(p)
            pack = make_pack(p, dev)
            torch.cuda.synchronize()
            pack0 = pack.cpu()
            v = arguments(p, dev, pack)
            refused = [dict(HW=96), dict(HW=0), dict(HW=-64), dict(p_drop=1.0), dict(dtype=7)]
            refused += [{n: adv(v[n], 8)} for n in (('query', 'y', 'pack') if kind == 'fwd' else ('query', 'pack', 'dy', 'dquery', 'su2', 'du2'))]
            if kind == 'fwd':
                refused += [{n: None} for n in ('sq', 'so', 'sv1', 'su2')]
            for over, want in [(o, EINVAL) for o in refused] + [(dict(Z=0), OK), (dict(B=0), OK)]:
                rc = launch(p, dict(v, **over), raw=True)
                assert rc == want, (kind, dt, over, rc, want)
                if want != OK:
                    assert L.stj_last_error(), (kind, over)
                after = download(dev)
                for n, b in p.bufs.items():
                    assert torch.equal(bits(after[n]), bits(b.init)), (kind, dt, over, n)
                assert torch.equal(bits(pack.cpu()), bits(pack0)), (kind, dt, over, 'pack')
            # the unmodified argument list is legal
            assert launch(p, v, raw=True) == OK
            judge(p, download(dev))
        # stj_xattn_pack: bad dtype, misaligned pack, Z = 0
        from strajnet_amd import ops
        w = [ops._poff(dev['params'], GUARD + SETLAY[n][0]) for n in ('wq', 'wo', 'w1', 'w2')]
        for args, want in (((cs['zstride'], cs['Z'], v['pack'], 7), EINVAL), ((cs['zstride'], cs['Z'], adv(v['pack'], 8), ops.DTYPE_CODE[dt]), EINVAL),
                           ((cs['zstride'], 0, v['pack'], ops.DTYPE_CODE[dt]), OK)):
            assert L.stj_xattn_pack(*w, *args, ops._st()) == want, args
            if want != OK:
                assert L.stj_last_error()
            torch.cuda.synchronize()
            assert torch.equal(bits(pack.cpu()), bits(pack0)), ('pack', args)


def test_zz_report_xattn_error_ratios():
    """(runs last in this file) the largest ||err|| / bound per (entry point, dtype, output), under pytest -s"""
    print()
    print('\n'.join(XC.report_lines(_RATIOS, 'xattn abi')))
