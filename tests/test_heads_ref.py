"""_heads_cases.py on the CPU: the float64 statements against torch's own conv2d and autograd, the dispatch mirrors against hand-written
expectations for every row (path, tiles, grid, tiles per workgroup, decode branch), the exactness conditions of the integer twins, and
the judgement against the mutants it must reject."""
import pytest
import torch
import torch.nn.functional as Fn

import _heads_cases as HC
from _heads_cases import BF16, EINVAL, EUNSUPPORTED, F16, F32, F64, OK

SMALL = [cs for cs in HC.OC_CASES if not HC.on_device(cs)]


def _conv(X, W, bias):
    return Fn.conv2d(X.double().permute(0, 3, 1, 2), W.double().permute(3, 2, 0, 1), bias.double(), padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize('shape', [(2, 16, 32, 8), (1, 16, 16, 48)], ids=str)
def test_statements_equal_conv2d_and_autograd(shape):
    F, H, W, C = shape
    g = torch.Generator().manual_seed(5)
    X, Wt, b = torch.randn(F, H, W, C, generator=g, dtype=F64), torch.randn(3, 3, C, 2, generator=g, dtype=F64), torch.randn(2, generator=g, dtype=F64)
    G = torch.randn(F, H, W, 2, generator=g, dtype=F64)
    y = HC.fwd_ref(X, Wt, b)
    assert (y - _conv(X, Wt, b)).abs().max() < 1e-12
    Xr, Wr, br = X.clone().requires_grad_(), Wt.clone().requires_grad_(), b.clone().requires_grad_()
    _conv(Xr, Wr, br).backward(G)
    assert (HC.dx_sum(G, Wt) - Xr.grad).abs().max() < 1e-12
    assert (HC.dw_sum(X, G) - Wr.grad).abs().max() < 1e-11
    assert (G.sum((0, 1, 2)) - br.grad).abs().max() < 1e-11
    # under elu_in the gradient of conv(ELU(p)) with respect to p, X = ELU(p)
    p = torch.randn(F, H, W, C, generator=g, dtype=F64).requires_grad_()
    _conv(Fn.elu(p), Wt, b).backward(G)
    assert (HC.dx_sum(G, Wt) * HC.elu_prime(Fn.elu(p.detach())) - p.grad).abs().max() < 1e-12


@pytest.mark.parametrize('t_major', [0, 1])
def test_pair_head_and_gather_statements(t_major):
    """pair: channel 4t + 2h + o of conv2d per frame; gather(head's projection, unrounded) == the pair statement on ELU(pre)"""
    B, H, W = 2, 16, 32
    g = torch.Generator().manual_seed(7 + t_major)
    y48 = [torch.randn(8 * B, H, W, 48, generator=g, dtype=F64) for _ in (0, 1)]
    Wh = [torch.randn(3, 3, 48, 2, generator=g, dtype=F64) for _ in (0, 1)]
    b = [torch.randn(2, generator=g, dtype=F64) for _ in (0, 1)]
    ys = [_conv(y48[h], Wh[h], b[h]) for h in (0, 1)]
    Y = HC.pair_of(ys[0], ys[1], B, t_major)
    for bb in range(B):
        for t in range(8):
            f = t * B + bb if t_major else bb * 8 + t
            for h in (0, 1):
                assert torch.equal(Y[bb, :, :, 4 * t + 2 * h:4 * t + 2 * h + 2], ys[h][f])
    Z = []
    for h in (0, 1):
        z = torch.full((8 * B, H, W, 20), float('nan'), dtype=F64)           # channels 18, 19 are never read
        z[..., :18] = HC.head_proj(y48[h], Wh[h])
        Z.append(z)
    assert (HC.gather_ref(Z[0], Z[1], b[0], b[1], B, t_major) - Y).abs().max() < 1e-11


def test_head_statement_is_the_upconv_then_the_projection():
    cs = HC.HEAD_CASES[0]
    o = HC.head_operands(cs, F16, False)
    Z, S, pre = HC.head_ref(o.X, o.Wf, o.bias, o.Wh, F16)
    assert Z.shape == (1, 16, 32, 20) and bool((Z[..., 18:] == 0).all()) and bool((pre <= 0).any()) and bool((pre > 0).any())
    y = HC.elu(pre).to(F16).double()
    want = torch.einsum('fyxc,kco->fyxko', y, o.Wh.double().reshape(9, 48, 2)).reshape(1, 16, 32, 18).to(F16).double()
    assert torch.equal(Z[..., :18], want)
    assert bool((Z.abs() <= S * (1 + 2.0 ** -9) + 1e-30).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the mirrors against hand-written expectations
# ---------------------------------------------------------------------------------------------------------------------------------------
def _mf(nt, grid, per, full, decode, path):
    return dict(status=OK, path=path, ntiles=nt, grid=grid, per=per, full=full, decode=decode)


OC_EXPECT = {       # row name: (tiles, MFMA grid / per / workgroups walking `per` tiles, decode branch)      generic rows: decode None
    '8x16x16x48x8': (8, 8, 1, 8, 'plain'),
    '16x32x48x48x8': (96, 96, 1, 96, 'plain'),
    '8x32x64x48x8': (64, 64, 1, 64, 'swizzled'),
    '16x32x32x48x2-tmajor': (64, 64, 1, 64, 'swizzled'),
    '8x16x32x48x4': (16, 16, 1, 16, 'plain'),
    '8x128x208x48x8': (832, 768, 2, 64, 'swizzled'),
}
GENERIC_EXPECT = {  # row name: (tiles, forward grid, backward grid, backward tiles per workgroup, workgroups walking that many)
    '3x16x32x8x3': (6, 6, 6, 1, 6), '1x16x16x112x1': (1, 1, 1, 1, 1), '8x128x272x8x8': (1088, 1088, 1024, 2, 64),
    '2x16x32x40x2': (4, 4, 4, 1, 4), '1x16x16x48x1-pstride3': (1, 1, 1, 1, 1), '8x16x16x48x8-base4': (8, 8, 8, 1, 8),
    '8x16x16x48x8-wsnull': (8, 8, 8, 1, 8), '8x16x16x48x8-wsshort': (8, 8, 8, 1, 8), '8x16x16x48x8-f16bwd': (8, 8, 8, 1, 8),
    '2x16x16x48x2-tstride5': (2, 2, 2, 1, 2), '4x16x16x48x2-bstrideodd': (4, 4, 4, 1, 4),
}


@pytest.mark.parametrize('cs', HC.OC_CASES, ids=HC.case_id)
def test_outconv_mirror(cs):
    assert cs['name'] in OC_EXPECT or cs['name'] in GENERIC_EXPECT
    for which in ('fwd', 'bwd'):
        for dt, path in cs[which].items():
            for off in cs['offs']:
                geo = HC.oc_geometry(cs, dt, which, off)
                if cs['name'] in OC_EXPECT:
                    nt, grid, per, full, dec = OC_EXPECT[cs['name']]
                    assert path == ('FM' if which == 'fwd' else 'BM')
                    want = _mf(nt, grid, per, full, dec, path)
                    assert {k: geo[k] for k in want} == want, (which, dt, geo)
                else:
                    nt, gf, gb, perb, fullb = GENERIC_EXPECT[cs['name']]
                    want = _mf(nt, gf, 1, gf, None, 'FG') if which == 'fwd' else _mf(nt, gb, perb, fullb, None, 'BG')
                    assert path == want['path'] and {k: geo[k] for k in want} == want, (which, dt, geo)
    if cs['name'] in OC_EXPECT:                 # what the MFMA rows' other element types take
        assert HC.oc_geometry(cs, F16, 'bwd')['path'] == 'BG' and HC.oc_geometry(cs, F32, 'fwd')['path'] == 'FG'


def test_outconv_mirror_decode_regimes():
    F, H, W, C, Tn = 16, 32, 32, 48, 2
    d = HC.decode_facts(F, H, W, Tn, 4, H * W * 32)
    assert d == dict(decode='swizzled', time_outer=True, nt=8, S=8)
    assert HC.decode_facts(8, 16, 32, 4, 16 * 32 * 32, 4) == dict(decode='plain', time_outer=False, nt=4, S=4)
    assert HC.decode_facts(16, 32, 48, 8, 32 * 48 * 32, 4) == dict(decode='plain', time_outer=False, nt=8, S=12)


@pytest.mark.parametrize('cs', [c for c in HC.OC_CASES if c['name'] in OC_EXPECT], ids=HC.case_id)
def test_oc_decode_visits_every_tile_of_every_frame_once(cs):
    F, H, W, C, Tn = cs['shape']
    (ybs, yts, _), _ = HC.strides(cs)
    tx_n, ty_n = W // 16, H // 16
    seen = {HC.oc_decode(i, tx_n, ty_n, F, Tn, ybs, yts) for i in range(F * tx_n * ty_n)}
    assert seen == {(tx, ty, f) for tx in range(tx_n) for ty in range(ty_n) for f in range(F)}
    if HC.decode_facts(F, H, W, Tn, ybs, yts)['decode'] == 'swizzled':      # the 8 waypoints of a spatial tile: indices c + 8 t + 64 u
        nt = 8
        tx0, ty0, f0 = HC.oc_decode(0, tx_n, ty_n, F, Tn, ybs, yts)
        for t in range(nt):
            tx, ty, f = HC.oc_decode(8 * t, tx_n, ty_n, F, Tn, ybs, yts)
            assert (tx, ty) == (tx0, ty0) and f == (t * Tn if cs['order'] == 't' else t)


def test_generic_limits():
    """LDS (160 KiB) and 9 C <= 1024: C = 112 is the largest both admit, C = 120 is refused in both directions"""
    a = (1, 16, 16)
    s = (16 * 16 * 4, 4, 4)
    assert HC.outconv_fwd_geometry(F32, *a, 112, 1, *s)['path'] == 'FG' and HC.outconv_bwd_geometry(F32, *a, 112, 1, *s)['path'] == 'BG'
    assert HC.outconv_fwd_geometry(F32, *a, 120, 1, *s)['status'] == EUNSUPPORTED
    assert HC.outconv_bwd_geometry(F32, *a, 120, 1, *s)['status'] == EUNSUPPORTED
    assert 9 * 112 <= 1024 < 9 * 120 and (324 * 121 + 18 * 120) * 4 > 160 * 1024 >= (324 * 113 + 18 * 112 + 648) * 4
    for bad in (dict(H=24), dict(C=12), dict(F=0), dict(Tn=0), dict(F=12)):
        v = dict(F=8, H=16, W=16, C=48, Tn=8)
        v.update(bad)
        assert HC.outconv_fwd_geometry(BF16, v['F'], v['H'], v['W'], v['C'], v['Tn'], 8192, 4, 32)['status'] == EINVAL, bad
        assert HC.outconv_bwd_geometry(BF16, v['F'], v['H'], v['W'], v['C'], v['Tn'], 8192, 4, 32)['status'] == EINVAL, bad
    assert HC.outconv_bwd_geometry(BF16, 8, 16, 16, 48, 8, 8192, 4, 32, dW=False)['status'] == EINVAL
    assert HC.outconv_fwd_geometry(7, 8, 16, 16, 48, 8, 8192, 4, 32)['status'] == EINVAL
    # the stride-parity decision: any odd stride, or a base that is only 4-byte aligned, takes the generic kernels
    assert HC.outconv_fwd_geometry(BF16, 8, 16, 16, 48, 8, 8192, 4, 32)['path'] == 'FM'
    for s3, base in (((8193, 4, 32), 0), ((8192, 5, 32), 0), ((8192, 4, 33), 0), ((8192, 4, 32), 4)):
        assert HC.outconv_fwd_geometry(BF16, 8, 16, 16, 48, 8, *s3, base)['path'] == 'FG'
        assert HC.outconv_bwd_geometry(BF16, 8, 16, 16, 48, 8, *s3, base)['path'] == 'BG'
    assert HC.OCB_WS_BYTES == 2660352


PAIR_EXPECT = {'1x16x16x0': (1, 1, 1, 1), '2x32x48x1': (12, 12, 1, 12), '3x16x32x0': (6, 6, 1, 6), '3x144x304x1': (513, 257, 2, 256)}
HEAD_EXPECT = {'1x8x16': (1, 1, 1, 1), '3x16x48': (18, 18, 1, 18), '3x56x208': (273, 256, 2, 17)}
GATHER_EXPECT = {'1x16x16x0': (1, 1, 1, 1), '2x32x48x1': (12, 12, 1, 12), '3x16x32x0': (6, 6, 1, 6), '2x400x656x0': (2050, 2048, 2, 2),
                 '2x32x48x1-nan1819': (12, 12, 1, 12)}


@pytest.mark.parametrize('table,expect', [(HC.PAIR_CASES, PAIR_EXPECT), (HC.HEAD_CASES, HEAD_EXPECT), (HC.GATHER_CASES, GATHER_EXPECT)],
                         ids=['pair', 'head', 'gather'])
def test_pair_head_gather_mirrors(table, expect):
    assert sorted(expect) == sorted(cs['name'] for cs in table)
    for cs, dt in HC.rows(table):
        nt, grid, per, full = expect[cs['name']]
        geo = HC.geometry(cs, dt)
        assert geo['status'] == OK and geo['path'] == cs['path']
        assert (geo['ntiles'], geo['grid'], geo['per'], geo['full']) == (nt, grid, per, full), (cs['name'], geo)
    assert HC.pair_geometry(BF16, 3, 8, 144, 304, 48)['nb'] == 257
    for bad, st in ((dict(dt=F32), EUNSUPPORTED), (dict(C=40), EUNSUPPORTED), (dict(Tn=4), EUNSUPPORTED), (dict(H=24), EUNSUPPORTED), (dict(B=0), EINVAL)):
        v = dict(dt=BF16, B=1, Tn=8, H=16, W=16, C=48)
        v.update(bad)
        assert HC.pair_geometry(v['dt'], v['B'], v['Tn'], v['H'], v['W'], v['C'])['status'] == st, bad
    for bad in (dict(dt=F32), dict(Cin=128), dict(Hi=12), dict(Wi=8)):
        v = dict(dt=BF16, F=1, Hi=8, Wi=16, Cin=96)
        v.update(bad)
        assert HC.head_geometry(v['dt'], v['F'], v['Hi'], v['Wi'], v['Cin'], 48)['status'] == EUNSUPPORTED, bad
    assert HC.gather_geometry(F32, 1, 8, 16, 16)['status'] == EUNSUPPORTED and HC.gather_geometry(BF16, 1, 4, 16, 16)['status'] == EUNSUPPORTED
    assert HC.gather_geometry(BF16, 1, 8, 16, 24)['status'] == EUNSUPPORTED and HC.gather_geometry(BF16, 1, 8, 16, 16, True)['status'] == EUNSUPPORTED
    assert HC.gather_geometry(BF16, 0, 8, 16, 16)['status'] == EINVAL


def test_tables_hold_the_regimes_the_issue_names():
    assert len(HC.OC_CASES) == 17 and len(HC.oc_rows('fwd')) == 25 and len(HC.oc_rows('bwd')) == 22
    assert [cs['name'] for cs in HC.OC_CASES if HC.on_device(cs)] == ['8x128x208x48x8', '8x128x272x8x8']
    assert [cs['name'] for t in (HC.PAIR_CASES, HC.HEAD_CASES, HC.GATHER_CASES) for cs in t if HC.on_device(cs)] == \
        ['3x144x304x1', '3x56x208', '2x400x656x0']
    cs = HC.OC_CASES[10]                        # odd y_pstride: positions 0, 1 of every three are the statement's, the third stays pattern
    idx = HC.y_index(cs, 0).reshape(-1)
    assert HC.y_numel(cs) == 16 * 16 * 3 and set((idx % 3).tolist()) == {0, 1}
    cs = HC.OC_CASES[3]                         # t-major: frame f = t * B + b at b * H W 32 + 4 t
    idx = HC.y_index(cs, 2)
    assert int(idx[5 * 2 + 1, 0, 0, 0]) == 32 * 32 * 32 + 4 * 5 + 2 and int(idx[0, 1, 1, 1]) == 33 * 32 + 3
    for cs in HC.OC_CASES:                      # no two elements of a head share a position, and every one is inside the tensor
        if not HC.on_device(cs):
            for off in cs['offs']:
                idx = HC.y_index(cs, off).reshape(-1)
                assert idx.unique().numel() == idx.numel() and int(idx.max()) < HC.y_numel(cs) and int(idx.min()) >= 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# exactness of the integer twins
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cs', SMALL, ids=HC.case_id)
def test_integer_twin_is_exact_in_f32(cs):
    F, H, W, C, Tn = cs['shape']
    for dt in cs['fwd']:
        o = HC.oc_operands(cs, dt, True, 'fwd')
        R = HC.oc_reference(o, 'fwd')
        assert set(o.X.float().unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(o.W, o.Wraw)
        assert float(R.S.max()) <= 9 * C + 1 and torch.equal(R.Y, R.Y.round())
    for dt in cs['bwd']:
        for e in HC.ELU_MODES:
            o = HC.oc_operands(cs, dt, True, 'bwd', e)
            R = HC.oc_reference(o, 'bwd', e)
            assert set(o.X.float().unique().tolist()) <= ({-0.5, 0.0, 1.0, 2.0} if e else {-1.0, 0.0, 1.0})
            assert float(R.SdX.max()) <= 18 and torch.equal(2 * R.dX, (2 * R.dX).round()) and torch.equal(R.dX.to(dt).double(), R.dX)
            assert float(2 * R.SdW.max()) < 2 ** 24 and float(R.Sdb.max()) < 2 ** 24 and torch.equal(2 * R.dW, (2 * R.dW).round())
            assert bool((o.dW0 != 0).all()) and bool((o.db0 != 0).all())


def test_integer_twin_bounds_of_the_large_rows():
    """|dW| <= 2 F H W + 3 and |db| <= F H W + 3 stay below 2^24 (in halves: 2^23) at the rows evaluated on the device"""
    for cs in HC.OC_CASES:
        F, H, W, C, Tn = cs['shape']
        assert 2 * (2 * F * H * W + 3) < 2 ** 24


@pytest.mark.parametrize('cs,dt', HC.rows(HC.HEAD_CASES), ids=HC.case_id)
def test_head_integer_twin_stays_representable(cs, dt):
    o = HC.head_operands(cs, dt, True)
    R = HC.head_reference(o, dt)
    lim = HC.Z_LIMIT[dt]
    pre_max, z_max = float(R.pre.max()), float(R.Z.max())
    print(f"head {cs['name']} [{HC.case_id(dt)}]: max pre {pre_max}, max z {z_max} (limit {lim})")
    assert float(R.pre.min()) >= 0 and pre_max <= lim and z_max <= lim and z_max > 0
    assert torch.equal(R.pre, R.pre.round()) and torch.equal(R.Z, R.Z.round())
    assert torch.equal(R.Z[..., :18], HC.head_proj(R.pre, o.Wh))           # no rounding took place: the statement alone stays within the limits
    assert torch.equal(o.Wf.double(), o.Wf.double().round()) and float(o.Wf.double().min()) >= 0


def test_gather_and_pair_integer_twins():
    for cs, dt in HC.rows(HC.GATHER_CASES[:3]) + HC.rows(HC.GATHER_CASES[4:]):
        o = HC.gather_operands(cs, dt, True)
        R = HC.gather_reference(cs, o)
        assert float(R.S.max()) <= 10 and torch.equal(R.Y, R.Y.round()) and not bool(torch.isnan(R.Y).any())
        assert bool(torch.isnan(o.Z[0][..., 18:].float()).all()) == cs['nan'] and (cs['nan'] or bool((o.Z[0][..., 18:] == 0).all()))
    for cs, dt in HC.rows(HC.PAIR_CASES[:3]):
        R = HC.pair_reference(cs, HC.pair_operands(cs, dt, True))
        assert float(R.S.max()) <= 9 * 48 + 1 and torch.equal(R.Y, R.Y.round())
    a, b = (HC.gather_operands(HC.GATHER_CASES[k], BF16, False) for k in (1, 4))    # the NaN row differs from its twin in channels 18, 19 alone
    assert torch.equal(HC.bits(a.Z[1][..., :18].contiguous()), HC.bits(b.Z[1][..., :18].contiguous()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the judgement: passes the statement, rejects every mutant
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', HC.MUTANTS)
def test_judgement_rejects(kind):
    table, k = HC.MUTANT_ROW[kind]
    cs = HC.TABLES[table][k]
    assert HC.judge_all('correct', HC.produce(cs, BF16)) == []
    fails = HC.judge_all(kind, HC.mutant(kind))
    print(f'{kind}: {len(fails)} judgements failed: ' + ' | '.join(fails)[:400])
    assert fails, kind


def test_judgement_rejects_on_the_random_twin_too():
    """a dropped corner tap and a touched guard on the random twin of the first row"""
    cs = HC.OC_CASES[0]
    o = HC.oc_operands(cs, BF16, False, 'fwd')
    R = HC.oc_reference(o, 'fwd')
    idx = HC.y_index(cs, 2)
    g = HC.gate('FM', BF16)
    flat, init = HC.flat_with(HC.y_numel(cs), F32, idx, R.Y)
    assert HC.judge('ok', 'Y', flat, init, idx, R.Y, R.S, False, g, {}) == []
    W2 = o.W.clone()
    W2[0, 0] = 0
    flat2, _ = HC.flat_with(HC.y_numel(cs), F32, idx, HC.fwd_ref(o.X, W2, o.bias))
    assert HC.judge('tap', 'Y', flat2, init, idx, R.Y, R.S, False, g, {})
    flat3 = flat.clone()
    flat3[HC.GUARD - 1] = 0.0
    assert HC.judge('guard', 'Y', flat3, init, idx, R.Y, R.S, False, g, {})
    flat4 = flat.clone()
    flat4[HC.GUARD + 5] = 1.0                    # a channel of another head
    assert HC.judge('other head', 'Y', flat4, init, idx, R.Y, R.S, False, g, {})


def test_gates():
    for path in HC.PATHS:
        for dt in (F32, BF16, F16):
            assert HC.gate(path, dt) <= HC.bound(path, dt) <= HC.EPS_ELEM[dt]
    assert set(k[0] for k in HC.MEASURED) <= set(HC.PATHS)
