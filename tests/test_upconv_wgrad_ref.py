"""The float64 statements, the dispatch mirror and the judgement of _upconv_cases.py, tested without a GPU.

  * dweff_ref, fold_ref, prep_ref and chain_ref against torch's float64 autograd of conv2d(interpolate(x, 2, 'nearest'), W, padding=1) + bias
    at tiny shapes (Hi != Wi, Hi = 1 and Wi = 1 among them): fold_ref(dweff_ref(X, dP)) is the kernel gradient, conv2d with the folded taps of
    prep_ref on the low-res map is the up-sampled convolution.
  * <prep_ref(W), G> == <W, fold_ref(G)> in exact integers: fold is the adjoint of prep.
  * expected_path over the table returns the path each row names, every one of the twelve paths has a row, the launch mirror states the
    strips the table promises, and 9 * 4 * F Hi Wi < 2^24 for every row (the exact twin's condition).
  * sensitivity: six mutated statements (one chunk dropped, the last strip dropped, taps r swapped for a = 1, the halo test with Hi and Wi
    exchanged, one frame's right halo column counted twice, the bias gradient missing one column parity) must each leave the judgement of
    test_upconv_wgrad_abi_gpu.py -- exceed the gate on the random twin AND differ on the exact twin -- on every row below 100000 pixels, and
    once on the 2304-chunk geometry with Cin, Cout = 8, 8 for the rows above.  On a square map the exchanged halo test is the identity, which
    is asserted instead: that mutation is what the rectangular rows are in the table for.
"""
import pytest
import torch
import torch.nn.functional as Fn

import _upconv_cases as UC
from _upconv_cases import BF16, F32, F64

TINY = [(2, 3, 5, 8, 16), (1, 1, 1, 8, 8), (3, 4, 2, 16, 8), (2, 1, 6, 8, 8), (2, 5, 1, 8, 16)]


def _autograd(X, dP):
    """float64 autograd through torch's own up-sample and convolution: (dW [3,3,Cin,Cout], dbias [Cout])"""
    Cin, Cout = X.shape[3], dP.shape[3]
    W = torch.zeros(Cout, Cin, 3, 3, dtype=F64, requires_grad=True)
    b = torch.zeros(Cout, dtype=F64, requires_grad=True)
    y = Fn.conv2d(Fn.interpolate(X.permute(0, 3, 1, 2), scale_factor=2, mode='nearest'), W, b, padding=1)
    (y * dP.permute(0, 3, 1, 2)).sum().backward()
    return W.grad.permute(2, 3, 1, 0), b.grad


@pytest.mark.parametrize('shape', TINY, ids=str)
def test_statements_against_float64_autograd(shape):
    F, Hi, Wi, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    X = torch.randn(F, Hi, Wi, Cin, generator=g, dtype=F64)
    dP = torch.randn(F, 2 * Hi, 2 * Wi, Cout, generator=g, dtype=F64)
    dW, db = _autograd(X, dP)
    dweff, dbias = UC.dweff_ref(X, dP)
    scale = float(dW.abs().max())
    assert float((UC.fold_ref(dweff) - dW).abs().max()) <= 1e-13 * scale
    assert float((dbias - db).abs().max()) <= 1e-13 * float(db.abs().max())
    cW, cb = UC.chain_ref(X, dP)
    assert float((cW - dW).abs().max()) <= 1e-13 * scale and float((cb - db).abs().max()) <= 1e-13 * float(db.abs().max())
    # prep_ref: the up-sampled convolution equals, phase by phase, the 2x2 convolution of the low-res map with the folded taps
    W = torch.randn(3, 3, Cin, Cout, generator=g, dtype=F64)
    y = Fn.conv2d(Fn.interpolate(X.permute(0, 3, 1, 2), scale_factor=2, mode='nearest'), W.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    Wf, Wd = UC.prep_ref(W)
    Xp = UC.pad_ring(X)
    for pt, a, b, r, s in UC.phases():
        if r or s:
            continue
        acc = sum(Xp[:, a + rr:a + rr + Hi, b + ss:b + ss + Wi] @ Wf[a * 8 + b * 4 + rr * 2 + ss].t() for rr in range(2) for ss in range(2))
        assert float((acc - y[:, a::2, b::2]).abs().max()) <= 1e-13 * float(y.abs().max())
    for pt, a, b, r, s in UC.phases():
        assert torch.equal(Wd[(2 - a - 2 * r + 1) * 4 + (2 - b - 2 * s + 1)], Wf[pt].t())
    assert sorted((2 - a - 2 * r + 1) * 4 + (2 - b - 2 * s + 1) for _, a, b, r, s in UC.phases()) == list(range(16))


def test_fold_is_the_adjoint_of_prep_in_exact_integers():
    g = torch.Generator().manual_seed(11)
    for Cin, Cout in ((8, 8), (24, 40)):
        W = torch.randint(-3, 4, (3, 3, Cin, Cout), generator=g).double()
        G = torch.randint(-3, 4, (16, Cout, Cin), generator=g).double()
        Wf, Wd = UC.prep_ref(W)
        assert float((Wf * G).sum()) == float((W * UC.fold_ref(G)).sum())
        assert bool((Wf == Wf.round()).all()) and float(Wf.abs().max()) <= 12


def test_table_reaches_every_path_and_keeps_the_exact_twin_exact():
    seen = set()
    for cs, dt in UC.rows():
        assert UC.expected_path(dt, *cs['shape']) == cs['path'], (cs['name'], dt)
        seen.add(cs['path'])
        geo = UC.launch_geometry(dt, *cs['shape'])
        for k, v in cs.get('geo', {}).items():
            assert geo[k] == v, (cs['name'], k, geo[k], v)
        assert 9 * 4 * UC.pixels(cs) + 64 < 2 ** 24, cs['name']            # + the starting contents (<= 3 each, four folded)
        assert all(c % 8 == 0 for c in cs['shape'][3:])                     # 16-byte rows in every element type
        for parts in (p for p in UC.DB_MODES if p and p > 1):
            for bud in cs['budgets']:
                assert UC.launch_geometry(dt, *cs['shape'], bud)['grid'] % parts, (cs['name'], parts)     # no copy is favoured by the grid
    assert seen == set(UC.PATHS)
    # the same shape in the other 16-bit type and in f32 takes the generic kernel
    assert UC.expected_path(BF16, 2, 8, 32, 96, 48) == 'TR36/32' and UC.expected_path(F32, 2, 8, 32, 96, 48) == 'G36'
    big = next(c for c in UC.CASES if c['shape'] == (64, 64, 64, 96, 48))
    assert set(big['budgets']) == set(UC.BUDGET_GEO)
    for bud, want in UC.BUDGET_GEO.items():
        geo = UC.launch_geometry(BF16, *big['shape'], bud)
        assert {k: geo[k] for k in want} == want, (bud, geo)
    # one chunk below the threshold the 512-thread kernel is not taken; neither when Hi is no multiple of 256 / CW
    assert UC.expected_path(BF16, 63, 64, 64, 96, 48) == 'TR36/32' and UC.expected_path(BF16, 128, 36, 64, 96, 48) == 'TR36/32'
    assert UC.expected_path(BF16, 2048, 8, 16, 96, 48) == 'TR36/16'


def _sensitivity(cs, dt):
    P = UC.pixels(cs)
    F, Hi, Wi, Cin, Cout = cs['shape']
    gate = UC.GATE[UC.expected_path(dt, *cs['shape'])]
    for exact in (False, True):
        X, dP = UC.operands(cs, dt, exact)
        R = UC.reference(X, dP)
        start = UC.starts(cs, dt, exact, 1, zero=not exact)
        got = dict(dweff=start['dweff'].double() + R.dweff, db=start['db'].double() + R.db)
        fails, _ = UC.judge_values('unmutated', exact, gate, R, start, got, P)
        assert not fails, fails                                               # the statement itself passes
        for kind in UC.MUTATIONS:
            w, b = UC.mutated(kind, cs, dt, X, dP, R)
            got = dict(dweff=start['dweff'].double() + w, db=start['db'].double() + b)
            fails, _ = UC.judge_values(kind, exact, gate, R, start, got, P)
            if kind == 'halo_hw_swapped' and Hi == Wi:
                assert not fails and torch.equal(w, R.dweff), (cs['name'], kind)
            else:
                assert fails, f"{cs['name']} [{dt}] {'exact' if exact else 'random'} twin: the judgement accepts the mutation {kind}"


@pytest.mark.parametrize('cs', [c for c in UC.CASES if UC.pixels(c) < UC.BIG], ids=UC.case_id)
def test_judgement_rejects_every_mutation(cs):
    _sensitivity(cs, cs['dts'][-1] if BF16 not in cs['dts'] else BF16)


def test_judgement_rejects_every_mutation_at_2304_chunks():
    """the rows above 100000 pixels, once: the 2304-chunk geometry (9, 64, 512) with 8 x 8 channels, the path and strips of the real row"""
    ref_row = next(c for c in UC.CASES if c['shape'] == (9, 64, 512, 40, 24))
    cs = dict(ref_row, shape=(9, 64, 512, 8, 8))
    assert UC.launch_geometry(BF16, *cs['shape']) == UC.launch_geometry(BF16, *ref_row['shape'])
    _sensitivity(cs, BF16)
