"""The float64 statements, the dispatch mirrors, the tables and the judgement of _upconv_fwd_cases.py, tested without a GPU.

  * fwd_pre, dgrad_sum, elu' and the skip sums against torch's float64 conv2d(interpolate(x, 2, 'nearest'), W, padding=1) and its autograd input
    gradient, equal to the bit on integer data, on rectangular maps (Hi = 1 and Wi = 1 among them).
  * the mirrors return the path written in every table row; their walker and sequence counts match the hand-written values of the rows that
    state them; every path of the three mirrors has a row, and every forward and dgrad path a row with Hi != Wi; the 2^31 refusal of the
    128 <- 96 wave-specialised input gradient and the switch (ws = False) are mirrored here only.
  * the bf16 hand-over condition (sum over the 16 taps of |partial| <= 256) on the exact twin of every wave-specialised dgrad row.
  * sensitivity: the mutated statements (a tap dropped at one map border, the in-map test with Hi and Wi exchanged, the right halo column read
    twice, one tile left unwritten, the last row written one row too far, elu' from dX's own sign, Y2 rounded once) must each leave the
    judgement on BOTH twins, on every row that evaluates on the CPU, at F = 1 where a row has more than 64 tiles.  On a square map the
    exchanged in-map test is the identity, which is asserted instead.
"""
import pytest
import torch

import _upconv_fwd_cases as UF
from _upconv_fwd_cases import BF16, ELU, F16, F32, F64, NONE

TINY = [(2, 3, 5, 8, 16), (1, 1, 1, 8, 8), (3, 4, 2, 16, 8), (2, 1, 6, 8, 8), (2, 5, 1, 8, 16)]


@pytest.mark.parametrize('shape', TINY, ids=str)
def test_statements_equal_conv2d_autograd_on_integers(shape):
    F, Hi, Wi, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    X = torch.randint(-1, 2, (F, Hi, Wi, Cin), generator=g).double()
    W = torch.randint(-1, 2, (3, 3, Cin, Cout), generator=g).double()
    b = torch.randint(-1, 2, (Cout,), generator=g).double()
    dP = torch.randint(-1, 2, (F, 2 * Hi, 2 * Wi, Cout), generator=g).double()
    xe = torch.tensor([-0.5, 0.0, 1.0, 2.0], dtype=F64)[torch.randint(0, 4, (F, Hi, Wi, Cin), generator=g)]
    Wf, Wd = UF.prep_ref(W)
    assert float(Wf.abs().max()) <= 4 and float(Wd.abs().max()) <= 4
    pre = UF.fwd_pre(X, Wf, b)
    assert torch.equal(pre, UF.conv_ref(X, W, b, NONE))
    assert torch.equal(UF.elu(pre), UF.conv_ref(X, W, b, ELU))
    s = UF.dgrad_sum(dP, Wd)
    assert torch.equal(s, UF.conv_dgrad_ref(dP, W, shape))
    assert torch.equal(s * UF.elu_prime(xe), UF.conv_dgrad_ref(dP, W, shape, xe))
    assert set(UF.elu_prime(xe).unique().tolist()) <= {0.5, 1.0}
    # the tap-wise magnitudes bound the sum; the padded forms are the plain ones
    s2, mag = UF.dgrad_sum(dP, Wd, tap_abs=True)
    assert torch.equal(s2, s) and bool((mag >= s.abs()).all())
    # the skip sums as the header states them, in bf16: two separate adds
    R1 = torch.randint(-1, 2, dP.shape, generator=g).to(BF16)
    R2 = torch.randint(-1, 2, dP.shape, generator=g).to(BF16)
    y = UF.elu(pre).to(BF16)
    assert torch.equal((y + R1) + R2, ((y.double() + R1.double()).to(BF16).double() + R2.double()).to(BF16))


def test_tables_reach_every_path():
    for kind, paths in (('fwd', UF.FWD_PATHS), ('res', UF.RES_PATHS), ('dgrad', UF.DGRAD_PATHS)):
        seen, rect = set(), set()
        for cs, dt in UF.rows(kind):
            assert UF.expected_path(cs, dt) == cs['path'], (cs['name'], dt)
            F, Hi, Wi, Cin, Cout = cs['shape']
            assert Cin % 8 == 0 and Cout % 8 == 0
            seen.add(cs['path'])
            if Hi != Wi:
                rect.add(cs['path'])
            geo = UF.geometry(cs, dt)
            for k, v in cs.get('geo', {}).items():
                assert geo[k] == v, (cs['name'], k, geo[k], v)
        assert seen == set(paths), (kind, set(paths) - seen)
        assert kind == 'res' or rect == set(paths), (kind, set(paths) - rect)      # (res runs the forward's FPS kernels)


def test_mirror_walkers_and_sequences_by_hand():
    # forward, 96 channels: ct = 2 cout tiles of 48, 256 / 2 = 128 walkers for 5 * 5 * 6 = 150 tiles
    assert UF.fwd_geometry(BF16, 5, 40, 96, 96, 96, ELU) == dict(path='FWS96/E', ntiles=150, ct=2, walkers=128, grid=256)
    # 128 channels, three cout groups: 3 * 6 * 6 = 108 tiles on 80 walkers; 8 tiles on 8; 12 ragged tiles on 16
    assert UF.fwd_geometry(BF16, 3, 48, 96, 128, 96, ELU) == dict(path='FWS128/E+X3', ntiles=108, ct=3, walkers=80, grid=240)
    assert UF.fwd_geometry(F16, 2, 16, 32, 128, 96, ELU) == dict(path='FWS128/E+X3', ntiles=8, ct=3, walkers=8, grid=24)
    assert UF.fwd_geometry(F16, 2, 12, 40, 128, 96, ELU) == dict(path='FWS128/R+X3', ntiles=12, ct=3, walkers=16, grid=48)
    # 12 whole tiles: the walker grid would be 16 wide, so the 2-D grid with a tile for each of its 12 walkers; 16 whole tiles: 16 walkers
    assert UF.fwd_geometry(BF16, 3, 16, 32, 128, 96, ELU) == dict(path='FWS128/E', ntiles=12, ct=3, walkers=12, grid=36)
    assert UF.fwd_geometry(BF16, 4, 16, 32, 128, 96, ELU)['path'] == 'FWS128/E+X3'
    assert UF.fwd_geometry(BF16, 1, 8, 16 * 7, 128, 96, ELU)['path'] == 'FWS128/E'          # 7 tiles: below the walker grid's 8
    assert UF.fwd_geometry(BF16, 1, 8, 16, 128, 64, ELU) == dict(path='FWS128/E', ntiles=1, ct=2, walkers=1, grid=2)
    # partial sums: 16-row tiles iff Hi % 16 == 0; a 16-column tile holds the 8-column map
    assert UF.fwd_geometry(BF16, 1, 32, 16, 384, 192, ELU) == dict(path='FPS16', ntiles=2, ct=6, walkers=2, grid=12)
    assert UF.fwd_geometry(BF16, 2, 8, 8, 384, 192, ELU) == dict(path='FPS8', ntiles=2, ct=6, walkers=2, grid=12)
    # input gradient
    assert UF.dgrad_geometry(BF16, 5, 64, 112, 96, 48) == dict(path='DWS2/V3', ntiles=280, ct=1, walkers=256, grid=256)
    assert UF.dgrad_geometry(BF16, 3, 56, 112, 128, 96) == dict(path='DWS', ntiles=147, ct=2, walkers=128, grid=256)
    # pipelined: ct = 6 cin tiles -> 256 / 6 = 42 -> 40 sequences at most; 48 tiles need ceil(48 / n) rounded up to 4 slots: 4 for n = 40, 32,
    # 24 and 16, 8 for n = 8 -> 16 sequences of 3 tiles
    assert UF.dgrad_geometry(BF16, 3, 32, 64, 384, 192) == dict(path='DPF', ntiles=48, ct=6, walkers=16, nseq8=16, grid=96)
    assert UF.dgrad_geometry(F16, 1, 8, 16, 192, 128) == dict(path='DPF', ntiles=1, ct=3, walkers=1, nseq8=8, grid=24)
    assert UF.dgrad_geometry(F16, 1, 16, 32, 384, 192) == dict(path='DPF', ntiles=4, ct=6, walkers=4, nseq8=8, grid=48)
    # 192 <- 128 at 64 x 64, F = 64 (the model's layer): 2048 tiles, ct = 3 -> 80 sequences, 26 tiles each -> 28 slots; 72 need 32
    assert UF.dgrad_geometry(BF16, 64, 64, 64, 192, 128)['walkers'] == 80


def test_mirror_refusals_and_element_types():
    # fp16 and f32 at the wave-specialised dgrad shapes take the generic kernels; fp16 takes the pipelined one
    assert UF.expected_dgrad_path(F16, 2, 8, 16, 96, 48) == 'DG6' and UF.expected_dgrad_path(F32, 2, 8, 16, 96, 48) == 'DG6'
    assert UF.expected_dgrad_path(F16, 1, 8, 16, 128, 96) == 'DG4' and UF.expected_dgrad_path(F16, 1, 8, 16, 192, 128) == 'DPF'
    assert UF.expected_dgrad_path(F32, 1, 8, 16, 192, 128) == 'DG4' and UF.expected_dgrad_path(BF16, 1, 8, 24, 192, 128) == 'DG4'
    assert UF.expected_dgrad_path(BF16, 1, 8, 16, 288, 24) == 'DG6' and UF.expected_dgrad_path(BF16, 1, 8, 16, 192, 24) == 'DG4'
    # the halo loader's 32-bit byte offsets: F * 4 Hi Wi * 96 * 2 bytes below 2^31, else the generic kernel
    assert UF.expected_dgrad_path(BF16, 170, 128, 128, 128, 96) == 'DWS' and UF.expected_dgrad_path(BF16, 171, 128, 128, 128, 96) == 'DG4'
    assert 170 * 4 * 128 * 128 * 96 * 2 < 2 ** 31 <= 171 * 4 * 128 * 128 * 96 * 2
    # the switch
    assert UF.expected_dgrad_path(BF16, 2, 8, 16, 96, 48, ws=False) == 'DG6' and UF.expected_dgrad_path(BF16, 1, 8, 16, 192, 128, ws=False) == 'DG4'
    assert UF.expected_fwd_path(BF16, 2, 8, 16, 96, 48, ELU, ws=False) == 'FG3' and UF.expected_fwd_path(BF16, 1, 16, 16, 192, 128, ELU, ws=False) == 'FG4'
    # forward: f32 and act != ELU are generic at every shape
    for shape in ((2, 8, 16, 96, 48), (1, 8, 16, 128, 96), (1, 16, 16, 192, 128)):
        assert UF.expected_fwd_path(F32, *shape, ELU)[:2] == 'FG' and UF.expected_fwd_path(BF16, *shape, NONE)[:2] == 'FG'
    assert UF.expected_fwd_path(BF16, 1, 16, 16, 192, 40, ELU) == 'FG3' and UF.expected_fwd_path(BF16, 1, 16, 16, 144, 128, ELU) == 'FG4'
    # stj_upconv_fwd_res: the refusals of the issue
    sh = (1, 16, 16, 192, 128)
    assert UF.expected_res_path(BF16, *sh) == 'RES/FPS16' and UF.expected_res_path(BF16, *sh, True, False, False) == 'RES/FPS16'
    assert UF.expected_res_path(F32, *sh) is None and UF.expected_res_path(BF16, 1, 16, 16, 128, 128) is None
    assert UF.expected_res_path(BF16, 1, 16, 16, 192, 40) is None and UF.expected_res_path(BF16, *sh, r1=False) is None
    assert UF.expected_res_path(BF16, *sh, True, True, False) is None and UF.expected_res_path(BF16, *sh, True, False, True) is None


@pytest.mark.parametrize('cs', [c for c in UF.DGRAD_CASES if c['path'].startswith('DWS')], ids=UF.case_id)
def test_bf16_hand_over_condition(cs):
    """every grouping of the 16 taps into bf16 partials stays an exactly representable integer on the exact twin: sum |tap partial| <= 256"""
    assert cs['sparse'] and cs['dts'] == (BF16,)
    o = UF.operands(cs, BF16, True)
    worst = UF.dws_condition(o)
    print(f"{cs['name']}: largest sum over the taps of |partial| = {worst:.0f}")
    assert worst <= 256, (cs['name'], worst)
    assert set(o.dP.double().unique().tolist()) <= {-1.0, 0.0, 1.0} and set(o.Xelu.double().unique().tolist()) <= {-0.5, 0.0, 1.0, 2.0}


def _small(cs):
    """the row, at F = 1 where it has more than 64 tiles"""
    F, Hi, Wi, Cin, Cout = cs['shape']
    return dict(cs, shape=(1, Hi, Wi, Cin, Cout)) if UF.ntiles_of(F, Hi, Wi) > 64 else cs


def _dt_of(cs):
    return BF16 if BF16 in cs['dts'] else cs['dts'][-1]


def _plain(cs, dt, R):
    return UF.elu(R.pre).to(dt)


@pytest.mark.parametrize('cs', [c for c in UF.FWD_CASES + UF.RES_CASES if not UF.on_device(_small(c))], ids=UF.case_id)
def test_forward_judgement_rejects_every_mutation(cs):
    cs, dt = _small(cs), _dt_of(cs)
    F, Hi, Wi, Cin, Cout = cs['shape']
    kinds = UF.FWD_MUTATIONS if cs['kind'] == 'fwd' or 'r2' not in cs['skips'] else UF.RES_MUTATIONS
    for exact in (False, True):
        o = UF.operands(cs, dt, exact)
        R = UF.reference(cs, o)
        plain = _plain(cs, dt, R) if cs['kind'] == 'res' and not exact else None
        g = UF.gate(cs['path'], dt)
        fails, _ = UF.judge_fwd('statement', cs, dt, exact, g, o, R, UF.mutated_fwd(None, cs, dt, o, R), plain)
        assert not fails, fails
        for kind in kinds:
            fails, _ = UF.judge_fwd(kind, cs, dt, exact, g, o, R, UF.mutated_fwd(kind, cs, dt, o, R), plain)
            if kind == 'halo_hw_swapped' and Hi == Wi:
                assert not fails, (cs['name'], kind)
            else:
                assert fails, f"{cs['name']} [{dt}] {'exact' if exact else 'random'} twin: the judgement accepts the mutation {kind}"


@pytest.mark.parametrize('cs', [c for c in UF.DGRAD_CASES if not UF.on_device(_small(c))], ids=UF.case_id)
def test_dgrad_judgement_rejects_every_mutation(cs):
    cs, dt = _small(cs), _dt_of(cs)
    F, Hi, Wi, Cin, Cout = cs['shape']
    for exact in (False, True):
        o = UF.operands(cs, dt, exact)
        R = UF.reference(cs, o)
        g = UF.gate(cs['path'], dt)
        for xelu in UF.XELU_MODES:
            fails, _ = UF.judge_dgrad('statement', cs, dt, exact, g, o, R, xelu, *UF.mutated_dgrad(None, cs, dt, o, R, xelu))
            assert not fails, fails
            for kind in UF.DGRAD_MUTATIONS:
                if kind == 'elu_from_own_sign' and not xelu:
                    continue
                fails, _ = UF.judge_dgrad(kind, cs, dt, exact, g, o, R, xelu, *UF.mutated_dgrad(kind, cs, dt, o, R, xelu))
                if kind == 'halo_hw_swapped' and Hi == Wi:
                    assert not fails, (cs['name'], kind)
                else:
                    assert fails, f"{cs['name']} [{dt}] {'exact' if exact else 'random'} twin, Xelu {xelu}: the judgement accepts the mutation {kind}"


def test_gates_never_exceed_the_project_bound():
    for (path, dt), m in UF.MEASURED.items():
        assert path in UF.FWD_PATHS + UF.RES_PATHS + UF.DGRAD_PATHS and m > 0
    for kind in UF.TABLES:
        for cs, dt in UF.rows(kind):
            m = UF.MEASURED[cs['path'], UF.case_id(dt)]                    # every (path, element type) of the tables was measured
            assert UF.gate(cs['path'], dt) == min(4 * m, UF.EPS_ELEM[dt])
