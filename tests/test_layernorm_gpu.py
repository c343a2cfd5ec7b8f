"""The LayerNorm entry points (stj_layernorm_fwd, stj_layernorm_res_fwd, stj_layernorm_bwd, stj_layernorm_bwd_chain and
stj_layernorm_bwd_chain_supported) per dispatch path, against float64 statements that share none of the kernels' logic.

Every case calls the C ABI with raw pointers into flat buffers (ops.call; lib() where a return code other than STJ_OK is expected).  Cases,
layout, references and the judge live in _layernorm_cases.py and are themselves tested on the CPU by test_layernorm_ref.py.  The
references are index arithmetic on float64 copies of the flat buffers the kernel saw: biased variance, eps (as the float the ABI takes)
inside the square root; the gather form's logical row (b, i, j) = [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)]; run row // group_rows
uses parameter set run % ngroups, gstride floats further; y = LN(x) gamma + beta (+ res); dx (+ dres); dgamma[g], dbeta[g] summed over
the rows of group g.  Backward cases hand the kernel the float64 mean / rstd rounded to f32: backward is judged on its own.

Judgement, per case: |got - ref| <= EPS T per element, T in float64 from |operands| only, EPS = EPS_ELEM[dt] (test_ops_gpu) for outputs
stored in dt and EPS_ELEM[float32] for mean, rstd, dgamma, dbeta whatever the storage type (reductions of at most 24 per-lane adds and
6 shuffle steps; at most 4096 rows per parameter sum):
  y      T = (|x| + |mu|) rstd |gamma| + |beta| + |res|
  mean   T = mean_c |x|
  rstd   T = rstd (1 + (var + EPS A^2) / (var + eps)),  A = mean_c |x|,  EPS = EPS_ELEM[float32].  Derivation: the kernels take the variance in a second
         pass over d_c = x_c - m, m the computed mean = mu + e with |e| <= EPS A (the bound on `mean`).  sum_c (x_c - mu) = 0, so
         mean_c d_c^2 = var + e^2 exactly: the first order in e cancels, and the |mu| / sigma amplification of the variance enters squared,
         e^2 / var <= EPS^2 (A / sigma)^2.  Rounding d_c, the squares and their sum adds theta (var + e^2), |theta| <= EPS.  With
         v = var + eps and rstd = v^-1/2, |d rstd| / rstd <= |dv| / (2 v) + EPS (the rsqrt and the store), and
         |dv| <= e^2 + EPS (var + e^2) <= EPS (var + EPS A^2) (1 + EPS):  |d rstd| <= EPS rstd (1 + (var + EPS A^2) / (var + eps)).
         (On a constant row var = 0 and the term is EPS A^2 / eps: the computed mean of a constant need not be that constant.)
  dx     T = rstd (|gg| + mean_c |gg| + |xh| mean_c(|gg| |xh|)) + |dres|,  gg = dy gamma,  xh = (x - mean) rstd
  dgamma T = sum_rows |dy| |xh| + |start value|;   dbeta  T = sum_rows |dy| + |start value|   ("+=": both start non-zero)
  chain  d2 = dLN2(dy) at x2 in float64, rounded once to dt (the documented hand-over), T as dx; dx1 = dLN1(d2) at x1.  The kernel's d2
         may land on the neighbouring dt value where its f32 result lies across a rounding boundary from the float64 one:
         |delta d2| <= EPS[dt] |d2|.  LN1's backward is linear in its incoming gradient, so the difference reaches dx1 as at most
         EPS[dt] rstd1 (|D| + mean_c |D| + |xh1| mean_c(|D| |xh1|)) with D = |d2| |gamma1| -- T of dx1 is the dx expression at gg = d2 gamma1
         plus this one -- and the two sums LN1 takes over d2 as at most EPS[dt] sum_rows |d2| |xh1| and EPS[dt] sum_rows |d2|: dgamma1 /
         dbeta1 are judged with EPS_ELEM[float32] T + EPS_ELEM[dt] (that sum).  dgamma2 / dbeta2 do not pass through d2.
Exact-arithmetic twin of every backward case: the same addresses and geometry, dy and gamma integers in {-3..3}, x in {-2..2}, mean = 0,
rstd = 1 or 1/2 handed in, integer starting values.  Every dy xh and every partial sum is a multiple of 1/2 below 2^24 in any order: summed
over the copies dgamma / dbeta must EQUAL the float64 reference (atomics, sub-runs and partial copies included); dx must equal the
reference rounded once to dt where C is a power of two (it divides by C) and meets the bound elsewhere.  In the chain the twin is exact for
dgamma2 / dbeta2 always, for d2 at a power-of-two C, for dgamma1 / dbeta1 while 2^11 rows C <= 2^24 and for dx1 at C = 8 (the counts are in
_layernorm_cases._prepare_chain); the rest meets the bounds.  With more workgroups than copies every copy must receive a share in the twin.
Guard bands: every tensor, inputs included, lies in an allocation filled with the NaN patterns of test_gemm_gpu.PAT, 64 elements in front
and behind and in every gap between parameter sets and partial copies; after the call all but the output elements is compared bitwise, an
output nobody wrote is still NaN, and in the gather form the whole [B, res, res, C0] map of dx must have been written.
Inputs: +-U[0.25, 1) (test_gemm_gpu.draw) mixed with rows around +-64 of spread 1, constant rows, all-zero rows and one row of magnitude
~1e4, spread with period 11 and forced onto the last four rows; no inf, no NaN.

profiles/test_layernorm_gpu_kernels.txt is the record of one rocprofv3 --kernel-trace --stats run of this module alone: it shows every
ln_fwd2_kernel / ln_bwd2_kernel<T, 16 | 32 | 64, 1 | 2 | 3> (16x1, 32x1, 64x1, 64x2, 64x3), ln_fwd_kernel / ln_bwd_kernel<T, 24> and
ln_bwd_chain_kernel<T, 16 | 32 | 64>, each for float, bf16 and f16.  Not reached, on purpose: the grid caps (2048 / 4096 forward workgroups, 256 backward workgroups: they need more than the 4096 rows
EPS_ELEM[float32] is stated for, bar 64x3 backward whose 4-row pass reaches 256 at 1024 rows -- not in the matrix); beta misaligned on its
own (gamma misaligned takes the same branch); ngroups > 1 with group_rows <= 0 is no refusal in stj_layernorm_bwd (one run of
parameter set 0: test_backward_without_group_rows_is_one_run holds it to that).
"""
import pytest
import torch

import _layernorm_cases as LC
from _layernorm_cases import DTYPES, F32, chaincase, gcase, judge, lncase, matrix, prepare
from test_gemm_gpu import bits

pytestmark = pytest.mark.gpu

_RATIOS = []
OK, EINVAL, EUNSUPPORTED = 0, -1, -3


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


def abi(p, dev, **over):
    """(entry point, argument list) of the call a Prep describes; `over` replaces arguments by name"""
    from strajnet_amd import ops
    cs = p.cs
    v = {k: ops._poff(dev[k], b.base) for k, b in p.bufs.items()}
    v.update(rows=cs['rows'], C=cs['C'], eps=float(cs['eps']), dtype=ops.DTYPE_CODE[p.dt], stream=ops._st())
    if p.kind == 'chain':
        v.update(nparts2=cs['np2'], part_stride2=cs['ps2'], nparts1=cs['np1'], part_stride1=cs['ps1'])
        if not cs['d2out']:
            v['d2out'] = None
        name = 'stj_layernorm_bwd_chain'
        order = ('dy', 'x2', 'gamma2', 'mean2', 'rstd2', 'x1', 'gamma1', 'mean1', 'rstd1', 'd2out', 'dx1', 'dgamma2', 'dbeta2', 'dgamma1', 'dbeta1', 'rows', 'C',
                 'nparts2', 'part_stride2', 'nparts1', 'part_stride1', 'dtype', 'stream')
    else:
        v.update(gather_res=cs['gres'], C0=cs['C0'], group_rows=cs['group_rows'], ngroups=cs['ngroups'], gstride=cs['gstride'], nparts=cs['nparts'],
                 part_stride=cs['pstride'])
        v.setdefault('dres', None)
        if p.kind == 'bwd':
            name = 'stj_layernorm_bwd'
            order = ('dy', 'x', 'gamma', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta', 'rows', 'C', 'gather_res', 'C0', 'group_rows', 'ngroups', 'gstride', 'dres',
                     'nparts', 'part_stride', 'dtype', 'stream')
        elif cs['res']:
            name = 'stj_layernorm_res_fwd'
            order = ('x', 'gamma', 'beta', 'res', 'y', 'mean', 'rstd', 'rows', 'C', 'eps', 'group_rows', 'ngroups', 'gstride', 'dtype', 'stream')
        else:
            name = 'stj_layernorm_fwd'
            order = ('x', 'gamma', 'beta', 'y', 'mean', 'rstd', 'rows', 'C', 'eps', 'gather_res', 'C0', 'group_rows', 'ngroups', 'gstride', 'dtype', 'stream')
    assert not set(over) - set(v), set(over) - set(v)
    v.update(over)
    return name, [ops._p(v[k]) if (v[k] is None or isinstance(v[k], ops.vp)) else v[k] for k in order]


def upload(p):
    return {k: b.init.cuda() for k, b in p.bufs.items()}


def download(dev):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in dev.items()}


def run_case(cs, dt):
    from strajnet_amd import ops
    for kind in cs['kinds']:
        for exact in ((False,) if kind == 'fwd' else (False, True)):
            p = prepare(cs, dt, kind, exact)
            dev = upload(p)
            name, args = abi(p, dev)
            ops.call(name, *args)
            judge(p, download(dev), _RATIOS, per_copy=True)


def run_family(family, dt):
    """Every case of one row of the matrix in one test; all cases run, and the failure names each case that missed with its own message."""
    cases = matrix(dt)[family]
    failed = []
    for cs in cases:
        try:
            run_case(cs, dt)
        except AssertionError as e:
            failed.append(f"{cs['name']} [{dt}]: {e}")
    assert not failed, f'{len(failed)} of {len(cases)} cases failed:\n' + '\n'.join(failed)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_v2_instantiations(dt):
    run_family('v2', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_v1_for_each_reason(dt):
    run_family('v1', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_patch_merging_gather(dt):
    run_family('gather', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_parameter_groups(dt):
    run_family('groups', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_partial_copies(dt):
    run_family('parts', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_res_forward_and_dres(dt):
    run_family('res', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_backward_chain(dt):
    run_family('chain', dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_backward_without_group_rows_is_one_run(dt):
    """stj_layernorm_bwd with ngroups > 1 and group_rows <= 0 is not refused (the forward entry points refuse it): all rows form one run of
    parameter set 0, the other sets' gradients keep their starting values.  Vector and scalar kernels, bound and exact twin.
    This pins today's behaviour, it is no contract: when backward is made to refuse like forward, turn this into a case of test_refusals_write_nothing."""
    from strajnet_amd import ops
    for C in (96, 100 if dt != F32 else 98):
        for exact in (False, True):
            p = prepare(lncase(f'no_group_rows_C{C}', 150, C, ngroups=2, group_rows=150, gstride=C + 8, dres=True, kinds=('bwd',)), dt, 'bwd', exact)
            dev = upload(p)
            name, args = abi(p, dev, group_rows=0)
            ops.call(name, *args)
            judge(p, download(dev), _RATIOS)


def test_chain_supported_follows_the_header_rule():
    """C a positive multiple of the 16-byte vector (4 f32 / 8 16-bit elements), at most 64 vectors; a known dtype"""
    from strajnet_amd import ops
    from strajnet_amd._lib import lib
    for dt in DTYPES:
        vn = LC.vn_of(dt)
        for C in (-8, 0, 1, 4, 8, 12, 16, 96, 100, 128, 252, 256, 260, 264, 384, 504, 512, 516, 520, 768, 1536):
            want = int(C > 0 and C % vn == 0 and C // vn <= 64)
            assert lib().stj_layernorm_bwd_chain_supported(C, ops.DTYPE_CODE[dt]) == want, (C, dt)
    assert lib().stj_layernorm_bwd_chain_supported(96, 7) == 0


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_refusals_write_nothing(dt):
    """Each refusal returns its code before any launch (and rows = 0 returns STJ_OK); every buffer is bit-identical afterwards.  The buffers are
    real ones of the stated geometry (with slack behind x and dx), so no argument list here describes an out-of-bounds access."""
    from strajnet_amd._lib import lib
    wide = 1600 if dt == F32 else 1537
    plain, gath = lncase('refuse', 40, 96, dres=True), gcase('refuse_gather', 1, 4, 24, tail=4096)
    grp = lncase('refuse_groups', 40, 96, ngroups=2, group_rows=10, gstride=96, res=True)
    chain, chain_odd = chaincase('refuse_chain', 40, 96, np2=2, ps2=96, np1=2, ps1=96), chaincase('refuse_chain_C', 8, 100 if dt != F32 else 98)
    calls = [(lncase('refuse_wide', 4, wide), 'fwd', {}, EUNSUPPORTED), (lncase('refuse_wide', 4, wide), 'bwd', {}, EUNSUPPORTED),
             (lncase('refuse_wide', 4, wide, res=True), 'fwd', {}, EUNSUPPORTED),
             (gath, 'fwd', dict(C0=48), EINVAL), (gath, 'fwd', dict(gather_res=3), EINVAL),
             (grp, 'fwd', dict(group_rows=0), EINVAL), (dict(grp, res=False), 'fwd', dict(group_rows=-5), EINVAL),
             (plain, 'bwd', dict(nparts=0), EINVAL), (plain, 'bwd', dict(nparts=-1), EINVAL), (plain, 'bwd', dict(nparts=2, part_stride=95), EINVAL),
             (dict(gath, dres=True), 'bwd', {}, EINVAL),
             (chain_odd, 'chain', {}, EUNSUPPORTED),
             (chain, 'chain', dict(nparts2=0), EINVAL), (chain, 'chain', dict(nparts1=2, part_stride1=95), EINVAL)]
    calls += [(chain, 'chain', {k: None}, EINVAL) for k in ('dy', 'x2', 'x1', 'dx1', 'gamma2', 'gamma1', 'mean2', 'rstd2', 'mean1', 'rstd1', 'dgamma2', 'dbeta2',
                                                           'dgamma1', 'dbeta1')]
    calls += [(chain, 'chain', {k: 'off'}, EINVAL) for k in ('dy', 'x2', 'x1', 'dx1', 'd2out')]
    calls += [(c, k, dict(rows=0), OK) for c, k in ((plain, 'fwd'), (dict(plain, res=True), 'fwd'), (plain, 'bwd'), (chain, 'chain'))]
    calls += [(plain, 'fwd', dict(rows=-3), OK)]
    for cs, kind, over, want in calls:
        from strajnet_amd import ops
        p = prepare(cs, dt, kind, False)
        dev = upload(p)
        over = {k: (ops._poff(dev[k], p.bufs[k].base + 1) if v == 'off' else v) for k, v in over.items()}
        name, args = abi(p, dev, **over)
        rc = getattr(lib(), name)(*args)
        assert rc == want, (cs['name'], kind, over, rc, want)
        if rc != OK:
            assert name.replace('stj_', '').split('_')[0] in lib().stj_last_error().decode(), (cs['name'], lib().stj_last_error())
        after = download(dev)
        for k, b in p.bufs.items():
            assert torch.equal(bits(after[k]), bits(b.init)), (cs['name'], kind, over, k)
    # the unmodified argument lists are legal
    for cs, kind in ((plain, 'fwd'), (plain, 'bwd'), (gath, 'fwd'), (grp, 'fwd'), (chain, 'chain')):
        p = prepare(cs, dt, kind, False)
        dev = upload(p)
        name, args = abi(p, dev)
        assert getattr(lib(), name)(*args) == OK
        judge(p, download(dev))


def test_zz_report_layernorm_error_ratios():
    """(runs last in this file) the largest |err| / T per (entry point, path, dtype, output), under pytest -s"""
    LC.report(_RATIOS, 'layernorm')
