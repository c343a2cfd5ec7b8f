"""Per-kernel parity: every HIP op (forward + backward) against a float64 PyTorch-CPU statement of the same op.

Tolerances: f32 mode (exact-f32 MFMA, the parity mode) ~1e-4 relative-to-scale; bf16 mode ~3e-2; fp16 mode ~5e-3.
All calls go through the C-ABI library via strajnet_amd.ops.
The up-conv weight gradient (stj_upconv_prep / _wgrad / _fold) is held per dispatch path, in exact integers and per element against float64,
by test_upconv_wgrad_abi_gpu.py; the test_upconv cases here reach its generic and 256-thread kernels only.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def tol(dt):
    # bf16: 2e-2 of the tensor maximum (round 3: 4e-2).  Swept on MI355X: every op-level test passes at 2e-2; at 1e-2 only the three
    # C = 384 fused attention-half cases fail (the kernels of the timed step have their own per-element bounds in
    # test_timed_kernels_gpu.py, test_wgrad_sk_gpu.py and test_inference_heads_in_upconv_epilogue)
    return {torch.float32: 2e-4, torch.bfloat16: 2e-2, torch.float16: 6e-3}[dt]


RMS_WEIGHT = 2.5


def rel_err(a, ref, rms_weight=None):
    """max( max |a - ref| / max |ref| ,  RMS_WEIGHT * rms(a - ref) / rms(ref) ): the worst element against the tensor's scale AND the
    error of the tensor as a whole.  (Round 5: the first term alone lets every element be off by the tolerance x the tensor maximum; the
    second holds the root-mean-square error to tol / 2.5 -- 8e-3 in bf16, 2.4e-3 in fp16, 8e-5 in f32 -- of the root-mean-square value, which a dropped tap, a wrong scale
    or a systematically mis-rounded operand does not pass.  Measured on MI355X: the largest rms ratio of any bf16 case in this file is
    printed by `pytest -s` through STJ_TEST_REPORT.)"""
    a = a.detach().double().cpu()
    ref = ref.detach().double().cpu()
    d = a - ref
    e_max = float(d.abs().max() / (ref.abs().max() + 1e-12))
    e_rms = float(d.pow(2).mean().sqrt() / (ref.pow(2).mean().sqrt() + 1e-12))
    _SEEN.append((e_max, e_rms))
    return max(e_max, (RMS_WEIGHT if rms_weight is None else rms_weight) * e_rms)


_SEEN = []

# Per-element bound for the GEMM-shaped ops (round 5; the timed kernels have theirs in test_timed_kernels_gpu.py): every product term
# carries at most four storage roundings the float64 reference does not have (an operand the kernel folds or rounds -- folded conv
# weights, dpre --, up to two intermediates -- the output heads' input gradient passes its phase partials through LDS in 16 bits --, the
# stored result), so |got - ref| <= 4 * 2^-p * sum_k |a_k b_k| per element (bf16: 2^-7, the EPS_ACT of the timed tests), with the sum evaluated
# in float64 on |operands|; f32 storage: exact products, float32 accumulation over K <= 3456 terms.  A dropped tap, a halo column read
# twice or one tile's flush lost moves single elements by whole terms and fails here whatever the tensor maximum is.
EPS_ELEM = {torch.float32: 2.0 ** -17, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
_ELEM = []


def elem_check(name, got, ref, bound, dt):
    got, ref, bound = got.detach().double().cpu(), ref.detach().double().cpu(), bound.detach().double().cpu().abs()
    ratio = float(((got - ref).abs() / (bound + 1e-300)).max())
    _ELEM.append((dt, name, ratio))
    assert ratio <= EPS_ELEM[dt], f'{name}: max |err| / sum |terms| = {ratio:.3e} over the per-element bound {EPS_ELEM[dt]:.3e}'



def mk_param(shape, dt, scale=0.1, seed=0):
    from strajnet_amd.ops import Param
    g = torch.Generator().manual_seed(seed)
    m = (torch.randn(shape, generator=g) * scale).cuda().requires_grad_(True)
    grad = torch.zeros(shape, device='cuda')
    m.grad = grad
    c = m.detach() if dt == torch.float32 else m.detach().to(dt)
    return Param('p', shape, m, c, grad)


def rnd(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    return x.to(dt).cuda()


def ref_of(t):
    """float64 CPU leaf holding exactly the values the kernel saw."""
    return t.detach().double().cpu().requires_grad_(True)


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('M,K,N,act,use_res', [(300, 96, 288, 0, False), (1000, 384, 96, 0, True), (77, 5, 64, 2, False),
                                               (64, 2, 384, 0, False), (513, 384, 126, 0, False), (4096, 96, 48, 2, False),
                                               # tile kernels at a few thousand rows (these were row-streaming shapes while its threshold was 2048 rows;
                                               # linear_rs_try takes M >= 16384 now -- that kernel is tested in test_gemm_gpu.py::test_row_streaming):
                                               # fwd [K,N] and dgrad [N,K] forms, ragged M, N % 64 != 0, bias+ELU, residual
                                               (2100, 96, 288, 0, True), (4133, 384, 96, 2, False), (2048, 192, 136, 0, False),
                                               (2050, 288, 96, 0, True), (2304, 128, 384, 2, False)])
def test_linear(dt, M, K, N, act, use_res):
    from strajnet_amd import ops
    pw, pb = mk_param((K, N), dt, 0.2, 1), mk_param((N,), dt, 0.2, 2)
    x = rnd((M, K), dt, 3).requires_grad_(True)
    res = rnd((M, N), dt, 4).requires_grad_(True) if use_res else None
    y = ops.linear(x, pw, pb, act, res)
    xr, wr, br = ref_of(x), ref_of(pw.c), ref_of(pb.master)
    yr = xr @ wr + br
    if act == 2:
        yr = F.elu(yr)
    rr = None
    if use_res:
        rr = ref_of(res)
        yr = yr + rr
    assert rel_err(y, yr) < tol(dt)
    g = rnd((M, N), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pw.grad, wr.grad) < tol(dt)
    assert rel_err(pb.grad, br.grad) < tol(dt)
    if use_res:
        assert rel_err(res.grad, rr.grad) < tol(dt)
    # per element, against sum |terms| (ELU: |ELU(a)| <= |a|, 1-Lipschitz, ELU' <= 1)
    xa, wa, ga = xr.detach().abs(), wr.detach().abs(), g.double().cpu().abs()
    elem_check('linear y', y, yr, xa @ wa + br.detach().abs() + (rr.detach().abs() if use_res else 0.0), dt)
    elem_check('linear dx', x.grad, xr.grad, ga @ wa.t(), dt)
    elem_check('linear dw', pw.grad, wr.grad, xa.t() @ ga, dt)
    elem_check('linear db', pb.grad, br.grad, ga.sum(0), dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('rows,C,eps', [(1000, 96, 1e-5), (300, 384, 1e-3), (64, 128, 1e-3), (50, 768, 1e-5)])
def test_layernorm(dt, rows, C, eps):
    from strajnet_amd import ops
    pg, pb = mk_param((C,), dt, 0.3, 1), mk_param((C,), dt, 0.3, 2)
    with torch.no_grad():
        pg.master.add_(1.0)
    x = rnd((rows, C), dt, 3, 2.0).requires_grad_(True)
    y = ops.layernorm(x, pg, pb, eps)
    xr, gr, br = ref_of(x), ref_of(pg.master), ref_of(pb.master)
    yr = F.layer_norm(xr, (C,), gr, br, eps)
    assert rel_err(y, yr) < tol(dt)
    g = rnd((rows, C), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pg.grad, gr.grad) < tol(dt)
    assert rel_err(pb.grad, br.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('rows,C', [(300, 96), (257, 384), (64, 100)])
def test_layernorm_res(dt, rows, C):
    """LayerNorm(x) + res from one pass (v2 vector path; C = 100 is the scalar v1 path in the 16-bit types only -- in f32 100 is a whole
    number of 4-element vectors and takes v2 too; test_layernorm_gpu.py reaches v1 in every type); d res = dy."""
    from strajnet_amd import ops
    pg, pb = mk_param((C,), dt, 0.3, 1), mk_param((C,), dt, 0.3, 2)
    x = rnd((rows, C), dt, 3, 2.0).requires_grad_(True)
    r = rnd((rows, C), dt, 4, 2.0).requires_grad_(True)
    y = ops.layernorm(x, pg, pb, 1e-3, res=r)
    xr, rr, gr, br = ref_of(x), ref_of(r), ref_of(pg.master), ref_of(pb.master)
    yr = F.layer_norm(xr, (C,), gr, br, 1e-3) + rr
    assert rel_err(y, yr) < tol(dt)
    g = rnd((rows, C), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert torch.equal(r.grad, g)
    assert rel_err(pg.grad, gr.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_layernorm_merge_gather(dt):
    from strajnet_amd import ops
    B, res, C0 = 2, 16, 96
    pg, pb = mk_param((4 * C0,), dt, 0.3, 1), mk_param((4 * C0,), dt, 0.3, 2)
    x = rnd((B, res * res, C0), dt, 3).requires_grad_(True)
    y = ops.layernorm(x, pg, pb, 1e-5, gather_res=res)
    xr, gr, br = ref_of(x), ref_of(pg.master), ref_of(pb.master)
    xx = xr.view(B, res, res, C0)
    cat = torch.cat([xx[:, 0::2, 0::2], xx[:, 1::2, 0::2], xx[:, 0::2, 1::2], xx[:, 1::2, 1::2]], -1)   # modules.py:282-286
    yr = F.layer_norm(cat.reshape(B, -1, 4 * C0), (4 * C0,), gr, br, 1e-5)
    assert rel_err(y, yr) < tol(dt)
    g = rnd(tuple(y.shape), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pg.grad, gr.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_unary(dt):
    from strajnet_amd import ops
    for fn, rf in ((ops.gelu, lambda t: F.gelu(t, approximate='tanh')), (ops.elu, F.elu),
                   (lambda t: ops.tanh_scale(t, 8.0), lambda t: torch.tanh(t) * 8.0)):
        x = rnd((1000, 37), dt, 1, 2.0).requires_grad_(True)
        y = fn(x)
        xr = ref_of(x)
        yr = rf(xr)
        assert rel_err(y, yr) < tol(dt)
        g = rnd((1000, 37), dt, 2)
        y.backward(g)
        yr.backward(g.double().cpu())
        assert rel_err(x.grad, xr.grad) < tol(dt)


def _win_ref(qkv, table, B, res, heads, shift):
    """float64 restatement with the index formulation of oracle/torch_ref.py."""
    from oracle.torch_ref import _win_index, _region_id
    C = heads * 32
    N = 64
    idx = _win_index(res, 8, shift, qkv.device)
    nW = idx.shape[0]
    t = qkv[:, idx].view(B, nW, N, 3, heads, 32)
    q, k, v = t[..., 0, :, :], t[..., 1, :, :], t[..., 2, :, :]
    att = torch.einsum('bwnhd,bwmhd->bwhnm', q * 32 ** -0.5, k)
    c = torch.arange(8)
    yy, xx = torch.meshgrid(c, c, indexing='ij')
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    ridx = (yy[:, None] - yy[None, :] + 7) * 15 + (xx[:, None] - xx[None, :] + 7)
    att = att + table[ridx].permute(2, 0, 1)
    if shift > 0:
        lab = _region_id(res, 8, shift, qkv.device)
        labw = lab.view(res // 8, 8, res // 8, 8).permute(0, 2, 1, 3).reshape(nW, N)
        att = att + ((labw[:, :, None] != labw[:, None, :]).double() * -100.0)[None, :, None]
    o = torch.einsum('bwhnm,bwmhd->bwnhd', att.softmax(-1), v).reshape(B, nW * N, C)
    return torch.zeros(B, res * res, C, dtype=torch.float64).index_copy(1, idx.reshape(-1), o)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('res,heads,shift', [(16, 3, 0), (16, 3, 4), (32, 6, 4), (8, 12, 0)])
def test_win_attn(dt, res, heads, shift):
    from strajnet_amd import ops
    B, C = 2, heads * 32
    pt = mk_param((225, heads), dt, 0.5, 1)
    qkv = rnd((B, res * res, 3 * C), dt, 2).requires_grad_(True)
    out = ops.win_attn(qkv, pt, B, res, heads, shift)
    qr, tr = ref_of(qkv), ref_of(pt.master)
    outr = _win_ref(qr, tr, B, res, heads, shift)
    assert rel_err(out, outr) < tol(dt)
    g = rnd(tuple(out.shape), dt, 3)
    out.backward(g)
    outr.backward(g.double().cpu())
    assert rel_err(qkv.grad, qr.grad) < tol(dt)
    assert rel_err(pt.grad, tr.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('Bt,Nq,Nk,H,d,masks,use_bias', [(6, 11, 11, 4, 64, 'qk', False), (5, 11, 11, 4, 80, 'qk', False), (3, 16, 16, 2, 24, '', False),
                                                        (2, 64, 64, 6, 64, 'qk', False),
                                                        (3, 256, 64, 3, 42, 'k', False), (2, 64, 64, 8, 48, '', True)])
def test_mha_core(dt, Bt, Nq, Nk, H, d, masks, use_bias):
    from strajnet_amd import ops
    q = rnd((Bt, Nq, H * d), dt, 1).requires_grad_(True)
    k = rnd((Bt, Nk, H * d), dt, 2).requires_grad_(True)
    v = rnd((Bt, Nk, H * d), dt, 3).requires_grad_(True)
    g = torch.Generator().manual_seed(4)
    qv = (torch.rand((Bt, Nq), generator=g) > 0.3).int().cuda() if 'q' in masks else None
    kv = (torch.rand((Bt, Nk), generator=g) > 0.3).int().cuda() if 'k' in masks else None
    if kv is not None:
        kv[0] = 0                                   # one fully masked batch entry -> uniform softmax (tfa -1e10 semantics)
    bias = (torch.randn((Bt, H, Nq, Nk), generator=g)).cuda().requires_grad_(True) if use_bias else None
    scale = 1.0 / math.sqrt(d)
    o = ops.mha_core(q, k, v, H, d, scale, qvalid=qv, kvalid=kv, bias=bias)
    qr, kr, vr = ref_of(q), ref_of(k), ref_of(v)
    lg = torch.einsum('bnhd,bmhd->bhnm', qr.view(Bt, Nq, H, d), kr.view(Bt, Nk, H, d)) * scale
    br = None
    if use_bias:
        br = ref_of(bias)
        lg = lg + br
    m = torch.ones(Bt, Nq, Nk, dtype=torch.bool)
    if qv is not None:
        m &= qv.cpu().bool()[:, :, None]
    if kv is not None:
        m &= kv.cpu().bool()[:, None, :]
    lg = torch.where(m[:, None], lg, lg + (-10e9 - lg).detach())     # value -1e10, gradient of the add passes through
    orf = torch.einsum('bhnm,bmhd->bnhd', lg.softmax(-1), vr.view(Bt, Nk, H, d)).reshape(Bt, Nq, H * d)
    assert rel_err(o, orf) < tol(dt)
    go = rnd(tuple(o.shape), dt, 5)
    o.backward(go)
    orf.backward(go.double().cpu())
    assert rel_err(q.grad, qr.grad) < tol(dt)
    assert rel_err(k.grad, kr.grad) < tol(dt)
    assert rel_err(v.grad, vr.grad) < tol(dt)
    if use_bias:
        assert rel_err(bias.grad, br.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_small_attn_matches_layerwise_with_dropout(dt):
    """stj_small_attn_* (one launch per direction for <= 16 queries / keys) against the layer-by-layer path it replaces (GEMM, softmax, dropout,
    GEMM) with attention dropout on: the SAME Philox draws of the [Bt,H,N,N] coefficients, so values and gradients agree to rounding."""
    from strajnet_amd import ops
    Bt, N, H, d = 40, 11, 4, 80
    q, k, v = (rnd((Bt, N, H * d), dt, 30 + i).requires_grad_(True) for i in range(3))
    g = torch.Generator().manual_seed(4)
    qv = (torch.rand((Bt, N), generator=g) > 0.3).int().cuda()
    qv[1] = 0
    go = rnd((Bt, N, H * d), dt, 5)
    res = []
    for small in (True, False):
        ops.SMALL_ATTN = small
        try:
            dctx = ops.DropCtx('cuda', seed=21)
            dctx.begin()
            drop = (0.1, dctx.snap, dctx.site('a', (Bt, H, N, N), 0.1))
            for t in (q, k, v):
                t.grad = None
            o = ops.mha_core(q, k, v, H, d, d ** -0.5, qvalid=qv, kvalid=qv, drop=drop)
            o.backward(go)
            res.append([o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone(), dctx.mask('a').clone()])
        finally:
            ops.SMALL_ATTN = True
    assert torch.equal(res[0][4], res[1][4]) and 0.05 < 1.0 - float(res[0][4].float().mean()) < 0.15
    for a, b in zip(res[0][:4], res[1][:4]):
        assert rel_err(a, b) < (2e-5 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize('dt', DTYPES)
def test_fg_bias(dt):
    from strajnet_amd import ops
    from oracle.torch_ref import _sample
    B, G, Hh = 2, 8, 8
    HW = Hh * Hh
    pt = mk_param((2 * Hh - 1, 2 * Hh - 1, G), dt, 0.5, 1)
    off = (rnd((B, G, HW, 2), dt, 2, 3.0)).requires_grad_(True)
    bias = ops.fg_bias(off, pt, Hh, Hh)
    offr, tr = ref_of(off), ref_of(pt.master)
    ii, jj = torch.meshgrid(torch.arange(Hh, dtype=torch.float64), torch.arange(Hh, dtype=torch.float64), indexing='ij')
    ref = torch.stack((jj, ii), -1).view(1, 1, HW, 2)
    pos = offr + ref
    disp = ref.view(1, 1, HW, 1, 2) - pos.view(B, G, 1, HW, 2)
    warp = torch.stack((disp[..., 1], disp[..., 0]), -1)
    tab = tr.permute(2, 0, 1)[None].expand(B, -1, -1, -1).reshape(B * G, 2 * Hh - 1, 2 * Hh - 1, 1)
    br = _sample(tab, warp.reshape(B * G, HW, HW, 2)).view(B, G, HW, HW)
    assert rel_err(bias, br) < (1e-4 if dt == torch.float32 else 1e-4)
    g = torch.randn(B, G, HW, HW, generator=torch.Generator().manual_seed(3))
    bias.backward(g.cuda())
    br.backward(g.double())
    assert rel_err(pt.grad, tr.grad) < tol(dt)
    if dt == torch.float32:     # bf16 offsets land on exact integers, where TF's clip gradient (0) != grid_sample's one-sided one
        assert rel_err(off.grad, offr.grad) < tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_agent_branch_ops(dt):
    """trajNet plumbing (stj_agent_prep) and branch sums (stj_agent_mix / _sum) against the torch expressions they replace."""
    from strajnet_amd import ops
    B, n_obs, n_occ, T, C = 3, 5, 3, 11, 64
    A = n_obs + n_occ
    g = torch.Generator().manual_seed(0)
    obs, occ = torch.randn(B, n_obs, T, 8, generator=g), torch.randn(B, n_occ, T, 8, generator=g)
    obs[0, 1] = 0.0                                   # an absent agent
    occ[1, 2, 3:, 0] = 0.0                            # invalid steps
    obs[2, :, :, 0] = 0.0                             # a scene without observed agents
    x5, v3, vt, cmi, cmf = ops.agent_prep(obs.cuda(), occ.cuda(), dt)
    tr = torch.cat([obs, occ], 1)
    valid = tr[..., 0] != 0
    assert torch.equal(vt.cpu(), valid.reshape(B * A, T).int())
    assert torch.equal(cmi.cpu(), valid.any(-1).int())
    assert torch.equal(cmf.float().cpu(), valid.any(-1).float())
    assert torch.equal(x5.cpu(), tr[..., :5].to(dt).reshape(-1, 5))
    assert torch.equal(v3.cpu(), tr[:, :, 0, 5:].to(dt).reshape(-1, 3))
    enc, value = rnd((B, A, C), dt, 1).requires_grad_(True), rnd((B, A, C), dt, 2).requires_grad_(True)
    embed = rnd((A, C), dt, 3).requires_grad_(True)
    concat, qin = ops.agent_mix(enc, embed, cmf)
    out = ops.agent_sum(enc, value, embed)
    er, vr, mr, cr = ref_of(enc), ref_of(value), ref_of(embed), cmf.double().cpu()
    cref = er * cr[..., None]
    assert rel_err(concat, cref) < tol(dt) and rel_err(qin, cref + mr[None]) < tol(dt) and rel_err(out, er + vr + mr[None]) < tol(dt)
    g1, g2, g3 = rnd((B, A, C), dt, 4), rnd((B, A, C), dt, 5), rnd((B, A, C), dt, 6)
    torch.autograd.backward([concat, qin, out], [g1, g2, g3])
    torch.autograd.backward([cref, cref + mr[None], er + vr + mr[None]], [g1.double().cpu(), g2.double().cpu(), g3.double().cpu()])
    assert rel_err(enc.grad, er.grad) < tol(dt)
    assert rel_err(value.grad, vr.grad) < tol(dt)
    assert rel_err(embed.grad, mr.grad) < 2 * tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_agent_out_fused_tail(dt):
    """stj_agent_out_fwd / _bwd (enc + value + embed, obs_norm | occ_norm by agent index: trajNet.py:171-187) against float64 and against the
    layer-by-layer composition it replaces (agent_sum, two slice LayerNorms, concat): same values, same gradients."""
    from strajnet_amd import ops
    B, n_obs, A, C = 3, 48, 64, 384
    enc, value = rnd((B, A, C), dt, 1).requires_grad_(True), rnd((B, A, C), dt, 2).requires_grad_(True)
    embed = rnd((A, C), dt, 3).requires_grad_(True)
    g = rnd((B, A, C), dt, 4)
    res = []
    for fused in (True, False):
        ps = [mk_param((C,), dt, 0.3, 10 + i) for i in range(4)]
        with torch.no_grad():
            ps[0].master.add_(1.0); ps[2].master.add_(1.0)
        for t in (enc, value, embed):
            t.grad = None
        if fused:
            y = ops.agent_out(enc, value, embed, ps[0], ps[1], ps[2], ps[3], n_obs, 1e-3)
        else:
            out = ops.agent_sum(enc, value, embed)
            y = torch.cat([ops.layernorm(out[:, :n_obs].contiguous(), ps[0], ps[1], 1e-3), ops.layernorm(out[:, n_obs:].contiguous(), ps[2], ps[3], 1e-3)], 1)
        y.backward(g)
        res.append([y.detach().clone(), enc.grad.clone(), value.grad.clone(), embed.grad.clone()] + [p_.grad.clone() for p_ in ps])
    for a, b in zip(*res):
        assert rel_err(a, b) < (1e-5 if dt == torch.float32 else 1e-2)
    er, vr, mr = ref_of(enc), ref_of(value), ref_of(embed)
    pr = [ref_of(p_.master) for p_ in ps]
    o = ((er + vr).to(dt).double() + mr).to(dt).double()   # the kernels round the first sum to the storage type, then the second
    yr = torch.cat([F.layer_norm(o[:, :n_obs], (C,), pr[0], pr[1], 1e-3), F.layer_norm(o[:, n_obs:], (C,), pr[2], pr[3], 1e-3)], 1)
    yr.backward(g.double().cpu())
    assert rel_err(res[0][0], yr) < tol(dt)
    assert rel_err(res[0][1], er.grad) < tol(dt) and rel_err(res[0][3], mr.grad) < 2 * tol(dt)
    for i in range(4):
        assert rel_err(res[0][4 + i], pr[i].grad) < 2 * tol(dt), i


@pytest.mark.parametrize('dt', DTYPES)
def test_mha_core_with_fg_bias_inside(dt):
    """mha_core(fg_off=, fg=) == mha_core(bias=fg_bias(off)): same kernels, the bias gradient just never leaves the op."""
    from strajnet_amd import ops
    B, G, Hh, d = 2, 8, 8, 16
    HW = Hh * Hh
    q, k, v = (rnd((B, HW, G * d), dt, 10 + i).requires_grad_(True) for i in range(3))
    off = rnd((B, G, HW, 2), dt, 2, 3.0).requires_grad_(True)
    go = rnd((B, HW, G * d), dt, 5)
    res = []
    for inside in (False, True):
        pt = mk_param((2 * Hh - 1, 2 * Hh - 1, G), dt, 0.5, 1)
        for t in (q, k, v, off):
            t.grad = None
        if inside:
            o = ops.mha_core(q, k, v, G, d, d ** -0.5, fg_off=off, fg=(pt, Hh, Hh))
        else:
            o = ops.mha_core(q, k, v, G, d, d ** -0.5, bias=ops.fg_bias(off, pt, Hh, Hh))
        o.backward(go)
        res.append([o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone(), off.grad.clone(), pt.grad.clone()])
    for i, (a, b) in enumerate(zip(*res)):
        if i < 4:
            assert torch.equal(a, b)
        else:               # offset / table gradients are accumulated with f32 atomics: same terms, run-dependent order
            assert rel_err(b, a) < 1e-5


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('B,Hh,G,gc,C2', [(2, 16, 8, 48, 384), (1, 8, 4, 24, 64)])
def test_fg_offset_head(dt, B, Hh, G, gc, C2):
    """Both halves of the FG-MSA offset head against dense float64 statements (FG_MSA.py:136-146, modules.py:827-831)."""
    from strajnet_amd import ops
    HW = Hh * Hh
    p1, p2, pb2 = mk_param((1, 1, gc, 2), dt, 0.2, 1), mk_param((1, 1, 2, C2), dt, 0.3, 2), mk_param((C2,), dt, 0.1, 3)
    o = rnd((B, Hh, Hh, G * gc), dt, 4).requires_grad_(True)
    qres = rnd((B, HW, C2), dt, 5).requires_grad_(True)
    scale = Hh / 2.0
    off = ops.fg_offset(o, p1, scale, G)
    query = ops.fg_query(off, p2, pb2, qres=qres)                 # [G,B,HW,C2]
    fh = ops.fg_query(off, p2, pb2)                               # [B,G,HW,C2]
    orf, qr, w1, w2, b2 = ref_of(o), ref_of(qres), ref_of(p1.master), ref_of(p2.master), ref_of(pb2.master)
    offr = torch.tanh(orf.view(B, HW, G, gc).permute(0, 2, 1, 3) @ w1.view(gc, 2)) * scale
    assert rel_err(off, offr) < tol(dt)
    offq = off.detach().double().cpu()                            # the second half sees the rounded offsets
    fhr = offq @ w2.view(2, C2).detach() + b2.detach()
    assert rel_err(fh, fhr) < tol(dt)
    assert rel_err(query, fhr.permute(1, 0, 2, 3) + qr.detach()[None]) < tol(dt)
    # gradients: both consumers of off at once (autograd adds their offset gradients)
    g1, g2, g3 = rnd(tuple(query.shape), dt, 6), rnd(tuple(fh.shape), dt, 7), rnd(tuple(off.shape), dt, 8)
    torch.autograd.backward([query, fh, off], [g1, g2, g3])
    fr = offr @ w2.view(2, C2) + b2
    torch.autograd.backward([fr.permute(1, 0, 2, 3) + qr[None], fr, offr],
                            [g1.double().cpu(), g2.double().cpu(), g3.double().cpu()])
    t = tol(dt) * (1 if dt == torch.float32 else 2)
    assert rel_err(qres.grad, qr.grad) < t
    assert rel_err(o.grad, orf.grad) < t
    assert rel_err(p1.grad, w1.grad) < t
    assert rel_err(p2.grad, w2.grad) < t
    assert rel_err(pb2.grad, b2.grad) < t


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('F_,Hi,Cin,Cout', [(2, 8, 384, 192), (2, 16, 192, 128), (1, 32, 128, 96), (1, 32, 96, 48), (3, 16, 96, 48),
                                            (2, 24, 96, 48),       # 24 x 24: ragged tiles (guarded movers of the 96 <- 48 input gradient)
                                            (2, 24, 128, 96), (1, 8, 128, 96)])    # the wave-specialised forward at 128 -> 96 (round 6): ragged tiles; fewer tiles than one walker set (2-D grid)
def test_upconv(dt, F_, Hi, Cin, Cout):
    from strajnet_amd import ops
    pw, pb = mk_param((3, 3, Cin, Cout), dt, 0.05, 1), mk_param((Cout,), dt, 0.1, 2)
    x = rnd((F_, Hi, Hi, Cin), dt, 3).requires_grad_(True)
    y = ops.upconv(x, pw, pb)
    xr, wr, br = ref_of(x), ref_of(pw.master), ref_of(pb.master)
    up = F.interpolate(xr.permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
    yr = F.elu(F.conv2d(up, wr.permute(3, 2, 0, 1), br, padding=1)).permute(0, 2, 3, 1)
    assert rel_err(y, yr) < tol(dt)
    g = rnd(tuple(y.shape), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pw.grad, wr.grad) < tol(dt)
    assert rel_err(pb.grad, br.grad) < tol(dt)
    # per element: the same graph on |operands| without the ELU (|ELU(a)| <= |a|, ELU' <= 1) gives sum |terms| of all four results
    xa, wa, ba = ref_of(x.detach().abs()), ref_of(pw.master.detach().abs()), ref_of(pb.master.detach().abs())
    ya = F.conv2d(F.interpolate(xa.permute(0, 3, 1, 2), scale_factor=2, mode='nearest'), wa.permute(3, 2, 0, 1), ba, padding=1).permute(0, 2, 3, 1)
    ya.backward(g.double().cpu().abs())
    elem_check('upconv y', y, yr, ya, dt)
    elem_check('upconv dx', x.grad, xr.grad, xa.grad, dt)
    elem_check('upconv dw', pw.grad, wr.grad, wa.grad, dt)
    elem_check('upconv db', pb.grad, br.grad, ba.grad, dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_outconv_pair(dt):
    from strajnet_amd import ops
    B, Tn, H, C = 2, 8, 32, 48
    ps = [mk_param((3, 3, C, 2), dt, 0.1, 1), mk_param((2,), dt, 0.1, 2), mk_param((3, 3, C, 2), dt, 0.1, 3), mk_param((2,), dt, 0.1, 4)]
    xo = rnd((B * Tn, H, H, C), dt, 5).requires_grad_(True)
    xf = rnd((B * Tn, H, H, C), dt, 6).requires_grad_(True)
    out = ops.outconv_pair(xo, xf, *ps, B, Tn)
    refs = [ref_of(p.master) for p in ps]
    xor_, xfr = ref_of(xo), ref_of(xf)

    def cv(t, w, b):
        return F.conv2d(t.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)
    y = torch.cat([cv(xor_, refs[0], refs[1]), cv(xfr, refs[2], refs[3])], -1).view(B, Tn, H, H, 4)
    outr = y.permute(0, 2, 3, 1, 4).reshape(B, H, H, 4 * Tn)                  # modules.py:838
    assert rel_err(out, outr) < tol(dt)
    g = torch.randn(B, H, H, 4 * Tn, generator=torch.Generator().manual_seed(7))
    out.backward(g.cuda())
    outr.backward(g.double())
    assert rel_err(xo.grad, xor_.grad) < tol(dt)
    assert rel_err(xf.grad, xfr.grad) < tol(dt)
    for p, r in zip(ps, refs):
        assert rel_err(p.grad, r.grad) < tol(dt)
    refa = [ref_of(p.master.detach().abs()) for p in ps]
    xoa, xfa = ref_of(xo.detach().abs()), ref_of(xf.detach().abs())
    ya = torch.cat([cv(xoa, refa[0], refa[1]), cv(xfa, refa[2], refa[3])], -1).view(B, Tn, H, H, 4).permute(0, 2, 3, 1, 4).reshape(B, H, H, 4 * Tn)
    ya.backward(g.double().abs())
    elem_check('outconv y', out, outr, ya, dt)
    elem_check('outconv dxo', xo.grad, xor_.grad, xoa.grad, dt)
    elem_check('outconv dxf', xf.grad, xfr.grad, xfa.grad, dt)
    for i, (p, r, ra) in enumerate(zip(ps, refs, refa)):
        elem_check(f'outconv dparam{i}', p.grad, r.grad, ra.grad, dt)


def test_outconv_generic_lds_grows_with_channels():
    """Raw stj_outconv_fwd / stj_outconv_bwd in f32 (always the generic kernels, whose dynamic LDS grows with the run-time C) at
    C = 8, 48, 64, 8 in one process and in this order: forward (324 (C + 1) + 18 C) * 4 bytes = 12 KB, 67 KB, 89 KB, 12 KB, i.e. below the
    64 KB default limit, over it, larger again, smaller again.  A reservation made once per kernel instead of per size fails the C = 64
    launch with a status code.  One 16 x 16 tile of one frame; references and bounds as in test_outconv_pair."""
    from strajnet_amd import _lib, ops
    L = _lib.lib()
    dt, H = torch.float32, 16
    cases = {}
    for C in (8, 48, 64, 8):
        if C not in cases:
            x, w, b = rnd((1, H, H, C), dt, 5), rnd((3, 3, C, 2), dt, 1, 0.1), rnd((2,), dt, 2, 0.1)
            g = rnd((1, H, H, 2), dt, 7)
            xr, wr, br = ref_of(x), ref_of(w), ref_of(b)
            xa, wa, ba = ref_of(x.abs()), ref_of(w.abs()), ref_of(b.abs())

            def cv(t, w_, b_):
                return F.conv2d(t.permute(0, 3, 1, 2), w_.permute(3, 2, 0, 1), b_, padding=1).permute(0, 2, 3, 1)
            yr, ya = cv(xr, wr, br), cv(xa, wa, ba)
            yr.backward(g.double().cpu())
            ya.backward(g.double().cpu().abs())
            cases[C] = (x, w, b, g, (yr, xr, wr, br), (ya, xa, wa, ba))
        x, w, b, g, (yr, xr, wr, br), (ya, xa, wa, ba) = cases[C]
        y, dx, dw, db = torch.empty_like(g), torch.empty_like(x), torch.zeros_like(w), torch.zeros_like(b)      # dW / db are "+="
        p = lambda t: ops.vp(t.data_ptr())
        rc_f = L.stj_outconv_fwd(p(x), p(w), p(b), p(y), 1, H, H, C, 1, H * H * 2, 2, 2, 0, ops._st())
        assert rc_f == 0, (C, rc_f, L.stj_last_error().decode())
        rc_b = L.stj_outconv_bwd(p(x), p(w), p(g), p(dx), p(dw), p(db), 1, H, H, C, 1, H * H * 2, 2, 2, 0, ops.vp(0), 0, 0, ops._st())
        assert rc_b == 0, (C, rc_b, L.stj_last_error().decode())
        torch.cuda.synchronize()
        for name, got, ref, bound in (('y', y, yr, ya), ('dx', dx, xr.grad, xa.grad), ('dw', dw, wr.grad, wa.grad), ('db', db, br.grad, ba.grad)):
            e = rel_err(got, ref)
            print(f'outconv generic C={C} {name}: rel_err {e:.3e}')
            assert e < tol(dt), (C, name, e)
            elem_check(f'outconv generic C={C} {name}', got, ref, bound, dt)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('t_major', [True, False])
def test_inference_heads_in_upconv_epilogue(dt, t_major):
    """stj_upconv_fwd_head + stj_outconv_pair_gather (inference: the [F,H,W,48] level never exists) against the two-kernel path
    (stj_upconv_fwd + stj_outconv_pair_fwd) and float64 (modules.py:746-748 at 96 -> 48, :767-770, :838).  The fused form rounds the nine
    per-pixel projections z[q][tap, o] to the activation dtype before summing them; both paths see y and the head weights in the
    activation dtype.  Gates per element, against sum |W| |y| over taps and channels, at twice the measured ratios: two-kernel <= 0.6 eps, fused <= 0.8 eps."""
    from strajnet_amd import ops
    B, Tn, Hi, Wi = 2, 8, 16, 32
    pu = [[mk_param((3, 3, 96, 48), dt, 0.05, 3 + 10 * i), mk_param((48,), dt, 0.1, 4 + 10 * i)] for i in range(2)]
    po = [mk_param((3, 3, 48, 2), dt, 0.1, 5), mk_param((2,), dt, 0.1, 6), mk_param((3, 3, 48, 2), dt, 0.1, 7), mk_param((2,), dt, 0.1, 8)]
    xs = [rnd((Tn * B, Hi, Wi, 96), dt, 9 + i) for i in range(2)]
    with torch.no_grad():
        assert ops.upconv_head_ok(Hi, Wi, pu[0][0], dt, Tn)
        ys = [ops.upconv(x, *p) for x, p in zip(xs, pu)]
        two = ops.outconv_pair(ys[0], ys[1], *po, B, Tn, t_major=t_major)
        zs = [ops.upconv_head(x, p[0], p[1], ph) for x, p, ph in zip(xs, pu, (po[0], po[2]))]
        out = ops.heads_gather(zs[0], zs[1], po[1], po[3], B, Tn, t_major=t_major)
    torch.cuda.synchronize()
    assert out.shape == two.shape == (B, 2 * Hi, 2 * Wi, 4 * Tn)
    assert float(zs[0][..., 18:].abs().max()) == 0.0 and float(zs[1][..., 18:].abs().max()) == 0.0       # the 6 padding channels

    def upr(t, w, b):
        u = F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
        return F.elu(F.conv2d(u, w.permute(3, 2, 0, 1), b, padding=1)).permute(0, 2, 3, 1)
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    refs, bounds = [], []
    for x, p, (pw, pb) in zip(xs, pu, ((po[0], po[1]), (po[2], po[3]))):
        y = upr(x.double().cpu(), p[0].master.detach().double().cpu(), p[1].master.detach().double().cpu())                 # [F,H,W,48]
        w = pw.master.detach().double().cpu()
        z = torch.einsum('fhwc,ijco->fhwijo', y, w)                                                                          # z[q][tap, o]
        zp = F.pad(z, (0, 0, 0, 0, 0, 0, 1, 1, 1, 1))
        H, W = y.shape[1], y.shape[2]
        o = sum(zp[:, i:i + H, j:j + W, i, j, :] for i in range(3) for j in range(3)) + pb.master.detach().double().cpu()
        za = F.pad(torch.einsum('fhwc,ijco->fhwijo', y.abs(), w.abs()), (0, 0, 0, 0, 0, 0, 1, 1, 1, 1))                       # sum_c |W| |y| per tap
        a = sum(za[:, i:i + H, j:j + W, i, j, :] for i in range(3) for j in range(3)) + pb.master.detach().double().cpu().abs()
        refs.append(o); bounds.append(a)
    def arrange(parts):
        y = torch.cat(parts, -1)
        y = y.view(Tn, B, *y.shape[1:]).permute(1, 0, 2, 3, 4) if t_major else y.view(B, Tn, *y.shape[1:])
        return y.permute(0, 2, 3, 1, 4).reshape(B, y.shape[2], y.shape[3], 4 * Tn)
    ref, bound = arrange(refs), arrange(bounds)
    e_two = (two.double().cpu() - ref).abs()
    e_fused = (out.double().cpu() - ref).abs()
    # the two-kernel path sees y rounded to the activation dtype (relative eps / 2 per term); the fused one z rounded once more
    assert float((e_two - 0.6 * eps * bound - 1e-6).max()) <= 0, float((e_two / (bound + 1e-30)).max())        # measured 0.30 eps
    assert float((e_fused - 0.8 * eps * bound - 1e-6).max()) <= 0, float((e_fused / (bound + 1e-30)).max())    # measured 0.38-0.40 eps
    print(f'inference heads {dt}: max |err| / sum|W||y|: two-kernel {float((e_two / bound).max()):.2e}, fused {float((e_fused / bound).max()):.2e} (eps {eps:.2e})')


@pytest.mark.parametrize('dt', DTYPES)
def test_decoder_tail_fused_elu_bwd(dt):
    """up(128->96) -> up(96->48) -> output heads with the ELU' passes folded into the consumers' backward kernels
    (grad_is_pre / x_is_elu_out, t-major frames) == the unfused chain in f64 (modules.py:746-748,767-770,838)."""
    from strajnet_amd import ops
    B, Tn, H0 = 1, 8, 8
    p1 = [mk_param((3, 3, 128, 96), dt, 0.05, 1), mk_param((96,), dt, 0.1, 2)]
    p0 = [mk_param((3, 3, 96, 48), dt, 0.05, 3), mk_param((48,), dt, 0.1, 4)]
    po = [mk_param((3, 3, 48, 2), dt, 0.1, 5), mk_param((2,), dt, 0.1, 6), mk_param((3, 3, 48, 2), dt, 0.1, 7), mk_param((2,), dt, 0.1, 8)]
    xs = [rnd((Tn * B, H0, H0, 128), dt, 9 + i).requires_grad_(True) for i in range(2)]
    hs = [ops.upconv(ops.upconv(x, *p1, True, False), *p0, True, True) for x in xs]
    out = ops.outconv_pair(hs[0], hs[1], *po, B, Tn, t_major=True, x_is_elu_out=True)

    def upr(t, w, b):
        u = F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode='nearest')
        return F.elu(F.conv2d(u, w.permute(3, 2, 0, 1), b, padding=1)).permute(0, 2, 3, 1)

    def cv(t, w, b):
        return F.conv2d(t.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1).permute(0, 2, 3, 1)
    r1, r0, ro = [ref_of(p.master) for p in p1], [ref_of(p.master) for p in p0], [ref_of(p.master) for p in po]
    xr = [ref_of(x) for x in xs]
    hr = [upr(upr(x, *r1), *r0) for x in xr]
    H = 4 * H0
    y = torch.cat([cv(hr[0], ro[0], ro[1]), cv(hr[1], ro[2], ro[3])], -1).view(Tn, B, H, H, 4)      # frames t-major
    outr = y.permute(1, 2, 3, 0, 4).reshape(B, H, H, 4 * Tn)
    assert rel_err(out, outr) < tol(dt)
    g = torch.randn(B, H, H, 4 * Tn, generator=torch.Generator().manual_seed(7))
    out.backward(g.cuda())
    outr.backward(g.double())
    for x, r in zip(xs, xr):
        assert rel_err(x.grad, r.grad) < 2 * tol(dt)
    for p, r in zip(p1 + p0 + po, r1 + r0 + ro):
        assert rel_err(p.grad, r.grad) < 2 * tol(dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_grouped_conv3(dt):
    from strajnet_amd import ops
    N, H, G, Cg = 2, 16, 8, 48
    pw, pb = mk_param((3, 3, Cg, G * Cg), dt, 0.05, 1), mk_param((G * Cg,), dt, 0.1, 2)
    x = rnd((N, H, H, G * Cg), dt, 3).requires_grad_(True)
    y = ops.grouped_conv3(x, pw, pb, G)
    xr, wr, br = ref_of(x), ref_of(pw.c), ref_of(pb.master)
    yr = F.conv2d(xr.permute(0, 3, 1, 2), wr.permute(3, 2, 0, 1), br, padding=1, groups=G).permute(0, 2, 3, 1)
    assert rel_err(y, yr) < tol(dt)
    g = rnd(tuple(y.shape), dt, 5)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pw.grad, wr.grad) < tol(dt)
    assert rel_err(pb.grad, br.grad) < tol(dt)
    xa, wa, ba = ref_of(x.detach().abs()), ref_of(pw.c.detach().abs()), ref_of(pb.master.detach().abs())
    ya = F.conv2d(xa.permute(0, 3, 1, 2), wa.permute(3, 2, 0, 1), ba, padding=1, groups=G).permute(0, 2, 3, 1)
    ya.backward(g.double().cpu().abs())
    elem_check('grouped conv y', y, yr, ya, dt)
    elem_check('grouped conv dx', x.grad, xr.grad, xa.grad, dt)
    elem_check('grouped conv dw', pw.grad, wr.grad, wa.grad, dt)
    elem_check('grouped conv db', pb.grad, br.grad, ba.grad, dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_maxpool(dt):
    from strajnet_amd import ops
    x = rnd((20, 11, 320), dt, 1).requires_grad_(True)
    y = ops.maxpool_time(x)
    xr = ref_of(x)
    yr = xr.amax(-2)
    assert rel_err(y, yr) < 1e-6
    g = rnd((20, 320), dt, 2)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < 1e-6


def test_patch_im2col():
    from strajnet_amd import ops
    B, H = 2, 32
    ogm = torch.randn(B, H, H, 11, 2).cuda()
    cols = ops.patch_im2col(ogm, 11, 2, 22, torch.float32)
    w = torch.randn(4, 4, 11, 96, dtype=torch.float64)
    ref = F.conv2d(ogm[..., 0].double().cpu().permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=4).permute(0, 2, 3, 1).reshape(-1, 96)
    got = cols.double().cpu() @ w.reshape(-1, 96)
    assert rel_err(got, ref) < 1e-6


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('Cin,ch_stride,nch', [(11, 2, 22), (3, 1, 3), (2, 1, 2)])
@pytest.mark.parametrize('with_add,with_norm2', [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize('B,H', [(2, 64), (1, 40)])            # 512 tokens = whole workgroups; 100 tokens = a ragged last one
def test_patch_embed_fused(dt, Cin, ch_stride, nch, with_add, with_norm2, B, H):
    """stj_patch_embed_fwd (PatchEmbed + LN [+ add] [+ LN2] in one launch, modules.py:437-446,572-590) and its backward (two LN
    backward launches + the queued weight gradient) vs float64, and vs the im2col + dense + LayerNorm launches it replaces."""
    from strajnet_amd import ops
    assert ops.patch_embed_ok(Cin, 96, dt)
    K, C = 16 * Cin, 96
    src = rnd((B, H, H, nch), torch.float32, 1)
    M = B * (H // 4) ** 2
    add = rnd((M, C), dt, 2) if with_add else None
    dy = rnd((M, C), dt, 3)

    def params():
        ps = dict(w=mk_param((4, 4, Cin, C), dt, 0.2, 4), b=mk_param((C,), dt, 0.1, 5), g=mk_param((C,), dt, 0.5, 6), be=mk_param((C,), dt, 0.1, 7))
        ps['g'].master.data += 1.0
        if with_norm2:
            ps['g2'], ps['be2'] = mk_param((C,), dt, 0.5, 8), mk_param((C,), dt, 0.1, 9)
            ps['g2'].master.data += 1.0
        return ps

    def run(fused):
        ps = params()
        a = add.clone().requires_grad_(True) if with_add else None
        if fused:
            y = ops.patch_embed(src, ps['w'], ps['b'], ps['g'], ps['be'], Cin, ch_stride, nch, dt, 1e-5, a, ps.get('g2'), ps.get('be2'))
        else:
            cols = ops.patch_im2col(src, Cin, ch_stride, nch, dt)
            y = ops.layernorm(ops.linear(cols, ps['w'], ps['b']), ps['g'], ps['be'], 1e-5, res=a)
            if with_norm2:
                y = ops.layernorm(y, ps['g2'], ps['be2'], 1e-5)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), (a.grad.detach() if with_add else None), {k: v.grad.detach().clone() for k, v in ps.items()}, ps

    y1, da1, g1, ps = run(True)
    y0, da0, g0, _ = run(False)
    # float64 statement on the values the kernels saw (compute-dtype weights, f32 bias / gamma / beta masters)
    x64 = src.double().cpu()[..., ::ch_stride][..., :Cin] if ch_stride > 1 else src.double().cpu()
    w = ref_of(ps['w'].c)
    leaves = {k: ref_of(ps[k].master) for k in ps if k != 'w'}
    a64 = ref_of(add) if with_add else None
    pre = F.conv2d(x64.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=4).permute(0, 2, 3, 1).reshape(M, C) + leaves['b']
    r = F.layer_norm(pre, (C,), leaves['g'], leaves['be'], 1e-5)
    if with_add:
        r = r + a64
    if with_norm2:
        r = F.layer_norm(r, (C,), leaves['g2'], leaves['be2'], 1e-5)
    r.backward(dy.double().cpu())
    t = tol(dt)
    assert rel_err(y1, r) < t, rel_err(y1, r)
    assert rel_err(y1, r) <= max(2.0 * rel_err(y0, r), 1e-6), (rel_err(y1, r), rel_err(y0, r))       # never further from float64 than the path it replaces
    if with_add:
        assert rel_err(da1, a64.grad) < t
    assert rel_err(g1['w'], w.grad) < t, rel_err(g1['w'], w.grad)
    for k, v in leaves.items():
        assert rel_err(g1[k], v.grad) < t, (k, rel_err(g1[k], v.grad))
    # against the launches it replaces: same roundings (pre and the sum are rounded to the storage type before they are
    # normalised in both), only the f32 summation order of the product differs
    assert rel_err(y1, y0) < (1e-5 if dt == torch.float32 else t)
    for k in g1:
        assert rel_err(g1[k], g0[k]) < (1e-4 if dt == torch.float32 else t), k
    if with_norm2:      # the two LayerNorm backward passes as one launch (stj_layernorm_bwd_chain, the default) vs two stj_layernorm_bwd launches
        ops.LN_CHAIN = False
        try:
            _, da2, g2, _ = run(True)
        finally:
            ops.LN_CHAIN = True
        for k in g1:     # same arithmetic (the intermediate gradient is rounded to the storage type in both), f32 summation order of the parameter sums
            assert rel_err(g1[k], g2[k]) < 1e-4, (k, rel_err(g1[k], g2[k]))
        if with_add:     # the intermediate gradient: the row sums are taken in another order, an element may round to the neighbouring 16-bit value
            assert rel_err(da1, da2) < (1e-6 if dt == torch.float32 else 2e-3)


def test_loss_and_gate():
    """Fused loss (fwd + d/dlogits) and the AUC gate vs the oracle restatements."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from strajnet_amd import ops
    from oracle import np_ref, torch_ref
    cfg = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
    x = np_ref.make_inputs(cfg, 2)
    Hg = x['gt_obs'].shape[2]
    rng = np.random.default_rng(0)
    logits = rng.normal(0, 2, (2, Hg, Hg, 32)).astype(np.float32)
    # predicted flow on a 1/16 lattice (never an integer): sample coordinates and bilinear weights are then exact in float32, so
    # the float64 oracle sees the same joint probability q -- the BCE-on-probabilities gradients go like 1/q and would otherwise
    # carry the 1 % coordinate rounding of q ~ 1e-5 pixels, which is float32 arithmetic (the reference's too), not the formula
    fl = logits.reshape(2, Hg, Hg, 8, 4)[..., 2:]
    fl[...] = (np.round(fl * 8) + 0.5) / 8
    x['gt_obs'][:, 3] = 0
    x['gt_occ'][:, 3] = 0                        # waypoint 3: no positives -> AUC 0 -> gate 0 (loss.py:137)
    gt = {k: torch.as_tensor(x[k]).cuda() for k in ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow')}
    lt = torch.as_tensor(logits).cuda().requires_grad_(True)
    # flags: the train.py:195-196 set, the constructor defaults (focal), use_pred with and without focal, no_use_warp
    combos = [dict(use_focal_loss=False), dict(use_focal_loss=True), dict(use_focal_loss=False, use_pred=True),
              dict(use_focal_loss=True, use_pred=True), dict(use_focal_loss=True, no_use_warp=True)]
    for flags in combos:
        for use_gt in (True, False):
            lt.grad = None
            loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(Hg, Hg, 8), replica=2.0, use_gt=use_gt, **flags)
            d = loss_fn(get_pred_waypoint_logits(lt), warpped_gt(gt['gt_obs'], gt['gt_occ'], gt['gt_flow'], gt['origin_flow']), None)
            ref, gates = np_ref.ogm_flow_loss(logits, x['gt_obs'], x['gt_occ'], x['gt_flow'], x['origin_flow'], replica=2.0,
                                              use_gt=use_gt, return_gates=True, **flags)
            if use_gt:
                assert gates[3] == 0.0 and sum(gates) == 7.0
                g, auc = ops.auc_gate(gt['gt_obs'], gt['gt_occ'], gt['gt_flow'], gt['origin_flow'], return_auc=True)
                assert g.cpu().tolist() == gates
            for k in ref:
                v = float(d[k].detach()) if torch.is_tensor(d[k]) else float(d[k])
                assert abs(v - float(ref[k])) <= 3e-5 * abs(float(ref[k])) + 1e-6, (flags, k, v, float(ref[k]))
            sum(d.values()).backward()
            lr = torch.as_tensor(logits).double().requires_grad_(True)
            gtr = {k: torch.as_tensor(x[k]).double() for k in gt}
            dr = torch_ref.loss(lr, gtr['gt_obs'], gtr['gt_occ'], gtr['gt_flow'], gtr['origin_flow'], replica=2.0, use_gt=use_gt, **flags)
            sum(dr.values()).backward()
            assert rel_err(lt.grad, lr.grad) < 1e-4, flags
    d0 = OGMFlow_loss(OccupancyFlowTaskConfig(Hg, Hg, 8))                  # the reference's own defaults construct and run
    assert d0.use_focal_loss and not d0.use_gt and not d0.use_pred
    # differentiating `.total` alone takes the one-upstream-scalar path of stj_loss_bwd (flag bit 3): same d/dlogits as the sum of the
    # four entries; mixed use (one entry + total) goes through the general path
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(Hg, Hg, 8), replica=2.0, use_gt=True, use_focal_loss=False)
    tw = warpped_gt(gt['gt_obs'], gt['gt_occ'], gt['gt_flow'], gt['origin_flow'])
    lt.grad = None
    sum(loss_fn(get_pred_waypoint_logits(lt), tw, None).values()).backward()
    g_sum = lt.grad.clone()
    lt.grad = None
    (3.0 * loss_fn(get_pred_waypoint_logits(lt), tw, None).total).backward()
    assert rel_err(lt.grad, 3.0 * g_sum) < 1e-6
    lt.grad = None
    d = loss_fn(get_pred_waypoint_logits(lt), tw, None)
    (d.total + d['flow']).backward()
    lt.grad2, lt.grad = lt.grad.clone(), None
    d = loss_fn(get_pred_waypoint_logits(lt), tw, None)
    (sum(d.values()) + d['flow']).backward()
    assert rel_err(lt.grad2, lt.grad) < 1e-6


def test_loss_one_pass_gradient_for_an_announced_unit_upstream():
    """stj_loss_coef + stj_loss_fwd_bwd (OGMFlow_loss.unit_grad + prepare(), the captured train step's path) against the two-pass path
    stj_loss_fwd / stj_loss_bwd: same coefficients (bit for bit), same loss values, same d/dlogits; another upstream gradient than the
    announced tensor takes the general kernel."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from strajnet_amd import ops
    from oracle import np_ref
    cfg = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
    x = np_ref.make_inputs(cfg, 3)
    Hg = x['gt_obs'].shape[2]
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 2, (3, Hg, Hg, 32)).astype(np.float32)
    x['gt_obs'][:, 3] = 0
    x['gt_occ'][:, 3] = 0                        # waypoint 3: gate 0
    x['gt_flow'][:, 5] = 0                       # waypoint 5: no pixel with a true flow (denominator 0: coefficient 0)
    gt = {k: torch.as_tensor(x[k]).cuda() for k in ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow')}
    lt = torch.as_tensor(logits).cuda().requires_grad_(True)
    one = torch.ones((), dtype=torch.float32, device='cuda')
    combos = [dict(use_focal_loss=False), dict(use_focal_loss=True), dict(use_focal_loss=False, use_pred=True),
              dict(use_focal_loss=True, use_pred=True), dict(use_focal_loss=True, no_use_warp=True)]
    for flags in combos:
        for use_gt in (True, False):
            tw = warpped_gt(gt['gt_obs'], gt['gt_occ'], gt['gt_flow'], gt['origin_flow'])
            ref_fn = OGMFlow_loss(OccupancyFlowTaskConfig(Hg, Hg, 8), replica=2.0, use_gt=use_gt, **flags)
            lt.grad = None
            d0 = ref_fn(get_pred_waypoint_logits(lt), tw, None)
            d0.total.backward(one)
            g_two = lt.grad.clone()
            fn = OGMFlow_loss(OccupancyFlowTaskConfig(Hg, Hg, 8), replica=2.0, use_gt=use_gt, **flags)
            fn.unit_grad = one
            # the coefficients from the ground truth alone are the ones the forward sums give
            gate = ops.auc_gate(*(gt[k] for k in ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow'))) if use_gt else torch.ones(8, device='cuda')
            coef = ops.loss_coef(gt['gt_flow'], gate, fn.ogm_weight, fn.occ_weight, fn.flow_origin_weight, fn.replica, fn._flags())
            sums, loss, coef2 = torch.zeros(32 * 40, device='cuda'), torch.empty(5, device='cuda'), torch.empty(32, device='cuda')
            ops.call('stj_loss_fwd', ops._p(lt.detach()), ops._p(gt['gt_obs']), ops._p(gt['gt_occ']), ops._p(gt['gt_flow']), ops._p(gt['origin_flow']),
                     ops._p(gate), ops._p(sums), ops._p(loss), ops._p(coef2), 3, Hg, Hg, fn.ogm_weight, fn.occ_weight, fn.flow_origin_weight,
                     fn.replica, fn._flags(), ops._st())
            assert torch.equal(coef, coef2), (flags, use_gt, coef, coef2)
            if use_gt:       # the gate's histogram pass counting the flow pixels on the way: the same gate, the same coefficients
                gate3, coef3 = ops.auc_gate_coef(gt['gt_obs'], gt['gt_occ'], gt['gt_flow'], gt['origin_flow'], fn.ogm_weight, fn.occ_weight,
                                                 fn.flow_origin_weight, fn.replica, fn._flags())
                assert torch.equal(gate3, gate) and torch.equal(coef3, coef)
            assert float(coef[4 * 5 + 2]) == 0.0 and (not use_gt or float(coef[4 * 3 + 3]) == 0.0)
            hits = ops.LOSS_FUSED_STATS['hits']
            fn.prepare(tw)
            lt.grad = None
            d1 = fn(get_pred_waypoint_logits(lt), tw, None)
            d1.total.backward(one)
            assert ops.LOSS_FUSED_STATS['hits'] == hits + 1
            for k in ('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe'):
                a, b = float(d1[k]), float(d0[k])
                assert abs(a - b) <= 2e-6 * abs(b) + 1e-9, (flags, use_gt, k, a, b)          # f32 summation order of the partial sums
            assert rel_err(lt.grad, g_two) < 1e-6, (flags, use_gt)
            # not the announced tensor: the general kernel
            miss = ops.LOSS_FUSED_STATS['misses']
            fn.prepare(tw)
            lt.grad = None
            (3.0 * fn(get_pred_waypoint_logits(lt), tw, None).total).backward()
            assert ops.LOSS_FUSED_STATS['misses'] == miss + 1
            assert rel_err(lt.grad, 3.0 * g_two) < 1e-6
            # a second backward through a retained graph: the stored gradient was handed over once, the general kernel answers
            fn.prepare(tw)
            lt.grad = None
            tot = fn(get_pred_waypoint_logits(lt), tw, None).total
            tot.backward(one, retain_graph=True)
            tot.backward(one)
            assert rel_err(lt.grad, 2.0 * g_two) < 1e-6
            # no prepare(): the two-pass path, whatever was announced
            lt.grad = None
            fn(get_pred_waypoint_logits(lt), tw, None).total.backward(one)
            assert ops.LOSS_FUSED_STATS['hits'] == hits + 2 and rel_err(lt.grad, g_two) < 1e-6


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('rows,C', [(1000, 96), (257, 384), (64, 100)])
def test_layernorm_skip(dt, rows, C):
    """(LayerNorm(x), x): the gradient of the skip output is added inside the LN backward kernel (v2 and v1 paths)."""
    from strajnet_amd import ops
    pg, pb = mk_param((C,), dt, 0.3, 1), mk_param((C,), dt, 0.3, 2)
    with torch.no_grad():
        pg.master.add_(1.0)
    x = rnd((rows, C), dt, 3, 2.0).requires_grad_(True)
    y, xs = ops.layernorm_skip(x, pg, pb, 1e-5)
    assert torch.equal(xs, x)
    xr, gr, br = ref_of(x), ref_of(pg.master), ref_of(pb.master)
    yr = F.layer_norm(xr, (C,), gr, br, 1e-5)
    g1, g2 = rnd((rows, C), dt, 5), rnd((rows, C), dt, 6)
    ((y.float() * g1.float()).sum() + (xs.float() * g2.float()).sum()).backward()
    ((yr * g1.double().cpu()).sum() + (xr * g2.double().cpu()).sum()).backward()
    assert rel_err(x.grad, xr.grad) < tol(dt)
    assert rel_err(pg.grad, gr.grad) < tol(dt)
    # only the skip output used: LayerNorm contributes nothing
    x2 = rnd((rows, C), dt, 7).requires_grad_(True)
    _, xs2 = ops.layernorm_skip(x2, pg, pb, 1e-5)
    (xs2.float() * g2.float()).sum().backward()
    assert rel_err(x2.grad, g2.double().cpu()) < 1e-6


@pytest.mark.parametrize('dt', DTYPES)
def test_dropout_op(dt):
    """stj_dropout: y = [res +] keep * x / (1 - p); per-element and per-sample (DropPath) draws; backward re-derives the mask;
    stj_dropout_mask exports exactly the mask the forward used."""
    from strajnet_amd import ops
    dctx = ops.DropCtx('cuda', seed=5)
    dctx.begin()
    x = rnd((6, 37, 50), dt, 1).requires_grad_(True)
    r = rnd((6, 37, 50), dt, 2).requires_grad_(True)
    y = ops.dropout(x, 0.1, dctx, 'a')
    m = dctx.mask('a').double().cpu()
    assert m.shape == (6, 37, 50) and abs(float(m.mean()) - 0.9) < 0.02
    assert rel_err(y, ref_of(x).detach() * m / 0.9) < (1e-6 if dt == torch.float32 else 5e-3)
    y2 = ops.dropout(x, 0.3, dctx, 'b', res=r, per_sample=True)
    m2 = dctx.mask('b').double().cpu()
    assert m2.shape == (6,)
    assert rel_err(y2, ref_of(r).detach() + ref_of(x).detach() * m2.view(6, 1, 1) / 0.7) < (1e-6 if dt == torch.float32 else 5e-3)
    g = rnd((6, 37, 50), dt, 3)
    (y.float() * g.float()).sum().backward()
    assert rel_err(x.grad, g.double().cpu() * m / 0.9) < (1e-6 if dt == torch.float32 else 5e-3)
    x.grad = None
    (y2.float() * g.float()).sum().backward()
    assert rel_err(x.grad, g.double().cpu() * m2.view(6, 1, 1) / 0.7) < (1e-6 if dt == torch.float32 else 5e-3)
    assert rel_err(r.grad, g.double().cpu()) < 1e-6
    # a size the vectorised kernels take (n % 8 == 0, 16-byte aligned): per-ELEMENT decisions there too (the f16 instantiation once shared one
    # decision among the 8 elements of a vector)
    x8 = rnd((4, 16, 64), dt, 7)
    y8 = ops.dropout(x8, 0.4, dctx, 'v')
    m8 = dctx.mask('v').double().cpu()
    assert rel_err(y8, x8.double().cpu() * m8 / 0.6) < (1e-6 if dt == torch.float32 else 5e-3)
    # streams: another site or another step gives another mask, the same (step, site) the same one
    ma = dctx.mask('a').clone()
    dctx.begin()
    ops.dropout(x, 0.1, dctx, 'a')
    assert not torch.equal(ma, dctx.mask('a'))
    # per-sample draws over many samples follow the rate
    xs = torch.ones(4096, 8, device='cuda', dtype=dt)
    ops.dropout(xs, 0.25, dctx, 'c', per_sample=True)
    assert abs(float(dctx.mask('c').double().mean()) - 0.75) < 0.03


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('B,N,C,p_drop', [(3, 64, 96, 0.0), (4, 256, 96, 0.3), (2, 128, 192, 0.3), (3, 64, 384, 0.0), (1, 80, 96, 0.0),
                                          (8, 256, 384, 0.3), (1, 80, 384, 0.3), (8, 1024, 384, 0.3), (1, 80, 192, 0.3), (8, 1024, 192, 0.3)])
def test_swin_mlp_fused(dt, B, N, C, p_drop):
    """csrc/swin_fused.hip: x + DropPath(fc2(gelu(fc1(LN(x))))) in one kernel, and its backward (dx, LN gamma/beta, both weight
    and bias gradients) vs float64 autograd on the same statement (modules.py:260, :40-46, :18-29, :137-151).  Row counts that
    are not a multiple of the block's rows exercise the tail guards.  C = 384 runs the split form: (row block, hidden slice)
    workgroups + the finishing launch; C = 192 below 32768 rows the form whose two hidden slices meet inside the launch.
    (Per dispatch path, through the raw C ABI and judged per row against float64: tests/test_swin_abi_gpu.py with _swin_cases.py.)"""
    from strajnet_amd import ops
    pg, pb = mk_param((C,), dt, 0.3, 1), mk_param((C,), dt, 0.3, 2)
    with torch.no_grad():
        pg.master.add_(1.0)
    pw1, pb1 = mk_param((C, 4 * C), dt, 0.1, 3), mk_param((4 * C,), dt, 0.2, 4)
    pw2, pb2 = mk_param((4 * C, C), dt, 0.1, 5), mk_param((C,), dt, 0.2, 6)
    x = rnd((B, N, C), dt, 7, 2.0).requires_grad_(True)
    dctx = None
    if p_drop > 0:
        dctx = ops.DropCtx('cuda', seed=11)
        dctx.begin()
    y = ops.swin_mlp(x, pg, pb, pw1, pb1, pw2, pb2, 1e-5, dctx, 'dp', p_drop, rows_per_sample=N)
    keep = torch.ones(B, dtype=torch.float64)
    if p_drop > 0:
        keep = dctx.mask('dp').double().cpu() / (1.0 - p_drop)
        assert keep.shape == (B,)
    xr, gr, br = ref_of(x), ref_of(pg.master), ref_of(pb.master)
    w1r, b1r, w2r, b2r = ref_of(pw1.c), ref_of(pb1.master), ref_of(pw2.c), ref_of(pb2.master)
    hr = F.layer_norm(xr, (C,), gr, br, 1e-5) @ w1r + b1r
    hr = 0.5 * hr * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (hr + 0.044715 * hr ** 3)))
    yr = xr + keep.view(B, 1, 1) * (hr @ w2r + b2r)
    t = tol(dt)
    assert rel_err(y, yr) < t
    g = rnd((B, N, C), dt, 9)
    y.backward(g)
    yr.backward(g.double().cpu())
    assert rel_err(x.grad, xr.grad) < t
    for nm, p_, r_ in (('gamma', pg, gr), ('beta', pb, br), ('w1', pw1, w1r), ('b1', pb1, b1r), ('w2', pw2, w2r), ('b2', pb2, b2r)):
        assert rel_err(p_.grad, r_.grad) < 2 * t, nm


@pytest.mark.parametrize('B,N', [(8, 4096), (32, 4096)])
def test_swin_mlp_fused_c96_wide_row_counts(B, N):
    """The eight-wave 128-row form of the C = 96 MLP kernels, which the op-level test above never reaches: 32768 rows (the bench's stage 0:
    192-column weight chunks since round 6) and 131072 rows (B = 32 inference / cfg-512: 96-column chunks), bf16 against float64.
    (Per dispatch path, through the raw C ABI and judged per row against float64: tests/test_swin_abi_gpu.py with _swin_cases.py.)"""
    test_swin_mlp_fused(torch.bfloat16, B, N, 96, 0.3)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('B,res,C,shift,p_drop', [(2, 16, 96, 0, 0.0), (3, 16, 96, 4, 0.3), (2, 16, 192, 4, 0.3), (1, 32, 192, 0, 0.0), (2, 8, 96, 0, 0.0),
                                                  (3, 16, 384, 4, 0.3), (1, 16, 384, 0, 0.0), (2, 8, 384, 0, 0.3), (1, 64, 384, 4, 0.3), (8, 32, 192, 4, 0.3)])
def test_swin_attn_half_fused(dt, B, res, C, shift, p_drop):
    """csrc/swin_fused.hip: x + DropPath(proj(window_attention(LN(x) Wqkv + b))) in one kernel (modules.py:225-258,103-134,189-216)
    and its backward (GEMMs + window-attention backward on the saved operands) vs float64 autograd on the index formulation.
    (Per dispatch path, through the raw C ABI and judged per row against float64: tests/test_swin_abi_gpu.py with _swin_cases.py.)"""
    from strajnet_amd import ops
    heads = C // 32
    N = res * res
    pg, pb = mk_param((C,), dt, 0.3, 1), mk_param((C,), dt, 0.3, 2)
    with torch.no_grad():
        pg.master.add_(1.0)
    pwq, pbq = mk_param((C, 3 * C), dt, 0.15, 3), mk_param((3 * C,), dt, 0.2, 4)
    pt = mk_param((225, heads), dt, 0.5, 5)
    pwp, pbp = mk_param((C, C), dt, 0.1, 6), mk_param((C,), dt, 0.2, 7)
    x = rnd((B, N, C), dt, 8, 2.0).requires_grad_(True)
    dctx = None
    if p_drop > 0:
        dctx = ops.DropCtx('cuda', seed=13)
        dctx.begin()
    y = ops.swin_attn_half(x, pg, pb, pwq, pbq, pt, pwp, pbp, B, res, shift, 1e-5, dctx, 'dp', p_drop)
    keep = torch.ones(B, dtype=torch.float64)
    if p_drop > 0:
        keep = dctx.mask('dp').double().cpu() / (1.0 - p_drop)
    refs = [ref_of(t) for t in (x, pg.master, pb.master, pwq.c, pbq.master, pt.master, pwp.c, pbp.master)]
    xr, gr, br, wqr, bqr, tr, wpr, bpr = refs
    qkvr = F.layer_norm(xr, (C,), gr, br, 1e-5) @ wqr + bqr
    yr = xr + keep.view(B, 1, 1) * (_win_ref(qkvr, tr, B, res, heads, shift) @ wpr + bpr)
    t = tol(dt)
    assert rel_err(y, yr, 1.4 if (C == 384 and dt != torch.float32) else None) < t
    # inference form (no saved operands) gives the same result
    with torch.no_grad():
        if dctx is not None:
            dctx.n = 0              # re-register the same site id for the repeated call
        y2 = ops.swin_attn_half(x.detach(), pg, pb, pwq, pbq, pt, pwp, pbp, B, res, shift, 1e-5, dctx, 'dp', p_drop)
    assert torch.equal(y2, y.detach())
    g = rnd((B, N, C), dt, 9)
    y.backward(g)
    yr.backward(g.double().cpu())
    # the C = 384 kernels hold the window's q | k | v tile, P and dS in the 16-bit type in LDS over 12 heads: rms error up to 1.4e-2 of the
    # rms value in bf16 (every other case of this file stays under 8e-3: RMS_WEIGHT)
    rw = 1.4 if (C == 384 and dt != torch.float32) else None
    assert rel_err(x.grad, xr.grad, rw) < 2 * t
    for nm, p_, r_ in (('gamma', pg, gr), ('beta', pb, br), ('wqkv', pwq, wqr), ('bqkv', pbq, bqr), ('table', pt, tr), ('wproj', pwp, wpr),
                       ('bproj', pbp, bpr)):
        assert rel_err(p_.grad, r_.grad, rw) < 2 * t, nm


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,res,shift', [(8, 16, 4), (2, 32, 0), (4, 32, 4)])          # 6 / 6 / 2 head slices, 8 / 8 / 4 hidden slices
def test_swin384_block_split_vs_layerwise_vs_f64(dt, B, res, shift):
    """One whole C = 384 Swin block (the 16 x 16 stage of cfg-256, the 32 x 32 stage of cfg-512): the split fused kernels
    ((window, head slice) / (row block, hidden slice) workgroups + finishing launches) against float64, and never noticeably
    further from it than the layer-by-layer HIP path on the same operands -- output, dx and all 13 parameter gradients.
    (Per dispatch path, through the raw C ABI and judged per row against float64: tests/test_swin_abi_gpu.py with _swin_cases.py.)"""
    from strajnet_amd import ops
    C, heads, N = 384, 12, res * res
    names = ['g1', 'b1n', 'wq', 'bq', 'tab', 'wp', 'bp', 'g2', 'b2n', 'w1', 'bb1', 'w2', 'bb2']
    shapes = [(C,), (C,), (C, 3 * C), (3 * C,), (225, heads), (C, C), (C,), (C,), (C,), (C, 4 * C), (4 * C,), (4 * C, C), (C,)]
    scales = [0.3, 0.3, 0.1, 0.2, 0.5, 0.1, 0.2, 0.3, 0.3, 0.1, 0.2, 0.1, 0.2]
    x = rnd((B, N, C), dt, 7, 2.0).requires_grad_(True)
    g = rnd((B, N, C), dt, 9)
    res_ = []
    for fused in (True, False):
        P = {n: mk_param(sh, dt, sc, 20 + i) for i, (n, sh, sc) in enumerate(zip(names, shapes, scales))}
        with torch.no_grad():
            P['g1'].master.add_(1.0); P['g2'].master.add_(1.0)
        x.grad = None
        if fused:
            y = ops.swin_attn_half(x, P['g1'], P['b1n'], P['wq'], P['bq'], P['tab'], P['wp'], P['bp'], B, res, shift, 1e-5)
            y = ops.swin_mlp(y, P['g2'], P['b2n'], P['w1'], P['bb1'], P['w2'], P['bb2'], 1e-5, rows_per_sample=N)
        else:
            h, sk = ops.layernorm_skip(x, P['g1'], P['b1n'], 1e-5)
            a = ops.win_attn(ops.linear(h, P['wq'], P['bq']), P['tab'], B, res, heads, shift)
            y1 = ops.linear(a, P['wp'], P['bp'], res=sk)
            h, sk = ops.layernorm_skip(y1, P['g2'], P['b2n'], 1e-5)
            y = ops.linear(ops.gelu(ops.linear(h, P['w1'], P['bb1'])), P['w2'], P['bb2'], res=sk)
        y.backward(g)
        torch.cuda.synchronize()
        res_.append([y.detach().clone(), x.grad.clone()] + [P[n].grad.clone() for n in names])
    R = {n: ref_of(P[n].c if len(P[n].shape) == 2 and n != 'tab' else P[n].master) for n in names}
    xr = ref_of(x)
    qkvr = F.layer_norm(xr, (C,), R['g1'], R['b1n'], 1e-5) @ R['wq'] + R['bq']
    y1r = xr + _win_ref(qkvr, R['tab'], B, res, heads, shift) @ R['wp'] + R['bp']
    hr = F.layer_norm(y1r, (C,), R['g2'], R['b2n'], 1e-5) @ R['w1'] + R['bb1']
    hr = 0.5 * hr * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (hr + 0.044715 * hr ** 3)))
    yr = y1r + hr @ R['w2'] + R['bb2']
    yr.backward(g.double().cpu())
    refs = [yr, xr.grad] + [R[n].grad for n in names]

    def nrm(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / (b.norm() + 1e-30))
    rep = [f'{n}: split {nrm(f, r):.2e} layerwise {nrm(u, r):.2e}' for n, f, u, r in zip(['y', 'dx'] + names, res_[0], res_[1], refs)]
    print('\n'.join(rep))
    for n, f, u, r in zip(['y', 'dx'] + names, res_[0], res_[1], refs):
        assert nrm(f, r) <= 1.5 * nrm(u, r) + 1e-3, rep


def test_nadam_step_matches_keras_formula():
    """stj_nadam_step vs the Keras Nadam recurrences in float64 over three steps."""
    from strajnet_amd.optim import Nadam
    torch.manual_seed(0)
    n = 1003
    w = torch.randn(n, device='cuda')
    w0 = w.double().cpu().clone()
    g = torch.zeros(n, device='cuda')
    opt = Nadam(w, g, lr=1e-2)
    m = torch.zeros(n, dtype=torch.float64); v = torch.zeros(n, dtype=torch.float64); wr = w0.clone()
    b1, b2, eps, prod = 0.9, 0.999, 1e-7, 1.0
    for t in range(1, 4):
        gt = torch.randn(n, device='cuda')
        g.copy_(gt)
        opt.step()
        gd = gt.double().cpu()
        mu_t = b1 * (1 - 0.5 * 0.96 ** (0.004 * t)); mu_n = b1 * (1 - 0.5 * 0.96 ** (0.004 * (t + 1)))
        prod_t = prod * mu_t; prod_n = prod_t * mu_n; prod = prod_t
        m = b1 * m + (1 - b1) * gd; v = b2 * v + (1 - b2) * gd * gd
        wr = wr - 1e-2 * ((1 - mu_t) * gd / (1 - prod_t) + mu_n * m / (1 - prod_n)) / ((v / (1 - b2 ** t)).sqrt() + eps)
    assert rel_err(w, wr) < 1e-5


@pytest.mark.parametrize('dt', DTYPES)
def test_gemm_group_matches_single_launches(dt):
    """stj_gemm_group_begin/_end: five GEMMs of different shapes, orientations, batch counts and epilogues recorded into grouped
    launches (4 + 1) give bit-identical results to five single launches (plain outputs) / the same sums up to f32 atomic order
    (split-K accumulation).  An empty group and a group of one are legal."""
    from strajnet_amd import ops
    code = ops.DTYPE_CODE[dt]
    dev = 'cuda'

    def r(*shape, seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(shape, generator=g) * 0.5).to(dev).to(dt)
    M, K, N = 300, 96, 130
    x, w, wt = r(M, K, seed=1), r(K, N, seed=2), r(N, K, seed=3)
    dy = r(M, N, seed=4)
    bias = torch.randn(N, device=dev)
    q, k = r(6, 50, 4 * 32, seed=5), r(6, 40, 4 * 32, seed=6)

    def run(grouped):
        y1 = torch.empty(M, N, device=dev, dtype=dt)          # NN + bias + ELU
        y2 = torch.empty(M, N, device=dev, dtype=dt)          # NT (weight stored [N,K])
        dx = torch.empty(M, K, device=dev, dtype=dt)          # dy w^T
        gw = torch.zeros(K, N, device=dev)                    # x^T dy, split-K, f32 atomics, + column sums
        gb = torch.zeros(N, device=dev)
        S = torch.empty(6, 4, 50, 40, device=dev)             # batched q k^T over (batch, head), f32 out
        import contextlib
        with (ops.gemm_group() if grouped else contextlib.nullcontext()):
            ops.gemm(x, w, y1, M, N, K, (0, 0, K, 1), (0, 0, N, 1), (0, 0, N), code, bias=bias, act=ops.ACT_ELU)
            ops.gemm(x, wt, y2, M, N, K, (0, 0, K, 1), (0, 0, 1, K), (0, 0, N), code)
            ops.gemm(dy, w, dx, M, K, N, (0, 0, N, 1), (0, 0, 1, N), (0, 0, K), code)
            ops.gemm(x, dy, gw, K, N, M, (0, 0, 1, K), (0, 0, N, 1), (0, 0, N), code, c_f32=1, accumulate=1, splitk=0, colsum=gb)
            ops.gemm(q, k, S, 50, 40, 32, (50 * 128, 32, 128, 1), (40 * 128, 32, 1, 128), (4 * 50 * 40, 50 * 40, 40), code, nb=(6, 4),
                     alpha=0.25, c_f32=1)
        torch.cuda.synchronize()
        return y1, y2, dx, gw, gb, S
    a, b = run(False), run(True)
    for i in (0, 1, 2, 5):
        assert torch.equal(a[i], b[i]), i
    for i in (3, 4):
        assert rel_err(b[i], a[i]) < 1e-5, i
    ref = (x.double() @ w.double())
    assert rel_err(b[0], F.elu(ref + bias.double())) < tol(dt)
    assert rel_err(b[3], x.double().t() @ dy.double()) < tol(dt)
    with ops.gemm_group():
        pass
    y = torch.empty(M, N, device=dev, dtype=dt)
    with ops.gemm_group():
        ops.gemm(x, w, y, M, N, K, (0, 0, K, 1), (0, 0, N, 1), (0, 0, N), code)
    assert rel_err(y, ref) < tol(dt)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('F_,Hi,Cin,Cout,two', [(3, 16, 192, 128, True), (2, 8, 384, 192, False)])
def test_upconv_add_fused_skip(dt, F_, Hi, Cin, Cout, two):
    """Decoder skip sums in the up-conv epilogue (stj_upconv_fwd_res / stj_elu_res_bwd) against the up-conv followed by elementwise adds:
    forward bit-identical (every sum is rounded like a separate add), gradients equal up to the rounding of ELU'(y - r) vs ELU'(u)."""
    from strajnet_amd import ops
    x0 = rnd((F_, Hi, Hi, Cin), dt, 1)
    r1 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 2)
    r2 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 3) if two else None
    g1 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 4)
    g2 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 5)

    def run(fused):
        pw, pb = mk_param((3, 3, Cin, Cout), dt, 0.03, seed=7), mk_param((Cout,), dt, 0.1, seed=8)
        x = x0.clone().requires_grad_(True)
        a = r1.clone().requires_grad_(True)
        b = r2.clone().requires_grad_(True) if two else None
        keep, ops.FUSED_SKIP_TRAIN = ops.FUSED_SKIP_TRAIN, fused
        try:
            out = ops.upconv_add(x, pw, pb, a, b)
        finally:
            ops.FUSED_SKIP_TRAIN = keep
        y, y2 = out if two else (out, None)
        loss = (y.float() * g1.float()).sum() + ((y2.float() * g2.float()).sum() if two else 0.0)
        loss.backward()
        ops.wgrad_join_now(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return y, y2, x.grad, a.grad, (b.grad if two else None), pw.grad.clone(), pb.grad.clone()
    u = run(False)
    for mode in (True,):             # sums in the up-conv epilogue + the fused backward
        f = run(mode)
        assert torch.equal(f[0], u[0])
        if two:
            assert torch.equal(f[1], u[1])
            assert torch.equal(f[4], u[4])
        for i in (2, 3, 5, 6):
            assert rel_err(f[i], u[i]) < (2e-2 if dt == torch.bfloat16 else 3e-3), (mode, i)


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('F_,Hi,Cin,Cout,two', [(3, 16, 192, 128, True), (2, 8, 384, 192, False)])
def test_upconv_add_skips_pre_contract_bit_identical(dt, F_, Hi, Cin, Cout, two):
    """The decoder level whose skips are ELU outputs of linear_z (the time-collapsed Conv3D skips): upconv_add(skips_pre=True) + linear_z(grad_is_pre=True)
    -- ONE stj_skip_junction_bwd for the level's three ELU' products -- against the forms it replaces (stj_elu_res_bwd / the plain adds, then one
    stj_unary_bwd per skip): outputs and every gradient BIT-identical (the junction rounds where the separate passes rounded)."""
    from strajnet_amd import ops
    Ci = 96
    R = F_ // (F_) * (2 * Hi) * (2 * Hi)            # rows per time slice: the skips are [Z = F_, R, Cout] (shared input [R, Ci])
    x0 = rnd((F_, Hi, Hi, Cin), dt, 1)
    s0 = rnd((R, Ci), dt, 2)
    g1 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 4)
    g2 = rnd((F_, 2 * Hi, 2 * Hi, Cout), dt, 5)

    def run(junction):
        pw, pb = mk_param((3, 3, Cin, Cout), dt, 0.03, seed=7), mk_param((Cout,), dt, 0.1, seed=8)
        ws = [mk_param((F_, Ci, Cout), dt, 0.1, seed=20 + i) for i in range(2 if two else 1)]
        bs = [mk_param((Cout,), dt, 0.1, seed=30 + i) for i in range(len(ws))]
        x = x0.clone().requires_grad_(True)
        skin = [s0.clone().requires_grad_(True) for _ in ws]
        assert ops.skips_pre_ok(dt)        # the training form of the 16-bit modes: the junction is what the model takes here
        sk = [ops.linear_z(si, w.master, w.c[0], Ci * Cout, b.master.detach(), 0, w.grad[0], Ci * Cout, b.grad, F_, act=ops.ACT_ELU, shared_x=True,
                           grad_is_pre=junction) for si, w, b in zip(skin, ws, bs)]
        out = ops.upconv_add(x, pw, pb, sk[0], sk[1] if two else None, skips_pre=junction)
        y, y2 = out if two else (out, None)
        loss = (y.float() * g1.float()).sum() + ((y2.float() * g2.float()).sum() if two else 0.0)
        loss.backward()
        ops.wgrad_join_now(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return [y, y2, x.grad, pw.grad.clone(), pb.grad.clone()] + [t.grad for t in skin] + [w.grad.clone() for w in ws] + [b.grad.clone() for b in bs]
    a, b = run(True), run(False)
    names = ['y', 'y2', 'dx', 'dW', 'db', 'dskip_in', 'dskip_in2', 'dWs', 'dWs2', 'dbs', 'dbs2']
    if not two:
        names = [n for n in names if not n.endswith('2') or n == 'y2']
    for n, u, v in zip(names, a, b):
        if u is not None:
            # activations / input gradients: the same arithmetic; weight gradients: f32 atomics of the stream-K launch (order-dependent last bits)
            if n in ('dW', 'db', 'dWs', 'dWs2', 'dbs', 'dbs2'):
                assert rel_err(u, v) < 1e-5, n
            elif n.startswith('dskip_in'):        # (few rows: linear_z sums the Z slices' input gradients with f32 atomics, then rounds)
                assert rel_err(u, v) < (1e-2 if dt == torch.bfloat16 else 2e-3), n
            else:
                assert torch.equal(u, v), n


def test_zz_report_error_ratios():
    """(runs last in this file) the largest max-norm and rms error ratios any comparison above produced, for the record in DESIGN 2a"""
    if _SEEN:
        print(f'\nop-level comparisons: {len(_SEEN)}; largest max-norm ratio {max(e for e, _ in _SEEN):.3e}, largest rms ratio {max(r for _, r in _SEEN):.3e}')
    for dt in DTYPES:
        rs = [(r, n) for d, n, r in _ELEM if d == dt]
        if rs:
            r, n = max(rs)
            print(f'per-element checks {str(dt):16s}: {len(rs)}; largest |err| / sum |terms| {r:.3e} ({n}), bound {EPS_ELEM[dt]:.3e}')
