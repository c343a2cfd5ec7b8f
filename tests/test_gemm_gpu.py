"""stj_gemm across its dispatch paths, and the four helpers beside it, against float64 statements that share none of the kernels' logic.

Every case goes through the C ABI (ops.gemm / ops.gemm_group / ops.call) with raw pointers into flat buffers, exactly as the model addresses
its flat parameter / gradient buffers.  `gemm_ref` evaluates

    C[z1,z2][m,n] = act(alpha * sum_s sum_k A[z1 sAb1 + z2 sAb2 + s sAkb + m sAm + k sAk] * B[...] + bias[z1 sBias1 + z2 sBias2 + n]) + res[...]

in float64 by index arithmetic (torch.as_strided on CPU copies of the same flat buffers, the same element strides); it never looks at
orientation flags, tiles or vector legality.  Judgement, per case:
  * per element |got - ref| <= EPS_ELEM * T with T = |alpha| sum |a||b| + |bias| + |res| (+ |C0| when accumulating); a dtype-stored output
    uses its dtype's EPS_ELEM, an f32 output (c_f32, accumulate, colsum) of any operand type the f32 value (exact products, f32 accumulation
    over K * nkb <= 3456 terms).  ELU is 1-Lipschitz; GELU cases multiply T by max |gelu'| evaluated in float64.
  * an exact-arithmetic twin: the same addresses with integer operands from {-3..3}, integer bias / residual / C0, alpha 1 or 0.25, no
    activation.  Every product and every f32 partial sum is then exact in any order (9 K nkb + |C0| < 2^24), so an f32 output must EQUAL the
    float64 reference -- split-K atomics included -- and a dtype-stored output must equal the reference rounded once.
  * every output (and colsum) lies inside a larger allocation filled with a NaN bit pattern: >= 64 elements in front, behind and in every
    row gap; after the call everything but the output elements is compared bitwise, and an output element nobody wrote is still NaN.
  * accumulate cases start from a non-zero C (and colsum): "+=" is the contract.
Random operands are drawn as +-U[0.25, 1): sums still cancel, but no term and no bound falls into the subnormal range of fp16 / bf16, where a
bound relative to T does not describe the format.

Which kernels the matrix reaches is recorded in profiles/test_gemm_gpu_kernels.txt (rocprofv3 --kernel-trace --stats of this module alone).
Not reached, on purpose: deep-k instantiations in f32 (none exist: the deep body is 16-bit only); deep-k inside a group of two or more
(group_flush drops the flag); linear_rs with GELU, f32 output, split-K, K segments or a transposed activation (refused by linear_rs_try: the
cases on the far side of each refusal are here and run the tile kernels); the 'problem too large for a group' branch (needs > 2^20 tiles).
"""
import contextlib
import ctypes

import pytest
import torch

from test_ops_gpu import EPS_ELEM

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT16 = [torch.bfloat16, torch.float16]
GUARD = 64
PAT = {4: 0x7FA5A5A5, 2: 0x7FA5}          # NaN in f32, bf16 and fp16
IVIEW = {4: torch.int32, 2: torch.int16}
_RATIOS = []                               # (dtype, path, case, ratio, eps)


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib as L
    L.lib()


def rup8(x):
    return (x + 7) // 8 * 8


def gelu_slope_max():
    """max |d/dx gelu_tanh(x)| in float64 (the maximum is flat, a 1e-5 grid resolves it to ~1e-11)"""
    x = torch.linspace(-6.0, 6.0, 1200001, dtype=torch.float64)
    k = 0.7978845608028654
    u = k * (x + 0.044715 * x ** 3)
    t = torch.tanh(u)
    d = 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)
    return float(d.abs().max())


GELU_SLOPE = gelu_slope_max()


def gelu64(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def draw(n, dt, gen, exact, lim=3, scale=1.0):
    """n values of dtype dt on the CPU: integers in [-lim, lim] (exact twin) or +-U[0.25, 1) * scale"""
    if exact:
        return torch.randint(-lim, lim + 1, (n,), generator=gen).to(dt)
    mag = torch.rand(n, generator=gen) * 0.75 + 0.25
    sgn = torch.randint(0, 2, (n,), generator=gen) * 2 - 1
    return (mag * sgn * scale).to(dt)


def pattern(n, dt):
    es = torch.empty(0, dtype=dt).element_size()
    return torch.full((n,), PAT[es], dtype=IVIEW[es]).view(dt)


def bits(t):
    return t.view(IVIEW[t.element_size()])


def place(R, Cc, c_contig, ld, nkb, nb, bz, off, seg_mis):
    """Layout of an operand whose element (r, c) of segment s of batch (z1, z2) sits at off + z1 s1 + z2 s2 + s sseg + r sr + c sc."""
    if ld is None:
        ld = Cc if c_contig else R
    sr, sc = (ld, 1) if c_contig else (1, ld)
    span = max(1, (max(R, 1) - 1) * sr + (max(Cc, 1) - 1) * sc + 1)
    sseg = rup8(span) + (1 if seg_mis else 0)
    s2 = rup8(nkb * sseg) + 8
    s1 = nb[1] * s2 + 16
    if bz == 'zero':
        s1 = s2 = 0
    elif bz == 'zero1':
        s1 = 0
    elif bz == 'zero2':
        s1, s2 = s2, 0
    total = off + (nb[0] - 1) * s1 + (nb[1] - 1) * s2 + (nkb - 1) * sseg + span
    return dict(sr=sr, sc=sc, sseg=sseg, s1=s1, s2=s2, base=GUARD + off, size=GUARD + total + GUARD + 8)


def case(name, path, M, N, K, ta=0, tb=0, **kw):
    d = dict(name=name, path=path, M=M, N=N, K=K, ta=ta, tb=tb, lda=None, ldb=None, ldc=None, a_off=0, b_off=0, c_off=0, nb=(1, 1),
             a_bz='tight', b_bz='tight', bias=None, bias_per=False, res=None, ldres=None, act=0, alpha=1.0, c_f32=0, acc=0, splitk=1,
             colsum=False, nkb=1, a_seg_mis=False, b_seg_mis=False, group=False, c_pad=24, big=False)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    assert d['K'] * d['nkb'] <= 3456
    return d


class Prep:
    pass


def prepare(cs, dt, exact, seed=0):
    """Flat device buffers for one case, the ABI arguments, and the float64 reference."""
    from strajnet_amd import ops
    g = torch.Generator().manual_seed(1000 + seed)
    M, N, K, nb, nkb = cs['M'], cs['N'], cs['K'], cs['nb'], cs['nkb']
    alpha = cs['alpha'] if not exact else (1.0 if cs['alpha'] == 1.0 else 0.25)
    act = 0 if exact else cs['act']
    out_dt = torch.float32 if cs['c_f32'] else dt
    p = Prep()
    p.cs, p.dt, p.exact, p.out_dt = cs, dt, exact, out_dt
    p.path = cs['path'].replace('deep-k', 'plain (f32 has no deep-k)') if dt == torch.float32 else cs['path']
    la = place(M, K, not cs['ta'], cs['lda'], nkb, nb, cs['a_bz'], cs['a_off'], cs['a_seg_mis'])
    lb = place(K, N, bool(cs['tb']), cs['ldb'], nkb, nb, cs['b_bz'], cs['b_off'], cs['b_seg_mis'])
    A = draw(la['size'], dt, g, exact)
    B = draw(lb['size'], dt, g, exact)
    sz5a, st5a = (nb[0], nb[1], nkb, M, K), (la['s1'], la['s2'], la['sseg'], la['sr'], la['sc'])
    sz5b, st5b = (nb[0], nb[1], nkb, K, N), (lb['s1'], lb['s2'], lb['sseg'], lb['sr'], lb['sc'])
    # ---- output placement
    ldc = cs['ldc'] if cs['ldc'] is not None else N
    sC2 = M * ldc + cs['c_pad']
    sC1 = nb[1] * sC2 + 40
    c_base = GUARD + cs['c_off']
    c_size = c_base + (nb[0] - 1) * sC1 + (nb[1] - 1) * sC2 + max(M, 1) * ldc + GUARD
    Cinit = pattern(c_size, out_dt)
    idx = torch.as_strided(torch.arange(c_size), (nb[0], nb[1], M, N), (sC1, sC2, ldc, 1), c_base)
    C0 = None
    if cs['acc']:
        C0 = draw(idx.numel(), torch.float32, g, exact, lim=50, scale=4.0).reshape(idx.shape)
        Cinit[idx.reshape(-1)] = C0.reshape(-1)
    # ---- bias / colsum (both addressed with the bias batch strides) / residual
    sb2, sb1 = (rup8(N) + 4, nb[1] * (rup8(N) + 4) + 4) if cs['bias_per'] else (0, 0)
    v_base = GUARD + (1 if cs['bias'] == 'off1' else 0)
    v_size = v_base + (nb[0] - 1) * sb1 + (nb[1] - 1) * sb2 + N + GUARD
    bias = draw(v_size, torch.float32, g, exact, lim=4) if cs['bias'] else None
    cs_init = cs_idx = CS0 = None
    if cs['colsum']:
        cs_init = pattern(v_size, torch.float32)
        cs_idx = torch.as_strided(torch.arange(v_size), (nb[0], nb[1], N), (sb1, sb2, 1), v_base)
        CS0 = draw(cs_idx.numel(), torch.float32, g, exact, lim=50, scale=4.0).reshape(cs_idx.shape)
        cs_init[cs_idx.reshape(-1)] = CS0.reshape(-1)
    res = None
    ldres = cs['ldres'] if cs['ldres'] is not None else rup8(N) + 8
    sR2 = M * ldres + 8
    sR1 = nb[1] * sR2 + 8
    r_base = GUARD + (1 if cs['res'] == 'mis' else 0)
    if cs['res']:
        res = draw(r_base + (nb[0] - 1) * sR1 + (nb[1] - 1) * sR2 + max(M, 1) * ldres + GUARD, dt, g, exact, lim=4)
    # ---- float64 reference by index arithmetic on the flat arrays
    A5 = torch.as_strided(A.double(), sz5a, st5a, la['base'])
    B5 = torch.as_strided(B.double(), sz5b, st5b, lb['base'])
    Ac = A5.permute(0, 1, 3, 2, 4).reshape(nb[0], nb[1], M, nkb * K)
    Bc = B5.reshape(nb[0], nb[1], nkb * K, N)
    P = Ac @ Bc
    T = abs(alpha) * (Ac.abs() @ Bc.abs())
    ref = alpha * P
    if bias is not None:
        bv = torch.as_strided(bias.double(), (nb[0], nb[1], 1, N), (sb1, sb2, 0, 1), v_base)
        ref = ref + bv
        T = T + bv.abs()
    if act == ops.ACT_ELU:
        ref = torch.where(ref > 0, ref, torch.expm1(ref))
    elif act == ops.ACT_GELU:
        ref = gelu64(ref)
        T = T * GELU_SLOPE
    if res is not None:
        rv = torch.as_strided(res.double(), (nb[0], nb[1], M, N), (sR1, sR2, ldres, 1), r_base)
        ref = ref + rv
        T = T + rv.abs()
    if C0 is not None:
        ref = ref + C0.double()
        T = T + C0.double().abs()
    p.ref, p.T, p.idx, p.Cinit = ref, T, idx, Cinit
    if cs['colsum']:
        p.cs_ref = CS0.double() + Bc.sum(2)
        p.cs_T = CS0.double().abs() + Bc.abs().sum(2)
        p.cs_idx, p.cs_init = cs_idx, cs_init
    # ---- device copies and ABI arguments
    p.A, p.B, p.C = A.cuda(), B.cuda(), Cinit.cuda()
    p.bias = bias.cuda() if bias is not None else None
    p.res = res.cuda() if res is not None else None
    p.colsum = cs_init.cuda() if cs['colsum'] else None
    p.args = (ops._poff(p.A, la['base']), ops._poff(p.B, lb['base']), ops._poff(p.C, c_base), M, N, K,
              (la['s1'], la['s2'], la['sr'], la['sc']), (lb['s1'], lb['s2'], lb['sr'], lb['sc']), (sC1, sC2, ldc), ops.DTYPE_CODE[dt])
    p.kw = dict(bias=ops._poff(p.bias, v_base) if bias is not None else None, sBias=(sb1, sb2),
                res=ops._poff(p.res, r_base) if res is not None else None, sRes=(sR1, sR2, ldres), nb=nb, act=act, alpha=alpha,
                c_f32=cs['c_f32'], accumulate=cs['acc'], splitk=cs['splitk'],
                colsum=ops._poff(p.colsum, v_base) if cs['colsum'] else None, kseg=(nkb, la['sseg'], lb['sseg']))
    return p


def launch(p):
    from strajnet_amd import ops
    queued = ops.gemm(*p.args, **p.kw)
    assert queued is False          # raw pointers: launched (or recorded into the open group), never handed to the deferred schedule


def _judge_buf(p, label, dev_buf, init, idx, ref, T, out_dt):
    got_flat = dev_buf.cpu()
    keep = torch.ones(init.numel(), dtype=torch.bool)
    keep[idx.reshape(-1)] = False
    bad = (bits(got_flat)[keep] != bits(init)[keep]).nonzero()
    assert bad.numel() == 0, f'{label}: {bad.numel()} guard elements changed, first at flat index {int(keep.nonzero()[bad[0, 0]])}'
    got = got_flat[idx.reshape(-1)].reshape(idx.shape).double()
    if p.exact:
        want = ref.to(out_dt).double()
        ne = (got != want)
        assert not bool(ne.any()), (f'{label}: {int(ne.sum())} of {ne.numel()} elements differ from the exact result, first '
                                    f'{tuple(ne.nonzero()[0].tolist())}: got {float(got[ne][0])}, want {float(want[ne][0])}')
        return
    eps = EPS_ELEM[out_dt]
    ratio = float(((got - ref).abs() / (T + 1e-300)).max()) if got.numel() else 0.0
    _RATIOS.append((p.dt, p.path + (' [colsum]' if label.endswith('colsum') else ''), p.cs['name'], ratio, eps))
    print(f'{label:60s} {str(p.dt):15s} max |err| / sum |terms| = {ratio:.3e}  (bound {eps:.3e})')
    assert ratio <= eps, f'{label}: max |err| / sum |terms| = {ratio:.3e} over the per-element bound {eps:.3e}'


def judge(p):
    torch.cuda.synchronize()
    label = p.cs['name'] + (' (exact twin)' if p.exact else '')
    _judge_buf(p, label, p.C, p.Cinit, p.idx, p.ref, p.T, p.out_dt)
    if p.cs['colsum']:
        _judge_buf(p, label + ' colsum', p.colsum, p.cs_init, p.cs_idx, p.cs_ref, p.cs_T, torch.float32)


def run_case(cs, dt):
    from strajnet_amd import ops
    for exact in ((False,) if cs['big'] else (False, True)):
        p = prepare(cs, dt, exact)
        with (ops.gemm_group() if cs['group'] else contextlib.nullcontext()):
            launch(p)
        judge(p)


def run_row(cases, dt):
    """Every case of one row of the matrix in one test (the suite's per-test garbage collection and device drain cost more than a case does);
    all cases run, and the failure names each case that missed with its own message."""
    failed = []
    for cs in cases:
        try:
            run_case(cs, dt)
        except AssertionError as e:
            failed.append(f"{cs['name']} [{dt}]: {e}")
    assert not failed, f'{len(failed)} of {len(cases)} cases failed:\n' + '\n'.join(failed)


# ------------------------------------------------------------------------------------------------------------------------------------------
# The case matrix.  `path` is the label of the error-ratio table; the comment of a case names the condition in launch_gemm that sends it there.
# ------------------------------------------------------------------------------------------------------------------------------------------
ORI = [('NN', 0, 0), ('NT', 0, 1), ('TN', 1, 0), ('TT', 1, 1)]       # second letter T: B stored [K,N] (n contiguous, tb = 1)


def ld_of(M, N, K, ta, tb, pad=0):
    """leading strides, padded to a multiple of 8 elements (+ pad): vector staging legal although the extents are ragged"""
    return dict(lda=rup8(M if ta else K) + pad, ldb=rup8(N if tb else K) + pad)


ORIENT = []
for o, ta, tb in ORI:
    # tiles64 = 16 * 18 = 288 >= 256: 64x64 tiles; K = 77 is no multiple of BK (64 / 32) or 8: last chunk of each row takes the scalar fallback
    ORIENT.append(case(f'tile64_{o}', 'tile 64x64', 1001, 1093, 77, ta, tb, ldc=1104, bias='vec', **ld_of(1001, 1093, 77, ta, tb)))
    # tiles64 = 4 < 256, M, N >= 32, not accumulating: 32x32 tiles
    ORIENT.append(case(f'tile32_{o}', 'tile 32x32', 100, 70, 77, ta, tb, ldc=80, bias='vec', **ld_of(100, 70, 77, ta, tb)))

STAGING = []
for o, ta, tb in ORI:
    # (a) 16-bit, K > 128, vecA && vecB, K, M, N % 8 == 0: deep-k body; K = 200 / 328 leave a tail chunk range the clamped loads must zero
    STAGING.append(case(f'deep64_{o}', 'deep-k 64x64', 1024, 1088, 200, ta, tb, bias='vec', act=2))
    STAGING.append(case(f'deep32_{o}', 'deep-k 32x32', 104, 72, 328, ta, tb, res='vec'))
    # (b) aligned but K <= 128 -> plain body, vector loads
    STAGING.append(case(f'plainvec_k128_{o}', 'plain, vector loads', 104, 72, 128, ta, tb))
    # (b) K > 128 but M % 8 != 0 -> plain body, vector loads (the row-contiguous operand's last chunk is scalar)
    STAGING.append(case(f'plainvec_m_ragged_{o}', 'plain, vector loads', 1001, 1088, 200, ta, tb, ldc=1088, **ld_of(1001, 1088, 200, ta, tb)))
    # (c) leading stride 42 (the [3,384,42] head layout) / odd, for A and for B separately: vecA / vecB = 0, scalar staging of that operand
    STAGING.append(case(f'ld42_A_{o}', 'plain, scalar staging', 40, 40, 40, ta, tb, lda=42, ldb=40))
    STAGING.append(case(f'ld42_B_{o}', 'plain, scalar staging', 40, 40, 40, ta, tb, lda=40, ldb=42))
    STAGING.append(case(f'ldodd_A_{o}', 'plain, scalar staging', 104, 72, 200, ta, tb, lda=209, ldb=200 if not tb else 72))
    STAGING.append(case(f'ldodd_B_{o}', 'plain, scalar staging', 104, 72, 200, ta, tb, lda=200 if not ta else 104, ldb=211))
    # (d) base pointer one element off 16 bytes, strides legal
    STAGING.append(case(f'off1_A_{o}', 'plain, scalar staging', 104, 72, 200, ta, tb, a_off=1))
    STAGING.append(case(f'off1_B_{o}', 'plain, scalar staging', 104, 72, 200, ta, tb, b_off=1))

TINY = [
    case('M_lt_32', 'tile 64x64', 7, 70, 40, bias='vec'),                     # M < 32: 64x64 tiles although tiles64 < 256
    case('N_lt_32', 'tile 64x64', 70, 5, 40, 0, 1, bias='vec'),
    case('K_lt_8', 'tile 32x32', 40, 40, 5, bias='vec'),                      # K < 8: no full chunk, every element through the scalar fallback
    case('K_lt_8_TT', 'tile 32x32', 40, 40, 5, 1, 1),
    case('K_eq_1', 'tile 32x32', 33, 47, 1, bias='vec', res='vec'),           # sAk == 1 with K = 1
    case('K_eq_1_M_eq_1', 'tile 64x64', 1, 1, 1),
    case('K_eq_0', 'tile 32x32', 40, 40, 0, bias='vec', act=2, res='vec'),    # K = 0 without accumulate: act(bias) + res
    case('K_eq_0_nobias', 'tile 64x64', 9, 40, 0),                            # ... and plain zeros
    case('K_eq_0_acc', 'split-K atomics', 40, 40, 0, c_f32=1, acc=1),         # K = 0 with accumulate: every slice is empty, C unchanged
    case('K_eq_0_acc_auto', 'split-K atomics', 40, 40, 0, c_f32=1, acc=1, splitk=0, colsum=True),
]

BATCH = [
    # nb = (6, 4), distinct strides on both levels; batched q k^T form (NT would be [N,K] k-contiguous = tb 0)
    case('nb64_distinct', 'batched', 50, 40, 32, nb=(6, 4), alpha=0.25, c_f32=1, ldc=40),
    case('nb64_ldc_gt_N', 'batched', 50, 40, 32, 0, 1, nb=(6, 4), ldc=56, bias='vec', bias_per=True),        # per-batch bias, ldc > N
    case('nb64_shared_A', 'batched', 50, 40, 72, nb=(6, 4), a_bz='zero', ldc=48, res='vec', ldres=56),       # zero stride on A, ldres != ldc
    case('nb64_shared_B', 'batched', 50, 40, 72, 1, 1, nb=(6, 4), b_bz='zero', ldc=43, res='mis', ldres=45),  # zero stride on B (shared weight)
    case('nb64_shared_A_level1', 'batched', 36, 33, 20, nb=(6, 4), a_bz='zero1', b_bz='zero2', bias='off1', bias_per=True),
    case('nb64_deep', 'deep-k 32x32', 40, 48, 264, 0, 1, nb=(2, 3), bias='vec', bias_per=True, ldc=56),
    case('nb_tile64', 'batched', 200, 136, 72, 1, 0, nb=(6, 4), ldc=136, **ld_of(200, 136, 72, 1, 0)),       # tiles64 = 4*3*24 = 288: 64x64 tiles from the batch count
]

EPI = []
for nm, ta, tb in (('NN', 0, 0), ('TT', 1, 1)):
    for bias in (None, 'vec'):
        for act in (0, 2, 1):
            for res in (None, 'vec', 'mis'):
                for cf in (0, 1):
                    # N % 8 != 0 with vecC legal (ldc = 104): the last chunk of every row takes the scalar form, the others the vector form
                    if nm == 'TT' and (bias is None or act == 0):
                        continue
                    EPI.append(case(f'epi_{nm}_b{int(bias is not None)}_a{act}_r{res or "no"}_f{cf}', 'epilogue f32 store' if cf else 'epilogue dtype store',
                                    70, 99, 72, ta, tb, ldc=104, bias=bias, act=act, res=res, c_f32=cf, **ld_of(70, 99, 72, ta, tb)))
EPI += [
    case('epi_alpha_quarter', 'epilogue dtype store', 70, 99, 72, alpha=0.25, ldc=104, bias='vec', res='vec', act=1),
    case('epi_alpha_negative', 'epilogue dtype store', 70, 99, 72, alpha=-1.5, ldc=104, bias='vec', res='mis'),
    case('epi_alpha_negative_f32', 'epilogue f32 store', 70, 99, 72, 0, 1, alpha=-1.5, ldc=104, bias='vec', c_f32=1),
    case('epi_ldc_odd', 'epilogue dtype store', 70, 99, 72, ldc=101, bias='vec', res='vec', act=2),          # vecC = 0: every store scalar
    case('epi_c_off1', 'epilogue dtype store', 70, 96, 72, ldc=104, c_off=1, bias='off1', res='vec'),        # C base off 16 bytes
    case('epi_f32_ldc_odd', 'epilogue f32 store', 70, 96, 72, ldc=99, c_f32=1, bias='vec', act=2),
    case('epi_tile64_gelu_res', 'epilogue dtype store', 1001, 1093, 40, ldc=1104, bias='vec', act=1, res='vec', ldres=1096),
    case('epi_deep_gelu_res_mis', 'deep-k 32x32', 104, 72, 200, bias='vec', act=1, res='mis', ldres=73),
]

SPLITK = []
for sk in (1, 3, 8, 16):
    # explicit splitk with accumulate; gridDim.y % 8 == 0 (8, 16 with nb = 1) takes the XCD-aware work map, 3 does not
    SPLITK.append(case(f'splitk{sk}_TN', 'split-K atomics', 96, 130, 1000, 1, 1, c_f32=1, acc=1, splitk=sk, colsum=True, ldc=136,
                       **ld_of(96, 130, 1000, 1, 1)))
    SPLITK.append(case(f'splitk{sk}_bias_NN', 'split-K atomics', 70, 99, 333, c_f32=1, acc=1, splitk=sk, bias='vec'))     # bias added once, by slice 0
SPLITK += [
    # deep-k body under split-K (16-bit: K > 128, all aligned): 192-element k-tiles, K = 1000 -> 6 tiles over 16 slices: 10 empty slices
    case('splitk16_deep_TN', 'split-K atomics, deep-k', 96, 128, 1000, 1, 1, c_f32=1, acc=1, splitk=16, colsum=True),
    case('splitk_gt_ktiles', 'split-K atomics', 70, 99, 100, c_f32=1, acc=1, splitk=16, bias='vec'),            # 2 (4 in f32) k-tiles, 16 slices
    case('splitk_gt_ktiles_colsum', 'split-K atomics', 70, 99, 100, 1, 1, c_f32=1, acc=1, splitk=8, colsum=True),
    # auto: tiles64 = 1 -> s = min(768, 96, ktiles / 2): K = 1037 -> 17 (33) k-tiles -> 8 (16)
    case('splitk_auto_ge8', 'split-K atomics', 64, 64, 1037, 1, 1, c_f32=1, acc=1, splitk=0, colsum=True, **ld_of(64, 64, 1037, 1, 1)),
    case('splitk_auto_ge8_deep', 'split-K atomics, deep-k', 64, 64, 1040, 1, 1, c_f32=1, acc=1, splitk=0, colsum=True),
    case('splitk_auto_1', 'split-K atomics', 64, 64, 100, 1, 1, c_f32=1, acc=1, splitk=0),                      # ktiles / 2 < 2 -> 1
    case('splitk_auto_1_colsum', 'split-K atomics', 70, 40, 60, 1, 1, c_f32=1, acc=1, splitk=0, colsum=True),
    case('splitk_batched_colsum', 'split-K atomics', 70, 99, 333, 1, 1, nb=(2, 3), c_f32=1, acc=1, splitk=4, colsum=True, bias_per=True,
         **ld_of(70, 99, 333, 1, 1)),                                                                              # gridDim.y = 24: XCD map with batches
    case('splitk_batched_auto', 'split-K atomics', 70, 99, 333, 1, 1, nb=(2, 3), c_f32=1, acc=1, splitk=0, colsum=True, bias_per=True),
    case('splitk3_batched_bias', 'split-K atomics', 70, 99, 333, nb=(2, 3), c_f32=1, acc=1, splitk=3, bias='vec', bias_per=True),
]

KSEG = []
for nkb in (2, 8):
    for mis in (False, True):
        t = f'nkb{nkb}_{"mis" if mis else "vec"}'
        # K = 72 per segment: ragged against BK (64 / 32); a_seg_mis / b_seg_mis make sAkb / sBkb odd -> vecA / vecB dropped
        KSEG.append(case(f'{t}_store_NN', 'K segments', 70, 99, 72, nkb=nkb, a_seg_mis=mis, b_seg_mis=mis, bias='vec', act=2, ldc=104))
        KSEG.append(case(f'{t}_store_TT', 'K segments', 70, 99, 77, 1, 1, nkb=nkb, a_seg_mis=mis, b_seg_mis=mis, res='vec',
                         **ld_of(70, 99, 77, 1, 1)))
        # 2 (3 in f32) k-tiles per segment, splitk = 3 / 5: slices cross segment boundaries
        KSEG.append(case(f'{t}_acc_splitk3_TN', 'K segments, split-K', 70, 99, 72, 1, 1, nkb=nkb, a_seg_mis=mis, b_seg_mis=mis, c_f32=1, acc=1,
                         splitk=3, colsum=True, **ld_of(70, 99, 72, 1, 1)))
        KSEG.append(case(f'{t}_acc_splitk5_NN', 'K segments, split-K', 70, 99, 77, nkb=nkb, a_seg_mis=mis, b_seg_mis=mis, c_f32=1, acc=1,
                         splitk=5, bias='vec'))
KSEG += [
    case('nkb2_deep', 'K segments, deep-k', 104, 72, 200, 0, 1, nkb=2, bias='vec'),                  # deep-k body walking two segments
    case('nkb8_deep_acc_splitk8', 'K segments, deep-k', 96, 128, 200, 1, 1, nkb=8, c_f32=1, acc=1, splitk=8, colsum=True),
    case('nkb8_shared_A_batched', 'K segments', 70, 99, 72, 1, 1, nkb=8, nb=(2, 3), a_bz='zero', c_f32=1, acc=1, splitk=0),
]

# Row-streaming kernel (linear_rs_try): 16-bit, M >= rs_min_m = 16384, K in {96, 128, 192, 288, 384}, N % 8 == 0, everything 16-byte legal,
# activation none / ELU.  tb = 1: weight [K,N]; tb = 0: weight [N,K].
RS = []
_rs_m = [16384, 16385, 16384 + 77, 16384 + 127]
_rs_n = [8, 96, 136]
_rs_epi = [dict(), dict(bias='vec', act=2), dict(bias='vec', res='vec'), dict(res='vec', act=2)]
for i, Kk in enumerate((96, 128, 192, 288, 384)):
    for tb in (1, 0):
        j = 2 * i + tb
        Mm, Nn = _rs_m[j % 4], _rs_n[j % 3]
        RS.append(case(f'rs_K{Kk}_{"KN" if tb else "NK"}_M{Mm}_N{Nn}', 'row-streaming', Mm, Nn, Kk, 0, tb, ldc=Nn + 8, **_rs_epi[j % 4]))
RS += [
    case('rs_M131072_KN', 'row-streaming', 131072, 96, 96, 0, 1, ldc=104, bias='vec', act=2, big=True),
    case('rs_batched_KN', 'row-streaming', 16384 + 77, 40, 128, 0, 1, nb=(1, 2), ldc=48, bias='vec', bias_per=True, res='vec'),
    # one case on each side of every refusal that is cheap to hit: these run the tile kernels (deep-k or plain) at the same size
    case('rs_refused_M16383', 'row-streaming boundary (tile kernels)', 16383, 96, 96, 0, 1, ldc=104, bias='vec', act=2),
    case('rs_taken_M16384', 'row-streaming', 16384, 96, 96, 0, 1, ldc=104, bias='vec', act=2),
    case('rs_refused_N100', 'row-streaming boundary (tile kernels)', 16384, 100, 96, 0, 1, ldb=104, ldc=104, bias='vec'),
    case('rs_refused_bias_off16', 'row-streaming boundary (tile kernels)', 16384, 96, 96, 0, 1, ldc=104, bias='off1'),
    case('rs_refused_gelu', 'row-streaming boundary (tile kernels)', 16384, 96, 96, 0, 0, ldc=104, bias='vec', act=1),
    case('rs_refused_res_mis', 'row-streaming boundary (tile kernels)', 16384, 96, 96, 0, 0, ldc=104, res='mis'),
    case('rs_taken_res_vec', 'row-streaming', 16384, 96, 96, 0, 0, ldc=104, res='vec'),
]

GROUP1 = []
for c in ORIENT:           # the 16-way switch of group_flush for a group of one, plain ...
    GROUP1.append(dict(c, name='group1_' + c['name'], path='group of one, ' + c['path'], group=True))
for c in STAGING:          # ... and deep
    if c['name'].startswith('deep'):
        GROUP1.append(dict(c, name='group1_' + c['name'], path='group of one, ' + c['path'], group=True))
GROUP1 += [
    case('group1_splitk_auto', 'group of one, split-K', 64, 64, 1037, 1, 1, c_f32=1, acc=1, splitk=0, colsum=True, group=True,
         **ld_of(64, 64, 1037, 1, 1)),
    case('group1_NT32_res', 'group of one, tile 32x32', 100, 70, 40, 0, 1, ldc=72, bias='vec', res='vec', group=True),
]


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_orientation_x_tile(dt):
    run_row(ORIENT, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_staging_path(dt):
    run_row(STAGING, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_tiny_and_degenerate(dt):
    run_row(TINY, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_k0_accumulate_and_empty_problems_write_nothing(dt):
    """K = 0 with accumulate leaves C bit-identical (run_case above already holds it to C0 exactly; here bitwise, with a bias that must NOT be
    added: no slice has work); M = 0, N = 0, nb1 = 0 and nb2 = 0 return OK and write nothing."""
    from strajnet_amd import ops
    for cs in (case('K0_acc_bits', '-', 40, 40, 0, c_f32=1, acc=1, splitk=1),
               case('M0', '-', 40, 40, 16), case('N0', '-', 40, 40, 16), case('nb1_0', '-', 40, 40, 16), case('nb2_0', '-', 40, 40, 16)):
        p = prepare(cs, dt, False)
        a = list(p.args)
        kw = dict(p.kw)
        if cs['name'] == 'M0':
            a[3] = 0
        elif cs['name'] == 'N0':
            a[4] = 0
        elif cs['name'] == 'nb1_0':
            kw['nb'] = (0, 1)
        elif cs['name'] == 'nb2_0':
            kw['nb'] = (1, 0)
        ops.gemm(*a, **kw)
        torch.cuda.synchronize()
        assert torch.equal(bits(p.C.cpu()), bits(p.Cinit)), cs['name']


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_batches(dt):
    run_row(BATCH, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_epilogues(dt):
    run_row(EPI, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_split_k(dt):
    run_row(SPLITK, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_k_segments(dt):
    run_row(KSEG, dt)


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_row_streaming(dt):
    run_row(RS, dt)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_group_of_one(dt):
    run_row(GROUP1, dt)


def _named(cases, name):
    return next(c for c in cases if c['name'] == name)


@pytest.mark.parametrize('exact', [False, True], ids=['random', 'exact'])
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_group_of_six_flushes_at_four(dt, exact):
    """Six problems of one dtype in one group (GG_MAX = 4: early flush, then a group of two), every orientation, both tile sizes, a deep-k
    candidate (the group kernel runs it with the plain body) and two split-K problems with auto splitk; each against float64, guards checked."""
    from strajnet_amd import ops
    specs = [_named(ORIENT, 'tile64_NN'), _named(ORIENT, 'tile32_TT'), _named(STAGING, 'deep32_NT'), _named(SPLITK, 'splitk_auto_ge8'),
             _named(ORIENT, 'tile32_TN'), _named(SPLITK, 'splitk_batched_auto')]
    ps = [prepare(dict(c, path='group kernel'), dt, exact, seed=i) for i, c in enumerate(specs)]
    with ops.gemm_group():
        for p in ps:
            launch(p)
    for p in ps:
        judge(p)


@pytest.mark.parametrize('exact', [False, True], ids=['random', 'exact'])
@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_group_dtype_change_flushes(dt, exact):
    """A dtype change mid-group flushes what was recorded: [dt, dt, other, other, dt] -> groups of 2, 2 and 1."""
    from strajnet_amd import ops
    other = torch.float16 if dt != torch.float16 else torch.float32
    specs = [(_named(ORIENT, 'tile32_NT'), dt), (_named(EPI, 'epi_ldc_odd'), dt), (_named(ORIENT, 'tile32_TN'), other),
             (_named(SPLITK, 'splitk_auto_1_colsum'), other), (_named(STAGING, 'deep32_TT'), dt)]
    ps = [prepare(dict(c, path='group kernel, dtype change'), d, exact, seed=10 + i) for i, (c, d) in enumerate(specs)]
    with ops.gemm_group():
        for p in ps:
            launch(p)
    for p in ps:
        judge(p)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_argument_errors(dt):
    """Every STJ_EINVAL branch at the top of stj_gemm raises through ops.call with a message and leaves C bit-identical."""
    from strajnet_amd import ops
    from strajnet_amd._lib import StjError
    p = prepare(case('einval', '-', 40, 40, 16, bias='vec', res='vec', colsum=False), dt, False)
    pa = prepare(case('einval_acc', '-', 40, 40, 16, c_f32=1, acc=1, colsum=True), dt, False)
    from strajnet_amd._lib import lib
    blank = ctypes.create_string_buffer(int(lib().stj_gemm_group_workspace_bytes()))      # zeroed host memory: no magic

    def abi(q, **over):
        A, B, C, M, N, K, sA, sB, sC, code = q.args
        k = dict(q.kw)
        v = dict(A=A, B=B, C=C, bias=k['bias'], res=k['res'], colsum=k['colsum'], M=M, N=N, K=K, nb1=1, nb2=1, act=k['act'], alpha=1.0, dtype=code,
                 c_f32=k['c_f32'], accumulate=k['accumulate'], splitk=k['splitk'], nkb=1, group=None)
        v.update(over)
        return ('stj_gemm', ops._p(v['A']), ops._p(v['B']), ops._p(v['C']), ops._p(v['bias']), ops._p(v['res']), ops._p(v['colsum']),
                v['M'], v['N'], v['K'], v['nb1'], v['nb2'], sA[0], sA[1], sA[2], sA[3], sB[0], sB[1], sB[2], sB[3], sC[0], sC[1], sC[2],
                k['sBias'][0], k['sBias'][1], k['sRes'][0], k['sRes'][1], k['sRes'][2], v['act'], v['alpha'], v['dtype'], v['c_f32'],
                v['accumulate'], v['splitk'], v['nkb'], 0, 0, v['group'], ops._st())
    bad = [('negative K', p, dict(K=-1)), ('negative splitk', pa, dict(splitk=-1)), ('nkb < 1', p, dict(nkb=0)),
           ('accumulate without c_f32', p, dict(accumulate=1, bias=None, res=None)),
           ('splitk != 1 without accumulate', p, dict(splitk=2)), ('auto splitk without accumulate', p, dict(splitk=0)),
           ('colsum with bias', pa, dict(bias=p.kw['bias'])), ('colsum without accumulate', pa, dict(accumulate=0)),
           ('accumulate with activation', pa, dict(act=ops.ACT_ELU, colsum=None)), ('accumulate with residual', pa, dict(res=p.kw['res'], colsum=None)),
           ('nb1 * nb2 * splitk > 65535', pa, dict(nb1=256, nb2=64, splitk=4)), ('nb1 * nb2 > 65535', p, dict(nb1=256, nb2=256)),
           ('uninitialised group', p, dict(group=ctypes.cast(blank, ctypes.c_void_p))), ('bad dtype', p, dict(dtype=7))]
    for what, q, over in bad:
        with pytest.raises(StjError) as ei:
            ops.call(*abi(q, **over))
        msg = str(ei.value)
        assert 'stj_gemm' in msg and len(msg.split(':', 1)[1].strip()) > 0, (what, msg)
        torch.cuda.synchronize()
        assert torch.equal(bits(q.C.cpu()), bits(q.Cinit)), what
        if q.colsum is not None:
            assert torch.equal(bits(q.colsum.cpu()), bits(q.cs_init)), what
    ops.call(*abi(p))                     # the unmodified arguments are legal
    judge(p)


# ------------------------------------------------------------------------------------------------------------------------------------------
# The helpers beside it
# ------------------------------------------------------------------------------------------------------------------------------------------
COLSUM = [(1, 3, 3, 0), (63, 100, 104, 0), (64, 2100, 2104, 0), (65, 2100, 2101, 0), (65, 8, 8, 0), (64, 1030, 1032, 1),
          (40000, 100, 104, 0), (40000, 7, 7, 1), (33000, 24, 24, 0)]


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_colsum_exact(dt):
    """out[n] += sum_m X[m,n]: N below one vector, ragged, above 256 vectors (second column pass); M around one row strip and above 512 * 64
    (rows_per_block grows); ld > N; vector-legal and misaligned X.  Integer X in {-3..3} and an integer pre-fill: every f32 partial sum is
    exact (3 * 40000 < 2^24), so out must equal the float64 column sums whatever order the atomics land in."""
    for M, N, ld, off in COLSUM:
        _colsum_exact(dt, M, N, ld, off)


def _colsum_exact(dt, M, N, ld, off):
    from strajnet_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N)
    X = draw(GUARD + off + M * ld + GUARD, dt, g, True)
    out0 = pattern(GUARD + N + GUARD, torch.float32)
    pre = draw(N, torch.float32, g, True, lim=100)
    out0[GUARD:GUARD + N] = pre
    Xd, od = X.cuda(), out0.cuda()
    ops.call('stj_colsum', ops._poff(Xd, GUARD + off), ops._poff(od, GUARD), M, N, ld, ops.DTYPE_CODE[dt], ops._st())
    torch.cuda.synchronize()
    ref = pre.double() + torch.as_strided(X.double(), (M, N), (ld, 1), GUARD + off).sum(0)
    got = od.cpu()
    assert torch.equal(got[GUARD:GUARD + N].double(), ref), (M, N, ld, off)
    assert torch.equal(bits(got[:GUARD]), bits(out0[:GUARD])) and torch.equal(bits(got[GUARD + N:]), bits(out0[GUARD + N:])), (M, N, ld, off)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_colsum_random(dt):
    from strajnet_amd import ops
    M, N, ld = 3456, 100, 104
    g = torch.Generator().manual_seed(5)
    X = draw(GUARD + M * ld + GUARD, dt, g, False)
    pre = draw(N, torch.float32, g, False)
    Xd, od = X.cuda(), pre.cuda()
    ops.call('stj_colsum', ops._p(Xd[GUARD:]), ops._p(od), M, N, ld, ops.DTYPE_CODE[dt], ops._st())
    torch.cuda.synchronize()
    xv = torch.as_strided(X.double(), (M, N), (ld, 1), GUARD)
    ref, T = pre.double() + xv.sum(0), pre.double().abs() + xv.abs().sum(0)
    ratio = float(((od.cpu().double() - ref).abs() / T).max())
    _RATIOS.append((dt, 'stj_colsum', 'colsum_random', ratio, EPS_ELEM[torch.float32]))
    assert ratio <= EPS_ELEM[torch.float32], ratio
    with pytest.raises(Exception):
        ops.call('stj_colsum', ops._p(Xd), ops._p(od), M, N, ld, 9, ops._st())


def _f32_from_bits(b):
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in b], dtype=torch.int32).view(torch.float32)


def _cast_specials(dt):
    drop = 16 if dt == torch.bfloat16 else 13          # mantissa bits the target drops
    half = 1 << (drop - 1)
    b = []
    for base in (0x3F800000, 0x40490000, 0xBF800000, 0xC2F70000, 0x3F7FE000 if drop == 13 else 0x3F7F0000):
        base &= ~((1 << drop) - 1)
        for odd in (0, 1):                             # exact ties below an even and below an odd mantissa, and one bit either side of each
            m = base | (odd << drop)
            b += [m | half, m | (half - 1), m | (half + 1), m]
    b += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF]
    x = _f32_from_bits(b)
    extra = [65504.0, 65519.996, 65520.0, -65520.0, 1e5, -1e5, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 * 1.0001, 1e-7, 6.1e-5,
             2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-39, -1e-39, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -149, 1e-45]
    return torch.cat([x, torch.tensor(extra, dtype=torch.float32)])


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_cast_f32_to_16_rounds_to_nearest_even_like_torch(dt):
    """f32 -> bf16 / fp16 equals torch.Tensor.to(dt) on the CPU bitwise (round to nearest even, what TensorFlow's cast does too): ties in both
    directions, the largest finite values, overflow, target subnormals, +-0, +-inf; NaN stays NaN.  n = 1, 7, the specials, 3 M + 1 random."""
    from strajnet_amd import ops
    sp = _cast_specials(dt)
    g = torch.Generator().manual_seed(3)
    big = torch.randn(3_000_001, generator=g) * torch.logspace(-6, 4, 3_000_001)
    for src in (sp, sp[:1], sp[3:10], big):
        n = src.numel()
        dst0 = pattern(GUARD + n + GUARD, dt)
        s, d = src.cuda(), dst0.cuda()
        ops.call('stj_cast', ops._p(s), 0, ops._poff(d, GUARD), ops.DTYPE_CODE[dt], n, ops._st())
        torch.cuda.synchronize()
        got, want = d.cpu(), src.to(dt)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got[GUARD:GUARD + n]), nan)
        gb, wb = bits(got[GUARD:GUARD + n])[~nan], bits(want)[~nan]
        ne = (gb != wb).nonzero()
        assert ne.numel() == 0, f'{ne.numel()} differ; first: f32 {float(src[~nan][ne[0, 0]])!r} -> got bits {int(gb[ne[0, 0]]) & 0xffff:#06x}, torch {int(wb[ne[0, 0]]) & 0xffff:#06x}'
        assert torch.equal(bits(got[:GUARD]), bits(dst0[:GUARD])) and torch.equal(bits(got[GUARD + n:]), bits(dst0[GUARD + n:]))


@pytest.mark.parametrize('dt', DT16, ids=str)
def test_cast_16_to_f32_exact_and_copies(dt):
    """16-bit -> f32 is exact for all 65536 bit patterns (NaN stays NaN); same-type copies are bit-identical; bf16 <-> fp16 is STJ_EINVAL."""
    from strajnet_amd import ops
    from strajnet_amd._lib import StjError
    code = ops.DTYPE_CODE[dt]
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)
    s = allb.cuda()
    d = torch.zeros(65536, device='cuda')
    ops.call('stj_cast', ops._p(s), code, ops._p(d), 0, 65536, ops._st())
    torch.cuda.synchronize()
    want, got = allb.float(), d.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])
    g = torch.Generator().manual_seed(4)
    for t, c in ((dt, code), (torch.float32, 0)):
        for n in (1, 7, 1_000_003):
            src = (torch.randn(n, generator=g) * 10).to(t)
            dst0 = pattern(GUARD + n + GUARD, t)
            sd, dd = src.cuda(), dst0.cuda()
            ops.call('stj_cast', ops._p(sd), c, ops._poff(dd, GUARD), c, n, ops._st())
            torch.cuda.synchronize()
            got = dd.cpu()
            assert torch.equal(bits(got[GUARD:GUARD + n]), bits(src))
            assert torch.equal(bits(got[:GUARD]), bits(dst0[:GUARD])) and torch.equal(bits(got[GUARD + n:]), bits(dst0[GUARD + n:]))
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    o0 = pattern(64, other)
    od = o0.cuda()
    with pytest.raises(StjError) as ei:
        ops.call('stj_cast', ops._p(s), code, ops._p(od), ops.DTYPE_CODE[other], 64, ops._st())
    assert 'stj_cast' in str(ei.value)
    torch.cuda.synchronize()
    assert torch.equal(bits(od.cpu()), bits(o0))


def _window(t):
    return range(max(0, 3 - t), min(7, 10 - t) + 1)


@pytest.mark.parametrize('dt', DTYPES, ids=str)
def test_time_collapse(dt):
    """Wz[t] = sum_{j = max(0, 3 - t)}^{min(7, 10 - t)} W[j] (the statement of test_conv3d_time_collapse in test_oracle_kat.py), written out in
    float64.  f32 output: within one f32 rounding per addend; 16-bit output: the float64 sum rounded once, the sum taken up to that f32 error."""
    for n in (1, 1237, 96 * 128, 96 * 192):          # one element, an odd count, Cin * Cout of the decoder's skips
        _time_collapse(dt, n)


def _time_collapse(dt, n):
    from strajnet_amd import ops
    g = torch.Generator().manual_seed(n)
    W = torch.randn(8, n, generator=g)
    out0 = pattern(GUARD + 8 * n + GUARD, dt)
    Wd, od = W.cuda(), out0.cuda()
    ops.call('stj_time_collapse', ops._p(Wd), ops._poff(od, GUARD), n, ops.DTYPE_CODE[dt], ops._st())
    torch.cuda.synchronize()
    W64 = W.double()
    ref = torch.stack([sum(W64[j] for j in _window(t)) for t in range(8)])
    e = 8 * 2.0 ** -24 * torch.stack([sum(W64[j].abs() for j in _window(t)) for t in range(8)])
    got = od.cpu()
    y = got[GUARD:GUARD + 8 * n].reshape(8, n).double()
    if dt == torch.float32:
        assert bool(((y - ref).abs() <= e).all()), (n, float(((y - ref).abs() / e).max()))
    else:
        lo, hi = (ref - e).to(dt).double(), (ref + e).to(dt).double()
        assert bool(((y >= lo) & (y <= hi)).all()), n
    assert torch.equal(bits(got[:GUARD]), bits(out0[:GUARD])) and torch.equal(bits(got[GUARD + 8 * n:]), bits(out0[GUARD + 8 * n:]))


@pytest.mark.parametrize('n', [1, 1237, 96 * 128])
def test_time_fold_accumulates_and_is_adjoint(n):
    """dW[j] += sum over the t whose window contains j of dWz[t], from a pre-filled dW; and <collapse(W), G> == <W, fold(G)> in float64."""
    from strajnet_amd import ops
    g = torch.Generator().manual_seed(n + 1)
    G, W, pre = torch.randn(8, n, generator=g), torch.randn(8, n, generator=g), torch.randn(8, n, generator=g)
    buf0 = pattern(GUARD + 8 * n + GUARD, torch.float32)
    buf0[GUARD:GUARD + 8 * n] = pre.reshape(-1)
    Gd, bd = G.cuda(), buf0.cuda()
    ops.call('stj_time_fold', ops._p(Gd), ops._poff(bd, GUARD), n, ops._st())
    torch.cuda.synchronize()
    G64 = G.double()
    add = torch.stack([sum((G64[t] for t in range(8) if j in _window(t)), torch.zeros(n, dtype=torch.float64)) for j in range(8)])
    addabs = torch.stack([sum((G64[t].abs() for t in range(8) if j in _window(t)), torch.zeros(n, dtype=torch.float64)) for j in range(8)])
    got = bd.cpu()
    y = got[GUARD:GUARD + 8 * n].reshape(8, n).double()
    e = 9 * 2.0 ** -24 * (pre.double().abs() + addabs)
    assert bool(((y - (pre.double() + add)).abs() <= e).all())
    assert torch.equal(bits(got[:GUARD]), bits(buf0[:GUARD])) and torch.equal(bits(got[GUARD + 8 * n:]), bits(buf0[GUARD + 8 * n:]))
    # adjointness, both kernels in f32 from the device
    Wd, cz, fz = W.cuda(), torch.empty(8, n, device='cuda'), torch.zeros(8, n, device='cuda')
    ops.call('stj_time_collapse', ops._p(Wd), ops._p(cz), n, 0, ops._st())
    ops.call('stj_time_fold', ops._p(Gd), ops._p(fz), n, ops._st())
    torch.cuda.synchronize()
    lhs, rhs = float((cz.cpu().double() * G64).sum()), float((W.double() * fz.cpu().double()).sum())
    scale = float((cz.cpu().double() * G64).abs().sum())
    assert abs(lhs - rhs) <= 1e-6 * scale, (lhs, rhs, scale)


def test_fold_parts():
    """g[idx[i]] += parts[i]; parts[i] = +0.0 for i < n: idx with repeats into a pre-filled g, parts with zeros, negatives and one -0.0 (integer
    values: the atomics are exact in any order); beyond n nothing is touched; a null pointer is STJ_EINVAL."""
    from strajnet_amd import ops
    from strajnet_amd._lib import StjError
    gen = torch.Generator().manual_seed(9)
    n, tail, ng = 100_003, 77, 5000
    idx = torch.randint(0, ng, (n + tail,), generator=gen)
    parts = torch.randint(-5, 6, (n + tail,), generator=gen).float()
    parts[123] = -0.0
    assert int((parts[:n] == 0).sum()) > 100 and int((parts[:n] < 0).sum()) > 100
    g0 = pattern(GUARD + ng + GUARD, torch.float32)
    pre = torch.randint(-100, 101, (ng,), generator=gen).float()
    g0[GUARD:GUARD + ng] = pre
    gd, idd, pd = g0.cuda(), idx.cuda(), parts.cuda()
    ops.call('stj_fold_parts', ops._poff(gd, GUARD), ops._p(idd), ops._p(pd), n, ops._st())
    torch.cuda.synchronize()
    ref = pre.double().index_add(0, idx[:n], parts[:n].double())
    got = gd.cpu()
    assert torch.equal(got[GUARD:GUARD + ng].double(), ref)
    assert torch.equal(bits(got[:GUARD]), bits(g0[:GUARD])) and torch.equal(bits(got[GUARD + ng:]), bits(g0[GUARD + ng:]))
    pa = pd.cpu()
    assert bool((bits(pa[:n]) == 0).all())                       # +0.0 bitwise, the -0.0 included
    assert torch.equal(bits(pa[n:]), bits(parts[n:]))
    for a in ((None, idd, pd), (gd, None, pd), (gd, idd, None)):
        with pytest.raises(StjError) as ei:
            ops.call('stj_fold_parts', ops._p(a[0]), ops._p(a[1]), ops._p(a[2]), n, ops._st())
        assert 'stj_fold_parts' in str(ei.value)


def test_zz_report_gemm_error_ratios():
    """(runs last in this file) the largest |err| / sum |terms| per (dtype, path), for the table in DESIGN.md"""
    best = {}
    for dt, path, name, r, eps in _RATIOS:
        k = (str(dt), path)
        if k not in best or r > best[k][0]:
            best[k] = (r, name, eps)
    print()
    for (dt, path), (r, name, eps) in sorted(best.items()):
        print(f'gemm per-element {dt:15s} {path:42s} largest |err| / sum |terms| {r:.3e} ({name}), bound {eps:.3e}')
