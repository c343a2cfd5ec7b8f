"""A `dtype` outside enum stj_dtype at the raw C ABI: the entry points that used to run their f32 kernel for any unknown code.

Every such entry must return STJ_EINVAL, name itself in stj_last_error() and launch nothing.  Each pointer argument is a buffer of its
own, far larger than the f32 form of the call could touch and filled with a sentinel bit pattern, so a library that does run the f32
kernel stays inside its buffers and merely fails the test (return 0, output overwritten).  Shapes are the smallest that pass the
argument checks in front of the type switch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BAD = 7                     # not an stj_dtype
EINVAL = -1
NBYTES = 256 * 1024         # per pointer argument; the largest tensor any case below names is 16 x 32 x 8 f32 = 16 KiB
SENTINEL = 0xA5

P = object()                # a sentinel-filled device buffer of its own
ST = object()               # the current stream
RNG = object()              # the {seed, step} state of a DropCtx

# entry -> arguments in header order (dtype = BAD)
CASES = {
    # elementwise, n = 64
    'stj_unary_fwd': (P, P, 64, 1, 1.0, BAD, ST),
    'stj_unary_bwd': (P, P, P, 64, 2, 1.0, BAD, ST),
    'stj_elu_res_bwd': (P, P, P, P, P, P, 64, BAD, ST),
    'stj_dropout': (P, None, P, 64, 1, 0.5, RNG, 0, BAD, ST),
    # max over the middle axis: outer = 2, Tn = 3, C = 8
    'stj_maxpool_fwd': (P, P, P, 2, 3, 8, BAD, ST),
    'stj_maxpool_bwd': (P, P, P, P, 2, 3, 8, BAD, ST),
    # softmax: batch = 1, H = 1, Nq = 4, Nk = 8 (4 rows)
    'stj_softmax_fwd': (P, P, None, None, None, 1, 1, 4, 8, BAD, ST),
    'stj_softmax_bwd': (P, P, P, 4, 8, BAD, ST),
    # LayerNorm: rows = 2, C = 8, one parameter group
    'stj_layernorm_fwd': (P, P, P, P, P, P, 2, 8, 1e-5, 0, 0, 0, 1, 0, BAD, ST),
    'stj_layernorm_res_fwd': (P, P, P, P, P, P, P, 2, 8, 1e-5, 0, 1, 0, BAD, ST),
    'stj_layernorm_bwd': (P, P, P, P, P, P, P, P, 2, 8, 0, 0, 0, 1, 0, None, 1, 0, BAD, ST),
    # window attention: B = 1, one 8 x 8 window, one head
    'stj_win_attn_fwd': (P, P, P, 1, 8, 1, 0, BAD, ST),
    'stj_win_attn_bwd': (P, P, P, P, P, 1, 1, 8, 1, 0, BAD, ST),
    # FG-MSA offset head (B = 1, HW = 16, G = 1, gc = 8, C2 = 8) and sampled bias (B = G = 1, 2 x 2 map)
    'stj_fg_offset_fwd': (P, P, P, P, P, P, P, 1, 16, 1, 8, 8, 1.0, 0, BAD, ST),
    'stj_fg_offset_bwd': (P, P, P, P, P, P, P, P, P, P, P, P, 1, 16, 1, 8, 8, 1.0, 0, BAD, ST),
    'stj_fg_bias_fwd': (P, P, P, 1, 1, 2, 2, BAD, ST),
    'stj_fg_bias_bwd': (P, P, P, P, P, 1, 1, 2, 2, BAD, ST),
    # up-conv: F = 1, one 8 x 16 input tile, Cin = Cout = 8
    'stj_upconv_prep': (P, P, P, 8, 8, BAD, ST),
    'stj_upconv_fwd': (P, P, P, P, 1, 8, 16, 8, 8, 2, BAD, ST),
    'stj_upconv_dgrad': (P, P, P, None, 1, 8, 16, 8, 8, BAD, ST),
    'stj_upconv_wgrad': (P, P, P, None, 1, 1, 8, 16, 8, 8, 0, BAD, ST),
    # output heads: F = 1, 16 x 16, C = 8, Tn = 1, Y [1, 16, 16, 4]
    'stj_outconv_fwd': (P, P, P, P, 1, 16, 16, 8, 1, 1024, 4, 4, BAD, ST),
    'stj_outconv_bwd': (P, P, P, P, P, P, 1, 16, 16, 8, 1, 1024, 4, 4, 0, None, 0, BAD, ST),
    # im2col helpers: one 4 x 4 patch of one channel; N = 1, 2 x 2, G = 1, Cg = 4
    'stj_im2col_patch': (P, P, 1, 4, 4, 1, 1, 1, BAD, ST),
    'stj_im2col3': (P, P, 1, 2, 2, 1, 4, BAD, ST),
    'stj_col2im3': (P, P, 1, 2, 2, 1, 4, BAD, ST),
}


@pytest.mark.parametrize('entry', sorted(CASES))
def test_unknown_dtype_is_refused(lib_built, entry):
    assert torch.cuda.is_available()
    from strajnet_amd import _lib, ops
    L = _lib.lib()
    state = ops.DropCtx('cuda', seed=3).state
    bufs, args = [], []
    for a in CASES[entry]:
        if a is P:
            bufs.append(torch.full((NBYTES,), SENTINEL, dtype=torch.uint8, device='cuda'))
            assert bufs[-1].data_ptr() % 16 == 0
            args.append(ops.vp(bufs[-1].data_ptr()))
        elif a is ST:
            args.append(ops._st())
        elif a is RNG:
            args.append(ops.vp(state.data_ptr()))
        else:
            args.append(ops.vp(0) if a is None else a)
    assert len(args) == len(_lib.SIGNATURES[entry])
    rc = getattr(L, entry)(*args)
    torch.cuda.synchronize()
    msg = L.stj_last_error().decode()
    print(f'{entry}: rc = {rc}, last error = {msg!r}')
    assert rc == EINVAL
    assert msg and entry in msg
    for i, b in enumerate(bufs):
        assert bool((b == SENTINEL).all()), f'{entry}: pointer argument {i} was written'
