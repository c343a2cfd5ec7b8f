"""The device-state Nadam step (csrc/optim.hip: stj_gradnorm_partials, stj_nadam_prepare, stj_nadam_apply) through the raw C ABI and
through optim.DeviceNadam / graph.GraphedTrainStep(optimizer=), against the float64 references of _optim_cases.py.

Bounds.  Sum of squares: 1e-9 relative (the f32 -> f64 squares are exact; a double sum of n <= 2^23 non-negative terms is within
n 2^-53 < 1e-9 of the exact one in any order).  coef: 2^-23 relative of the float64 reference rounded to float32 (the rounding of the
store, plus a last-bit difference between two float64 libm's moved across a float32 rounding boundary); state[0..4]: 1e-12 relative.
Weights after an update: rel_err < 1e-5 against float64 (the gate of tests/test_ops_gpu.py, test_nadam_step_matches_keras_formula),
1e-6 against the host-state optim.Nadam.  No case and no element is excluded; the only either-side acceptance is the learning rate at
the geometric restarts _optim_cases.schedule_values names (steps 10, 30, 70 of COS_GEOM, 45657 of COS_TRAIN).
"""
import ctypes

import numpy as np
import pytest
import torch

import _optim_cases as OC

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
B1, B2, EPS = 0.9, 0.999, 1e-7


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


def _ptr(t, off=0):
    return vp(0) if t is None else vp(t.data_ptr() + off)


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _f64(t):
    return t.detach().cpu().double().numpy()


_GRADS = {}


def grad(n, seed):
    """The seeded gradient on the host (float32) -- made once, never written."""
    if (n, seed) not in _GRADS:
        _GRADS[(n, seed)] = OC.gradient(n, seed)
    return _GRADS[(n, seed)]


def partials_of(g):
    from strajnet_amd import _lib
    p = torch.full((OC.PARTS,), float('nan'), dtype=torch.float64, device='cuda')
    _lib.call('stj_gradnorm_partials', _ptr(g), g.numel(), _ptr(p), _stream())
    torch.cuda.synchronize()
    return p.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- stj_gradnorm_partials
@pytest.mark.parametrize('n', OC.SIZES)
def test_gradnorm_partials_accuracy_repeatability_overwrite(n):
    """Sum of the partials against float64 within 1e-9; two calls bitwise equal; every slot of a NaN-filled buffer overwritten (at n = 1
    all but one workgroup have no element and store 0.0)."""
    g = torch.from_numpy(grad(n, 1)).cuda()
    a, b = partials_of(g), partials_of(g)
    want = float(np.sum(grad(n, 1).astype(np.float64) ** 2))
    got = float(np.sum(a))
    print(f'n {n}: sum of squares {got!r} vs float64 {want!r}, rel {abs(got - want) / want:.3e}')
    assert np.all(np.isfinite(a)), 'a slot was not written'
    assert a.tobytes() == b.tobytes()
    assert OC.close(got, want, 1e-9)
    if n == 1:
        x = float(grad(1, 1)[0])
        assert np.count_nonzero(a) == 1 and a[0] == x * x


@pytest.mark.parametrize('n', OC.SIZES)
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_gradnorm_partials_nonfinite(n, bad):
    """One NaN or one +inf at the first element, a middle element or the last (tail) element makes the fold non-finite."""
    for pos in sorted({0, n // 2, n - 1}):
        g = torch.from_numpy(grad(n, 2)).cuda()
        g[pos] = bad
        s = float(np.sum(partials_of(g)))
        assert not np.isfinite(s), (n, pos, bad, s)
    assert np.isfinite(np.sum(partials_of(torch.from_numpy(grad(n, 2)).cuda())))


# ---------------------------------------------------------------------------------------------------------------- stj_nadam_prepare
PREPARE_CASES = [(OC.CONSTANT, 0), (OC.COS_ARITH, 5), (OC.COS_GEOM, 5), (OC.COS_GEOM, 25), (OC.COS_GEOM, 65), (OC.COS_TRAIN, 45657),
                 (OC.CUSTOM, 0), (OC.CUSTOM, 3995)]


@pytest.mark.parametrize('sched,start', PREPARE_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_prepare_ten_consecutive_calls(sched, start):
    """Ten consecutive calls from `iterations` = start (m_schedule the product the reference has there): coef and state after each."""
    from strajnet_amd import _lib
    ref = OC.RefState(sched, B1, B2, iterations=start)
    state = torch.from_numpy(ref.state()).cuda()
    sc = torch.from_numpy(OC.encode(sched)).cuda()
    coef = torch.full((8,), -7.0, device='cuda')
    for k in range(10):
        _lib.call('stj_nadam_prepare', _ptr(state), _ptr(sc), vp(0), _ptr(coef), vp(0), vp(0), B1, B2, 1.0, 0.0, 1.0, 0, _stream())
        torch.cuda.synchronize()
        want = ref.prepare()
        c, s = coef.cpu().numpy(), state.cpu().numpy()
        step = start + k
        lrs = ref.lr_values
        print(f'{sched[0]} step {step}: coef {c[:6].tolist()} state {s[:5].tolist()} reference lr {lrs}')
        assert any(OC.close(float(c[0]), OC.f32(v), 2.0 ** -23) for v in lrs), (step, float(c[0]), lrs)
        for i in range(1, 6):
            assert OC.close(float(c[i]), OC.f32(want[i]), 2.0 ** -23), (step, i, float(c[i]), want[i])
        assert c[6] == 0.0 and c[7] == 0.0
        r = ref.state()
        assert s[0] == r[0] and OC.close(s[1], r[1], 1e-12) and s[2] == 0.0 and s[3] == 0.0, (step, s, r)
        assert any(OC.close(s[4], v, 1e-12) for v in lrs), (step, s[4], lrs)
        assert np.all(s[5:] == 0.0)


def test_prepare_running_loss_sums_and_norm():
    """losses / running: count and the four sums x loss_scale on every call; with partials: state[3] = gscale sqrt(sum), the clip scale."""
    from strajnet_amd import _lib
    ref = OC.RefState(OC.CONSTANT, B1, B2, clipnorm=1.0)
    state = torch.from_numpy(ref.state()).cuda()
    sc = torch.from_numpy(OC.encode(OC.CONSTANT)).cuda()
    coef = torch.zeros(8, device='cuda')
    running = torch.zeros(5, dtype=torch.float64, device='cuda')
    parts = np.zeros(OC.PARTS)
    parts[3], parts[200] = 9.0, 16.0                       # sum 25: norm 5 x gscale .5 = 2.5
    p = torch.from_numpy(parts).cuda()
    want_run = np.zeros(5)
    for k in range(3):
        lv = np.array([1.5, 0.25, 3.0, 0.125], dtype=np.float32) * (k + 1)
        losses = torch.from_numpy(lv).cuda()
        _lib.call('stj_nadam_prepare', _ptr(state), _ptr(sc), _ptr(p), _ptr(coef), _ptr(losses), _ptr(running), B1, B2, 0.5, 1.0, 2.0, 0, _stream())
        torch.cuda.synchronize()
        want = ref.prepare(25.0, 0.5)
        want_run += np.concatenate([[1.0], lv.astype(np.float64) * 2.0])
        assert np.array_equal(running.cpu().numpy(), want_run)
        c, s = coef.cpu().numpy(), state.cpu().numpy()
        assert s[3] == 2.5 and c[4] == np.float32(0.5 / 2.5) and OC.close(float(c[4]), OC.f32(want[4]), 2.0 ** -23)


# ---------------------------------------------------------------------------------------------------------------- optim.DeviceNadam
def _weights(n):
    return OC.gradient(n, 100)


@pytest.mark.parametrize('n', OC.SIZES)
def test_device_nadam_three_steps(n):
    """Three steps under a schedule against the float64 update (rel_err < 1e-5) and against the host-state optim.Nadam on the same
    gradients at a constant rate (<= 1e-6 relative)."""
    from strajnet_amd.optim import CosineDecayRestarts, DeviceNadam, Nadam
    w = torch.from_numpy(_weights(n)).cuda()
    g = torch.zeros(n, device='cuda')
    opt = DeviceNadam(w, g, lr=CosineDecayRestarts(1e-2, 10, t_mul=2.0, m_mul=0.9))
    ref = OC.RefNadam(_weights(n), ('cosine', 1e-2, 10.0, 2.0, 0.9, 0.0))
    wd, wh = torch.from_numpy(_weights(n)).cuda(), torch.from_numpy(_weights(n)).cuda()
    dev, host = DeviceNadam(wd, g, lr=1e-2), Nadam(wh, g, lr=1e-2)
    for t in range(3):
        g.copy_(torch.from_numpy(grad(n, 10 + t)))
        opt.step()
        dev.step()
        host.step()
        ref.step(grad(n, 10 + t))
    torch.cuda.synchronize()
    e = OC.rel_err(_f64(w), ref.w)
    d = float((wd - wh).abs().max() / wh.abs().max())
    print(f'n {n}: vs float64 {e:.3e}; vs host Nadam {d:.3e}; lr {float(opt.lr)!r} iterations {float(opt.iterations)}')
    assert e < 1e-5
    assert d <= 1e-6
    assert OC.rel_err(_f64(opt.m), ref.m) < 1e-5 and OC.rel_err(_f64(opt.v), ref.v) < 1e-5
    assert float(opt.iterations) == 3.0 and float(opt.skipped) == 0.0 and float(opt.grad_norm) == 0.0
    assert OC.close(float(opt.lr), ref.s.lr, 1e-12)


def _scaled_gradient(n, seed, norm):
    g = grad(n, seed).astype(np.float64)
    return (g * (norm / np.sqrt(np.sum(g * g)))).astype(np.float32)


def test_clip():
    """Norm 10 under global_clipnorm = 1: the float64 update of g / 10; norm 0.5: bit-identical to no clip; grad_norm reads both."""
    from strajnet_amd.optim import DeviceNadam
    n = 1003
    g10, g05 = _scaled_gradient(n, 20, 10.0), _scaled_gradient(n, 21, 0.5)
    w = torch.from_numpy(_weights(n)).cuda()
    g = torch.from_numpy(g10).cuda()
    opt = DeviceNadam(w, g, lr=1e-2, global_clipnorm=1.0)
    opt.step()
    norm = float(np.sqrt(np.sum(g10.astype(np.float64) ** 2)))
    ref = OC.RefNadam(_weights(n), ('constant', 1e-2))
    ref.step(g10.astype(np.float64) / norm)                        # g / 10, the norm as float64 sees the float32 gradient
    clipped = OC.RefNadam(_weights(n), ('constant', 1e-2), clipnorm=1.0)
    clipped.step(g10)
    assert OC.close(float(opt.grad_norm), 10.0, 1e-6) and OC.close(float(opt.grad_norm), norm, 1e-12)
    e = OC.rel_err(_f64(w), ref.w)
    print(f'clip: norm {float(opt.grad_norm)!r}; update vs float64 of g/10 {e:.3e}; coef gscale {float(opt.coef[4])!r}')
    assert e < 1e-5 and OC.rel_err(_f64(w), clipped.w) < 1e-5
    assert OC.close(float(opt.coef[4]), OC.f32(1.0 / norm), 2.0 ** -23)
    # within the norm: the same bits as an optimizer that does not clip
    wa, wb = torch.from_numpy(_weights(n)).cuda(), torch.from_numpy(_weights(n)).cuda()
    g.copy_(torch.from_numpy(g05))
    a, b = DeviceNadam(wa, g, lr=1e-2, global_clipnorm=1.0), DeviceNadam(wb, g, lr=1e-2)
    for _ in range(2):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert torch.equal(wa, wb) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.coef, b.coef)
    assert OC.close(float(a.grad_norm), 0.5, 1e-6) and float(b.grad_norm) == 0.0


def test_skip_nonfinite():
    """A NaN in step 2 of 3 with skip_nonfinite: that step changes nothing but `skipped`, the norm and the loss means; step 3 is the
    update with t = 2.  Without the flag the same input makes w non-finite."""
    from strajnet_amd.optim import DeviceNadam, LOSS_MEAN_KEYS
    n = 1003
    gs = [grad(n, 30), grad(n, 31).copy(), grad(n, 32)]
    gs[1][n - 2] = np.nan
    w = torch.from_numpy(_weights(n)).cuda()
    g = torch.zeros(n, device='cuda')
    losses = torch.tensor([1.0, 2.0, 3.0, 4.0], device='cuda')
    opt = DeviceNadam(w, g, lr=1e-2, skip_nonfinite=True)
    opt.attach_loss_means(losses, 2.0)
    ref = OC.RefNadam(_weights(n), ('constant', 1e-2), skip_nonfinite=True)
    for t in range(3):
        before = [x.clone() for x in (w, opt.m, opt.v, opt.state)]
        g.copy_(torch.from_numpy(gs[t]))
        losses.fill_(float(t + 1))
        opt.step()
        ref.step(gs[t])
        torch.cuda.synchronize()
        if t == 1:
            assert torch.equal(w, before[0]) and torch.equal(opt.m, before[1]) and torch.equal(opt.v, before[2])
            assert torch.equal(opt.state[:2], before[3][:2]) and torch.equal(opt.state[4:], before[3][4:])
            assert float(opt.iterations) == 1.0 and float(opt.skipped) == 1.0 and not np.isfinite(float(opt.grad_norm))
            assert float(opt.coef[5]) == 0.0
    assert float(opt.iterations) == 2.0 and float(opt.skipped) == 1.0 and ref.s.iterations == 2
    assert OC.rel_err(_f64(w), ref.w) < 1e-5 and bool(torch.isfinite(w).all())
    assert OC.close(float(opt.state[1]), ref.s.m_schedule, 1e-12)
    r = opt.loss_result()
    assert float(opt.running[0]) == 3.0 and tuple(r) == LOSS_MEAN_KEYS and all(v == 4.0 for v in r.values())      # mean of 1, 2, 3 x 2
    opt.reset_loss_means()
    assert all(v == 0.0 for v in opt.loss_result().values())
    # without the flag the NaN propagates, as in Keras
    w2 = torch.from_numpy(_weights(n)).cuda()
    plain = DeviceNadam(w2, g, lr=1e-2)
    g.copy_(torch.from_numpy(gs[1]))
    plain.step()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(w2).all()) and float(plain.iterations) == 1.0


def test_step_is_capturable():
    """step() (three launches: clip + skip on) captured at n = 1003 and replayed three times with g rewritten between the replays equals
    three eager steps from the same start bit for bit -- what the host-scalar Nadam cannot do."""
    from strajnet_amd.optim import CosineDecayRestarts, DeviceNadam
    n = 1003
    kw = dict(global_clipnorm=30.0, skip_nonfinite=True)
    we, wg = torch.from_numpy(_weights(n)).cuda(), torch.from_numpy(_weights(n)).cuda()
    ge, gg = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    eager = DeviceNadam(we, ge, lr=CosineDecayRestarts(1e-2, 2, t_mul=1.0, m_mul=0.5), **kw)
    graphed = DeviceNadam(wg, gg, lr=CosineDecayRestarts(1e-2, 2, t_mul=1.0, m_mul=0.5), **kw)
    for t in range(3):                                   # (also loads the kernels before the capture)
        ge.copy_(torch.from_numpy(_scaled_gradient(n, 40 + t, 20.0 * (t + 1))))
        eager.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step()
    torch.cuda.synchronize()
    assert float(graphed.iterations) == 0.0 and torch.equal(wg, torch.from_numpy(_weights(n)).cuda())       # a capture runs nothing
    for t in range(3):
        gg.copy_(torch.from_numpy(_scaled_gradient(n, 40 + t, 20.0 * (t + 1))))
        graph.replay()
    torch.cuda.synchronize()
    assert float(graphed.iterations) == 3.0
    for a, b in ((we, wg), (eager.m, graphed.m), (eager.v, graphed.v), (eager.state, graphed.state), (eager.coef, graphed.coef)):
        assert torch.equal(a, b)
    assert float(graphed.coef[4]) == np.float32(30.0 / float(graphed.grad_norm))          # the third step (norm 60) was clipped


def test_state_dict_round_trip():
    from strajnet_amd.optim import DeviceNadam
    n = 1003
    w, g = torch.from_numpy(_weights(n)).cuda(), torch.from_numpy(grad(n, 50)).cuda()
    a = DeviceNadam(w, g, lr=1e-2)
    a.step()
    sd = a.state_dict()
    assert set(sd) == {'m', 'v', 'state'} and all(not t.is_cuda for t in sd.values())
    w2 = w.clone()
    b = DeviceNadam(w2, g, lr=1e-2)
    b.load_state_dict(sd)
    a.step()
    b.step()
    torch.cuda.synchronize()
    assert torch.equal(w, w2) and torch.equal(a.state, b.state) and float(b.iterations) == 2.0
    with pytest.raises(ValueError):
        b.load_state_dict({'m': sd['m'], 'v': sd['v']})


def test_refusals():
    """Misaligned buffers and n < 0: STJ_EINVAL with the entry's name in the message, nothing launched, the outputs untouched.  The
    class refuses what optim.Nadam refuses."""
    from strajnet_amd import _lib
    from strajnet_amd.optim import DeviceNadam
    L = _lib.lib()
    EINVAL = _lib.ENUMS['stj_status']['STJ_EINVAL']
    n = 64
    f = lambda val, k=n + 4: torch.full((k,), val, device='cuda')
    w, g, m, v = f(1.0), f(2.0), f(3.0), f(4.0)
    parts = torch.full((OC.PARTS + 1,), -7.0, dtype=torch.float64, device='cuda')
    state = torch.full((9,), 5.0, dtype=torch.float64, device='cuda')
    sc = torch.from_numpy(OC.encode(OC.CONSTANT)).cuda()
    coef = torch.full((12,), -7.0, device='cuda')
    losses, running = torch.ones(4, device='cuda'), torch.full((5,), 3.0, dtype=torch.float64, device='cuda')
    st = _stream()

    def refused(rc, entry):
        assert rc == EINVAL and L.stj_last_error().decode().startswith(entry + ': '), (rc, L.stj_last_error())
    refused(L.stj_gradnorm_partials(_ptr(g, 4), n, _ptr(parts), st), 'stj_gradnorm_partials')
    refused(L.stj_gradnorm_partials(_ptr(g), n, _ptr(parts, 4), st), 'stj_gradnorm_partials')
    refused(L.stj_gradnorm_partials(_ptr(g), -1, _ptr(parts), st), 'stj_gradnorm_partials')
    refused(L.stj_gradnorm_partials(_ptr(g), n, vp(0), st), 'stj_gradnorm_partials')
    for bad in ((_ptr(w, 4), _ptr(g), _ptr(m), _ptr(v), n, _ptr(coef)), (_ptr(w), _ptr(g, 4), _ptr(m), _ptr(v), n, _ptr(coef)),
                (_ptr(w), _ptr(g), _ptr(m, 4), _ptr(v), n, _ptr(coef)), (_ptr(w), _ptr(g), _ptr(m), _ptr(v, 4), n, _ptr(coef)),
                (_ptr(w), _ptr(g), _ptr(m), _ptr(v), n, _ptr(coef, 4)), (_ptr(w), _ptr(g), _ptr(m), _ptr(v), -1, _ptr(coef)),
                (_ptr(w), _ptr(g), _ptr(m), _ptr(v), n, vp(0))):
        refused(L.stj_nadam_apply(*bad, B1, B2, EPS, st), 'stj_nadam_apply')
    tail = (B1, B2, 1.0, 0.0, 1.0)
    refused(L.stj_nadam_prepare(_ptr(state, 4), _ptr(sc), vp(0), _ptr(coef), vp(0), vp(0), *tail, 0, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(_ptr(state), _ptr(sc), _ptr(parts, 4), _ptr(coef), vp(0), vp(0), *tail, 0, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(_ptr(state), _ptr(sc), vp(0), _ptr(coef, 4), vp(0), vp(0), *tail, 0, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(_ptr(state), _ptr(sc), vp(0), _ptr(coef), _ptr(losses), vp(0), *tail, 0, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(_ptr(state), _ptr(sc), vp(0), _ptr(coef), vp(0), _ptr(running), *tail, 0, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(_ptr(state), _ptr(sc), vp(0), _ptr(coef), vp(0), vp(0), *tail, 2, st), 'stj_nadam_prepare')
    refused(L.stj_nadam_prepare(vp(0), _ptr(sc), vp(0), _ptr(coef), vp(0), vp(0), *tail, 0, st), 'stj_nadam_prepare')
    assert L.stj_nadam_apply(_ptr(w), _ptr(g), _ptr(m), _ptr(v), 0, _ptr(coef), B1, B2, EPS, st) == 0          # n = 0: nothing to do
    torch.cuda.synchronize()
    for t, val in ((w, 1.0), (g, 2.0), (m, 3.0), (v, 4.0), (parts, -7.0), (state, 5.0), (coef, -7.0), (running, 3.0)):
        assert bool((t == val).all())
    with pytest.raises(ValueError):
        DeviceNadam(w, g.double())
    with pytest.raises(ValueError):
        DeviceNadam(w, g[:8])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceNadam(w.cpu(), g.cpu())
    with pytest.raises(ValueError, match='global_clipnorm'):
        DeviceNadam(w, g, global_clipnorm=0.0)
    opt = DeviceNadam(w, g)
    opt.attach_loss_means(None, 1.0)
    with pytest.raises(RuntimeError, match='no loss tensor'):
        opt.step()
    with pytest.raises(ValueError):
        opt.attach_loss_means(torch.ones(5, device='cuda'), 1.0)


# ---------------------------------------------------------------------------------------------------------------- the captured train step
def test_graphed_train_step_with_optimizer():
    """CFG128, B = 1, bf16, training=False (no draw differs between passes).  Construction -- two warm-up passes and the capture --
    leaves weights, moments, optimizer state and running sums bit for bit; each of three replays moves the weights by the float64 update
    of the gradients that replay left in model.flat_grads() (exact with respect to the order of the gradients' atomics, unlike a
    comparison of two runs); the loss means are the means of the three steps' losses x replica."""
    from oracle import np_ref
    from strajnet_amd import (STrajNet, OGMFlow_loss, OccupancyFlowTaskConfig, DeviceNadam, CosineDecayRestarts)
    from strajnet_amd.graph import GraphedTrainStep
    from strajnet_amd.optim import LOSS_MEAN_KEYS
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.bfloat16)
    model.load_weights(np_ref.make_weights(CFG128, 0))
    xt = {k: torch.as_tensor(v).cuda() for k, v in np_ref.make_inputs(CFG128, 1).items()}
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=2.0, use_focal_loss=False, use_gt=True)
    sched = ('cosine', 1e-4, 10.0, 2.0, 0.9, 0.0)
    opt = DeviceNadam.for_model(model, lr=CosineDecayRestarts(*sched[1:3], t_mul=sched[3], m_mul=sched[4], alpha=sched[5]))
    with pytest.raises(ValueError, match=r'optimizer\.step\(\) after sync\.head_and_wait\(\)'):
        GraphedTrainStep(model, loss_fn, xt, training=False, split=True, optimizer=opt)
    assert not model.cut_encoder
    opt.attach_loss_means(None, loss_fn.replica)
    opt.m.fill_(0.25)                                    # (not the all-zero start: a restore that zeroes instead of copying would pass)
    opt.v.fill_(0.5)
    before = [t.clone() for t in opt.tensors()]
    shadow = model._cflat.clone()                        # the bf16 copy the kernels read
    step = GraphedTrainStep(model, loss_fn, xt, training=False, optimizer=opt)
    torch.cuda.synchronize()
    for t, b in zip(opt.tensors(), before):
        assert torch.equal(t, b)
    assert torch.equal(model._cflat, shadow)
    assert float(opt.iterations) == 0.0 and float(opt.running[0]) == 0.0
    ref = OC.RefNadam(_f64(model.flat_weights()), sched)
    ref.m[:], ref.v[:] = 0.25, 0.5
    seen = []
    for k in range(3):
        w0 = _f64(model.flat_weights())
        seen.append(_f64(step()) * loss_fn.replica)
        torch.cuda.synchronize()
        g = model.flat_grads().cpu().numpy()
        assert np.all(np.isfinite(g)) and np.any(g != 0.0)
        want = ref.step(g, w=w0)
        e = OC.rel_err(_f64(model.flat_weights()), want)
        moved = float(np.abs(_f64(model.flat_weights()) - w0).max())
        print(f'replay {k}: weights vs float64 update {e:.3e}; largest move {moved:.3e}; lr {float(opt.lr)!r}')
        assert e < 1e-5 and moved > 0.0
        assert OC.close(float(opt.lr), ref.s.lr, 1e-12)
    assert float(opt.iterations) == 3.0 and float(opt.skipped) == 0.0
    got, want = opt.loss_result(), np.mean(seen, axis=0)
    assert tuple(got) == LOSS_MEAN_KEYS
    for v, x in zip(got.values(), want):
        assert OC.close(v, float(x), 1e-6), (got, want)
    assert len({s.tobytes() for s in seen}) == 3          # the weights moved: three different losses
