"""The fused validation pass (stj_eval_fwd, csrc/eval.hip) through the raw C ABI on the cases of _eval_cases.py -- against float64,
against the four launches it replaces, for bitwise repeatability and workspace handling, running means and refusals -- and the
captured validation step (graph.GraphedEvalStep) against the eager one (evaluate.eval_step) on the model.

Bounds: the four losses within 3e-5 |ref| + 1e-6 of np_ref.ogm_flow_loss (the gate of tests/test_ops_gpu.py, test_loss_and_gate), the
seven metrics within 1e-4 max(1, |ref|) of np_ref.occupancy_flow_metrics (the gate of tests/test_model_gpu.py,
test_device_metrics_match_oracle), the gates equal to the oracle's.  No case and no element is excluded anywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

import _eval_cases as EC

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


_DEV = {}


def dev_case(shape, seed=0):
    """The case's arrays on the GPU (uploaded once, never written)."""
    key = (tuple(shape), seed)
    if key not in _DEV:
        _DEV[key] = {k: torch.from_numpy(v.copy()).cuda() for k, v in EC.make_case(*shape, seed).items()}
    return _DEV[key]


def _ptr(t, off=0):
    return vp(0) if t is None else vp(t.data_ptr() + off)


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def ws_bytes(shape):
    from strajnet_amd import _lib
    return int(_lib.lib().stj_eval_workspace_bytes(*shape))


def run_fused(shape, flags, no_warp=False, seed=0, ws=None, running=None, loss_scale=1.0):
    """stj_eval_fwd on a case -> dict of host float arrays: loss[5], metrics[7], gate[8], auc[8,4]."""
    from strajnet_amd import _lib
    c = dev_case(shape, seed)
    if ws is None:
        ws = torch.empty(ws_bytes(shape), dtype=torch.uint8, device='cuda')
    out = dict(loss=torch.full((5,), -7.0, device='cuda'), metrics=torch.full((7,), -7.0, device='cuda'),
               gate=torch.full((8,), -7.0, device='cuda'), auc=torch.full((8, 4), -7.0, device='cuda'))
    _lib.call('stj_eval_fwd', _ptr(c['logits']), _ptr(c['gt_obs']), _ptr(c['gt_occ']), _ptr(c['gt_flow']), _ptr(c['origin_flow']),
              _ptr(ws), _ptr(out['loss']), _ptr(out['metrics']), _ptr(out['gate']), _ptr(out['auc']), _ptr(running), *shape,
              EC.WEIGHTS['ogm_weight'], EC.WEIGHTS['occ_weight'], EC.WEIGHTS['flow_origin_weight'], EC.REPLICA, loss_scale,
              EC.loss_flags(flags, no_warp), _stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_separate(shape, flags, no_warp=False, seed=0):
    """The launches the fused pass replaces, on the same inputs: stj_loss_auc_gate + stj_loss_fwd + stj_loss_finalize + stj_metrics."""
    from strajnet_amd import _lib
    c = dev_case(shape, seed)
    gt = [_ptr(c[k]) for k in EC.GT_KEYS]
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device='cuda')
    gate, gauc, ghist = z(8), z(8), z(8 * 202, torch.int32)
    if flags['use_gt']:
        _lib.call('stj_loss_auc_gate', *gt, _ptr(ghist), _ptr(gate), _ptr(gauc), *shape, _stream())
    else:
        gate.fill_(1.0)
    w = (EC.WEIGHTS['ogm_weight'], EC.WEIGHTS['occ_weight'], EC.WEIGHTS['flow_origin_weight'], EC.REPLICA, EC.loss_flags(flags) & 7)
    sums, loss, coef = z(128 * 40), z(5), z(32)                      # stj_loss_fwd fills 32 of the 128 copies stj_loss_finalize folds
    _lib.call('stj_loss_fwd', _ptr(c['logits']), *gt, _ptr(gate), _ptr(sums), _ptr(loss), _ptr(coef), *shape, *w, _stream())
    loss.zero_()
    _lib.call('stj_loss_finalize', _ptr(sums), _ptr(gate), _ptr(loss), _ptr(coef), *shape, *w, _stream())
    mauc, met, mhist, msums = z(24), z(7), z(8 * 3 * 202, torch.int32), z(8 * 11)
    _lib.call('stj_metrics', _ptr(c['logits']), *gt, _ptr(mhist), _ptr(msums), _ptr(mauc), _ptr(met), *shape, 1,
              0 if no_warp else 1, _stream())
    torch.cuda.synchronize()
    auc = np.concatenate([gauc.cpu().numpy().reshape(8, 1), mauc.cpu().numpy().reshape(8, 3)], 1)
    return dict(loss=loss.cpu().numpy(), metrics=met.cpu().numpy(), gate=gate.cpu().numpy(), auc=auc)


def check_against_float64(got, shape, flags, no_warp=False, seed=0):
    ref_l, gates = EC._ref_loss(tuple(shape), seed, EC.flag_key(flags))
    ref_m = EC.ref_metrics(tuple(shape), no_warp, seed)
    print(f'{shape} {flags} no_warp={no_warp}: loss {got["loss"][:4].tolist()} / {list(ref_l)}; metrics {got["metrics"].tolist()} / {list(ref_m)}')
    assert got['gate'].tolist() == list(gates)
    for k, v, r in zip(EC.LOSS_KEYS, got['loss'], ref_l):
        assert abs(float(v) - r) <= 3e-5 * abs(r) + 1e-6, (shape, flags, k, float(v), r)
    assert float(got['loss'][4]) == float(np.float32(np.float32(np.float32(got['loss'][0] + got['loss'][1]) + got['loss'][2]) + got['loss'][3]))
    for i, (v, r) in enumerate(zip(got['metrics'], ref_m)):
        assert abs(float(v) - r) <= 1e-4 * max(1.0, abs(r)), (shape, flags, i, float(v), r)


@pytest.mark.parametrize('flags', [EC.TRAIN, EC.DEFAULTS], ids=['train', 'defaults'])
@pytest.mark.parametrize('shape', EC.SHAPES)
def test_against_float64(shape, flags):
    check_against_float64(run_fused(shape, flags), shape, flags)


@pytest.mark.parametrize('flags', EC.EXTRA, ids=['use_pred', 'no_use_warp', 'no_use_gt'])
def test_against_float64_other_flags(flags):
    shape = EC.SHAPES[1]
    got = run_fused(shape, flags)
    check_against_float64(got, shape, flags)
    if flags['no_use_warp']:
        assert float(got['loss'][3]) == 0.0


def test_against_float64_no_warp_metric():
    shape = EC.SHAPES[2]
    got = run_fused(shape, EC.TRAIN, no_warp=True)
    check_against_float64(got, shape, EC.TRAIN, no_warp=True)
    assert got['metrics'][5] == 0.0 and got['metrics'][6] == 0.0 and (got['auc'][:, 3] == 0.0).all()


def _err(v, r):
    return abs(float(v) - r) / abs(r) if r != 0 else abs(float(v))


@pytest.mark.parametrize('flags', [EC.TRAIN, EC.DEFAULTS], ids=['train', 'defaults'])
@pytest.mark.parametrize('shape', EC.SHAPES)
def test_against_the_launches_it_replaces(shape, flags):
    """Same integer histograms, same bucket function, same interpolation: gate and AUCs are EQUAL; every float output is never further
    from float64 than the path it replaces (tests/test_ops_gpu.py: err <= max(2 err_replaced, 1e-6))."""
    fused, sep = run_fused(shape, flags), run_separate(shape, flags)
    assert np.array_equal(fused['gate'], sep['gate'])
    if not flags['use_gt']:
        assert (fused['auc'][:, 0] == 0.0).all()                  # no gate histogram without use_gt
        sep['auc'][:, 0] = 0.0
    assert np.array_equal(fused['auc'], sep['auc']), (fused['auc'], sep['auc'])
    ref_l, _ = EC.ref_loss(shape, flags)
    ref_m = EC.ref_metrics(tuple(shape))
    for name, ref in (('loss', ref_l), ('metrics', ref_m)):
        for i, r in enumerate(ref):
            ef, es = _err(fused[name][i], r), _err(sep[name][i], r)
            print(f'{shape} {name}[{i}]: err fused {ef:.3e} separate {es:.3e}')
            assert ef <= max(2.0 * es, 1e-6), (shape, flags, name, i, ef, es)


def test_bitwise_repeatable_whatever_the_workspace_held():
    shape, other = EC.SHAPES[2], EC.SHAPES[1]
    n, pad = ws_bytes(shape), 4096
    assert n >= ws_bytes(other) and n % 16 == 0
    buf = torch.full((n + pad,), 0xFF, dtype=torch.uint8, device='cuda')
    buf[n:] = 0xA5                                                        # canary behind the stated size
    first = run_fused(shape, EC.TRAIN, ws=buf)
    run_fused(other, EC.DEFAULTS, ws=buf)                               # leaves another case's histograms and partial sums behind
    second = run_fused(shape, EC.TRAIN, ws=buf)
    third = run_fused(shape, EC.TRAIN)                                  # and a workspace the allocator hands out
    for k in first:
        assert first[k].tobytes() == second[k].tobytes() == third[k].tobytes(), k
        assert not (first[k] == -7.0).any(), k                            # every output element was written
    assert bool((buf[n:] == 0xA5).all())
    assert bool((buf[:n] != 0xFF).any())


def test_running_means():
    from strajnet_amd import Mean, OGMFlowMetrics, OGMFlow_loss, OccupancyFlowTaskConfig, eval_step
    from strajnet_amd.evaluate import LOSS_KEYS
    shape, seeds = EC.SHAPES[1], (0, 1, 2)
    B, H, W = shape
    singles = [run_fused(shape, EC.TRAIN, seed=s) for s in seeds]
    assert len({s['loss'].tobytes() for s in singles}) == 3
    running = torch.zeros(12, dtype=torch.float64, device='cuda')
    for s in seeds:
        got = run_fused(shape, EC.TRAIN, seed=s, running=running, loss_scale=EC.REPLICA)
        assert got['loss'].tobytes() == singles[s]['loss'].tobytes()      # the running state changes nothing else
    r = running.cpu().numpy()
    want = np.concatenate([np.mean([s['loss'][:4].astype(np.float64) * EC.REPLICA for s in singles], 0),
                           np.mean([s['metrics'].astype(np.float64) for s in singles], 0)])
    assert r[0] == 3.0
    assert np.all(np.abs(r[1:] / r[0] - want) <= 1e-6 * np.abs(want)), (r[1:] / r[0], want)
    run_fused(shape, EC.TRAIN, running=None)                              # NULL: nothing is updated
    assert np.array_equal(running.cpu().numpy(), r)
    # the host-side classes, fed the same three batches through eval_step (the "model" hands back the case's logits)
    class Replay:
        def __call__(self, ogm, map_img, training=True, **kw):
            assert training is False and not torch.is_grad_enabled()
            return ogm
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(H, W, 8), replica=EC.REPLICA, **EC.WEIGHTS, **EC.TRAIN)
    means, om = [Mean(k) for k in LOSS_KEYS], OGMFlowMetrics('val')
    for s in seeds:
        c = dev_case(shape, s)
        batch = dict(ogm=c['logits'], map_img=None, obs=None, occ=None, flow=None, **{k: c[k] for k in EC.GT_KEYS})
        d, m = eval_step(Replay(), loss_fn, batch, loss_means=means, metrics=om)
        assert [float(d[k]) for k in LOSS_KEYS] == singles[s]['loss'][:4].tolist() and float(d.total) == float(singles[s]['loss'][4])
        assert m.values.cpu().numpy().tobytes() == singles[s]['metrics'].tobytes()
    got = np.array([float(x.result()) for x in means] + list(om.get_result().values()))
    assert list(om.get_result()) == ['val_observed_auc', 'val_occluded_auc', 'val_observed_iou', 'val_occluded_iou', 'val_flow_epe',
                                     'val_flow_ogm_auc', 'val_flow_ogm_iou']
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want)), (got, want)
    assert abs(float(om.flow_ogm_auc.result()) - want[9]) <= 1e-6 * want[9]
    for x in means:
        x.reset_states()
    om.reset_states()
    running.zero_()
    assert all(float(x.result()) == 0.0 for x in means) and all(v == 0.0 for v in om.get_result().values())
    assert float(means[0]._state[1]) == 0.0 and float(running[0]) == 0.0


def test_refusals():
    from strajnet_amd import _lib, ops
    L = _lib.lib()
    shape = EC.SHAPES[0]
    c = dev_case(shape)
    ws = torch.empty(ws_bytes(shape), dtype=torch.uint8, device='cuda')
    loss, met = torch.full((5,), -7.0, device='cuda'), torch.full((7,), -7.0, device='cuda')
    running = torch.full((12,), 3.0, dtype=torch.float64, device='cuda')
    odd = torch.zeros(c['logits'].numel() + 4, device='cuda')
    tail = (EC.WEIGHTS['ogm_weight'], EC.WEIGHTS['occ_weight'], EC.WEIGHTS['flow_origin_weight'], EC.REPLICA, 1.0, EC.loss_flags(EC.TRAIN), _stream())
    gt = [_ptr(c[k]) for k in EC.GT_KEYS]
    rc = L.stj_eval_fwd(_ptr(odd, 4), *gt, _ptr(ws), _ptr(loss), _ptr(met), vp(0), vp(0), _ptr(running), *shape, *tail)
    assert rc == _lib.ENUMS['stj_status']['STJ_EINVAL'] and b'16-byte aligned' in L.stj_last_error()
    with pytest.raises(_lib.StjError, match='unknown flag bits'):
        _lib.call('stj_eval_fwd', _ptr(c['logits']), *gt, _ptr(ws), _ptr(loss), _ptr(met), vp(0), vp(0), _ptr(running), *shape, *tail[:5], 32, _stream())
    # B = 0: STJ_OK, nothing launched or written, running untouched
    assert L.stj_eval_fwd(_ptr(c['logits']), *gt, _ptr(ws), _ptr(loss), _ptr(met), vp(0), vp(0), _ptr(running), 0, shape[1], shape[2], *tail) == 0
    assert ws_bytes((0, shape[1], shape[2])) > 0
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((met == -7.0).all()) and bool((running == 3.0).all())
    cpu = {k: v.cpu() for k, v in c.items()}
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.eval_loss_metrics(cpu['logits'], *(cpu[k] for k in EC.GT_KEYS), 1000.0, 1000.0, 1000.0, 1.0, 9)
    with pytest.raises(ValueError):
        ops.eval_loss_metrics(c['logits'][..., :16], *(c[k] for k in EC.GT_KEYS), 1000.0, 1000.0, 1000.0, 1.0, 9)


def test_captured_step_equals_the_eager_step_bitwise():
    """CFG128, B = 2, the model as tests/test_model_gpu.py builds it: a GraphedEvalStep replay equals evaluate.eval_step bit for bit in
    logits, losses and metrics (neither the eval forward nor the fused pass has a floating-point atomic), and two replays on two
    batches leave the means the eager steps give.  That the step captures at all shows it has no host sync."""
    from strajnet_amd import STrajNet, OGMFlow_loss, OccupancyFlowTaskConfig, Mean, OGMFlowMetrics, eval_step
    from strajnet_amd.evaluate import LOSS_KEYS, METRIC_KEYS
    from strajnet_amd.graph import GraphedEvalStep
    from oracle import np_ref
    w = np_ref.make_weights(CFG128, 0)
    x = np_ref.make_inputs(CFG128, 2)
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float32)
    model.load_weights(w)
    b1 = {k: torch.from_numpy(v.copy()).cuda() for k, v in x.items()}
    b2 = {k: torch.roll(v, 1, 0).contiguous() for k, v in b1.items()}
    b2['gt_flow'] = b2['gt_flow'] * 0.5
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=2.0, use_focal_loss=False, use_gt=True)
    means, om = [Mean(k) for k in LOSS_KEYS], OGMFlowMetrics('val')
    eager = []
    for b in (b1, b2):
        d, m = eval_step(model, loss_fn, b, loss_means=means, metrics=om)
        eager.append((d.logits.clone(), d.packed.clone(), m.values.clone()))
    assert not torch.equal(eager[0][1], eager[1][1])
    step = GraphedEvalStep(model, loss_fn, b1)
    assert step.result() == dict.fromkeys(LOSS_KEYS + METRIC_KEYS, 0.0)       # the warm-up steps are in no mean
    for b, (lg, ls, mt) in zip((b1, b2), eager):
        losses, metrics = step(b)
        assert torch.equal(step.logits, lg) and torch.equal(losses, ls) and torch.equal(metrics, mt)
    res = step.result()
    want = dict(zip(LOSS_KEYS, (float(v.result()) for v in means)))
    want.update({k[len('val_'):]: v for k, v in om.get_result().items()})
    assert list(res) == list(want)
    for k in want:
        assert abs(res[k] - want[k]) <= 1e-12 * abs(want[k]), (k, res[k], want[k])
    assert float(step.running[0]) == 2.0
    step.reset()
    assert step.result() == dict.fromkeys(LOSS_KEYS + METRIC_KEYS, 0.0)
    del step
