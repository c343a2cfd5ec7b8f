"""GPU side of the challenge-format output: stj_quantize_waypoints against the reference's NumPy lines (flow: exact) and float64
(occupancy: off by one only at a rounding tie), the quantising epilogue of the inference heads' gather against the two-kernel form (every
byte), STrajNet.predict_quantized, GraphedForward(quantized=True), ResultDrain, and the metrics on a dequantised prediction."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


def _seeded_output(shape, scale, seed):
    """Normal logits of `scale` on the occupancy channels, flow of scale 60 (so that a share lies beyond +-128), with planted flow ties,
    values beyond the int8 range and negative zero, and planted occupancy logits 0 and +-40."""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(shape) * scale).astype(np.float32)
    y[..., 2::4] = (rng.standard_normal(y[..., 2::4].shape) * 60).astype(np.float32)
    y[..., 3::4] = (rng.standard_normal(y[..., 3::4].shape) * 60).astype(np.float32)
    flat = y.reshape(-1, 32)
    plant = np.array([0.5, 1.5, -0.5, 2.5, -1.5, 127.5, -128.5, 126.5, -127.5, 300.0, -300.0, -0.0, 0.0, 127.49, -128.49, 1e6, -1e6], np.float32)
    rows = rng.choice(flat.shape[0], 64 * len(plant), replace=False).reshape(64, len(plant))
    for r in rows:
        ch = rng.integers(0, 8, len(plant)) * 4 + rng.integers(2, 4, len(plant))
        flat[r, ch] = plant
    occ_plant = np.array([0.0, 40.0, -40.0, 100.0, -100.0, -0.0], np.float32)
    rows = rng.choice(flat.shape[0], 16 * len(occ_plant), replace=False).reshape(16, len(occ_plant))
    for r in rows:
        flat[r, rng.integers(0, 8, len(occ_plant)) * 4 + rng.integers(0, 2, len(occ_plant))] = occ_plant
    return y


def _occupancy_rule(q, x, tie_halfwidth=1e-4, share=1e-4, what=''):
    """q uint8 against rint(255 * sigmoid64(x)): every difference is exactly 1, occurs only within `tie_halfwidth` of a rounding tie, and
    at most `share` of the bytes differ.  Prints the figures before it asserts."""
    v = 255.0 / (1.0 + np.exp(-x.astype(np.float64)))
    d = q.astype(np.int64) - np.rint(v).astype(np.int64)
    bad = d != 0
    dist = np.abs(v - np.floor(v) - 0.5)
    print(f'{what}: {int(bad.sum())} of {bad.size} bytes differ from float64 ({bad.mean():.2e}), max |diff| {int(np.abs(d).max())}, '
          f'farthest from a tie {float(dist[bad].max()) if bad.any() else 0.0:.2e}')
    assert np.abs(d).max() <= 1
    assert not bad.any() or float(dist[bad].max()) < tie_halfwidth
    assert bad.mean() <= share


@pytest.mark.parametrize('shape', [(2, 128, 128, 32), (8, 256, 256, 32)])
@pytest.mark.parametrize('scale', [1.0, 4.0, 8.0])
def test_quantize_kernel_flow_exact_occupancy_vs_float64(shape, scale):
    """Flow: byte for byte the reference's np.clip(np.round(x), -128, 127).astype(int8), no tolerance.  Occupancy against float64: a byte
    may be off by one only where 255 * sigmoid64(x) is within 1e-4 of a tie (255 x 3 ulp of float32 at 1.0 = 9.1e-5, rounded up), and in at
    most 1e-4 of the bytes (a float32 NumPy restatement alone differs in 3.3e-6 to 6.7e-6 of them)."""
    from strajnet_amd import quantize_waypoints, quantize_reference
    y = _seeded_output(shape, scale, seed=int(scale) * 100 + shape[0])
    qw = quantize_waypoints(torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    B, H, W, _ = shape
    assert qw.buf.shape == (B, 32 * H * W) and qw.buf.dtype == torch.uint8
    robs, rocc, rflow = quantize_reference(y)
    assert np.array_equal(qw.flow.cpu().numpy(), rflow)
    obs, occ = qw.observed.cpu().numpy(), qw.occluded.cpu().numpy()
    yk = y.reshape(B, H, W, 8, 4).transpose(0, 3, 1, 2, 4)                          # [B,Tn,H,W,4]
    _occupancy_rule(np.stack([obs, occ], -1), yk[..., :2], what=f'quantize kernel {shape} scale {scale}')
    # and the layout: the raw bytes of (scene, waypoint) are the reference's
    host = qw.cpu()
    for b, k in ((0, 0), (B - 1, 7), (B // 2, 3)):
        raw = host.waypoint_bytes(b, k)
        assert raw[2] == rflow[b, k].tobytes() and len(raw[0]) == H * W
        assert raw[0] == obs[b, k].tobytes() and raw[1] == occ[b, k].tobytes()


def test_quantize_kernel_nan_and_unsupported_shapes():
    from strajnet_amd import quantize_waypoints
    from strajnet_amd._lib import StjError
    y = torch.zeros((1, 16, 16, 32), device='cuda')
    y[0, 3, 5, :] = float('nan')
    y[0, 4, 5, 2], y[0, 4, 5, 3], y[0, 4, 5, 0] = float('inf'), float('-inf'), float('inf')
    qw = quantize_waypoints(y)
    assert int(qw.observed[0, :, 3, 5].max()) == 0 and int(qw.occluded[0, :, 3, 5].max()) == 0 and int(qw.flow[0, :, 3, 5].abs().max()) == 0
    assert qw.flow[0, 0, 4, 5].tolist() == [127, -128] and int(qw.observed[0, 0, 4, 5]) == 255
    assert int(qw.observed[0, 0, 0, 0]) == 128
    with pytest.raises(StjError):
        quantize_waypoints(torch.zeros((1, 8, 8, 32), device='cuda'))              # H * W not a multiple of the kernel's run of 256 cells


@pytest.mark.parametrize('dt', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('geom', [(2, 128), (8, 256)])
@pytest.mark.parametrize('t_major', [0, 1])
def test_fused_gather_equals_gather_then_quantize(dt, geom, t_major):
    """stj_outconv_pair_gather_q == stj_quantize_waypoints(stj_outconv_pair_gather(...)), every byte: same kernel body, same summation
    order, the same two per-value rules."""
    from strajnet_amd._lib import call
    from strajnet_amd.ops import _p, _st, _dt, HEAD_CZ
    B, H = geom
    g = torch.Generator(device='cuda').manual_seed(17 + B + t_major)
    zs = []
    for i in range(2):
        # per-tap terms whose 9-neighbour sums have logit scale ~3 (occupancy branch) / flow scale ~45 (flow branch)
        z = torch.randn((8 * B, H, H, HEAD_CZ), generator=g, device='cuda') * (1.0 if i == 0 else 15.0)
        z[..., 18:] = 0
        zs.append(z.to(dt))
    b0 = torch.tensor([0.25, -0.5], device='cuda')
    b1 = torch.tensor([0.5, 1.5], device='cuda')                                    # the flow sums land on .0 / .5 often: 16-bit terms
    out = torch.empty((B, H, H, 32), dtype=torch.float32, device='cuda')
    q2 = torch.empty((B, 32 * H * H), dtype=torch.uint8, device='cuda')
    q1 = torch.empty_like(q2)
    call('stj_outconv_pair_gather', _p(zs[0]), _p(zs[1]), _p(b0), _p(b1), _p(out), B, 8, H, H, t_major, _dt(zs[0]), _st())
    call('stj_quantize_waypoints', _p(out), _p(q2), B, 8, H, H, _st())
    call('stj_outconv_pair_gather_q', _p(zs[0]), _p(zs[1]), _p(b0), _p(b1), _p(q1), B, 8, H, H, t_major, _dt(zs[0]), _st())
    torch.cuda.synchronize()
    assert torch.equal(q1, q2)
    n = 8 * H * H
    assert int(q1[:, :n].max()) > 200 and int(q1[:, :n].min()) < 50 and q1[:, 2 * n:].view(torch.int8).float().std() > 10      # not a trivial image


def _setup(dtype, B=2, seed=0):
    from strajnet_amd import STrajNet
    from oracle import np_ref
    w = np_ref.make_weights(CFG128, seed)
    x = np_ref.make_inputs(CFG128, B)
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=dtype)
    model.load_weights(w)
    xt = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
    return model, w, x, xt


def _args(xt):
    return (xt['ogm'], xt['map_img']), dict(obs=xt['obs'], occ=xt['occ'], mapt=None, flow=xt['flow'])


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_predict_quantized_equals_quantized_forward(dtype):
    """model.predict_quantized == quantize_waypoints(model(..., training=False)) exactly: fp16 takes the quantising gather (the float
    forward is taken under no_grad, where it runs the same inference heads), f32 the standalone kernel.  In f32 also against
    quantize_reference of the oracle's forward: the model's logits are gated at 1e-3 against the oracle, so a byte may differ by 1 where the
    oracle's 255 * sigmoid is within 255 * 0.25 * 1e-3 = 0.064 of a tie, flow where the oracle's value is within 1e-3 of a tie."""
    from strajnet_amd import quantize_waypoints, quantize_reference, QuantizedWaypoints
    from strajnet_amd import prof as kprof
    model, w, x, xt = _setup(dtype)
    a, kw = _args(xt)
    with torch.no_grad():
        out = model(*a, training=False, **kw)
    ref = quantize_waypoints(out)
    kprof.enable()
    got = model.predict_quantized(*a, **kw)
    torch.cuda.synchronize()
    names = ' '.join(kprof.disable())                # the recorded calls' keys: 'outconv_pair_gather_q[...]', 'quantize_waypoints[...]', ...
    assert isinstance(got, QuantizedWaypoints) and got.buf.shape == (2, 32 * 128 * 128)
    assert torch.equal(got.buf, ref.buf)
    if dtype == torch.float16:
        assert 'outconv_pair_gather_q[' in names and 'quantize_waypoints[' not in names
    else:
        assert 'quantize_waypoints[' in names and 'outconv_pair_gather_q[' not in names
    assert not model._quantize_heads
    if dtype == torch.float32:
        from oracle import np_ref
        o = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow']).astype(np.float64)
        ok = o.reshape(2, 128, 128, 8, 4).transpose(0, 3, 1, 2, 4)
        q = np.stack([got.observed.cpu().numpy(), got.occluded.cpu().numpy()], -1)
        _occupancy_rule(q, ok[..., :2], tie_halfwidth=0.064 + 1e-4, share=1.0, what='predict_quantized f32 vs oracle')
        fl = ok[..., 2:]
        rf = np.clip(np.rint(fl), -128, 127)
        d = got.flow.cpu().numpy().astype(np.int64) - rf.astype(np.int64)
        near = np.abs(fl - np.floor(fl) - 0.5) < 1e-3
        print(f'predict_quantized f32 flow vs oracle: {int((d != 0).sum())} of {d.size} bytes differ, {int(near.sum())} values within 1e-3 of a tie')
        assert np.abs(d).max() <= 1 and not (d != 0)[~near].any()


def test_graphed_forward_quantized_and_result_drain():
    """GraphedForward(quantized=True), with and without pipeline_agents, over three different batches == eager predict_quantized; without
    the flag the float32 tensor as before.  ResultDrain over five replays of alternating batches delivers each batch's bytes in order and
    untorn (against synchronous copies of a second run of the same batches)."""
    from strajnet_amd import QuantizedWaypoints, ResultDrain
    from strajnet_amd.graph import GraphedForward
    from oracle import np_ref
    model, w, x, xt = _setup(torch.float16)
    keys = ('ogm', 'map_img', 'obs', 'occ', 'flow')
    batches = [{k: xt[k] for k in keys}]
    for s in (77, 99):
        xs = np_ref.make_inputs(CFG128, 2, seed=s)
        batches.append({k: torch.as_tensor(xs[k]).cuda() for k in keys})
    exp = [model.predict_quantized(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow']).buf.clone() for b in batches]
    assert not torch.equal(exp[0], exp[1]) and not torch.equal(exp[1], exp[2])
    with torch.no_grad():
        f0 = model(batches[0]['ogm'], batches[0]['map_img'], training=False, obs=batches[0]['obs'], occ=batches[0]['occ'], flow=batches[0]['flow']).clone()
    plain = GraphedForward(model, batches[0])
    o = plain()
    assert isinstance(o, torch.Tensor) and o.dtype == torch.float32 and torch.equal(o, f0)
    del plain
    for pipe in (False, True):
        gf = GraphedForward(model, batches[0], pipeline_agents=pipe, quantized=True)
        assert isinstance(gf.out, QuantizedWaypoints)
        for i in (1, 0, 2, 1):
            o = gf(batches[i])
            assert o is gf.out and torch.equal(o.buf, exp[i]), (pipe, i)
        if pipe:
            gf.prefetch_agents(batches[2])
            assert torch.equal(gf(batches[2]).buf, exp[2])
        # ResultDrain: five replays of alternating batches
        order = [0, 1, 0, 2, 1]
        drain = ResultDrain(gf.out, depth=2)
        got = []
        try:
            for n, i in enumerate(order):
                gf(batches[i])
                drain.submit()
                if n >= 1:                                   # one batch in flight behind the replay
                    got.append(drain.take().buf.clone())
            got.append(drain.take().buf.clone())
            with pytest.raises(RuntimeError):
                drain.take()
        finally:
            drain.close()
        sync = [gf(batches[i]).buf.cpu() for i in order]    # the second run: synchronous copies
        assert len(got) == 5
        for n, (a, b) in enumerate(zip(got, sync)):
            assert torch.equal(a, b), (pipe, n)
            assert torch.equal(a, exp[order[n]].cpu())
        del gf, drain
    import gc
    gc.collect()
    torch.cuda.synchronize()


def test_metrics_on_dequantized_prediction():
    """compute_occupancy_flow_metrics on dequantize() of a quantised prediction: all seven fields finite, and the flow end-point error
    within 0.71 of the float prediction's (each flow component moves by at most 0.5, the error vector by at most sqrt(0.5); the triangle
    inequality carries that to the mean)."""
    from strajnet_amd import (OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt, compute_occupancy_flow_metrics,
                              apply_sigmoid_to_occupancy_logits, quantize_waypoints)
    from strajnet_amd.metrics import FIELDS
    model, w, x, xt = _setup(torch.float32)
    a, kw = _args(xt)
    with torch.no_grad():
        out = model(*a, training=False, **kw)
    cfg = OccupancyFlowTaskConfig(128, 128, 8)
    true_wp = warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow'])
    m_f = compute_occupancy_flow_metrics(cfg, true_wp, apply_sigmoid_to_occupancy_logits(get_pred_waypoint_logits(out)))
    m_q = compute_occupancy_flow_metrics(cfg, true_wp, quantize_waypoints(out).dequantize())
    vf, vq = [getattr(m_f, n) for n in FIELDS], [getattr(m_q, n) for n in FIELDS]
    print('metrics float / dequantised: ' + ', '.join(f'{n} {p:.6f} / {q:.6f}' for n, p, q in zip(FIELDS, vf, vq)))
    assert len(FIELDS) == 7 and all(np.isfinite(v) for v in vq)
    assert abs(m_q.vehicles_flow_epe - m_f.vehicles_flow_epe) <= 0.71
