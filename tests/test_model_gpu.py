"""End-to-end parity of the HIP path (STrajNet(...) call + OGMFlow_loss) against the CPU oracle.

Gate (BASELINE.json north_star): outputs match the reference within 1e-3 abs in the f32-storage parity mode.
The oracle is the in-repo restatement (PARITY UNPINNED by the reference itself: TensorFlow cannot run here).
Reduced geometry 128x128 (the oracle finishes in seconds); cfg-256 is covered by the committed golden fixture.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _report(msg):
    print(msg)
    try:
        os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
        with open(os.path.join(ROOT, 'gpurun_out', 'parity_report.txt'), 'a') as f:
            f.write(msg + '\n')
    except OSError:
        pass


CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
ABS_TOL_F32 = 1e-3          # north_star tolerance


def _setup(cfg, B, dtype, large_ogm=False, fg_msa=True, fg=True, seed=0):
    from strajnet_amd import STrajNet
    from oracle import np_ref
    w = np_ref.make_weights(cfg, seed, fg_msa=fg_msa, fg=fg, large_ogm=large_ogm)
    x = np_ref.make_inputs(cfg, B, large_ogm=large_ogm)
    model = STrajNet(cfg, fg_msa=fg_msa, fg=fg, large_ogm=large_ogm, dtype=dtype)
    model.load_weights(w)
    xt = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
    return model, w, x, xt


def _fwd(model, xt):
    return model(xt['ogm'], xt['map_img'], training=False, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])


def _auc_delta(y, ref, x):
    """occ-AUC parity (BASELINE metric): max over the 8 waypoints and both occupancy heads of
    |PR-AUC(gt, sigmoid(kernel logits)) - PR-AUC(gt, sigmoid(oracle logits))| with the Keras AUC(PR, 100 thresholds)."""
    from oracle import np_ref
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    worst = 0.0
    for t in range(8):
        for ch, gt in ((0, x['gt_obs']), (1, x['gt_occ'])):
            g = gt[:, t, :, :, 0]
            worst = max(worst, abs(np_ref.keras_auc_pr(g, sig(y[..., 4 * t + ch])) - np_ref.keras_auc_pr(g, sig(ref[..., 4 * t + ch]))))
    return worst


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


@pytest.mark.parametrize('fg_msa,fg', [(True, True), (False, False)])
def test_forward_parity_f32(fg_msa, fg):
    from oracle import np_ref
    model, w, x, xt = _setup(CFG128, 2, torch.float32, fg_msa=fg_msa, fg=fg)
    with torch.no_grad():
        y = _fwd(model, xt).cpu().numpy()
    ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'], fg_msa=fg_msa, fg=fg)
    err = np.abs(y - ref).max()
    dauc = _auc_delta(y, ref, x)
    _report(f'fwd f32 (fg_msa={fg_msa}, fg={fg}) 128x128 B=2: max-abs err {err:.3e} (ref scale {np.abs(ref).max():.2f}), |dPR-AUC| {dauc:.2e}')
    assert y.shape == ref.shape == (2, 128, 128, 32)
    assert err < ABS_TOL_F32
    assert dauc < 1e-5


def test_forward_parity_large_ogm_f32():
    """cfg-512 plumbing (map pad + skip centre-crops, modules.py:582-587,614-622) at the reduced 256 -> 128 geometry."""
    from oracle import np_ref
    cfg = dict(CFG128, input_size=(256, 256))
    model, w, x, xt = _setup(cfg, 1, torch.float32, large_ogm=True)
    with torch.no_grad():
        y = _fwd(model, xt).cpu().numpy()
    ref = np_ref.strajnet_forward(w, cfg, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'], large_ogm=True)
    err = np.abs(y - ref).max()
    _report(f'fwd f32 large_ogm 256->128 B=1: max-abs err {err:.3e}')
    assert err < ABS_TOL_F32


def test_train_step_parity_f32():
    """Loss dict + gradients of every trainable tensor vs torch autograd on the float64 restatement."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from oracle import torch_ref
    model, w, x, xt = _setup(CFG128, 2, torch.float32)
    model.zero_grad()
    out = _fwd(model, xt)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    total = sum(d.values())
    # two stages, because the flow-warp loss is only piecewise smooth in the predicted flow (bilinear sampling: floor() of the
    # warped position, occu_metric.py:345-409): where an f32 forward lands on the other side of an integer boundary than the
    # float64 one, that pixel's output gradient differs by O(1) of its size, and every flow-decoder weight gradient (a sum over
    # all pixels) inherits ~1e-3 of it.  Stage 1 checks the output gradient element-wise and tolerates a handful of such isolated
    # flips; stage 2 back-propagates the REFERENCE's output gradient through the HIP model, so every weight gradient is compared
    # on identical inputs and the tolerance can be tight.
    (g_out,) = torch.autograd.grad(total, out)
    pr = torch_ref.to_torch(w, torch.float64, requires_grad=True)
    xr = torch_ref.to_torch(x, torch.float64)
    yr = torch_ref.forward(pr, CFG128, xr['ogm'], xr['map_img'], xr['obs'], xr['occ'], xr['flow'])
    yr.retain_grad()
    dr = torch_ref.loss(yr, xr['gt_obs'], xr['gt_occ'], xr['gt_flow'], xr['origin_flow'], replica=1.0, use_gt=True)
    sum(dr.values()).backward()
    for k in dr:
        assert abs(float(d[k]) - float(dr[k])) < 1e-4 * abs(float(dr[k])) + 1e-5, (k, float(d[k]), float(dr[k]))
    dg = (g_out.double().cpu() - yr.grad).abs()
    gscale = float(yr.grad.abs().max())
    flips = int((dg > 1e-4 * gscale).sum())
    smooth = float(dg[dg <= 1e-4 * gscale].max()) / gscale
    assert flips <= 8, f'{flips} output-gradient elements differ from the float64 reference by more than 1e-4 of the largest'
    assert smooth < 1e-4
    out.backward(yr.grad.to(torch.float32).to(out.device))
    bad = []
    worst = 0.0
    gmax = max(float(pr[n].grad.abs().max()) for n in model.params)
    for n, p in model.params.items():
        g, gr = p.grad.double().cpu(), pr[n].grad
        scale = float(gr.abs().max())
        # tensors whose true gradient is identically zero (e.g. a key bias under softmax) only carry f32 noise:
        # floor the scale at 1e-6 of the largest gradient in the model
        e = float((g - gr).abs().max()) / (scale + 1e-6 * gmax)
        worst = max(worst, e)
        if e > 1e-3:
            bad.append((n, e, scale))
    _report(f'train step f32 128x128 B=2: losses ' + ', '.join(f'{k}={float(d[k]):.6f}' for k in d) +
            f'; output gradient: {flips} sampling-boundary flips, otherwise {smooth:.1e} of max; worst relative grad error '
            f'{worst:.3e} over {len(model.params)} tensors (reference output gradient back-propagated)')
    assert not bad, bad[:10]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_fused_stem_matches_layerwise_whole_model(dtype):
    """model.fused_stem (PatchEmbed + stem sums / norms as one launch per raster, csrc/patch_embed.hip) against the im2col + dense +
    LayerNorm launches it replaces, through the WHOLE model: logits, and the gradients of every stem parameter for one output gradient."""
    model, w, x, xt = _setup(CFG128, 2, dtype)
    g = torch.randn(2, 128, 128, 32, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    res = {}
    for fused in (True, False):
        model.fused_stem = fused
        model.zero_grad()
        out = _fwd(model, xt)
        out.backward(g)
        torch.cuda.synchronize()
        res[fused] = (out.detach().float().clone(), {n: p.grad.detach().clone() for n, p in model.params.items()
                                                      if n.startswith(('patch_embed', 'flow_norm', 'all_patch_norm'))})
    y1, g1 = res[True]
    y0, g0 = res[False]
    assert len(g1) == 16            # 3 x (kernel, bias, gamma, beta) + 2 x (gamma, beta)
    scale = float(y0.abs().max())
    err = float((y1 - y0).abs().max()) / scale
    worst = max(float((g1[n] - g0[n]).norm() / (g0[n].norm() + 1e-30)) for n in g1)
    _report(f'fused stem vs layer-by-layer stem ({dtype}): logits max-abs / scale {err:.2e}, worst stem parameter gradient rel-norm {worst:.2e}')
    # f32: same arithmetic up to the f32 summation order of one K <= 176 product; bf16: the bf16 roundings are in the same places, but a
    # flipped rounding of one token propagates through the network like any bf16 rounding
    assert err < (2e-5 if dtype == torch.float32 else 2e-2)
    assert worst < (2e-4 if dtype == torch.float32 else 5e-2)


def _oracle_masks(model, B):
    from oracle.masks import masks_from_model
    return masks_from_model(model, B)


def test_train_step_parity_training_true_f32():
    """training=True: DropPath + attention / FFN dropout drawn inside the HIP kernels; the oracle is fed the exported keep
    masks (the reference's own TF random stream cannot be reproduced).  Logits, losses and all gradients must match."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from oracle import np_ref, torch_ref
    B = 2
    model, w, x, xt = _setup(CFG128, B, torch.float32)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    model.zero_grad()
    out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    sum(d.values()).backward()
    masks = _oracle_masks(model, B)
    want = np_ref.dropout_sites(CFG128, B)
    assert set(masks) == set(want)
    for k, (shape, rate) in want.items():
        assert masks[k].shape == shape, (k, masks[k].shape, shape)
    big = np.concatenate([masks[f'cross_attn_obs{i}/dropout1'].ravel() for i in range(8)])
    assert abs(big.mean() - 0.9) < 0.01                                 # keep probability 1 - rate
    ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'], masks=masks)
    err = np.abs(out.detach().cpu().numpy() - ref).max()
    ref_eval = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'])
    assert np.abs(ref - ref_eval).max() > 1e-2                          # the masks do change the result
    assert err < ABS_TOL_F32
    pr = torch_ref.to_torch(w, torch.float64, requires_grad=True)
    xr = torch_ref.to_torch(x, torch.float64)
    yr = torch_ref.forward(pr, CFG128, xr['ogm'], xr['map_img'], xr['obs'], xr['occ'], xr['flow'], masks=masks)
    dr = torch_ref.loss(yr, xr['gt_obs'], xr['gt_occ'], xr['gt_flow'], xr['origin_flow'], replica=1.0, use_gt=True)
    sum(dr.values()).backward()
    gmax = max(float(pr[n].grad.abs().max()) for n in model.params)
    worst, bad = 0.0, []
    for n, p in model.params.items():
        g, gr = p.grad.double().cpu(), pr[n].grad
        e = float((g - gr).abs().max()) / (float(gr.abs().max()) + 1e-6 * gmax)
        worst = max(worst, e)
        if e > 2e-3:
            bad.append((n, e))
    _report(f'train step f32 training=True (exported masks) 128x128 B=2: fwd max-abs err {err:.3e}; worst relative grad error {worst:.3e}')
    assert not bad, bad[:10]
    # a second step draws different masks; the same step re-derives identical ones
    m1 = model.dropctx.mask('cross_attn_obs/dropout1').clone()
    assert torch.equal(m1, model.dropctx.mask('cross_attn_obs/dropout1'))
    with torch.no_grad():
        model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
    assert not torch.equal(m1, model.dropctx.mask('cross_attn_obs/dropout1'))


def test_graph_replay_matches_eager_and_redraws_masks():
    """hipGraph replay of the whole train step: same losses / gradients as the eager step (training=False, deterministic graph);
    with training=True every replay advances the device RNG counter and draws new masks."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from strajnet_amd.graph import GraphedTrainStep
    model, w, x, xt = _setup(CFG128, 2, torch.float32)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    model.zero_grad()
    out = _fwd(model, xt)
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    sum(d.values()).backward()
    g_eager = model.flat_grads().clone()
    l_eager = torch.stack([d[k].detach() for k in ('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')])
    step = GraphedTrainStep(model, loss_fn, xt, training=False)
    for _ in range(2):
        losses = step()
    torch.cuda.synchronize()
    assert torch.allclose(losses, l_eager, rtol=1e-5, atol=1e-6)
    denom = float(g_eager.abs().max())
    assert float((model.flat_grads() - g_eager).abs().max()) < 1e-4 * denom       # f32 atomics: order differs, values do not
    step_t = GraphedTrainStep(model, loss_fn, xt, training=True)
    c0 = int(model.dropctx.state[1])
    l1 = step_t().clone()
    l2 = step_t().clone()
    torch.cuda.synchronize()
    assert int(model.dropctx.state[1]) == c0 + 2
    assert not torch.equal(l1, l2)
    assert torch.isfinite(l1).all() and torch.isfinite(l2).all()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_config4_inference_graph_b32(dtype):
    """BASELINE config 4: inference-only batch 32 on one GPU, hipGraph-captured forward, fp16 MFMA path (v_mfma_f32_16x16x32_f16;
    bf16 runs the same test).  The replay must reproduce the eager forward bit for bit (the forward has no atomics) and follow
    new inputs."""
    from strajnet_amd.graph import GraphedForward
    from oracle import np_ref
    cfg = dict(CFG128, input_size=(256, 256))
    model, w, x, xt = _setup(cfg, 1, dtype)
    xs = np_ref.make_inputs(cfg, 4, seed=77)
    big = {k: torch.as_tensor(np.concatenate([v] * 8, 0)).cuda() for k, v in xs.items()}          # B = 32
    with torch.no_grad():
        eager = model(big['ogm'], big['map_img'], training=False, obs=big['obs'], occ=big['occ'], mapt=None, flow=big['flow']).clone()
    gf = GraphedForward(model, big)
    out = gf().clone()
    assert out.shape == (32, 256, 256, 32) and torch.isfinite(out).all()
    assert torch.equal(out, eager)
    assert torch.equal(out[:4], out[4:8])                        # replicated scenes -> identical rows (batch independence)
    big2 = {k: torch.roll(v, 1, 0) for k, v in big.items()}
    out2 = gf(big2)
    assert torch.equal(out2, torch.roll(eager, 1, 0))
    # the agent branch out of the graph, a batch ahead (GraphedForward(pipeline_agents=True)): same bits, with and without a prefetch,
    # over a sequence of different batches
    gp = GraphedForward(model, big, pipeline_agents=True)
    assert torch.equal(gp().clone(), eager)                     # no prefetch: the agent branch runs in front
    seq = [big2, big, {k: torch.roll(v, 3, 0) for k, v in big.items()}, big2]
    exp = [torch.roll(eager, 1, 0), eager, torch.roll(eager, 3, 0), torch.roll(eager, 1, 0)]
    gp.prefetch_agents(seq[0])
    for i, (bt, ex) in enumerate(zip(seq, exp)):
        o = gp(bt)
        if i + 1 < len(seq):
            gp.prefetch_agents(seq[i + 1])                      # overlaps this batch's main graph
        assert torch.equal(o.clone(), ex), i
    # the staged form: the next batch's tracks are copied in front of this replay, the branch runs under it (`next_batch=`); fresh
    # device tensors produced on the current stream right before the call (the case a stream-ordered upload makes)
    for i, (bt, ex) in enumerate(zip(seq, exp)):
        nxt = {k: v.clone() for k, v in seq[i + 1].items()} if i + 1 < len(seq) else None
        o = gp(bt, next_batch=nxt)
        assert torch.equal(o.clone(), ex), i
    # weights changed between a prefetch and the call: the stale encoding is dropped
    gp.prefetch_agents(big)
    w2 = {k: (v * 1.01 if k.startswith('traj_net/') else v) for k, v in w.items()}
    model.load_weights(w2)
    o_new = gp(big).clone()
    with torch.no_grad():
        e_new = model(big['ogm'], big['map_img'], training=False, obs=big['obs'], occ=big['occ'], mapt=None, flow=big['flow'])
    assert torch.equal(o_new, e_new) and not torch.equal(o_new, eager)
    model.load_weights(w)
    assert model.agent_override is None
    del gp, gf
    import gc
    gc.collect()
    torch.cuda.synchronize()


def test_config5_cfg512_deeper_stage_f32():
    """BASELINE config 5: 512x512 grid (large_ogm=True: 256^2 map, skips centre-cropped), window 8, deeper last Swin stage
    depths=[2,2,6], B=1, against the differentiable restatement in float64 at FULL size."""
    from oracle import np_ref, torch_ref
    cfg = dict(input_size=(512, 512), window_size=8, embed_dim=96, depths=[2, 2, 6], num_heads=[3, 6, 12])
    model, w, x, xt = _setup(cfg, 1, torch.float32, large_ogm=True)
    assert model.n_params == 20386444                          # 13 277 788 + 4 more 32x32x384 blocks
    with torch.no_grad():
        y = _fwd(model, xt)
        p, xr = torch_ref.to_torch(w), torch_ref.to_torch(x)
        ref = torch_ref.forward(p, cfg, xr['ogm'], xr['map_img'], xr['obs'], xr['occ'], xr['flow'], large_ogm=True)
    assert tuple(y.shape) == tuple(ref.shape) == (1, 256, 256, 32)
    err = float((y.double().cpu() - ref).abs().max())
    _report(f'fwd f32 cfg-512 depths [2,2,6] large_ogm B=1 (full size, vs torch_ref f64): max-abs err {err:.3e} (ref scale {float(ref.abs().max()):.2f}), {model.n_params} parameters')
    assert err < ABS_TOL_F32


def test_device_metrics_match_oracle():
    """compute_occupancy_flow_metrics (occu_metric.py:26-140) on device vs the oracle restatement, on the model's
    own output and the synthetic ground truth; packed fast path, hand-built WaypointGrids, probabilities and no_warp."""
    from strajnet_amd import (OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt, compute_occupancy_flow_metrics,
                              apply_sigmoid_to_occupancy_logits)
    from strajnet_amd.loss import WaypointGrids
    from oracle import np_ref
    model, w, x, xt = _setup(CFG128, 2, torch.float32)
    with torch.no_grad():
        out = _fwd(model, xt)
    cfg = OccupancyFlowTaskConfig(128, 128, 8)
    true_wp = warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow'])
    pred_wp = apply_sigmoid_to_occupancy_logits(get_pred_waypoint_logits(out))
    m = compute_occupancy_flow_metrics(cfg, true_wp, pred_wp)
    ref = np_ref.occupancy_flow_metrics(out.cpu().numpy(), x['gt_obs'], x['gt_occ'], x['gt_flow'], x['origin_flow'])
    got = [m.vehicles_observed_auc, m.vehicles_occluded_auc, m.vehicles_observed_iou, m.vehicles_occluded_iou, m.vehicles_flow_epe,
           m.vehicles_flow_warped_occupancy_auc, m.vehicles_flow_warped_occupancy_iou]
    _report('device metrics 128x128 B=2: ' + ', '.join(f'{a:.6f}/{b:.6f}' for a, b in zip(got, ref)) + ' (device/oracle)')
    for a, b in zip(got, ref):
        assert abs(a - b) < 1e-4 * max(1.0, abs(b)), (got, ref)
    # hand-built grids of probabilities (no packed tensors): same numbers
    hand = WaypointGrids()
    hand.vehicles.observed_occupancy = [t.clone() for t in pred_wp.vehicles.observed_occupancy]
    hand.vehicles.occluded_occupancy = [t.clone() for t in pred_wp.vehicles.occluded_occupancy]
    hand.vehicles.flow = [t.clone() for t in pred_wp.vehicles.flow]
    th = WaypointGrids()
    th.vehicles.observed_occupancy = [xt['gt_obs'][:, k] for k in range(8)]
    th.vehicles.occluded_occupancy = [xt['gt_occ'][:, k] for k in range(8)]
    th.vehicles.flow = [xt['gt_flow'][:, k] for k in range(8)]
    th.vehicles.flow_origin_occupancy = [xt['origin_flow'][:, k] for k in range(8)]
    m2 = compute_occupancy_flow_metrics(cfg, th, hand)
    assert torch.allclose(m2.values, m.values, atol=2e-6)
    m3 = compute_occupancy_flow_metrics(cfg, true_wp, pred_wp, no_warp=True)
    assert m3.vehicles_flow_warped_occupancy_auc == 0.0 and abs(m3.vehicles_flow_epe - m.vehicles_flow_epe) < 1e-5      # f32 atomics: summation order varies


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_train_loop_nadam_reduces_loss(dtype):
    """The pieces of train.py:199-249 together: model(training=True) -> OGMFlow_loss -> backward -> fused Nadam on the flat
    buffers -> device metrics.  Eight steps on one synthetic batch must lower the loss (and keep everything finite)."""
    from strajnet_amd import (OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt, Nadam,
                              compute_occupancy_flow_metrics, apply_sigmoid_to_occupancy_logits)
    model, w, x, xt = _setup(CFG128, 2, dtype)
    cfg = OccupancyFlowTaskConfig(128, 128, 8)
    loss_fn = OGMFlow_loss(cfg, replica=1.0, use_focal_loss=False, use_gt=True)
    opt = Nadam.for_model(model, lr=2e-4)
    true_wp = warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow'])
    hist = []
    for _ in range(8):
        model.zero_grad()
        out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
        logits = get_pred_waypoint_logits(out)
        d = loss_fn(logits, true_wp, None)
        total = sum(d.values())
        total.backward()
        opt.step()
        m = compute_occupancy_flow_metrics(cfg, true_wp, apply_sigmoid_to_occupancy_logits(logits))
        hist.append(float(total.detach()))
        assert np.isfinite(hist[-1]) and np.isfinite(m.vehicles_flow_epe)
    _report(f'train loop {dtype}: total loss over 8 Nadam steps (lr 2e-4) ' + ' -> '.join(f'{v:.1f}' for v in hist))
    assert hist[-1] < 0.8 * hist[0] and min(hist) < 0.6 * hist[0]


def test_save_and_load_weights_tf_checkpoint(tmp_path):
    """train.py:366 `model.save_weights('.../final_model.tf')` then inference.py:283 `model.load_weights(path)`: a second,
    differently initialised model must hold the first one's weights bit for bit and reproduce its outputs after loading the TF-format checkpoint,
    and a Nadam step taken after the load must start from the loaded weights (flat buffer and bf16 shadow both updated)."""
    import strajnet_amd
    model, w, x, xt = _setup(CFG128, 2, torch.bfloat16)
    path = str(tmp_path / 'final_model.tf')
    model.save_weights(path)
    assert sorted(os.listdir(tmp_path)) == ['final_model.tf.data-00000-of-00001', 'final_model.tf.index']
    other = strajnet_amd.STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.bfloat16, seed=123)
    y0 = _fwd(model, xt).float()
    assert (_fwd(other, xt).float() - y0).abs().max() > 0.1
    other.load_weights(path)
    assert torch.equal(_fwd(other, xt).float(), y0)                   # the eval forward has no atomics: bit for bit
    sd = other.state_dict()
    assert all(np.array_equal(sd[n], np.asarray(w[n], np.float32)) for n in w)
    with pytest.raises(KeyError):                                     # a deeper model must not half-load this checkpoint
        strajnet_amd.STrajNet(dict(CFG128, depths=[2, 2, 6]), fg_msa=True, fg=True, large_ogm=False).load_weights(path)


def test_upconv_wgrad_not_deferred_outside_the_model_graph():
    """The decoder's up-conv weight gradients are deferred to the model's flush point.  That decision is taken per op while the
    model's forward runs: an up-conv applied on its own afterwards -- even after a training forward whose backward never ran -- must
    launch its weight gradient itself (the deferral switch used to be a process global that stayed on)."""
    from strajnet_amd import ops
    model, w, x, xt = _setup(CFG128, 1, torch.float32)
    model.zero_grad()
    out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
    del out                                                     # forward only: no backward, no flush point ever runs
    pw, pb = model.params['decoder/upconv_0_0/kernel'], model.params['decoder/upconv_0_0/bias']
    model.zero_grad()
    xx = torch.randn(2, 8, 8, 96, device='cuda', requires_grad=True)
    y = ops.upconv(xx, pw, pb)
    y.sum().backward()
    torch.cuda.synchronize()
    assert float(pw.grad.abs().sum()) > 0 and float(xx.grad.abs().sum()) > 0
    g1 = pw.grad.clone()
    if pb.part is not None:
        model._fold_partials()
    assert float(pb.grad.abs().sum()) > 0
    # and again after a complete training step (flush point + join ran): same gradient increment
    model.zero_grad()
    out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
    out.sum().backward()
    torch.cuda.synchronize()
    model.zero_grad()
    y = ops.upconv(xx, pw, pb)
    y.sum().backward()
    torch.cuda.synchronize()
    assert float((pw.grad - g1).abs().max()) <= 1e-5 * float(g1.abs().max()), (float((pw.grad - g1).abs().max()), float(g1.abs().max()))


def test_side_streams_are_joined_after_backward():
    """Branches run on side streams and write their weight gradients straight into the flat buffer; work enqueued on the caller's
    stream right after backward() (here: a clone of the gradients) must already see all of it, and serial mode must agree."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    model, w, x, xt = _setup(CFG128, 2, torch.float32)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)

    def step():
        model.zero_grad()
        out = _fwd(model, xt)
        d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
        sum(d.values()).backward()
        return model.flat_grads().clone()           # enqueued on the current stream immediately, no synchronize
    assert model._streams[0] is not None and model._streams[1] is not None
    for _ in range(3):
        g_now = step()
        torch.cuda.synchronize()
        g_late = model.flat_grads().clone()
        assert torch.equal(g_now, g_late)
    model.serial = True
    g_serial = step()
    torch.cuda.synchronize()
    assert float((g_serial - g_late).abs().max()) < 1e-4 * float(g_late.abs().max())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_two_bucket_backward_matches_one_bucket(dtype):
    """Data-parallel overlap (dp.OverlappedGradSync): backward cut at the encoder outputs (model.cut_encoder -> backward() then
    backward_encoder()) must produce the gradients of the monolithic backward, the tail bucket must be FINAL after the first half
    (it is all-reduced while the second half runs), and the two-graph capture must replay to the same buffer."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from strajnet_amd.graph import GraphedTrainStep
    model, w, x, xt = _setup(CFG128, 2, dtype)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    k = model.bucket_split
    assert 0 < k < model.flat_grads().numel()
    assert k == model._offs['fg_msa/proj_q/kernel']

    def fwd_loss():
        model.zero_grad()
        out = _fwd(model, xt)
        d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
        return sum(d.values())
    fwd_loss().backward()
    g_one = model.flat_grads().clone()
    model.cut_encoder = True
    fwd_loss().backward()
    g_half = model.flat_grads().clone()                 # enqueued right after backward(): what the tail all-reduce would read
    model.backward_encoder()
    g_two = model.flat_grads().clone()
    torch.cuda.synchronize()
    scale = float(g_one.abs().max())
    tol_ = (1e-5 if dtype == torch.float32 else 2e-3) * scale     # atomics order (f32) / bf16 rounding of re-ordered sums
    assert float(g_half[:k].abs().max()) == 0.0                          # nothing of the encoder bucket before the second half
    assert torch.equal(g_half[k:], g_two[k:])                            # the tail bucket is final after the first half
    assert float((g_two - g_one).abs().max()) < tol_
    assert float(g_two[:k].abs().max()) > 0
    step = GraphedTrainStep(model, loss_fn, xt, training=False, split=True)
    seen = []
    for _ in range(2):
        step(between=lambda: seen.append(model.flat_grads()[k:].clone()))
    torch.cuda.synchronize()
    assert float((model.flat_grads() - g_one).abs().max()) < tol_
    assert float((seen[-1] - g_one[k:]).abs().max()) < tol_              # tail complete between the two replays
    model.cut_encoder = False


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_odd_batch_b3(dtype):
    """B = 3: row counts that are not multiples of the kernels' tile sizes (ragged tails of the GEMM / LayerNorm / conv grids).
    f32: forward within the 1e-3 gate and exact per-scene independence; bf16: same independence, loose error bound."""
    from oracle import np_ref
    model, w, x, xt = _setup(CFG128, 3, dtype)
    with torch.no_grad():
        y = _fwd(model, xt)
        one = {k: v[1:2].contiguous() for k, v in xt.items()}
        y1 = model(one['ogm'], one['map_img'], training=False, obs=one['obs'], occ=one['occ'], mapt=None, flow=one['flow'])
    ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'])
    err = np.abs(y.float().cpu().numpy() - ref).max()
    _report(f'fwd {dtype} B=3 128x128: max-abs err {err:.3e}')
    assert err < (ABS_TOL_F32 if dtype == torch.float32 else 0.25)        # bf16: 2x the measured 0.115
    # scene 1 alone == scene 1 inside the batch (no cross-sample op anywhere; deterministic kernels in forward)
    assert torch.equal(y[1:2], y1)


def test_bf16_mode_error_report():
    """bf16-storage throughput mode: measured error vs the f64 oracle (reported; bounded at twice the measured values)."""
    from oracle import np_ref
    model, w, x, xt = _setup(CFG128, 2, torch.bfloat16)
    with torch.no_grad():
        y = _fwd(model, xt).cpu().numpy()
    ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'])
    err = np.abs(y - ref).max()
    rms = float(np.sqrt(((y - ref) ** 2).mean()))
    dauc = _auc_delta(y, ref, x)
    _report(f'fwd bf16 128x128 B=2: max-abs err {err:.3e}, rms {rms:.3e} (ref scale {np.abs(ref).max():.2f}), |dPR-AUC| {dauc:.2e}')
    assert dauc < 2e-2
    assert np.isfinite(y).all()
    # bounds = 2x what MI355X measures (0.123 max-abs, 0.0207 rms on logits of scale 9.7): a regression of the bf16 path shows up here
    assert rms < 0.045 and err < 0.25, (rms, err)


def test_fp16_inference_mode_error_report():
    """fp16-storage inference mode (BASELINE config 4): 10 mantissa bits instead of bf16's 7 -> the error against the f64 oracle
    must come out several times below the bf16 mode's on the same inputs; a backward pass still runs (unscaled gradients)."""
    from oracle import np_ref
    ref = None
    errs = {}
    for dt in (torch.float16, torch.bfloat16):
        model, w, x, xt = _setup(CFG128, 2, dt)
        with torch.no_grad():
            y = _fwd(model, xt).float().cpu().numpy()
        if ref is None:
            ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'])
        assert np.isfinite(y).all()
        errs[dt] = (np.abs(y - ref).max(), float(np.sqrt(((y - ref) ** 2).mean())), _auc_delta(y, ref, x))
    e16, eb = errs[torch.float16], errs[torch.bfloat16]
    _report(f'fwd fp16 128x128 B=2: max-abs err {e16[0]:.3e}, rms {e16[1]:.3e}, |dPR-AUC| {e16[2]:.2e}   '
            f'(bf16 on the same inputs: {eb[0]:.3e} / {eb[1]:.3e} / {eb[2]:.2e})')
    assert e16[1] < 0.35 * eb[1] and e16[0] < 0.5 * eb[0] and e16[2] < 5e-3
    assert e16[0] < 0.03 and e16[1] < 0.006, e16            # 2x the measured 0.0145 max-abs / 0.0028 rms
    model, w, x, xt = _setup(CFG128, 1, torch.float16)
    model.zero_grad()
    out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
    out.float().square().mean().backward()
    g = model.flat_grads()
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_missing_library_fails_loudly(monkeypatch):
    from strajnet_amd import _lib
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libstrajnet_hip.so')
    with pytest.raises(_lib.StjError):
        _lib.lib()


def test_cpu_tensor_rejected():
    from strajnet_amd import ops
    with pytest.raises(RuntimeError):
        ops.gelu(torch.zeros(8))


def test_edge_cases_no_agents_all_agents_empty_rasters_f32():
    """Edge cases of the domain: scene 0 has NO valid agent (every obs/occ row is padding -> every tfa mask row is fully masked,
    the -1e10 additive mask then yields a uniform softmax), an empty occupancy raster and zero flow; scene 1 has
    every agent valid at every step.  Forward, loss (use_gt=False: the AUC gate of an all-empty waypoint is 0) and gradients
    against the oracle."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from oracle import np_ref, torch_ref
    w = np_ref.make_weights(CFG128, 0)
    x = np_ref.make_inputs(CFG128, 2)
    x['obs'][0] = 0; x['occ'][0] = 0; x['ogm'][0] = 0; x['flow'][0] = 0
    rng = np.random.default_rng(11)
    x['obs'][1] = rng.normal(0, 5, x['obs'][1].shape).astype(np.float32) + 0.5         # no exact zeros in column 0 -> all steps valid
    x['occ'][1] = rng.normal(0, 5, x['occ'][1].shape).astype(np.float32) + 0.5
    x['obs'][1][..., 0] = np.abs(x['obs'][1][..., 0]) + 0.1
    x['occ'][1][..., 0] = np.abs(x['occ'][1][..., 0]) + 0.1
    for k in ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow'):
        x[k][0] = 0                                                                     # nothing to predict in scene 0
    import strajnet_amd
    model = strajnet_amd.STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float32)
    model.load_weights(w)
    xt = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
    model.zero_grad()
    out = _fwd(model, xt)
    ref = np_ref.strajnet_forward(w, CFG128, x['ogm'], x['map_img'], x['obs'], x['occ'], x['flow'])
    err = np.abs(out.detach().cpu().numpy() - ref).max()
    assert np.isfinite(ref).all() and err < ABS_TOL_F32, err
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=False)
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    sum(d.values()).backward()
    pr = torch_ref.to_torch(w, torch.float64, requires_grad=True)
    xr = torch_ref.to_torch(x, torch.float64)
    yr = torch_ref.forward(pr, CFG128, xr['ogm'], xr['map_img'], xr['obs'], xr['occ'], xr['flow'])
    dr = torch_ref.loss(yr, xr['gt_obs'], xr['gt_occ'], xr['gt_flow'], xr['origin_flow'], replica=1.0, use_gt=False)
    sum(dr.values()).backward()
    for k in dr:
        assert abs(float(d[k].detach()) - float(dr[k].detach())) < 1e-4 * abs(float(dr[k].detach())) + 1e-5, k
    gmax = max(float(pr[n].grad.abs().max()) for n in model.params)
    worst = max(float((p.grad.double().cpu() - pr[n].grad).abs().max()) / (float(pr[n].grad.abs().max()) + 1e-6 * gmax)
                for n, p in model.params.items())
    _report(f'edge cases (no agents / all agents / empty rasters) 128x128 B=2 f32: fwd max-abs err {err:.3e}, worst relative grad error {worst:.3e}')
    assert worst < 2e-3


def test_bench_config_batch_permutation_bf16():
    """Size-independent property at the bench configuration (cfg-256, B=8, bf16): scenes are independent units, so
    permuting the batch permutes the outputs, leaves the (batch-mean) losses unchanged and leaves every gradient unchanged up to
    the order of f32 accumulation."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from oracle import np_ref
    cfg = dict(CFG128, input_size=(256, 256))
    model, w, x, xt = _setup(cfg, 8, torch.bfloat16)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(256, 256, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device='cuda')

    def run(t):
        model.zero_grad()
        out = _fwd(model, t)
        d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(t['gt_obs'], t['gt_occ'], t['gt_flow'], t['origin_flow']), None)
        sum(d.values()).backward()
        return out.detach().clone(), {k: float(v.detach()) for k, v in d.items()}, model.flat_grads().clone()
    o1, l1, g1 = run(xt)
    o2, l2, g2 = run({k: v[perm].contiguous() for k, v in xt.items()})
    assert torch.equal(o1[perm], o2)                                   # per-scene work is identical wherever the scene sits
    for k in l1:
        assert abs(l1[k] - l2[k]) <= 1e-5 * abs(l1[k]) + 1e-6, (k, l1[k], l2[k])
    assert float((g1 - g2).abs().max()) <= 2e-3 * float(g1.abs().max())
    _report(f'batch permutation cfg-256 B=8 bf16: outputs identical, losses equal, max grad diff '
            f'{float((g1 - g2).abs().max()):.2e} (|grad| max {float(g1.abs().max()):.2e})')


def test_bench_two_ranks_on_one_gpu():
    """The multi-process path of bench.py (rendezvous, replica-scaled loss, gradient all-reduce, Nadam, max-over-ranks timing, the
    all-reduce probe) end to end with two ranks sharing this GPU over gloo (STJ_BENCH_SHARE_GPU test hook; RCCL needs one device
    per rank).  Not a measurement -- it guards the driver's N>1 run against plumbing errors."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, STJ_BENCH_SHARE_GPU='1', MASTER_ADDR='127.0.0.1')
    res = {}
    for mode, extra in (('overlap', []), ('one_bucket', ['--no-overlap'])):
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', '29533', os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--batch', '2',
               '--full', '--no-kernel-timing', '--no-cpu-baseline'] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1, r.stdout[-2000:]                           # rank 0 only
        d = res[mode] = json.loads(lines[0])
        assert d['n_gpus'] == 2 and d['config']['global_batch'] == 4 and d['config']['parallelism'] == 'dp2'
        assert d['value'] > 0 and np.isfinite(d['loss']) and d['allreduce']['ms'] > 0 and d['allreduce']['mbytes'] > 50
        assert d['config']['optimizer_in_step'] and d['scaling'] == 'weak'
        assert d['distributed']['ranks'] == 2 and d['distributed']['ranks_seen_by_allreduce'] == 2
        assert d['distributed']['allreduce_overlapped_with_backward'] == (mode == 'overlap') == d['allreduce']['overlapped']
    # same seeds, same draws: three Nadam steps on all-reduced gradients must land on the same loss whichever way they were exchanged --
    # rank 0's own shard and the global batch (sum of the replica-scaled losses of both ranks)
    assert abs(res['overlap']['loss'] - res['one_bucket']['loss']) < 2e-3 * abs(res['one_bucket']['loss'])
    lg = [res[m]['distributed']['loss_global_batch'] for m in ('overlap', 'one_bucket')]
    assert abs(lg[0] - lg[1]) < 2e-3 * abs(lg[1]) and lg[1] > res['one_bucket']['loss']


def test_bench_plain_run_dumps_outputs(tmp_path):
    """bench.py without --full: the headline only (no extra passes after the timed region), `steps` and `ms_per_step` as asked, and
    --dump-outputs writing the losses and the gradient / weight samples of the timed step run from the seeded starting state, as
    float32.  That step does not depend on how many steps the run timed, so two runs of different lengths dump the same outputs up to
    the rounding of the f32 atomics in the weight gradients."""
    import json
    import subprocess
    import sys
    runs = []
    for i, steps in enumerate((3, 5)):
        d = tmp_path / f'run{i}'
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1', '--settle', '0', '--batch', '2',
               '--dump-outputs', str(d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(lines) == 1, r.stdout[-2000:]
        res = json.loads(lines[0])
        assert res['steps'] == steps and res['warmup'] == 1 and res['ms_per_step'] > 0 and res['value'] > 0
        assert res['unit'] == 'scenes/s' and res['higher_is_better'] and res['dtype'] == 'bf16'
        assert res['roofline'] is None and res['without_optimizer'] is None and res['cpu_baseline'] is None
        assert not {'families', 'parity_mode', 'with_input_feed', 'extra_configs'} & set(res)
        arrs = {f.stem: np.load(f) for f in d.glob('*.npy')}
        assert set(arrs) == {'loss', 'loss_terms', 'grads_sample', 'weights_sample'}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs['loss_terms'].shape == (4,) and abs(float(arrs['loss'][0]) - float(arrs['loss_terms'].sum())) <= 1e-4 * abs(float(arrs['loss'][0]))
        assert arrs['grads_sample'].shape == arrs['weights_sample'].shape and float(np.abs(arrs['grads_sample']).max()) > 0
        runs.append(arrs)
    a, b = runs
    # measured between pairs of runs: losses equal or 1e-7 apart; gradients within 1e-7 of their largest element, up to 1.5e-4 when an
    # intermediate rounds to the other bf16 value (bf16 steps are 3.9e-3 relative)
    np.testing.assert_allclose(a['loss_terms'], b['loss_terms'], rtol=1e-4)
    np.testing.assert_allclose(a['loss'], b['loss'], rtol=1e-4)
    gmax = float(np.abs(a['grads_sample']).max())
    assert float(np.abs(a['grads_sample'].astype(np.float64) - b['grads_sample']).max()) <= 1e-3 * gmax
    # Nadam's first update is ~1.056 lr sign(g) per element: where a gradient element's sign is within that rounding (measured at B = 8:
    # under 0.01 % of the weights differ by more than 1e-6) the two runs' weights lie up to 2.11 lr apart; the others agree to rounding
    dw = np.abs(a['weights_sample'].astype(np.float64) - b['weights_sample'])
    assert float(dw.max()) <= 2.2e-4 and int((dw > 1e-6).sum()) <= 0.01 * dw.size


def test_golden_train_step_gradients_f32():
    """One f32 train step of the HIP path against the committed gradient fixture (tests/golden/strajnet_128_b2_grads.npz, made by
    make_golden_grads.py from the float64 oracle): the four losses, the L2 norm of each of the 299 gradient tensors and eight
    small gradients element by element."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from oracle import np_ref
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'strajnet_128_b2_grads.npz'))
    model, w, x, xt = _setup(CFG128, 2, torch.float32, seed=int(g['weight_seed']))
    x2 = np_ref.make_inputs(CFG128, 2, seed=int(g['input_seed']))
    assert all(np.array_equal(x[k], x2[k]) for k in x)               # _setup's default input seed is the fixture's
    model.zero_grad()
    out = _fwd(model, xt)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    sum(d.values()).backward()
    for i, k in enumerate(('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')):
        assert abs(float(d[k].detach()) - float(g['loss'][i])) < 1e-4 * abs(float(g['loss'][i])) + 1e-5, k
    ref = dict(zip([str(n) for n in g['names']], g['grad_l2']))
    gmax = float(g['grad_l2'].max())
    worst = 0.0
    for n, p in model.params.items():
        e = abs(float(p.grad.double().norm()) - ref[n]) / (ref[n] + 1e-6 * gmax)
        worst = max(worst, e)
        assert e < 2e-3, (n, e)
    for k in g.files:
        if k.startswith('full:'):
            got, want = model.params[k[5:]].grad.double().cpu().numpy(), g[k]
            assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-9, k
    _report(f'golden train step 128x128 B=2 f32: worst relative error of the 299 gradient L2 norms {worst:.3e}')


def test_f32_golden_step_runs_the_fused_entry_points():
    """WHICH kernels the oracle gate covers, checked instead of narrated: the f32 golden train step (the one the two tests around this one
    hold against the float64 fixture) is run with every C-ABI call recorded (strajnet_amd.prof), and the set of entry points must contain
    the fused kernels the bf16 step times -- and must not contain the layer-by-layer ops they replace.  (Known 16-bit-only kernels, by
    their entry points' dispatch: the weight-stationary / wave-specialised decoder family behind stj_upconv_*, stj_outconv_pair_*,
    stj_wgrad_group, and the agent interaction block stj_agent_int_*: their f32 counterparts run here.)"""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    from strajnet_amd import prof
    model, w, x, xt = _setup(CFG128, 2, torch.float32)
    model.serial = True
    model.zero_grad()
    prof.enable()
    try:
        out = model(xt['ogm'], xt['map_img'], training=True, obs=xt['obs'], occ=xt['occ'], mapt=xt['mapt'], flow=xt['flow'])
        loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=1.0, use_focal_loss=False, use_gt=True)
        d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
        sum(d.values()).backward()
        torch.cuda.synchronize()
    finally:
        ev = prof.disable()
    fams = {prof.COST[k][0] for k in ev}
    called = set(fams) | {k for k in ev if k.startswith('stj_')}
    text = ' '.join(sorted(called))
    must = ['swin_attn_fwd', 'swin_attn_bwd', 'swin_mlp_fwd', 'swin_mlp_bwd', 'fgattn_fwd', 'fgattn_bwd', 'xattn_fwd', 'xattn_bwd', 'patch_embed_fwd',
            'agent_enc_fwd', 'agent_enc_bwd', 'agent_pack', 'fgoff_fwd', 'fgoff_bwd', 'fgoff_pack', 'loss_fwd', 'loss_bwd', 'upconv_fwd', 'upconv_dgrad', 'upconv_wgrad']
    for m in must:
        assert m in text, (m, text)
    for gone in ('small_attn', 'agent_prep', 'maxpool', 'fg_bias_fwd', 'im2col3', 'col2im3', 'win_attn_fwd', 'win_attn_bwd'):      # replaced ops: small_attn / agent_prep / maxpool by agent_enc; fg_bias by fgattn; im2col3 / col2im3 (+ LayerNorm, gelu, the offset kernel's first half) by fgoff; win_attn at every width (C = 384 in f32 since round 6: AttnCfg::KH)
        assert not any(k == gone or k.startswith(gone + '[') or k == 'stj_' + gone or k.startswith('stj_' + gone + '_') for k in called), (gone, text)      # (whole names: 'win_attn_fwd' is inside 'swin_attn_fwd')
    _report('f32 golden step entry points: ' + text)


def test_golden_train_step_gradients_cfg256_b8_f32():
    """BASELINE config 2's own geometry (cfg-256, B=8): one f32 train step of the HIP path against the committed fixture
    tests/golden/strajnet_256_b8_grads.npz (make_golden_grads.py --cfg256, float64 oracle): the four losses and the L2 norm of each of
    the 299 gradient tensors, plus three small gradients element by element."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'strajnet_256_b8_grads.npz'))
    cfg = dict(CFG128, input_size=(256, 256))
    model, w, x, xt = _setup(cfg, 8, torch.float32, seed=int(g['weight_seed']))
    model.zero_grad()
    out = _fwd(model, xt)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(256, 256, 8), replica=1.0, use_focal_loss=False, use_gt=True)
    d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    sum(d.values()).backward()
    for i, k in enumerate(('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')):
        assert abs(float(d[k].detach()) - float(g['loss'][i])) < 1e-4 * abs(float(g['loss'][i])) + 1e-5, (k, float(d[k].detach()), float(g['loss'][i]))
    ref = dict(zip([str(n) for n in g['names']], g['grad_l2']))
    gmax = float(g['grad_l2'].max())
    worst = 0.0
    for n, p in model.params.items():
        e = abs(float(p.grad.double().norm()) - ref[n]) / (ref[n] + 1e-6 * gmax)
        worst = max(worst, e)
        assert e < 2e-3, (n, e)
    for k in g.files:
        if k.startswith('full:'):
            got, want = model.params[k[5:]].grad.double().cpu().numpy(), g[k]
            assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-9, k
    _report(f'golden train step cfg-256 B=8 f32: worst relative error of the 299 gradient L2 norms {worst:.3e}')


def test_golden_cfg256_f32():
    """Full-size cfg-256 (BASELINE configs[0] geometry) against the committed golden fixture (tests/golden, made by the
    oracle): logits subsample, per-row checksums and the 4 loss scalars."""
    from strajnet_amd import OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'strajnet_256_b1.npz'))
    cfg = dict(CFG128, input_size=(256, 256))
    model, w, x, xt = _setup(cfg, 1, torch.float32, seed=int(g['weight_seed']))
    with torch.no_grad():
        out = _fwd(model, xt)
        loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(256, 256, 8), replica=1.0, use_focal_loss=False, use_gt=True)
        d = loss_fn(get_pred_waypoint_logits(out), warpped_gt(xt['gt_obs'], xt['gt_occ'], xt['gt_flow'], xt['origin_flow']), None)
    y = out.cpu().numpy().astype(np.float64)
    err = np.abs(y[0, ::4, ::4, :] - g['logits_sub']).max()
    rs = np.abs(y[0].sum((1, 2)) - g['logits_rowsum']).max()
    _report(f'golden cfg-256 B=1 f32: max-abs err on subsample {err:.3e}, row-checksum err {rs:.3e} '
            f'(|logit| max {float(g["logits_abs_max"]):.2f})')
    assert err < ABS_TOL_F32
    assert rs < 256 * 32 * 1e-4
    for i, k in enumerate(('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')):
        assert abs(float(d[k]) - float(g['loss'][i])) < 1e-4 * abs(float(g['loss'][i])) + 1e-5
