#!/usr/bin/env python
"""What the validation step's fused loss + metrics pass buys, measured with device events after warm-up, in one process.

  pass   stj_eval_fwd (one pass over the logits and the ground truth) against the sequence it replaces -- stj_loss_auc_gate +
         stj_loss_fwd + stj_loss_finalize + stj_metrics on the same tensors, their scratch re-zeroed by ONE fill per call (the least a
         caller needs: the ops wrappers take a fill each).  Per round the fused pass is timed once and the replaced sequence TWICE in
         a row, the two alternating over --rounds rounds of --calls calls: the spread of repeated runs of the replaced sequence
         ((max - min) / median over all its runs) is measured in the same call and is the margin of `not_slower`.
  step   graph.GraphedEvalStep (forward + fused pass + running means as one hipGraph) against an eager validation step assembled from
         GraphedForward + OGMFlow_loss + compute_occupancy_flow_metrics, the same way; scenes/s of both.
  scenes (--parts scenes) the per-scene pass stj_eval_scenes_fwd (rows, pooled result, state and table: all five launches)
         against stj_eval_fwd on the same inputs, and GraphedEvalStep(per_scene=True) against GraphedEvalStep(), the same way.  The step
         has a gate: slower by at most 2 % plus the measured spread of GraphedEvalStep()'s runs (`within_gate`).  Without --out the
         lines also go to profiles/eval_scenes_<date>.jsonl.

At --batches (default 8,32), 256 x 256, on bench.synth_batch scenes and N(0, 2) logits.  One JSON line per measurement.
Every device step runs inside this one process; run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='8,32')
ap.add_argument('--calls', type=int, default=200, help='calls per timed run')
ap.add_argument('--warmup', type=int, default=20)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--parts', default='pass,step', help='comma-separated: pass, step, scenes')
ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
a = ap.parse_args()
a.parts = a.parts.split(',')

import torch

import bench
from strajnet_amd import (STrajNet, OGMFlow_loss, OccupancyFlowTaskConfig, get_pred_waypoint_logits, warpped_gt,
                          compute_occupancy_flow_metrics, ops)
from strajnet_amd.graph import GraphedEvalStep, GraphedForward

assert torch.cuda.is_available(), 'bench_eval.py needs a GPU'
if 'scenes' in a.parts and not a.out:
    import datetime
    a.out = os.path.join(ROOT, 'profiles', f'eval_scenes_{datetime.date.today():%Y%m%d}.jsonl')
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
H = 256
GT = ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow')
W8 = (1000.0, 1000.0, 1000.0, 1.0)         # ogm, occ, flow-origin weights, replica (train.py:188-196)
FLAGS = 1                                   # the train.py:195-196 loss: warp term on, no focal, no use_pred (+ use_gt)


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


def timed(fn, calls):
    """ms per call of `calls` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def compare(new, old, calls):
    """-> (runs of new, runs of old): per round new once and old twice in a row, alternating."""
    for f in (new, old):
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    rn, ro = [], []
    for _ in range(a.rounds):
        rn.append(timed(new, calls))
        ro.append(timed(old, calls))
        ro.append(timed(old, calls))
    return rn, ro


def verdict(rn, ro):
    mn, mo = statistics.median(rn), statistics.median(ro)
    spread = (max(ro) - min(ro)) / mo
    return dict(new_ms=round(mn, 5), old_ms=round(mo, 5), new_runs=[round(v, 5) for v in rn], old_runs=[round(v, 5) for v in ro],
                old_spread=round(spread, 4), ratio=round(mn / mo, 4), not_slower=bool(mn <= mo * (1.0 + spread)))


def bench_pass(B, x):
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn((B, H, H, 32), generator=g) * 2.0).to(dev)
    gt = [x[k] for k in GT]
    p = ops._p
    ws = ops.eval_workspace(B, H, H, dev)
    loss, met = torch.empty(5, device=dev), torch.empty(7, device=dev)

    def fused():
        ops.call('stj_eval_fwd', p(logits), *map(p, gt), p(ws), p(loss), p(met), None, None, None, B, H, H, *W8, 1.0,
                 FLAGS | ops.EVAL_USE_GT, ops._st())
    # the replaced sequence's scratch as one buffer: gate histogram, loss sums, metric histograms and sums
    nh, ns, mh, ms = 8 * 202, 128 * 40, 8 * 3 * 202, 8 * 11
    scratch = torch.zeros(nh + ns + mh + ms, dtype=torch.int32, device=dev)
    ghist, sums, mhist, msums = scratch[:nh], scratch[nh:nh + ns].view(torch.float32), scratch[nh + ns:nh + ns + mh], scratch[nh + ns + mh:].view(torch.float32)
    gate, coef, loss2, mauc, met2 = (torch.empty(n, device=dev) for n in (8, 32, 5, 24, 7))

    def replaced():
        scratch.zero_()
        st = ops._st()
        ops.call('stj_loss_auc_gate', *map(p, gt), p(ghist), p(gate), None, B, H, H, st)
        ops.call('stj_loss_fwd', p(logits), *map(p, gt), p(gate), p(sums), p(loss2), p(coef), B, H, H, *W8, FLAGS, st)
        ops.call('stj_loss_finalize', p(sums), p(gate), p(loss2), p(coef), B, H, H, *W8, FLAGS, st)
        ops.call('stj_metrics', p(logits), *map(p, gt), p(mhist), p(msums), p(mauc), p(met2), B, H, H, 1, 1, st)
    rn, ro = compare(fused, replaced, a.calls)
    torch.cuda.synchronize()
    d = verdict(rn, ro)
    d.update(part='pass', batch=B, calls=a.calls, new='stj_eval_fwd', old='auc_gate+loss_fwd+loss_finalize+metrics',
             bytes_one_pass=4 * B * H * H * (32 + 8 * 5), loss_agree=bool(torch.allclose(loss, loss2, rtol=1e-4)),
             metrics_agree=bool(torch.allclose(met, met2, atol=1e-4)))
    emit(d)


def bench_step(B, x):
    model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.bfloat16, device=dev, seed=0, dropout_seed=0)
    cfg = OccupancyFlowTaskConfig(H, H, 8)
    loss_fn = OGMFlow_loss(cfg, ogm_weight=1000.0, occ_weight=1000.0, flow_weight=1.0, replica=1.0, flow_origin_weight=1000.0,
                           no_use_warp=False, use_pred=False, use_gt=True, use_focal_loss=False)
    step = GraphedEvalStep(model, loss_fn, x)
    fwd = GraphedForward(model, x)
    tw = warpped_gt(*(x[k] for k in GT))

    def eager():
        with torch.no_grad():
            logits = get_pred_waypoint_logits(fwd())
            loss_fn(logits, tw, None)
            compute_occupancy_flow_metrics(cfg, tw, packed_predictions(logits))
    calls = max(10, a.calls // 4)
    rn, ro = compare(step, eager, calls)
    torch.cuda.synchronize()
    d = verdict(rn, ro)
    d.update(part='step', batch=B, calls=calls, new='GraphedEvalStep', old='GraphedForward+OGMFlow_loss+compute_occupancy_flow_metrics',
             new_scenes_per_s=round(B / d['new_ms'] * 1e3, 1), old_scenes_per_s=round(B / d['old_ms'] * 1e3, 1), means=step.result())
    emit(d)
    del step, fwd


def bench_scenes_pass(B, x):
    g = torch.Generator().manual_seed(7)
    logits = (torch.randn((B, H, H, 32), generator=g) * 2.0).to(dev)
    gt = [x[k] for k in GT]
    p = ops._p
    ws, ws2 = ops.eval_workspace(B, H, H, dev), ops.eval_scenes_workspace(B, H, H, dev)
    loss, met, running = torch.empty(5, device=dev), torch.empty(7, device=dev), torch.zeros(12, dtype=torch.float64, device=dev)
    rows, pooled = torch.empty(B, 12, device=dev), torch.empty(12, device=dev)
    capacity = 1 << 16
    state, table = torch.zeros(2, 13, dtype=torch.float64, device=dev), torch.zeros(capacity, 12, device=dev)
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)

    def fused():
        ops.call('stj_eval_fwd', p(logits), *map(p, gt), p(ws), p(loss), p(met), None, None, p(running), B, H, H, *W8, 1.0,
                 FLAGS | ops.EVAL_USE_GT, ops._st())

    def scenes():
        ops.call('stj_eval_scenes_fwd', p(logits), *map(p, gt), None, p(ws2), p(rows), None, None, p(pooled), ops.vp(pooled.data_ptr() + 20),
                 None, None, p(state), p(table), p(cursor), capacity, B, H, H, *W8, 1.0, FLAGS | ops.EVAL_USE_GT, ops._st())
    rn, ro = compare(scenes, fused, a.calls)
    torch.cuda.synchronize()
    d = verdict(rn, ro)
    d.update(part='scenes_pass', batch=B, calls=a.calls, new='stj_eval_scenes_fwd', old='stj_eval_fwd', grid_per_scene=ops.eval_scenes_grid(H, H),
             pooled_agree=bool(torch.allclose(pooled[:5], loss, rtol=1e-5) and torch.allclose(pooled[5:], met, atol=1e-5)),
             rows_mean_flow=float(rows[:, 2].mean()), pooled_flow=float(pooled[2]), lib=os.path.basename(os.environ.get('STJ_LIB_PATH', '')))
    emit(d)


def bench_scenes_step(B, x):
    model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.bfloat16, device=dev, seed=0, dropout_seed=0)
    cfg = OccupancyFlowTaskConfig(H, H, 8)
    loss_fn = OGMFlow_loss(cfg, ogm_weight=1000.0, occ_weight=1000.0, flow_weight=1.0, replica=1.0, flow_origin_weight=1000.0,
                           no_use_warp=False, use_pred=False, use_gt=True, use_focal_loss=False)
    old = GraphedEvalStep(model, loss_fn, x)
    new = GraphedEvalStep(model, loss_fn, x, per_scene=True, capacity=1 << 16)
    new_replay, old_replay = new.graph.replay, old.graph.replay          # the replays alone: the inputs are loaded, live is all ones
    calls = max(10, a.calls // 4)
    rn, ro = compare(new_replay, old_replay, calls)
    torch.cuda.synchronize()
    d = verdict(rn, ro)
    d.update(part='scenes_step', batch=B, calls=calls, new='GraphedEvalStep(per_scene=True)', old='GraphedEvalStep()',
             within_gate=bool(d['new_ms'] <= d['old_ms'] * (1.02 + d['old_spread'])),
             new_scenes_per_s=round(B / d['new_ms'] * 1e3, 1), old_scenes_per_s=round(B / d['old_ms'] * 1e3, 1),
             means=new.result(), old_means=old.result(), scenes=new.scores.result())
    emit(d)
    del new, old


def packed_predictions(logits):
    """What metrics.apply_sigmoid_to_occupancy_logits hands the metrics on the packed path, without its 16 per-waypoint sigmoid launches
    (the metric kernel applies the sigmoid itself): the eager step is not charged for them."""
    from strajnet_amd.loss import WaypointGrids
    g = WaypointGrids()
    v = logits.vehicles
    g.vehicles.observed_occupancy, g.vehicles.occluded_occupancy, g.vehicles.flow = v.observed_occupancy, v.occluded_occupancy, v.flow
    g._packed_logits = logits._packed
    return g


for B in (int(b) for b in a.batches.split(',')):
    x = bench.synth_batch(B, 1234, dev)
    if 'pass' in a.parts:
        bench_pass(B, x)
    if 'step' in a.parts:
        bench_step(B, x)
    if 'scenes' in a.parts:
        bench_scenes_pass(B, x)
        bench_scenes_step(B, x)
    del x
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
