"""Seeded cases for the fused validation pass (stj_eval_fwd, csrc/eval.hip) and their float64 references, shared by
tests/test_eval_ref.py (CPU: what the cases exercise, from the oracle alone) and tests/test_eval_gpu.py.

The kernel does not depend on the model's geometry, so the shapes are the smallest at which it can go wrong:
    3 x  8 x  8   warp targets leave the tiny image on every side
    1 x 24 x 40   non-square: catches H / W swaps
    2 x 40 x 40   25 600 work items: no multiple of the workgroup size or of the grid stride
Logits are N(0, 2) with the predicted-flow channels snapped to the 1/16-offset lattice (round(8x) + 0.5) / 8 (sample coordinates and
bilinear weights are then exact in float32: tests/test_ops_gpu.py, test_loss_and_gate); the true flow is on a 1/8 lattice and zero on
~70 % of the pixels; occupancies and origin are binary (~15 % / 8 % / 25 %).  Waypoint 3 has no positive occupancy (gate 0),
waypoint 5 no pixel with a true flow (the divide_no_nan paths).
"""
import functools

import numpy as np

SHAPES = ((3, 8, 8), (1, 24, 40), (2, 40, 40))
WEIGHTS = dict(ogm_weight=1000.0, occ_weight=1000.0, flow_origin_weight=1000.0)
REPLICA = 2.0
# the train.py:195-196 flags and the constructor defaults (focal), then use_pred, no_use_warp and use_gt=False once each
TRAIN = dict(use_focal_loss=False, use_pred=False, no_use_warp=False, use_gt=True)
DEFAULTS = dict(use_focal_loss=True, use_pred=False, no_use_warp=False, use_gt=False)
EXTRA = (dict(TRAIN, use_pred=True), dict(TRAIN, no_use_warp=True), dict(TRAIN, use_gt=False))
LOSS_KEYS = ('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')
GT_KEYS = ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow')


@functools.lru_cache(maxsize=None)
def make_case(B, H, W, seed=0):
    """-> dict of float32 arrays: logits [B,H,W,32], gt_obs / gt_occ / origin_flow [B,8,H,W,1], gt_flow [B,8,H,W,2].  Treat as read-only."""
    rng = np.random.default_rng([seed, B, H, W])
    logits = rng.normal(0, 2, (B, H, W, 32)).astype(np.float32)
    fl = logits.reshape(B, H, W, 8, 4)[..., 2:]
    fl[...] = (np.round(fl * 8) + 0.5) / 8
    gt_obs = (rng.random((B, 8, H, W, 1)) < 0.15).astype(np.float32)
    gt_occ = (rng.random((B, 8, H, W, 1)) < 0.08).astype(np.float32)
    origin = (rng.random((B, 8, H, W, 1)) < 0.25).astype(np.float32)
    gt_flow = (np.round(rng.normal(0, 2, (B, 8, H, W, 2)) * 8) / 8).astype(np.float32)
    gt_flow *= (rng.random((B, 8, H, W, 1)) >= 0.7)
    gt_obs[:, 3] = 0
    gt_occ[:, 3] = 0
    gt_flow[:, 5] = 0
    c = dict(logits=logits, gt_obs=gt_obs, gt_occ=gt_occ, gt_flow=gt_flow, origin_flow=origin)
    for v in c.values():
        v.setflags(write=False)
    return c


def flag_key(flags):
    return tuple(sorted(flags.items()))


@functools.lru_cache(maxsize=None)
def _ref_loss(shape, seed, fkey):
    from oracle import np_ref
    c = make_case(*shape, seed)
    d, gates = np_ref.ogm_flow_loss(c['logits'], c['gt_obs'], c['gt_occ'], c['gt_flow'], c['origin_flow'], replica=REPLICA,
                                    return_gates=True, **WEIGHTS, **dict(fkey))
    return tuple(float(d[k]) for k in LOSS_KEYS), tuple(float(g) for g in gates)


def ref_loss(shape, flags, seed=0):
    """float64 oracle -> ((observed_xe, occluded_xe, flow, flow_warp_xe), gates[8]); computed once per (case, flags)."""
    return _ref_loss(tuple(shape), seed, flag_key(flags))


@functools.lru_cache(maxsize=None)
def ref_metrics(shape, no_warp=False, seed=0):
    """float64 oracle -> the seven metrics in the order of strajnet_amd.metrics.FIELDS; computed once per (case, no_warp)."""
    from oracle import np_ref
    c = make_case(*shape, seed)
    return tuple(np_ref.occupancy_flow_metrics(c['logits'], c['gt_obs'], c['gt_occ'], c['gt_flow'], c['origin_flow'], no_warp=no_warp))


def loss_flags(flags, no_warp=False):
    """stj_eval_fwd's flag word: bits 0-2 as stj_loss_fwd, bit 3 use_gt, bit 4 the metrics' no_warp."""
    return ((0 if flags['no_use_warp'] else 1) | (2 if flags['use_focal_loss'] else 0) | (4 if flags['use_pred'] else 0) |
            (8 if flags['use_gt'] else 0) | (16 if no_warp else 0))
