"""Cases for the per-scene validation pass (stj_eval_scenes_fwd, csrc/eval.hip) and their float64 references, shared by
tests/test_eval_scenes_ref.py (CPU) and tests/test_eval_scenes_gpu.py.  The inputs are _eval_cases.make_case's, as they are.

    3 x  8 x  8   exactly one workgroup's items (512) per scene: a scene boundary is a workgroup boundary; warp targets leave the image
    2 x 24 x 40   non-square
    3 x 40 x 44   14 080 items per scene, no multiple of 512: a scene's last workgroup is partial and must stop at the scene's end
    1 x 72 x 64   72 workgroups' worth of items: the stride path whenever stj_eval_scenes_grid(72, 64) < 72
The "empty" scene is scene 0 of 3 x 8 x 8 with gt_obs and gt_occ set to zero: every gate 0 under use_gt.

A scene's reference row is the oracle on that scene as a batch of one: float64[12] = observed_xe, occluded_xe, flow, flow_warp_xe,
their sum, the seven metrics.
"""
import functools

import numpy as np

import _eval_cases as EC

SHAPES = ((3, 8, 8), (2, 24, 40), (3, 40, 44), (1, 72, 64))
EMPTY_SHAPE = SHAPES[0]
ROW_KEYS = EC.LOSS_KEYS + ('total', 'observed_auc', 'occluded_auc', 'observed_iou', 'occluded_iou', 'flow_epe', 'flow_ogm_auc', 'flow_ogm_iou')
KEYS = ('logits',) + EC.GT_KEYS


@functools.lru_cache(maxsize=None)
def batch_case(shape, empty0=False, seed=0):
    """make_case's arrays; empty0: scene 0 without any vehicle occupancy (copies, read-only)."""
    c = EC.make_case(*shape, seed)
    if not empty0:
        return c
    c = {k: v.copy() for k, v in c.items()}
    c['gt_obs'][0] = 0
    c['gt_occ'][0] = 0
    for v in c.values():
        v.setflags(write=False)
    return c


def sub_case(shape, scenes, empty0=False, seed=0):
    """The sub-batch of the listed scenes, in that order."""
    c = batch_case(tuple(shape), empty0, seed)
    idx = list(scenes)
    return {k: np.ascontiguousarray(v[idx]) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def _ref(shape, scenes, fkey, no_warp, empty0, seed):
    from oracle import np_ref
    c = sub_case(shape, scenes, empty0, seed)
    with np.errstate(invalid='ignore', divide='ignore'):
        d, gates = np_ref.ogm_flow_loss(c['logits'], c['gt_obs'], c['gt_occ'], c['gt_flow'], c['origin_flow'], replica=EC.REPLICA,
                                        return_gates=True, **EC.WEIGHTS, **dict(fkey))
        m = np_ref.occupancy_flow_metrics(c['logits'], c['gt_obs'], c['gt_occ'], c['gt_flow'], c['origin_flow'], no_warp=no_warp)
    four = [float(d[k]) for k in EC.LOSS_KEYS]
    row = np.array(four + [four[0] + four[1] + four[2] + four[3]] + [float(v) for v in m], np.float64)
    row.setflags(write=False)
    return row, tuple(float(g) for g in gates)


def ref_pooled(shape, scenes, flags, no_warp=False, empty0=False, seed=0):
    """float64 oracle on the sub-batch of `scenes` -> (row float64[12], gates[8]); computed once."""
    return _ref(tuple(shape), tuple(scenes), EC.flag_key(flags), no_warp, empty0, seed)


def ref_rows(shape, flags, no_warp=False, empty0=False, seed=0):
    """-> (rows float64[B,12], gates [B][8]): the oracle on every scene alone."""
    both = [ref_pooled(shape, (b,), flags, no_warp, empty0, seed) for b in range(shape[0])]
    return np.stack([r for r, _ in both]), [g for _, g in both]


def grid_reference(H, W, maxg):
    """Workgroups per scene (csrc/eval_scene.h, evs_grid): one per 512 items of the scene's H*W*8, at most maxg."""
    return 0 if H <= 0 or W <= 0 else min(maxg, -(-H * W * 8 // 512))
