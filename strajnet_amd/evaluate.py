"""The validation half of the reference's training loop (train.py:252-282, metrics.py:4-71).

    eval_step(model, loss_fn, batch, loss_means=None, metrics=None, no_warp=False, scenes=None, live=None) -> (LossDict, OccupancyFlowMetrics)
    SceneScores(capacity, preflix='val', no_warp=False)   # every scene scored on its own: running means, a table of rows, worst(k)
    Mean(name)                                       # tf.keras.metrics.Mean over a device tensor: update_state never syncs
    OGMFlowMetrics(preflix='train', no_warp=False)   # metrics.py:4-59: update_state(metrics) / reset_states() / get_result()
    print_metrics(res_dict, preflix='train', no_warp=False)

val_step is the forward pass with training=False, OGMFlow_loss, compute_occupancy_flow_metrics, and the update of four Keras Means
of the losses and an OGMFlowMetrics.  Here loss and metrics come out of ONE pass over the logits and the ground truth
(ops.eval_loss_metrics, csrc/eval.hip) without floating-point atomics: the same batch gives the same bits in every run.  The
captured form, with the running means kept by the pass itself, is graph.GraphedEvalStep.

The reference's numbers are pooled over the batch, so they depend on the batch size, and a submission is scored one scenario at a time
(inference.py:258 runs batch(1)).  With a SceneScores the step takes the per-scene pass (ops.eval_scene_scores, stj_eval_scenes_fwd): one
row of losses and metrics per scene as a batch of one, and from the same pass the pooled numbers of the live scenes.
"""
import numpy as np
import torch

from . import ops
from .loss import LossDict, OGMFlow_loss, get_pred_waypoint_logits, warpped_gt
from .metrics import FIELDS, OccupancyFlowMetrics

LOSS_KEYS = ('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')
# metrics.py:7-18: the OGMFlowMetrics member of each field of FIELDS, in that order
METRIC_KEYS = ('observed_auc', 'occluded_auc', 'observed_iou', 'occluded_iou', 'flow_epe', 'flow_ogm_auc', 'flow_ogm_iou')


def _state_device():
    """Where a running mean lives unless told otherwise: the current GPU (host memory on a machine without one: bookkeeping only)."""
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


class Mean:
    """tf.keras.metrics.Mean: result() = sum of the values / their number, 0 when nothing was added (divide_no_nan).
    The state is a float64 device tensor [total, count]; update_state(value) adds a device scalar to it without a host sync, and
    result() is a device scalar too -- float(m.result()) is where the host waits."""

    def __init__(self, name='mean', device=None, state=None):
        self.name = name
        self._state = state if state is not None else torch.zeros(2, dtype=torch.float64, device=device or _state_device())

    def update_state(self, value):
        if torch.is_tensor(value):
            value = value.detach().to(device=self._state.device, dtype=torch.float64).reshape(())
        self._state[0] += value
        self._state[1] += 1

    def result(self):
        total, count = self._state[0], self._state[1]
        return torch.where(count != 0, total / torch.where(count != 0, count, torch.ones_like(count)), torch.zeros_like(total))

    def reset_states(self):
        self._state.zero_()


def _result_keys(preflix, no_warp):
    return [f'{preflix}_{k}' for k in (METRIC_KEYS[:5] if no_warp else METRIC_KEYS)]


class OGMFlowMetrics:
    """metrics.py:4-59.  One float64 device tensor [7][total, count] holds the state; the per-field members the reference's loop
    reads (train.py:330 `.flow_ogm_auc.result()`) are Means over its rows.  update_state adds a whole OccupancyFlowMetrics (its
    device tensor: no sync), get_result() is the one host sync."""

    def __init__(self, preflix='train', no_warp=False, device=None):
        self.preflix, self.no_warp = preflix, no_warp
        self._n = 5 if no_warp else 7
        self._state = torch.zeros(self._n, 2, dtype=torch.float64, device=device or _state_device())
        for i in range(self._n):
            setattr(self, METRIC_KEYS[i], Mean(METRIC_KEYS[i], state=self._state[i]))

    def reset_states(self):
        self._state.zero_()

    def update_state(self, metrics):
        values = getattr(metrics, 'values', None)
        if values is None:            # any object with the seven fields (occupancy_flow_metrics_pb2.OccupancyFlowMetrics)
            values = torch.tensor([float(getattr(metrics, f)) for f in FIELDS], dtype=torch.float64)
        self._state[:, 0] += values[:self._n].detach().to(device=self._state.device, dtype=torch.float64)
        self._state[:, 1] += 1

    def get_result(self):
        total, count = self._state[:, 0], self._state[:, 1]
        res = torch.where(count != 0, total / torch.where(count != 0, count, torch.ones_like(count)), torch.zeros_like(total))
        return dict(zip(_result_keys(self.preflix, self.no_warp), res.tolist()))


def print_metrics(res_dict, preflix='train', no_warp=False):
    """metrics.py:61-71: one block of labelled values from get_result()'s dict (plain Python: needs no GPU)."""
    r = lambda k: res_dict[f'{preflix}_{k}']
    lines = [f"|obs-AUC: {r('observed_auc')}|occ-AUC: {r('occluded_auc')}",
             f"|obs-IOU: {r('observed_iou')}|occ-IOU: {r('occluded_iou')}",
             f"| Flow-EPE: {r('flow_epe')}" + ('|' if no_warp else '')]
    if not no_warp:
        lines.append(f"|FlowOGM_AUC: {r('flow_ogm_auc')} |FlowOGM_IOU: {r('flow_ogm_iou')} |")
    print('\n ' + '\n'.join(lines))


def eval_flags(loss_fn, no_warp=False):
    """stj_eval_fwd's flag word of an OGMFlow_loss and the metrics' no_warp."""
    return loss_fn._flags() | (ops.EVAL_USE_GT if loss_fn.use_gt else 0) | (ops.EVAL_NO_WARP if no_warp else 0)


def eval_loss_metrics(loss_fn, pred_waypoint_logits, true_waypoints, no_warp=False, running=None, workspace=None):
    """OGMFlow_loss.__call__ + compute_occupancy_flow_metrics(apply_sigmoid_to_occupancy_logits(.)) as the one fused pass, forward
    only -> (LossDict, OccupancyFlowMetrics).  Hand-built WaypointGrids are packed first, as the loss and the metrics do."""
    logits, gt = _packed_inputs(loss_fn, pred_waypoint_logits, true_waypoints)
    loss, met = ops.eval_loss_metrics(logits, *gt, loss_fn.ogm_weight, loss_fn.occ_weight, loss_fn.flow_origin_weight, loss_fn.replica,
                                      eval_flags(loss_fn, no_warp), running=running, loss_scale=loss_fn.replica, workspace=workspace)
    return _loss_dict(loss_fn, loss), OccupancyFlowMetrics(met, no_warp)


def _packed_inputs(loss_fn, pred_waypoint_logits, true_waypoints):
    """-> (logits [B,H,W,32], (gt_obs, gt_occ, gt_flow, origin)) of two WaypointGrids, checked against the loss's config."""
    cfg = loss_fn.config
    n = cfg.num_waypoints
    if n != 8:
        raise NotImplementedError('num_waypoints must be 8')
    pv, tv = pred_waypoint_logits.vehicles, true_waypoints.vehicles
    if len(pv.observed_occupancy) != n or len(tv.observed_occupancy) != n:
        raise ValueError('expected 8 waypoints in both grids')
    logits = getattr(pred_waypoint_logits, '_packed', None)
    if logits is None:
        logits = torch.cat([torch.cat([pv.observed_occupancy[k], pv.occluded_occupancy[k], pv.flow[k]], -1) for k in range(n)], -1)
    gt = OGMFlow_loss._ground_truth(true_waypoints)
    B, H, W, C = logits.shape
    if (H, W) != (cfg.grid_height_cells, cfg.grid_width_cells) or C != 32:
        raise ValueError(f'logits must be [B,{cfg.grid_height_cells},{cfg.grid_width_cells},32]')
    return logits, gt


def _loss_dict(loss_fn, loss):
    d = LossDict({'observed_xe': loss[0], 'occluded_xe': loss[1], 'flow': loss[2],
                  'flow_warp_xe': loss[3] if not loss_fn.no_use_warp else 0.0})
    d.total, d.packed = loss[4], loss[:4]
    return d


def eval_step(model, loss_fn, batch, loss_means=None, metrics=None, no_warp=False, scenes=None, live=None):
    """train.py:252-282 in eager form: the forward pass with training=False under no_grad, the fused loss + metrics pass, and the
    updates of train.py:275-282 -- loss_means: four Means in the order of LOSS_KEYS (valid_loss, valid_loss_occ, valid_loss_flow,
    valid_loss_warp), each given its loss x replica; metrics: an OGMFlowMetrics.  Nothing here waits for the device.
    batch: ogm, map_img, obs, occ, flow [, mapt] and gt_obs, gt_occ, gt_flow, origin_flow (or a `true_waypoints` WaypointGrids).
    scenes: a SceneScores -- the step takes the per-scene pass: every live scene's row goes into `scenes` (and comes back as
    d.scene_rows [B,12]), and the returned losses and metrics, which loss_means / metrics are updated from, are the pooled result of
    the live scenes: one pass yields the reference's numbers and the per-scene table.  live: a device int32[B], or an int k = the
    first k scenes (a last short batch in a full-size buffer); scenes that are not live are never read."""
    if live is not None and scenes is None:
        raise ValueError('eval_step: live needs a SceneScores (scenes=)')
    with torch.no_grad():
        out = model(batch['ogm'], batch['map_img'], training=False, obs=batch['obs'], occ=batch['occ'], mapt=batch.get('mapt'),
                    flow=batch['flow'])
        tw = batch.get('true_waypoints')
        if tw is None:
            tw = warpped_gt(batch['gt_obs'], batch['gt_occ'], batch['gt_flow'], batch['origin_flow'])
        if scenes is None:
            d, m = eval_loss_metrics(loss_fn, get_pred_waypoint_logits(out), tw, no_warp=no_warp)
        else:
            d, m = eval_scene_loss_metrics(loss_fn, get_pred_waypoint_logits(out), tw, scenes, live=live, no_warp=no_warp)
        d.logits = out
        if loss_means is not None:
            for mean, k in zip(loss_means, LOSS_KEYS):
                mean.update_state((d[k].double() if torch.is_tensor(d[k]) else d[k]) * loss_fn.replica)
        if metrics is not None:
            metrics.update_state(m)
    return d, m


ROW_KEYS = LOSS_KEYS + ('total',) + METRIC_KEYS          # the columns of a scene's row


def live_mask(live, B, device):
    """live as stj_eval_scenes_fwd takes it: None, a device int32[B], or an int k -> [1] * k + [0] * (B - k)."""
    if live is None or torch.is_tensor(live):
        return live
    k = int(live)
    if not 0 <= k <= B:
        raise ValueError(f'live = {k} scenes of a batch of {B}')
    return (torch.arange(B, device=device) < k).to(torch.int32)


def eval_scene_loss_metrics(loss_fn, pred_waypoint_logits, true_waypoints, scenes, live=None, no_warp=False, workspace=None, rows=None,
                            pooled_out=None):
    """eval_loss_metrics through the per-scene pass: -> (LossDict, OccupancyFlowMetrics) of the POOLED live scenes, with d.scene_rows
    [B,12] (ROW_KEYS; zeros for a dead scene); the live rows are added to `scenes` (a SceneScores) on the device."""
    logits, gt = _packed_inputs(loss_fn, pred_waypoint_logits, true_waypoints)
    if scenes.no_warp != no_warp:
        raise ValueError('eval_scene_loss_metrics: the SceneScores was made for another no_warp')
    out = ops.eval_scene_scores(logits, *gt, loss_fn.ogm_weight, loss_fn.occ_weight, loss_fn.flow_origin_weight, loss_fn.replica,
                                eval_flags(loss_fn, no_warp), live=live_mask(live, logits.shape[0], logits.device), state=scenes.state,
                                table=scenes.table if scenes.capacity else None, cursor=scenes.cursor, loss_scale=loss_fn.replica,
                                workspace=workspace, rows=rows, pooled_out=pooled_out)
    d = _loss_dict(loss_fn, out['loss'])
    d.scene_rows = out['rows']
    return d, OccupancyFlowMetrics(out['metrics'], no_warp)


class SceneScores:
    """One row per validation scene, kept on the device: a running state (per-column sums and counts), a table of the rows in the order
    the scenes were fed, and the cursor into it.  eval_step(..., scenes=) / GraphedEvalStep(per_scene=True) add to them without a host
    sync; row i of the table is the i-th live scene fed (the caller keeps the scenario ids).

        reset()           zeroes state, table and cursor
        result()          one host sync -> {preflix_<key>: mean over the scenes where the column is finite, for ROW_KEYS (the five loss
                          columns x the loss's replica, as the step's Means), 'scenes', 'nonfinite_scenes', 'dropped'}
        rows()            the host float32[min(cursor, capacity)][12], one read
        worst(k, key)     row indices, worst first: descending for a loss column ('total', LOSS_KEYS; NaN rows first), ascending for a
                          metric column (METRIC_KEYS)
        reference(...)    the NumPy statement of what the device does to state, table and cursor

    Where this departs from tf.keras.metrics.Mean: a non-finite value is added to neither the sum nor the count of its column.  A scene
    without any vehicle occupancy has every gate 0 under use_gt, and the reference's loss then divides 0 by 0 (loss.py:164,167): its
    flow, flow_warp_xe and total are NaN, and a Keras Mean would turn the whole epoch's mean into NaN.  Such scenes are counted in
    'nonfinite_scenes' instead."""

    def __init__(self, capacity, preflix='val', no_warp=False, device=None):
        self.capacity, self.preflix, self.no_warp = int(capacity), preflix, no_warp
        if self.capacity < 0:
            raise ValueError('SceneScores: capacity must not be negative')
        dev = device or _state_device()
        self.state = torch.zeros(2, 13, dtype=torch.float64, device=dev)
        self.table = torch.zeros(self.capacity, 12, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)

    def reset(self):
        self.state.zero_()
        self.table.zero_()
        self.cursor.zero_()

    def keys(self):
        return ROW_KEYS[:10] if self.no_warp else ROW_KEYS

    def result(self):
        v = torch.cat([self.state.reshape(-1), self.cursor.to(torch.float64)]).tolist()         # the one host sync
        total, count, cursor = v[:13], v[13:26], int(v[26])
        res = {f'{self.preflix}_{k}': (total[i] / count[i] if count[i] else 0.0) for i, k in enumerate(self.keys())}
        res.update(scenes=int(total[12]), nonfinite_scenes=int(count[12]), dropped=max(0, cursor - self.capacity))
        return res

    def rows(self):
        both = torch.cat([self.table.reshape(-1).view(torch.int32), self.cursor.clamp(0, self.capacity).to(torch.int32)]).cpu().numpy()    # one read
        n = int(both[-1])
        return both[:-1].view(np.float32).reshape(self.capacity, 12)[:n].copy()

    def worst(self, k, key='total'):
        r = self.rows()
        col = r[:, ROW_KEYS.index(key)].astype(np.float64)
        if key in METRIC_KEYS:
            order = np.argsort(col, kind='stable')
        else:
            order = np.argsort(np.where(np.isnan(col), -np.inf, -col), kind='stable')
        return order[:max(int(k), 0)]

    @staticmethod
    def reference(rows, live, capacity, loss_scale, state=None, table=None, cursor=0):
        """What a sequence of calls leaves behind, in NumPy: rows = per call float32 [B,12] (a dead scene's row is ignored), live = per
        call None or B flags, loss_scale = float32 -> (state float64[2,13], table float32[capacity,12], cursor).  Live scenes in batch
        order: a finite column adds row[c] (x loss_scale for c < 5, the product taken in double) to state[0][c] and 1 to state[1][c], a
        non-finite one neither; state[0][12] counts the scenes, state[1][12] those with a non-finite column; the row is stored at
        table[cursor] when cursor < capacity; the cursor advances either way."""
        state = np.zeros((2, 13), np.float64) if state is None else np.array(state, np.float64)
        table = np.zeros((int(capacity), 12), np.float32) if table is None else np.array(table, np.float32)
        cursor, scale = int(cursor), np.float64(np.float32(loss_scale))
        for call_rows, call_live in zip(rows, live):
            call_rows = np.asarray(call_rows, np.float32).reshape(-1, 12)
            for b, row in enumerate(call_rows):
                if call_live is not None and not int(call_live[b]):
                    continue
                finite = np.isfinite(row)
                for c in range(12):
                    if finite[c]:
                        state[0, c] += np.float64(row[c]) * scale if c < 5 else np.float64(row[c])
                        state[1, c] += 1.0
                state[0, 12] += 1.0
                state[1, 12] += 0.0 if finite.all() else 1.0
                if 0 <= cursor < capacity:
                    table[cursor] = row
                cursor += 1
        return state, table, cursor
