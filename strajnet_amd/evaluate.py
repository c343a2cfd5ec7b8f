"""The validation half of the reference's training loop (train.py:252-282, metrics.py:4-71).

    eval_step(model, loss_fn, batch, loss_means=None, metrics=None, no_warp=False) -> (LossDict, OccupancyFlowMetrics)
    Mean(name)                                       # tf.keras.metrics.Mean over a device tensor: update_state never syncs
    OGMFlowMetrics(preflix='train', no_warp=False)   # metrics.py:4-59: update_state(metrics) / reset_states() / get_result()
    print_metrics(res_dict, preflix='train', no_warp=False)

val_step is the forward pass with training=False, OGMFlow_loss, compute_occupancy_flow_metrics, and the update of four Keras Means
of the losses and an OGMFlowMetrics.  Here loss and metrics come out of ONE pass over the logits and the ground truth
(ops.eval_loss_metrics, csrc/eval.hip) without floating-point atomics: the same batch gives the same bits in every run.  The
captured form, with the running means kept by the pass itself, is graph.GraphedEvalStep.
"""
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
    loss, met = ops.eval_loss_metrics(logits, *gt, loss_fn.ogm_weight, loss_fn.occ_weight, loss_fn.flow_origin_weight, loss_fn.replica,
                                      eval_flags(loss_fn, no_warp), running=running, loss_scale=loss_fn.replica, workspace=workspace)
    d = LossDict({'observed_xe': loss[0], 'occluded_xe': loss[1], 'flow': loss[2],
                  'flow_warp_xe': loss[3] if not loss_fn.no_use_warp else 0.0})
    d.total, d.packed = loss[4], loss[:4]
    return d, OccupancyFlowMetrics(met, no_warp)


def eval_step(model, loss_fn, batch, loss_means=None, metrics=None, no_warp=False):
    """train.py:252-282 in eager form: the forward pass with training=False under no_grad, the fused loss + metrics pass, and the
    updates of train.py:275-282 -- loss_means: four Means in the order of LOSS_KEYS (valid_loss, valid_loss_occ, valid_loss_flow,
    valid_loss_warp), each given its loss x replica; metrics: an OGMFlowMetrics.  Nothing here waits for the device.
    batch: ogm, map_img, obs, occ, flow [, mapt] and gt_obs, gt_occ, gt_flow, origin_flow (or a `true_waypoints` WaypointGrids)."""
    with torch.no_grad():
        out = model(batch['ogm'], batch['map_img'], training=False, obs=batch['obs'], occ=batch['occ'], mapt=batch.get('mapt'),
                    flow=batch['flow'])
        tw = batch.get('true_waypoints')
        if tw is None:
            tw = warpped_gt(batch['gt_obs'], batch['gt_occ'], batch['gt_flow'], batch['origin_flow'])
        d, m = eval_loss_metrics(loss_fn, get_pred_waypoint_logits(out), tw, no_warp=no_warp)
        d.logits = out
        if loss_means is not None:
            for mean, k in zip(loss_means, LOSS_KEYS):
                mean.update_state((d[k].double() if torch.is_tensor(d[k]) else d[k]) * loss_fn.replica)
        if metrics is not None:
            metrics.update_state(m)
    return d, m
