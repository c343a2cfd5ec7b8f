"""The training half of the reference's epoch loop (train.py:199-230) in eager form; graph.GraphedTrainStep(optimizer=) is the captured one.

    train_step(model, loss_fn, optimizer, batch, sync=None) -> the model's outputs [B,H,W,32]

zero_grad, the forward pass with training=True, OGMFlow_loss, backward, the data-parallel gradient SUM (MirroredStrategy's all-reduce
inside apply_gradients), optimizer.step(), and -- with an optim.DeviceNadam whose loss means are attached -- the update of the four
train-loss means of train.py:226-229, which that optimizer's prepare launch does itself.  Nothing here waits for the device.
"""
from . import dp
from .loss import get_pred_waypoint_logits, warpped_gt


def train_step(model, loss_fn, optimizer, batch, sync=None):
    """batch: ogm, map_img, obs, occ, flow [, mapt] and gt_obs, gt_occ, gt_flow, origin_flow (or a `true_waypoints` WaypointGrids).
    sync: a dp.OverlappedGradSync over `model` (model.cut_encoder must be True): the tail bucket's all-reduce runs under the encoder's
    backward.  Without one, a process group of more than one rank all-reduces the whole flat gradient after backward."""
    if sync is not None and not model.cut_encoder:
        raise ValueError('train_step: a dp.OverlappedGradSync needs model.cut_encoder = True (backward stops at the encoder outputs)')
    model.zero_grad()
    tw = batch.get('true_waypoints')
    if tw is None:
        tw = warpped_gt(batch['gt_obs'], batch['gt_occ'], batch['gt_flow'], batch['origin_flow'])
    out = model(batch['ogm'], batch['map_img'], training=True, obs=batch['obs'], occ=batch['occ'], mapt=batch.get('mapt'), flow=batch['flow'])
    d = loss_fn(get_pred_waypoint_logits(out), tw, None)
    d.total.backward()                       # observed_xe + occluded_xe + flow + flow_warp_xe (train.py:221)
    if sync is not None:
        sync.tail()
        model.backward_encoder()
        sync.head_and_wait()
    elif dp.world() > 1:
        dp.allreduce_flat_grads(model.flat_grads())
    if getattr(optimizer, 'loss_scale', None) is not None:
        optimizer.attach_loss_means(d.packed, optimizer.loss_scale)
    optimizer.step()
    return out

