"""What the cases of _eval_cases.py exercise, stated from the float64 oracle alone (no GPU), and the host-side names of the validation
step (strajnet_amd/evaluate.py: print_metrics, OGMFlowMetrics) against the reference's (metrics.py:4-71)."""
import numpy as np
import pytest

import _eval_cases as EC
from oracle import np_ref

# metrics.py:46-59 (get_result) and :61-71 (print_metrics): the keys behind the prefix, and the labels printed in front of the values
REF_KEYS = ('observed_auc', 'occluded_auc', 'observed_iou', 'occluded_iou', 'flow_epe', 'flow_ogm_auc', 'flow_ogm_iou')
REF_LABELS = ('obs-AUC', 'occ-AUC', 'obs-IOU', 'occ-IOU', 'Flow-EPE', 'FlowOGM_AUC', 'FlowOGM_IOU')


@pytest.mark.parametrize('shape', EC.SHAPES)
def test_cases_exercise_what_they_claim(shape):
    B, H, W = shape
    c = EC.make_case(*shape)
    losses, gates = EC.ref_loss(shape, EC.TRAIN)
    assert list(gates) == [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]                  # both values; waypoint 3 is gated off
    assert all(np.isfinite(v) and v > 0 for v in losses)
    m = EC.ref_metrics(shape)
    assert all(np.isfinite(v) and v != 0 for v in m)
    m0 = EC.ref_metrics(shape, no_warp=True)
    assert m0[5] == 0.0 and m0[6] == 0.0 and m0[:5] == m[:5]
    gf = c['gt_flow'].astype(np.float64)
    exists = (gf[..., 0] != 0) | (gf[..., 1] != 0)
    counts = exists.sum(axis=(0, 2, 3))
    assert counts[5] == 0 and all(counts[k] > 0 for k in range(8) if k != 5)     # waypoint 5: the flow term's and the EPE's 0 / 0
    assert 0.2 < exists[:, [0, 1, 2, 3, 4, 6, 7]].mean() < 0.4                   # ~70 % of the pixels carry no true flow
    # the predicted flow is on the 1/16-offset lattice, the true flow on the 1/8 lattice
    pf = c['logits'].reshape(B, H, W, 8, 4)[..., 2:].astype(np.float64)
    assert np.array_equal(pf * 8 - 0.5, np.round(pf * 8 - 0.5)) and np.array_equal(gf * 8, np.round(gf * 8))
    # warp targets leave the image on all four sides, and some stay inside
    xs, ys = np.arange(W)[None, None, :, None], np.arange(H)[None, :, None, None]
    tx, ty = xs + pf[..., 0], ys + pf[..., 1]
    assert (tx < 0).any() and (tx > W - 1).any() and (ty < 0).any() and (ty > H - 1).any()
    assert ((tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)).any()
    # every AUC histogram has both classes -- but for waypoint 3's three ground-truth labelled ones, empty of positives by construction
    ident = np.stack(np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing='xy'), -1)[None]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    y = c['logits'].astype(np.float64)
    for k in range(8):
        to, tc, org = (c[n].astype(np.float64)[:, k] for n in ('gt_obs', 'gt_occ', 'origin_flow'))
        ta = np.clip(to + tc, 0, 1)
        grounded = np.clip(sig(y[..., 4 * k:4 * k + 1]) + sig(y[..., 4 * k + 1:4 * k + 2]), 0, 1) * np_ref.sample(org, ident + pf[..., k, :])
        labels = dict(gate=ta != 0, observed=to != 0, occluded=tc != 0, warped=grounded != 0)
        for name, lab in labels.items():
            if k == 3 and name != 'warped':
                assert not lab.any()
            else:
                assert lab.any() and not lab.all(), (k, name)


def test_flag_words():
    assert EC.loss_flags(EC.TRAIN) == 1 | 8 and EC.loss_flags(EC.DEFAULTS) == 1 | 2
    assert [EC.loss_flags(f) for f in EC.EXTRA] == [1 | 4 | 8, 8, 1]
    assert EC.loss_flags(EC.TRAIN, no_warp=True) == 1 | 8 | 16


@pytest.mark.parametrize('no_warp', [False, True])
def test_metric_names_are_the_references(no_warp, capsys):
    from strajnet_amd import OGMFlowMetrics, print_metrics
    from strajnet_amd.evaluate import METRIC_KEYS
    assert METRIC_KEYS == REF_KEYS
    n = 5 if no_warp else 7
    m = OGMFlowMetrics(preflix='val', no_warp=no_warp, device='cpu')
    res = m.get_result()
    assert list(res) == [f'val_{k}' for k in REF_KEYS[:n]]
    assert all(v == 0.0 for v in res.values())                        # nothing added yet: divide_no_nan
    for k in REF_KEYS[:n]:                                            # the per-field members train.py:330 reads
        assert float(getattr(m, k).result()) == 0.0
    assert hasattr(m, 'flow_ogm_auc') == (not no_warp)
    vals = {f'val_{k}': (i + 1) / 8 for i, k in enumerate(REF_KEYS)}
    print_metrics(vals, 'val', no_warp)
    out = capsys.readouterr().out
    for i, (lab, k) in enumerate(zip(REF_LABELS, REF_KEYS)):
        assert (f'{lab}: {vals["val_" + k]}' in out) == (i < n), (lab, out)
    assert OGMFlowMetrics(device='cpu').preflix == 'train'


def test_mean_is_keras_mean_on_the_host_too():
    from strajnet_amd import Mean
    m = Mean('valid_loss', device='cpu')
    assert m.name == 'valid_loss' and float(m.result()) == 0.0
    for v in (1.0, 2.5, 4.0):
        m.update_state(v)
    assert float(m.result()) == 2.5
    m.reset_states()
    assert float(m.result()) == 0.0
