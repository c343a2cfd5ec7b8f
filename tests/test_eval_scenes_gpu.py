"""The per-scene validation pass (stj_eval_scenes_fwd, csrc/eval.hip) through the raw C ABI on the cases of _eval_scene_cases.py:
every row against float64 on that scene alone and against stj_eval_fwd on that scene as B = 1, that a row depends on its scene alone
(bit for bit), the empty scene, `live`, the pooled result, state / table / cursor against evaluate.SceneScores.reference, repeatability,
refusals, and the captured step (graph.GraphedEvalStep(per_scene=True)) against the eager one.

Bounds, the ones tests/test_eval_gpu.py uses for this pass: losses within 3e-5 |ref| + 1e-6 and metrics within 1e-4 max(1, |ref|) of the
oracle, gates equal, column 4 the float32 sum of columns 0-3 in order.  Outputs are pre-filled with -7 and the workspace with 0xFF.
No row and no element is left out.
"""
import ctypes

import numpy as np
import pytest
import torch

import _eval_cases as EC
import _eval_scene_cases as SC

pytestmark = pytest.mark.gpu
vp = ctypes.c_void_p
CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
FILL = -7.0


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


def _ptr(t, off=0):
    return vp(0) if t is None else vp(t.data_ptr() + off)


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _tail(flags, no_warp=False, loss_scale=1.0):
    return (EC.WEIGHTS['ogm_weight'], EC.WEIGHTS['occ_weight'], EC.WEIGHTS['flow_origin_weight'], EC.REPLICA, loss_scale,
            EC.loss_flags(flags, no_warp), _stream())


_DEV = {}


def dev(case_key, arrays):
    """Arrays on the GPU, uploaded once per key and never written."""
    if case_key not in _DEV:
        _DEV[case_key] = {k: torch.from_numpy(np.array(v)).cuda() for k, v in arrays.items()}
    return _DEV[case_key]


def dev_batch(shape, empty0=False):
    return dev(('batch', tuple(shape), empty0), SC.batch_case(tuple(shape), empty0))


def dev_sub(shape, scenes, empty0=False):
    return dev(('sub', tuple(shape), tuple(scenes), empty0), SC.sub_case(shape, scenes, empty0))


def ws_bytes(B, H, W):
    from strajnet_amd import _lib
    return int(_lib.lib().stj_eval_scenes_workspace_bytes(B, H, W))


def outputs(B):
    f = lambda *s: torch.full(s, FILL, device='cuda')
    return dict(rows=f(B, 12), gate=f(B, 8), auc=f(B, 8, 4), batch_loss=f(5), batch_metrics=f(7), batch_gate=f(8), batch_auc=f(8, 4))


def run_scenes(c, flags, no_warp=False, live=None, ws=None, state=None, table=None, cursor=None, capacity=None, loss_scale=1.0, out=None,
               check=True):
    """stj_eval_scenes_fwd on device arrays c -> dict of host arrays (rows, gate, auc, batch_*)."""
    from strajnet_amd import _lib
    B, H, W = c['logits'].shape[:3]
    if ws is None:
        ws = torch.full((ws_bytes(B, H, W),), 0xFF, dtype=torch.uint8, device='cuda')
    out = out or outputs(B)
    lv = None if live is None else torch.tensor(list(live), dtype=torch.int32, device='cuda')
    if capacity is None:
        capacity = 0 if table is None else table.shape[0]
    args = (_ptr(c['logits']), *(_ptr(c[k]) for k in EC.GT_KEYS), _ptr(lv), _ptr(ws), _ptr(out['rows']), _ptr(out['gate']), _ptr(out['auc']),
            _ptr(out['batch_loss']), _ptr(out['batch_metrics']), _ptr(out['batch_gate']), _ptr(out['batch_auc']), _ptr(state), _ptr(table),
            _ptr(cursor), int(capacity), B, H, W, *_tail(flags, no_warp, loss_scale))
    if check:
        _lib.call('stj_eval_scenes_fwd', *args)
    else:
        return _lib.lib().stj_eval_scenes_fwd(*args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_fwd(c, flags, no_warp=False):
    """stj_eval_fwd on device arrays c -> loss[5], metrics[7], gate[8], auc[8,4] on the host."""
    from strajnet_amd import _lib
    B, H, W = c['logits'].shape[:3]
    ws = torch.empty(int(_lib.lib().stj_eval_workspace_bytes(B, H, W)), dtype=torch.uint8, device='cuda')
    out = dict(loss=torch.full((5,), FILL, device='cuda'), metrics=torch.full((7,), FILL, device='cuda'),
               gate=torch.full((8,), FILL, device='cuda'), auc=torch.full((8, 4), FILL, device='cuda'))
    _lib.call('stj_eval_fwd', _ptr(c['logits']), *(_ptr(c[k]) for k in EC.GT_KEYS), _ptr(ws), _ptr(out['loss']), _ptr(out['metrics']),
              _ptr(out['gate']), _ptr(out['auc']), vp(0), B, H, W, *_tail(flags, no_warp))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32_total(row):
    return float(np.float32(np.float32(np.float32(row[0] + row[1]) + row[2]) + row[3]))


def check_row(row, ref, what, total=True):
    """One row float32[12] against the oracle's float64[12]: same NaN pattern, the bounds of the module docstring elsewhere."""
    print(f'{what}: got {row.tolist()} / ref {ref.tolist()}')
    assert np.isnan(row).tolist() == np.isnan(ref).tolist(), what
    for i in range(4):
        if not np.isnan(ref[i]):
            assert abs(float(row[i]) - ref[i]) <= 3e-5 * abs(ref[i]) + 1e-6, (what, SC.ROW_KEYS[i], float(row[i]), ref[i])
    if total:
        want = f32_total(row)
        assert (np.isnan(want) and np.isnan(row[4])) or float(row[4]) == want, (what, float(row[4]), want)
    for i in range(5, 12):
        assert abs(float(row[i]) - ref[i]) <= 1e-4 * max(1.0, abs(ref[i])), (what, SC.ROW_KEYS[i], float(row[i]), ref[i])


def check_rows(got, shape, flags, no_warp=False, empty0=False):
    ref, gates = SC.ref_rows(shape, flags, no_warp, empty0)
    assert got['rows'].shape == ref.shape
    for b in range(shape[0]):
        assert got['gate'][b].tolist() == list(gates[b]), (shape, b)
        check_row(got['rows'][b], ref[b], f'{shape} scene {b} {flags} no_warp={no_warp}')
    assert not (got['auc'] == FILL).any() and not (got['gate'] == FILL).any()


@pytest.mark.parametrize('flags', [EC.TRAIN, EC.DEFAULTS], ids=['train', 'defaults'])
@pytest.mark.parametrize('shape', SC.SHAPES)
def test_rows_against_float64(shape, flags):
    from strajnet_amd import _lib
    got = run_scenes(dev_batch(shape), flags)
    check_rows(got, shape, flags)
    if shape == (1, 72, 64):
        G = _lib.lib().stj_eval_scenes_grid(72, 64)
        assert 0 < G < 72 * 64 * 8 // 512 == 72                    # the stride path ran: fewer workgroups than 512-item pieces


@pytest.mark.parametrize('flags', EC.EXTRA, ids=['use_pred', 'no_use_warp', 'no_use_gt'])
def test_rows_against_float64_other_flags(flags):
    shape = SC.SHAPES[1]
    got = run_scenes(dev_batch(shape), flags)
    check_rows(got, shape, flags)
    if flags['no_use_warp']:
        assert (got['rows'][:, 3] == 0.0).all()


def test_rows_against_float64_no_warp_metric():
    shape = SC.SHAPES[2]
    got = run_scenes(dev_batch(shape), EC.TRAIN, no_warp=True)
    check_rows(got, shape, EC.TRAIN, no_warp=True)
    assert (got['rows'][:, 10:] == 0.0).all() and (got['auc'][:, :, 3] == 0.0).all()


def _err(v, r):
    return abs(float(v) - r) / abs(r) if r != 0 else abs(float(v))


@pytest.mark.parametrize('flags', [EC.TRAIN, EC.DEFAULTS], ids=['train', 'defaults'])
@pytest.mark.parametrize('shape', SC.SHAPES)
def test_against_eval_fwd_on_each_scene_alone(shape, flags):
    """Same per-item function, same histograms: gate and auc are EQUAL to stj_eval_fwd's on the scene as a batch of one, and every float
    is never further from float64 than twice stj_eval_fwd's error (floor 1e-6), the rule of test_against_the_launches_it_replaces."""
    got = run_scenes(dev_batch(shape), flags)
    ref, _ = SC.ref_rows(shape, flags)
    for b in range(shape[0]):
        one = run_fwd(dev_sub(shape, (b,)), flags)
        assert np.array_equal(got['gate'][b], one['gate']) and np.array_equal(got['auc'][b], one['auc']), (shape, b)
        theirs = np.concatenate([one['loss'], one['metrics']])
        for i in range(12):
            es, ef = _err(got['rows'][b, i], ref[b, i]), _err(theirs[i], ref[b, i])
            print(f'{shape} scene {b} {SC.ROW_KEYS[i]}: err scenes {es:.3e} eval_fwd {ef:.3e}')
            assert es <= max(2.0 * ef, 1e-6), (shape, b, SC.ROW_KEYS[i], es, ef)


def test_a_row_depends_on_its_scene_alone():
    shape = SC.SHAPES[2]
    B = shape[0]
    full = run_scenes(dev_batch(shape), EC.TRAIN)
    rev = run_scenes(dev_sub(shape, range(B - 1, -1, -1)), EC.TRAIN)
    for b in range(B):
        alone = run_scenes(dev_sub(shape, (b,)), EC.TRAIN)
        for k in ('rows', 'gate', 'auc'):
            assert np.array_equal(bits(full[k][b]), bits(alone[k][0])), (k, b)
            assert np.array_equal(bits(full[k][b]), bits(rev[k][B - 1 - b])), (k, b)
    assert len({full['rows'][b].tobytes() for b in range(B)}) == B
    # and with a NaN row in the batch: the empty scene alone, first of three, last of three
    shape = SC.EMPTY_SHAPE
    full = run_scenes(dev_batch(shape, True), EC.TRAIN)
    assert np.isnan(full['rows'][0]).any()
    alone = run_scenes(dev_sub(shape, (0,), True), EC.TRAIN)
    last = run_scenes(dev_sub(shape, (2, 1, 0), True), EC.TRAIN)
    assert np.array_equal(bits(full['rows'][0]), bits(alone['rows'][0])) and np.array_equal(bits(full['rows'][0]), bits(last['rows'][2]))
    assert np.array_equal(bits(full['rows'][1:]), bits(last['rows'][1::-1]))


def test_empty_scene():
    shape = SC.EMPTY_SHAPE
    state = torch.zeros(2, 13, dtype=torch.float64, device='cuda')
    got = run_scenes(dev_batch(shape, True), EC.TRAIN, state=state)
    check_rows(got, shape, EC.TRAIN, empty0=True)
    assert np.isnan(got['rows'][0]).tolist() == [False, False, True, True, True] + [False] * 7
    assert got['gate'][0].tolist() == [0.0] * 8
    s = state.cpu().numpy()
    assert s[1, :12].tolist() == [3.0, 3.0, 2.0, 2.0, 2.0] + [3.0] * 7
    assert s[0, 12] == 3.0 and s[1, 12] == 1.0 and np.isfinite(s).all()
    check_rows(run_scenes(dev_batch(shape, True), EC.DEFAULTS), shape, EC.DEFAULTS, empty0=True)     # no use_gt: nothing is NaN


def _poisoned(shape, dead):
    """The batch with the dead scenes' inputs overwritten: NaN in the logits and the flow, 1e30 in the occupancies and the origin."""
    c = {k: v.copy() for k, v in SC.batch_case(tuple(shape)).items()}
    for b in dead:
        c['logits'][b] = np.nan
        c['gt_flow'][b] = np.nan
        for k in ('gt_obs', 'gt_occ', 'origin_flow'):
            c[k][b] = 1e30
    return {k: torch.from_numpy(v).cuda() for k, v in c.items()}


def test_live():
    shape = SC.SHAPES[2]
    plain = run_scenes(dev_batch(shape), EC.TRAIN)
    state = torch.zeros(2, 13, dtype=torch.float64, device='cuda')
    cursor = torch.full((1,), 5, dtype=torch.int64, device='cuda')
    got = run_scenes(_poisoned(shape, (1,)), EC.TRAIN, live=(1, 0, 1), state=state, cursor=cursor)
    for k in ('rows', 'gate', 'auc'):
        assert np.array_equal(bits(got[k][[0, 2]]), bits(plain[k][[0, 2]])), k
        assert (got[k][1] == 0.0).all(), k
    s = state.cpu().numpy()
    assert s[0, 12] == 2.0 and s[1, 12] == 0.0 and s[1, :12].tolist() == [2.0] * 12 and int(cursor.item()) == 7
    assert np.isfinite(np.concatenate([got[k].ravel() for k in got])).all()          # nothing of the dead scene reached any output
    # every scene dead: nothing is added, the cursor stays, rows and the pooled outputs are zeros (the header's empty pool)
    before = state.clone()
    none = run_scenes(_poisoned(shape, (0, 1, 2)), EC.TRAIN, live=(0, 0, 0), state=state, cursor=cursor)
    assert torch.equal(state, before) and int(cursor.item()) == 7
    for k, v in none.items():
        assert (v == 0.0).all(), k


def check_pooled(got, shape, scenes, flags):
    ref, gates = SC.ref_pooled(shape, scenes, flags)
    fwd = run_fwd(dev_sub(shape, scenes), flags)
    assert np.array_equal(got['batch_gate'], fwd['gate']) and np.array_equal(got['batch_auc'], fwd['auc'])
    assert got['batch_gate'].tolist() == list(gates)
    check_row(np.concatenate([got['batch_loss'], got['batch_metrics']]), ref, f'{shape} pooled {tuple(scenes)}')


@pytest.mark.parametrize('shape', SC.SHAPES)
def test_pooled_result(shape):
    got = run_scenes(dev_batch(shape), EC.TRAIN)
    check_pooled(got, shape, range(shape[0]), EC.TRAIN)


def test_pooled_result_of_the_live_scenes():
    shape = SC.SHAPES[2]
    got = run_scenes(_poisoned(shape, (1,)), EC.TRAIN, live=(1, 0, 1))
    check_pooled(got, shape, (0, 2), EC.TRAIN)
    got = run_scenes(dev_batch(shape), EC.DEFAULTS, live=(0, 0, 1))
    check_pooled(got, shape, (2,), EC.DEFAULTS)


def test_state_and_table_over_three_calls():
    from strajnet_amd.evaluate import SceneScores
    shape, capacity, guard = SC.EMPTY_SHAPE, 5, 64
    scale = np.float32(EC.REPLICA)
    calls = [(True, None), (False, (0, 0, 0)), (False, (1, 0, 1)), (False, None)]     # 3 live (one with NaNs), 0, 2, 3: 8 rows for 5 slots
    state = torch.zeros(2, 13, dtype=torch.float64, device='cuda')
    cursor = torch.zeros(1, dtype=torch.int64, device='cuda')
    buf = torch.full((capacity * 12 + guard,), FILL, device='cuda')
    table = buf[:capacity * 12].view(capacity, 12)
    rows = []
    for empty0, live in calls:
        got = run_scenes(dev_batch(shape, empty0), EC.TRAIN, live=live, state=state, table=table, cursor=cursor, loss_scale=float(scale))
        rows.append(got['rows'])
    want_state, want_table, want_cursor = SceneScores.reference(rows, [lv for _, lv in calls], capacity, scale,
                                                                table=np.full((capacity, 12), FILL, np.float32))
    assert want_cursor == 8 and int(cursor.item()) == 8
    assert state.cpu().numpy().tobytes() == want_state.tobytes()
    assert np.array_equal(bits(table.cpu().numpy()), bits(want_table))
    assert bool((buf[capacity * 12:] == FILL).all())                          # the guard behind the table
    assert want_state[0, 12] == 8.0 and want_state[1, 12] == 1.0
    # capacity 0 with a table pointer: nothing is stored, the cursor counts
    cursor.zero_()
    before = buf.clone()
    run_scenes(dev_batch(shape), EC.TRAIN, table=buf[capacity * 12:], cursor=cursor, capacity=0)
    from strajnet_amd import _lib
    c = dev_batch(shape)
    out = outputs(3)
    ws = torch.empty(ws_bytes(*shape), dtype=torch.uint8, device='cuda')
    _lib.call('stj_eval_scenes_fwd', _ptr(c['logits']), *(_ptr(c[k]) for k in EC.GT_KEYS), vp(0), _ptr(ws), _ptr(out['rows']), vp(0), vp(0),
              vp(0), vp(0), vp(0), vp(0), vp(0), _ptr(buf, capacity * 48), _ptr(cursor), 0, *shape, *_tail(EC.TRAIN))
    torch.cuda.synchronize()
    assert int(cursor.item()) == 6 and torch.equal(buf.view(torch.int32), before.view(torch.int32))      # by bits: the table holds NaNs


def test_bitwise_repeatable_whatever_the_workspace_held():
    shape, other = SC.SHAPES[2], SC.SHAPES[1]
    n, pad = ws_bytes(*shape), 4096
    assert n >= ws_bytes(*other) and n % 16 == 0
    buf = torch.full((n + pad,), 0xFF, dtype=torch.uint8, device='cuda')
    buf[n:] = 0xA5
    first = run_scenes(dev_batch(shape), EC.TRAIN, ws=buf, live=(1, 0, 1))
    run_scenes(dev_batch(other), EC.DEFAULTS, ws=buf)                       # another case's histograms and sums are left behind
    second = run_scenes(dev_batch(shape), EC.TRAIN, ws=buf, live=(1, 0, 1))
    third = run_scenes(dev_batch(shape), EC.TRAIN, ws=torch.zeros(n, dtype=torch.uint8, device='cuda'), live=(1, 0, 1))
    for k in first:
        assert first[k].tobytes() == second[k].tobytes() == third[k].tobytes(), k
        assert not (first[k] == FILL).any(), k
    assert bool((buf[n:] == 0xA5).all())


def test_refusals():
    from strajnet_amd import _lib, ops
    L = _lib.lib()
    EINVAL = _lib.ENUMS['stj_status']['STJ_EINVAL']
    shape = SC.SHAPES[0]
    c = dev_batch(shape)
    B, H, W = shape
    ws = torch.full((ws_bytes(*shape) + 16,), 0xFF, dtype=torch.uint8, device='cuda')
    out = outputs(B)
    state = torch.full((27,), 3.0, dtype=torch.float64, device='cuda')
    cursor = torch.full((2,), 4, dtype=torch.int64, device='cuda')
    table = torch.full((4, 12), FILL, device='cuda')
    odd = torch.zeros(c['logits'].numel() + 4, device='cuda')
    oddf = torch.zeros(c['gt_flow'].numel() + 2, device='cuda')

    def call(logits=None, flow=None, wsp=None, st=_ptr(state), tb=_ptr(table), cu=_ptr(cursor), cap=4, b=B, flags=None):
        tail = list(_tail(EC.TRAIN))
        if flags is not None:
            tail[5] = flags
        return L.stj_eval_scenes_fwd(logits or _ptr(c['logits']), _ptr(c['gt_obs']), _ptr(c['gt_occ']), flow or _ptr(c['gt_flow']),
                                     _ptr(c['origin_flow']), vp(0), wsp or _ptr(ws), _ptr(out['rows']), _ptr(out['gate']), _ptr(out['auc']),
                                     _ptr(out['batch_loss']), _ptr(out['batch_metrics']), _ptr(out['batch_gate']), _ptr(out['batch_auc']),
                                     st, tb, cu, cap, b, H, W, *tail)
    refused = [(dict(logits=_ptr(odd, 4)), b'logits must be 16-byte'), (dict(flow=_ptr(oddf, 4)), b'gt_flow must be 8-byte'),
               (dict(wsp=_ptr(ws, 8)), b'workspace must be 16-byte'), (dict(st=_ptr(state, 4)), b'state must be 8-byte'),
               (dict(cu=_ptr(cursor, 4)), b'cursor must be 8-byte'), (dict(flags=32), b'unknown flag bits'), (dict(cap=-1), b'negative'),
               (dict(cu=vp(0)), b'needs a cursor'), (dict(b=65535), b'scenes per call')]
    for kw, msg in refused:
        assert call(**kw) == EINVAL and msg in L.stj_last_error(), (kw, L.stj_last_error())
    assert call(b=0) == 0                                   # B = 0: STJ_OK, nothing launched or written
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == FILL).all()), k
    assert bool((state == 3.0).all()) and bool((cursor == 4).all()) and bool((table == FILL).all()) and bool((ws == 0xFF).all())
    assert call() == 0                                      # and the same call without any of the faults goes through
    torch.cuda.synchronize()
    assert int(cursor[0]) == 7 and not bool((out['rows'] == FILL).any())
    cpu = {k: v.cpu() for k, v in c.items()}
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.eval_scene_scores(cpu['logits'], *(cpu[k] for k in EC.GT_KEYS), 1000.0, 1000.0, 1000.0, 1.0, 9)
    with pytest.raises(ValueError):
        ops.eval_scene_scores(c['logits'][..., :16], *(c[k] for k in EC.GT_KEYS), 1000.0, 1000.0, 1000.0, 1.0, 9)
    with pytest.raises(ValueError):
        ops.eval_scene_scores(c['logits'], *(c[k] for k in EC.GT_KEYS), 1000.0, 1000.0, 1000.0, 1.0, 9, live=torch.ones(B, device='cuda'))


def test_ops_binding_and_eval_step_on_the_cases():
    """ops.eval_scene_scores / evaluate.eval_step(scenes=, live=) against the raw ABI on a case (the "model" hands back the logits)."""
    from strajnet_amd import Mean, OGMFlowMetrics, OGMFlow_loss, OccupancyFlowTaskConfig, SceneScores, eval_step
    from strajnet_amd.evaluate import LOSS_KEYS
    shape = SC.SHAPES[2]
    B, H, W = shape
    c = dev_batch(shape)
    raw = run_scenes(c, EC.TRAIN, live=(1, 1, 0))

    class Replay:
        def __call__(self, ogm, map_img, training=True, **kw):
            assert training is False and not torch.is_grad_enabled()
            return ogm
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(H, W, 8), replica=EC.REPLICA, **EC.WEIGHTS, **EC.TRAIN)
    scores = SceneScores(4, 'val')
    means, om = [Mean(k) for k in LOSS_KEYS], OGMFlowMetrics('val')
    batch = dict(ogm=c['logits'], map_img=None, obs=None, occ=None, flow=None, **{k: c[k] for k in EC.GT_KEYS})
    d, m = eval_step(Replay(), loss_fn, batch, loss_means=means, metrics=om, scenes=scores, live=2)
    assert np.array_equal(bits(d.scene_rows.cpu().numpy()), bits(raw['rows']))
    assert d.packed.cpu().numpy().tobytes() == raw['batch_loss'][:4].tobytes() and float(d.total) == float(raw['batch_loss'][4])
    assert m.values.cpu().numpy().tobytes() == raw['batch_metrics'].tobytes()
    assert float(means[2].result()) == float(np.float64(raw['batch_loss'][2]) * EC.REPLICA)
    d2, _ = eval_step(Replay(), loss_fn, batch, scenes=scores)                     # all three: five rows fed into four slots
    res = scores.result()
    assert (res['scenes'], res['nonfinite_scenes'], res['dropped']) == (5, 0, 1)
    got = scores.rows()
    full = d2.scene_rows.cpu().numpy()
    assert got.shape == (4, 12) and np.array_equal(bits(got), bits(np.concatenate([raw['rows'][:2], full[:2]])))
    want, _, _ = SceneScores.reference([raw['rows'], full], [(1, 1, 0), None], 4, np.float32(EC.REPLICA))
    assert scores.state.cpu().numpy().tobytes() == want.tobytes()
    assert abs(res['val_flow'] - want[0, 2] / 5) <= 1e-12 * abs(want[0, 2])
    assert list(scores.worst(2, 'flow')) == list(np.argsort(-got[:, 2].astype(np.float64), kind='stable')[:2])
    with pytest.raises(ValueError):
        eval_step(Replay(), loss_fn, batch, live=2)


def test_captured_per_scene_step_equals_the_eager_step_bitwise():
    """CFG128, B = 2: GraphedEvalStep(per_scene=True, capacity=8) replays a full batch, then a batch of ONE scene (live = 1) -- rows,
    state, table and pooled numbers equal evaluate.eval_step(..., scenes=, live=) bit for bit, the short batch's do not change when the
    stale second slot holds NaN, and GraphedEvalStep() without per_scene gives what eval_step gives, as before."""
    from strajnet_amd import STrajNet, OGMFlow_loss, OccupancyFlowTaskConfig, SceneScores, eval_step
    from strajnet_amd.graph import GraphedEvalStep
    from oracle import np_ref
    w = np_ref.make_weights(CFG128, 0)
    x = np_ref.make_inputs(CFG128, 2)
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float32)
    model.load_weights(w)
    b1 = {k: torch.from_numpy(v.copy()).cuda() for k, v in x.items()}
    b2 = {k: torch.roll(v, 1, 0).contiguous() for k, v in b1.items()}
    b2['gt_flow'] = b2['gt_flow'] * 0.5
    short = {k: v[:1].contiguous() for k, v in b2.items()}
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(128, 128, 8), replica=2.0, use_focal_loss=False, use_gt=True)
    # eager: the full batch, then b2's first scene in a full-size buffer whose second slot still holds b1's
    scores = SceneScores(8)
    stale = {k: torch.cat([short[k], b1[k][1:]]) for k in b1}
    eager = []
    for b, live in ((b1, None), (stale, 1)):
        d, m = eval_step(model, loss_fn, b, scenes=scores, live=live)
        eager.append((d.scene_rows.clone(), d.packed.clone(), m.values.clone()))
    assert bool((eager[1][0][1] == 0).all()) and bool(torch.isfinite(eager[1][0][0]).all())
    step = GraphedEvalStep(model, loss_fn, b1, per_scene=True, capacity=8)
    assert step.scores.result()['scenes'] == 0 and step.result()['flow'] == 0.0        # the warm-up steps are in no state
    for b, (rows, ls, mt) in zip((b1, short), eager):
        losses, metrics = step(b)
        assert torch.equal(step.scene_rows, rows) and torch.equal(losses, ls) and torch.equal(metrics, mt)
    assert step.live.tolist() == [1, 0]
    assert torch.equal(step.scores.state, scores.state) and torch.equal(step.scores.table, scores.table)
    assert int(step.scores.cursor) == int(scores.cursor) == 3
    assert step.scores.result() == scores.result() and step.scores.result()['scenes'] == 3
    res = step.result()
    for i, k in enumerate(('observed_xe', 'occluded_xe', 'flow', 'flow_warp_xe')):
        want = (float(eager[0][1][i]) + float(eager[1][1][i])) * 2.0 / 2
        assert abs(res[k] - want) <= 1e-12 * abs(want), (k, res[k], want)
    assert float(step.running[0]) == 2.0
    # the stale second slot of everything the pass would read filled with NaN: the short batch's results do not move (the model's own
    # inputs keep their stale scene: its forward runs on all B slots, and slot 1's logits are then never read)
    for k in ('gt_obs', 'gt_occ', 'gt_flow', 'origin_flow'):
        step.static[k][1:].fill_(float('nan'))
    losses, metrics = step(short, live=1)
    assert torch.equal(step.scene_rows[0], eager[1][0][0]) and bool((step.scene_rows[1] == 0).all())
    assert int(step.scores.cursor) == 4 and torch.equal(step.scores.table[3], eager[1][0][0])
    step.reset()
    assert step.scores.result()['scenes'] == 0 and float(step.running[0]) == 0.0
    del step
    # without per_scene: the class as it was
    plain = GraphedEvalStep(model, loss_fn, b1)
    d, m = eval_step(model, loss_fn, b1)
    losses, metrics = plain(b1)
    assert torch.equal(losses, d.packed) and torch.equal(metrics, m.values) and not hasattr(plain, 'scores')
    with pytest.raises(ValueError):
        plain(b1, live=1)
    del plain
