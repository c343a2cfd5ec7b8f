"""The per-scene validation scores, stated without a GPU: what the float64 oracle says about the cases of _eval_scene_cases.py (why the
feature exists: the pooled numbers are not the mean of the scenes'; what an empty scene gives), the NumPy statement of the running
state, the score table and the cursor (evaluate.SceneScores.reference), and csrc/eval_scene.h compiled for the host against it."""
import os
import subprocess

import numpy as np
import pytest

import _eval_cases as EC
import _eval_scene_cases as SC
from test_deflate_dyn import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FLAGS = (EC.TRAIN, EC.DEFAULTS) + EC.EXTRA


@pytest.mark.parametrize('shape', SC.SHAPES)
def test_every_scene_row_is_finite(shape):
    for flags in ALL_FLAGS:
        rows, gates = SC.ref_rows(shape, flags)
        assert rows.shape == (shape[0], 12) and np.isfinite(rows).all(), (shape, flags)
        assert all(len(g) == 8 for g in gates)
    assert np.isfinite(SC.ref_rows(shape, EC.TRAIN, no_warp=True)[0]).all()


def test_the_pooled_value_is_not_the_mean_of_the_scenes():
    shape = SC.SHAPES[0]
    rows, _ = SC.ref_rows(shape, EC.TRAIN)
    pooled, _ = SC.ref_pooled(shape, range(shape[0]), EC.TRAIN)
    assert pooled[:4].tolist() == list(EC.ref_loss(shape, EC.TRAIN)[0])               # the pooled row IS the existing reference
    flow = SC.ROW_KEYS.index('flow')
    mean = rows[:, flow].mean()
    print('flow per scene', rows[:, flow], 'mean', mean, 'pooled', pooled[flow])
    assert abs(mean - pooled[flow]) > 1e-3 * abs(pooled[flow])
    # a single scene's row is the pooled oracle of that scene alone, whichever way it is asked for
    one, _ = SC.ref_pooled((1, 72, 64), (0,), EC.TRAIN)
    assert one.tolist() == SC.ref_rows((1, 72, 64), EC.TRAIN)[0][0].tolist()
    assert one[:4].tolist() == list(EC.ref_loss((1, 72, 64), EC.TRAIN)[0])


def test_the_empty_scene():
    shape = SC.EMPTY_SHAPE
    c = SC.batch_case(shape, True)
    assert not c['gt_obs'][0].any() and not c['gt_occ'][0].any() and c['gt_obs'][1].any()
    rows, gates = SC.ref_rows(shape, EC.TRAIN, empty0=True)
    assert gates[0] == (0.0,) * 8 and sum(gates[1]) == 7.0
    nan = np.isnan(rows[0])
    assert [k for k, n in zip(SC.ROW_KEYS, nan) if n] == ['flow', 'flow_warp_xe', 'total']      # the two terms, and with them their sum
    assert np.isfinite(rows[0][~nan]).all() and np.isfinite(rows[1:]).all()
    assert np.array_equal(rows[1:], SC.ref_rows(shape, EC.TRAIN)[0][1:])                        # the other scenes are what they were
    rows_d, _ = SC.ref_rows(shape, EC.DEFAULTS, empty0=True)
    assert np.isfinite(rows_d).all()                                                            # no use_gt: every gate 1


def _calls():
    """Three calls on a table of 5 rows: 3 live of 3 (one row with NaNs), none live of 2, 3 live of 4 (the table overflows by one)."""
    rng = np.random.default_rng(5)
    rows = [rng.normal(0, 3, (B, 12)).astype(np.float32) for B in (3, 2, 4)]
    rows[0][1, [2, 3, 4]] = np.nan
    rows[2][3, 7] = np.inf
    rows[1][:] = np.nan                           # dead rows: whatever they hold is ignored
    live = [None, [0, 0], [1, 0, 1, 1]]
    return rows, live


def test_scene_scores_reference():
    from strajnet_amd.evaluate import SceneScores
    rows, live = _calls()
    scale = np.float32(2.0)
    state, table, cursor = SceneScores.reference(rows, live, 5, scale)
    fed = [rows[0][0], rows[0][1], rows[0][2], rows[2][0], rows[2][2], rows[2][3]]              # append order = batch order of the live
    assert cursor == 6 and max(0, cursor - 5) == 1
    assert table.shape == (5, 12) and table.dtype == np.float32
    assert table.tobytes() == np.stack(fed[:5]).tobytes()                                       # NaNs included; the sixth row is dropped
    assert state[0, 12] == 6.0 and state[1, 12] == 2.0
    want_n = np.full(12, 6.0)
    want_n[[2, 3, 4]] -= 1
    want_n[7] -= 1
    assert state[1, :12].tolist() == want_n.tolist()
    for c in range(12):
        vals = [np.float64(r[c]) * (2.0 if c < 5 else 1.0) for r in fed if np.isfinite(r[c])]
        total = np.float64(0)
        for v in vals:
            total += v
        assert state[0, c] == total, c
    assert np.isfinite(state).all()
    # an all-dead call changes nothing; the calls compose
    s1, t1, c1 = SceneScores.reference(rows[:1], live[:1], 5, scale)
    s2, t2, c2 = SceneScores.reference(rows[1:2], live[1:2], 5, scale, state=s1, table=t1, cursor=c1)
    assert c2 == c1 == 3 and s2.tobytes() == s1.tobytes() and t2.tobytes() == t1.tobytes()
    s3, t3, c3 = SceneScores.reference(rows[2:], live[2:], 5, scale, state=s2, table=t2, cursor=c2)
    assert c3 == cursor and s3.tobytes() == state.tobytes() and t3.tobytes() == table.tobytes()
    # capacity 0: nothing is stored, everything is counted
    s0, t0, c0 = SceneScores.reference(rows, live, 0, scale)
    assert t0.shape == (0, 12) and c0 == 6 and s0.tobytes() == state.tobytes()


def test_scene_scores_host_side():
    """result(), rows() and worst() on a SceneScores whose device state is filled in by hand (host tensors: bookkeeping only)."""
    import torch
    from strajnet_amd.evaluate import LOSS_KEYS, METRIC_KEYS, ROW_KEYS, SceneScores
    assert ROW_KEYS == SC.ROW_KEYS == LOSS_KEYS + ('total',) + METRIC_KEYS
    rows, live = _calls()
    state, table, cursor = SceneScores.reference(rows, live, 5, np.float32(2.0))
    s = SceneScores(5, preflix='val', device='cpu')
    assert s.result() == dict({f'val_{k}': 0.0 for k in ROW_KEYS}, scenes=0, nonfinite_scenes=0, dropped=0) and s.rows().shape == (0, 12)
    s.state.copy_(torch.from_numpy(state)), s.table.copy_(torch.from_numpy(table)), s.cursor.fill_(cursor)
    res = s.result()
    assert list(res) == [f'val_{k}' for k in ROW_KEYS] + ['scenes', 'nonfinite_scenes', 'dropped']
    assert (res['scenes'], res['nonfinite_scenes'], res['dropped']) == (6, 2, 1)
    for i, k in enumerate(ROW_KEYS):
        assert res[f'val_{k}'] == state[0, i] / state[1, i]
    got = s.rows()
    assert got.shape == (5, 12) and got.tobytes() == table.tobytes()
    w = s.worst(3, 'total')
    assert w[0] == 1 and list(w[1:]) == list(np.argsort(-np.where(np.isnan(got[:, 4]), np.inf, got[:, 4]), kind='stable')[1:3])
    assert list(s.worst(5, 'observed_auc')) == list(np.argsort(got[:, 5], kind='stable'))
    assert len(s.worst(99)) == 5 and len(s.worst(0)) == 0
    assert list(SceneScores(3, no_warp=True, device='cpu').result())[:10] == [f'val_{k}' for k in ROW_KEYS[:10]]
    assert 'val_flow_ogm_auc' not in SceneScores(3, no_warp=True, device='cpu').result()
    s.reset()
    assert s.result()['scenes'] == 0 and s.rows().shape == (0, 12) and not s.table.any()
    with pytest.raises(ValueError):
        SceneScores(-1, device='cpu')


_HOST_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "%s"
int main() {
  char kind;
  while (scanf(" %%c", &kind) == 1) {
    if (kind == 'G') {
      int H, W;
      if (scanf("%%d %%d", &H, &W) != 2) return 2;
      printf("G %%d %%d\n", evs_grid(H, W), EVS_MAXG);
    } else if (kind == 'S') {
      long long capacity, cursor;
      unsigned int scale_bits;
      int ncalls;
      if (scanf("%%lld %%lld %%u %%d", &capacity, &cursor, &scale_bits, &ncalls) != 4) return 2;
      float scale;
      memcpy(&scale, &scale_bits, 4);
      double state[2 * EVS_STATE_COLS];
      for (int i = 0; i < 2 * EVS_STATE_COLS; ++i) state[i] = 0.0;
      const size_t nt = (size_t)capacity * EVS_COLS;
      float* table = (float*)calloc(nt ? nt : 1, nt ? sizeof(float) : 1);        /* exactly the table: a store beyond it is out of bounds */
      for (int q = 0; q < ncalls; ++q) {
        int B;
        if (scanf("%%d", &B) != 1) return 2;
        for (int b = 0; b < B; ++b) {
          int live;
          unsigned int bits[EVS_COLS];
          float row[EVS_COLS];
          if (scanf("%%d", &live) != 1) return 2;
          for (int c = 0; c < EVS_COLS; ++c) if (scanf("%%u", &bits[c]) != 1) return 2;
          memcpy(row, bits, sizeof(row));
          if (live) evs_commit(row, state, capacity ? table : (float*)0, &cursor, capacity, scale);
        }
      }
      printf("S %%lld", cursor);
      for (int i = 0; i < 2 * EVS_STATE_COLS; ++i) { unsigned long long u; memcpy(&u, &state[i], 8); printf(" %%llu", u); }
      for (size_t i = 0; i < nt; ++i) { unsigned int u; memcpy(&u, &table[i], 4); printf(" %%u", u); }
      printf("\n");
      free(table);
    } else {
      return 3;
    }
  }
  return 0;
}
'''


def host_cases():
    """(input lines, expected output lines) for the host program: the grid rule, and the three calls at capacities 5, 0 and 64."""
    from strajnet_amd.evaluate import SceneScores
    lines, want = [], []
    maxg = None
    hdr = open(os.path.join(ROOT, 'strajnet_amd', 'csrc', 'eval_scene.h')).read()
    for ln in hdr.split('\n'):
        if ln.startswith('#define EVS_MAXG '):
            maxg = int(ln.split()[2])
    assert maxg in (16, 32, 64)
    for H, W in ((8, 8), (24, 40), (40, 44), (72, 64), (128, 128), (256, 256), (1, 1), (0, 8), (8, -1), (3, 21)):
        lines.append(f'G {H} {W}')
        want.append(f'G {SC.grid_reference(H, W, maxg)} {maxg}')
    rows, live = _calls()
    scale = np.float32(2.0)
    for capacity, cursor0 in ((5, 0), (0, 0), (64, 0), (5, 4), (5, 7)):
        state, table, cursor = SceneScores.reference(rows, live, capacity, scale, cursor=cursor0)
        toks = [f'S {capacity} {cursor0} {int(scale.view(np.uint32))} {len(rows)}']
        for r, lv in zip(rows, live):
            toks.append(str(len(r)))
            for b in range(len(r)):
                toks.append(str(1 if lv is None else int(lv[b])))
                toks += [str(int(u)) for u in r[b].view(np.uint32)]
        lines.append(' '.join(toks))
        want.append(' '.join([f'S {cursor}'] + [str(int(u)) for u in state.reshape(-1).view(np.uint64)] +
                             [str(int(u)) for u in table.reshape(-1).view(np.uint32)]))
    return lines, want


def test_host_build_of_eval_scene_h_agrees_with_numpy(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host compiler')
    src, exe = tmp_path / 'eval_scene_host.cpp', tmp_path / 'eval_scene_host'
    src.write_text(_HOST_PROGRAM % os.path.join(ROOT, 'strajnet_amd', 'csrc', 'eval_scene.h'))
    r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', str(src), '-o', str(exe)], capture_output=True, text=True)        # host only
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = host_cases()
    r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split('\n')[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lines[i][:40], g[:200], w[:200])


def test_the_library_states_the_same_grid(lib_built):
    from strajnet_amd import _lib
    L = _lib.lib()
    G = L.stj_eval_scenes_grid(256, 256)
    assert G in (16, 32, 64)
    for H, W in ((8, 8), (24, 40), (40, 44), (72, 64), (128, 128), (0, 8)):
        assert L.stj_eval_scenes_grid(H, W) == SC.grid_reference(H, W, G)
    assert L.stj_eval_scenes_grid(8, 8) == 1 and L.stj_eval_scenes_grid(72, 64) < 72                  # 3 x 8 x 8: one workgroup per scene
    a, b = L.stj_eval_scenes_workspace_bytes(3, 40, 44), L.stj_eval_scenes_workspace_bytes(6, 40, 44)
    assert 0 < a < b and a % 16 == 0 and L.stj_eval_scenes_workspace_bytes(0, 8, 8) >= 0
