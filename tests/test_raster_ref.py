"""raster_reference (strajnet_amd/raster.py) against hand-worked answers, the motion-record parser and the test-record writer round trips,
and the yardstick of test_raster_gpu.py: the float32 statement against the float64 one on the two shared cases, with the caps on how much of
the output the ambiguity report may excuse.  No GPU."""
import numpy as np
import pytest

import _raster_cases as rc
from strajnet_amd import data
from strajnet_amd.raster import (AMBIGUITY_EPS, CUR, MAX_OBS, MAX_OCC, STEPS, Tracks, motion_example, pixel_rule, raster_example,
                                 raster_reference, tracks_from_motion_example)

CFG = rc.SMALL_CFG          # grid 128, SDC at (64, 80), 3.2 px/m; FOV grid 64, SDC at (32, 48)


def _rect(plane):
    ys, xs = np.nonzero(plane)
    assert plane[ys.min():ys.max() + 1, xs.min():xs.max() + 1].all(), 'not a full rectangle'
    return int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())


def test_axis_aligned_vehicle_at_the_sdc():
    """4.8 x 2.0 m along the SDC's heading: x in +-1 m -> rint(+-3.2) = +-3, y in +-2.4 m -> rint(+-7.68) = +-8; every step the same."""
    out, _ = raster_reference(rc.single_box(), CFG)
    for t in range(STEPS):
        assert _rect(out['ogm'][0, :, :, t, 0]) == (61, 67, 72, 88)
    assert out['ogm'][0, ..., 1].sum() == 0 and out['ok'][0] == 1
    assert not out['flow'].any()                       # a box that does not move has zero flow


@pytest.mark.parametrize('sdc_yaw', [np.pi / 2, -1.0])
def test_sdc_yaw_is_normalised(sdc_yaw):
    """Whatever the SDC's world yaw and position, its own box is the same rectangle."""
    out, _ = raster_reference(rc.single_box(sdc_yaw=sdc_yaw, sdc_xy=(1234.5, -987.25)), CFG)
    assert _rect(out['ogm'][0, :, :, CUR, 0]) == (61, 67, 72, 88)


def test_a_quarter_turn_of_the_sdc_turns_the_neighbour():
    """World frame, SDC yaw pi/2 (angle = 0: no rotation): a vehicle 10 m along world +x lies 32 px to the right."""
    z = np.zeros((1, 2, STEPS), np.float32)
    x = z.copy()
    x[0, 1] = 10.0
    yaw = z + np.float32(np.pi / 2)
    tr = Tracks(x=x, y=z, bbox_yaw=yaw, length=z + 4.8, width=z + 2.0, velocity_x=z, velocity_y=z, valid=z + 1, type=[[1, 1]], is_sdc=[[1, 0]])
    out, _ = raster_reference(tr, CFG)
    both = out['ogm'][0, :, :, CUR, 0]
    assert _rect(both[:, :80]) == (61, 67, 72, 88) and _rect(both[:, 80:]) == (61 + 32 - 80, 67 + 32 - 80, 72, 88)


def test_round_half_even():
    """The pixel rule rounds halves to even, like tf.round: x ppm = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2; y is negated first."""
    x = np.array([0.25, 0.75, 1.25, -0.25, -0.75, 0.3])
    qx, qy, px, py = pixel_rule(x, x, 2.0, 64, 80)
    assert qx.tolist() == [0.5, 1.5, 2.5, -0.5, -1.5, 0.6] and (qy == -qx).all()
    assert px.tolist() == [64, 66, 66, 64, 62, 65] and py.tolist() == [80, 78, 78, 80, 82, 79]
    q32 = pixel_rule(x.astype(np.float32), x.astype(np.float32), np.float32(2.0), 64, 80)
    assert q32[2].dtype == np.float32 and q32[2].tolist() == px.tolist()


def test_fov_clipping_and_class_routing():
    """A vehicle across the right border renders only inside; cyclists and pedestrians share class 1; type 4 renders nowhere."""
    extra = [rc._agent((19, 0), (19, 0), 0.0, 6.0, 2.0, 1), rc._agent((-10, 5), (-10, 5), 0.0, 1.0, 1.0, 2),
             rc._agent((-10, 10), (-10, 10), 0.0, 1.8, 0.6, 3), rc._agent((10, 10), (10, 10), 0.0, 4.0, 2.0, 4),
             rc._agent((0, 40), (0, 40), 0.0, 4.0, 2.0, 1)]
    out, _ = raster_reference(rc.single_box(extra=extra), CFG)
    veh, oth = out['ogm'][0, :, :, CUR, 0], out['ogm'][0, :, :, CUR, 1]
    right = veh[:, 100:]
    assert _rect(right) == (64 + round(16 * 3.2) - 100, 127 - 100, 80 - 3, 80 + 3)          # x from rint(51.2) = 51 to the border, y +-1 m
    assert _rect(oth[:56]) == (64 - 32 - 3, 64 - 32 + 3, 80 - 32 - 1, 80 - 32 + 1)          # the cyclist: 1.8 x 0.6 at (-10, 10)
    assert _rect(oth[56:]) == (64 - 32 - 2, 64 - 32 + 2, 80 - 16 - 2 - 56, 80 - 16 + 2 - 56)  # the pedestrian: 1 x 1 at (-10, 5)
    assert veh[:60, 80:].sum() == 0                    # type 4 at (10, 10) and the vehicle beyond the top border render nowhere
    assert veh.sum() == right.sum() + 7 * 17


def test_flow_of_a_ten_pixel_displacement():
    """A vehicle that moved 10 px = 3.125 m to the right between step 0 and step 10: flow = px(0) - px(10) = (-10, 0) on its step-10
    footprint, 0 elsewhere; moving ahead (up, -y in the image) gives (0, +10)."""
    for p0, want in (((-3.125 - 8, 5), (-10.0, 0.0)), ((-8, 5 - 3.125), (0.0, 10.0))):
        extra = [rc._agent(p0, (-8, 5), 0.0, 4.0, 2.0, 1)]
        out, _ = raster_reference(rc.single_box(extra=extra), CFG)
        foot = out['ogm'][0, :, :, CUR, 0].astype(bool)
        foot[:, 60:] = False                           # the SDC's own (static) box
        assert foot.sum() > 50
        assert (out['flow'][0][foot] == np.array(want)).all()
        assert not out['flow'][0][~foot].any()


def test_overlapping_boxes_give_the_count_weighted_mean():
    """Two equal vehicles on the same step-10 footprint, one displaced by -10 px and one by +20 px in x: each pixel holds as many points of
    either, so the mean is +5; a third of the first box alone (a sliver the second does not cover) keeps -10."""
    extra = [rc._agent((-8 - 3.125, 5), (-8, 5), 0.0, 4.0, 2.0, 1), rc._agent((-8 + 6.25, 5), (-8, 5), 0.0, 4.0, 2.0, 1)]
    out, _ = raster_reference(rc.single_box(extra=extra), CFG)
    foot = out['ogm'][0, :, :, CUR, 0].astype(bool)
    foot[:, 60:] = False
    assert (out['flow'][0][foot] == np.array([5.0, 0.0])).all()
    # unequal weights: the second vehicle with half the width covers the middle rows with twice the points per pixel
    extra[1] = rc._agent((-8 + 6.25, 5), (-8, 5), 0.0, 4.0, 1.0, 1)
    out, rep = raster_reference(rc.single_box(extra=extra), CFG)
    fl = out['flow'][0][foot]
    assert set(np.unique(fl[:, 0])) - {-10.0} and (fl[:, 0] >= -10).all() and (fl[:, 0] <= 20).all() and (fl[:, 0] == -10).any()
    # by hand at the centre pixel (38, 64): count the points of either box there
    pre = rep['pre'][0, :, CUR]
    px, py = np.rint(pre[..., 0]) + 64, np.rint(pre[..., 1]) + 80
    n1, n2 = ((px[1] == 38) & (py[1] == 64)).sum(), ((px[2] == 38) & (py[2] == 64)).sum()
    assert n1 > 0 and n2 > n1
    assert out['flow'][0, 64, 38, 0] == (-10.0 * n1 + 20.0 * n2) / (n1 + n2)


def test_no_flow_without_step_zero_and_for_other_classes():
    v = np.ones(STEPS)
    v[0] = 0
    extra = [rc._agent((-8 - 3.125, 5), (-8, 5), 0.0, 4.0, 2.0, 1, valid=v), rc._agent((8 - 3.125, 5), (8, 5), 0.0, 1.0, 1.0, 2)]
    out, _ = raster_reference(rc.single_box(extra=extra), CFG)
    assert not out['flow'].any() and out['ogm'][0, :, :, CUR, 0][:, :60].sum() > 50 and out['ogm'][0, :, :, 0, 0][:, :60].sum() == 0


def test_obs_order_padding_and_onehot():
    """FOV grid 64 with the SDC at (32, 48): x in [-10, 10) m, y in (-5, 15] m.  Nearest first by the last valid position; rows past the
    list are zero; the one-hot is tiled over all steps, also the invalid ones, and zero for type 4."""
    v = np.ones(STEPS)
    v[CUR] = 0                                          # the last valid step is 9
    extra = [rc._agent((6, 0), (6, 10), np.pi / 2, 4.0, 2.0, 1, valid=v),       # last valid at step 9: (6, 9) -> 10.8 m
             rc._agent((-3, 4), (-3, 4), 0.0, 1.0, 1.0, 2),                      # 5 m
             rc._agent((2, 2), (2, 2), 0.0, 1.0, 1.0, 4),                        # 2.83 m, type 4
             rc._agent((40, 40), (40, 40), 0.0, 4.0, 2.0, 1)]                    # far outside
    out, rep = raster_reference(rc.single_box(extra=extra), CFG)
    assert rep['in_box'][0].tolist() == [True, True, True, True, False]
    assert rep['obs_src'][0][:5].tolist() == [0, 3, 2, 1, -1]
    obs = out['obs'][0]
    assert not obs[4:].any() and obs.shape == (MAX_OBS, STEPS, 8)
    assert (obs[0, :, 5:] == [1, 0, 0]).all() and (obs[1, :, 5:] == 0).all() and (obs[2, :, 5:] == [0, 1, 0]).all()
    assert np.allclose(obs[2, :, :2], [-3, 4]) and np.allclose(obs[3, 9, :2], [6, 9]) and not obs[3, CUR, :5].any()
    assert (obs[3, :, 5:] == [1, 0, 0]).all()          # tiled over the invalid step too
    assert np.allclose(obs[3, 0, 2:4], [0, 10])        # the velocity, rotated into the frame
    assert np.allclose(obs[0, :, 4], 0.0)              # bbox_yaw is the unrotated world yaw (the SDC's is 0 here)


def test_obs_index_mixup_is_restated():
    """data_preprocessing.py:154-174: an in_box agent without a valid step is skipped in the distance list but not in valid_actor, so the
    rows after it come from the neighbouring agent.  Agent 1 has no valid step (its record holds -1: frame position near the SDC)."""
    extra = [rc._agent((1, 1), (1, 1), 0.0, 1.0, 1.0, 2, valid=np.zeros(STEPS)), rc._agent((-3, 4), (-3, 4), 0.0, 1.0, 1.0, 3)]
    tr = rc.single_box(extra=extra)
    for f in ('x', 'y'):
        getattr(tr, f)[0, 1] = 0.5                     # the invalid agent's stored position: inside the FOV
    out, rep = raster_reference(tr, CFG)
    assert rep['in_box'][0].tolist() == [True, True, True] and rep['obs_listed'][0].tolist() == [True, False, True]
    assert rep['obs_src'][0][:3].tolist() == [0, 1, -1]                          # the second-nearest LISTED agent is 2; the row shows agent 1
    assert not out['obs'][0, 1, :, :5].any() and (out['obs'][0, 1, :, 5:] == [0, 1, 0]).all()


def test_occ_keeps_only_approaching_agents():
    """Outside the FOV grid but within 64 cells of it: kept only when the first valid position is farther than the last."""
    extra = [rc._agent((25, 5), (15, 5), np.pi, 4.0, 2.0, 1),                    # approaching: kept, 15.8 m
             rc._agent((13, 5), (22, 5), 0.0, 4.0, 2.0, 1),                      # moving away: skipped
             rc._agent((14, 0), (14, 0), 0.0, 4.0, 2.0, 1),                      # standing still: first == last, skipped
             rc._agent((-30, 5), (-13, 0), 0.0, 1.0, 1.0, 2),                    # approaching, nearer: first
             rc._agent((80, 5), (60, 5), 0.0, 4.0, 2.0, 1)]                      # beyond the widened grid
    out, rep = raster_reference(rc.single_box(extra=extra), CFG)
    assert rep['occu_mask'][0].tolist() == [False, True, True, True, True, False]
    assert rep['occ_src'][0][:3].tolist() == [4, 1, -1]
    occ = out['occ'][0]
    assert occ.shape == (MAX_OCC, STEPS, 8) and not occ[2:].any()
    assert np.allclose(occ[0, CUR, :2], [-13, 0]) and (occ[0, :, 5:] == [0, 1, 0]).all() and np.allclose(occ[1, 0, :2], [25, 5])
    assert not out['obs'][0, 1:].any()                 # only the SDC is in the FOV


def test_scene_without_sdc_is_zero():
    tracks, cfg = rc.small_case()
    tr = tracks.scenes(slice(0, 1))
    tr.is_sdc[:] = 0
    out, rep = raster_reference(tr, cfg)
    assert out['ok'][0] == 0 and not any(out[k].any() for k in ('ogm', 'flow', 'obs', 'occ'))
    assert not rep['free'].any() and (rep['obs_src'] == -1).all()


# ---------------------------------------------------------------------------------------------------- parser and record round trips
def test_motion_example_round_trip():
    tracks, _ = rc.small_case()
    for b in range(tracks.B):
        got = tracks_from_motion_example(motion_example(tracks, b))
        for f in tracks.__dataclass_fields__:
            want = getattr(tracks, f)[b:b + 1]
            assert np.array_equal(getattr(got, f), want) and getattr(got, f).dtype == want.dtype, f
    with pytest.raises(ValueError, match='is missing'):
        tracks_from_motion_example(data.serialize_example_lists({'state/type': np.ones(3, np.float32)}))


def test_list_features_packed_and_unpacked():
    """FloatList / Int64List both packed (what the writer emits) and one value per tag; negative int64; bytes features stay parse_example's."""
    feats = {'f': np.array([1.5, -2.25, 3e9], np.float32), 'i': np.array([0, 1, -1, 2 ** 40, -2 ** 62], np.int64), 'b': b'xyz', 'e': np.zeros(0, np.float32)}
    payload = data.serialize_example_lists(feats)
    got = data.parse_example_lists(payload)
    assert np.array_equal(got['f'], feats['f']) and np.array_equal(got['i'], feats['i']) and got['i'].dtype == np.int64
    assert 'b' not in got and bytes(data.parse_example(payload)['b']) == b'xyz'
    ld, vi = data._ld, data._enc_varint
    unpacked_f = ld(2, b''.join(vi((1 << 3) | 5) + np.float32(v).tobytes() for v in feats['f']))
    unpacked_i = ld(3, b''.join(vi(1 << 3) + vi(int(v) & (2 ** 64 - 1)) for v in feats['i']))
    entries = b''.join(ld(1, ld(1, n.encode()) + ld(2, f)) for n, f in (('f', unpacked_f), ('i', unpacked_i)))
    got = data.parse_example_lists(ld(1, entries))
    assert np.array_equal(got['f'], feats['f']) and np.array_equal(got['i'], feats['i'])


def test_raster_example_round_trip():
    """raster_example -> serialize -> parse_example -> unpack_example_reference, raw and through pack_example: the float32 tensors the
    model is fed are the rasterised ones."""
    tracks, cfg = rc.small_case()
    out, _ = rc.reference('small', 'float32')
    rng = np.random.default_rng(0)
    half = cfg.grid // 2
    mi = rng.integers(-128, 128, (half, half, 3)).astype(np.int8)
    cl = rng.standard_normal((256, 10, 7))
    for b in range(tracks.B):
        ex = raster_example(out, b, mi, cl, f'scene-{b}')
        parsed = data.parse_example(data.serialize_example(ex))
        assert bytes(parsed['scenario/id']) == f'scene-{b}'.encode()
        for rec in (parsed, data.pack_example(parsed, grid=cfg.grid, out=half, test=True)):
            got = data.unpack_example_reference(rec, grid=cfg.grid, out=half, test=True)
            assert np.array_equal(got['ogm'], out['ogm'][b]) and np.array_equal(got['vec_flow'], out['flow'][b])
            assert np.array_equal(got['actors'], out['obs'][b]) and np.array_equal(got['occl_actors'], out['occ'][b])
            assert np.array_equal(got['map_image'], mi.astype(np.float32) / 256) and np.array_equal(got['centerlines'], cl.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the yardstick of the GPU test
def test_small_case_holds_what_it_promises():
    tracks, cfg = rc.small_case()
    out, rep = rc.reference('small')
    veh = out['ogm'][..., 0]
    for b in range(2):
        assert veh[b, :, 127, CUR].any() or veh[b, :, 0, CUR].any()                 # a box on the grid border
        assert veh[b, 0, :, CUR].any()                                             # the 12 m vehicle reaches the top border
        assert veh[b, :, :, 2].sum() < veh[b, :, :, 1].sum()                        # an agent invalid at step 2
        assert (out['ogm'][b, :, :, CUR, 0] * out['ogm'][b, :, :, CUR, 1]).any()    # a pedestrian / cyclist over a vehicle
        n = np.count_nonzero(out['flow'][b].any(-1))
        assert 0 < n < veh[b, :, :, CUR].sum()                                      # a vehicle without step 0 has no flow
        vals = np.unique(out['flow'][b].reshape(-1, 2), axis=0)
        assert any(v[0] != int(v[0]) or v[1] != int(v[1]) for v in vals)            # overlapping vehicles: a non-integer mean
    assert not rc._offenders(tracks, cfg) and rep['occ_src'][:, 0].min() >= -1


@pytest.mark.parametrize('name', ['small', 'full'])
def test_float32_statement_against_float64(name):
    """Every float32 / float64 disagreement in ogm lies on a free pixel; the pre-rounding coordinates of the boxes that render deviate by
    less than eps / 4; masks and order agree; and the caps on what the report excuses hold."""
    tracks, cfg = {'small': rc.small_case, 'full': rc.full_case}[name]()
    o64, r64 = rc.reference(name)
    o32, r32 = rc.reference(name, 'float32')
    diff = o32['ogm'] != o64['ogm']
    print(f'{name}: ogm set {int(o64["ogm"].sum())}, differing {int(diff.sum())}, free {int(r64["free"].sum())}')
    assert not (diff & ~r64['free']).any()
    draw = r64['drawable']
    near = draw[..., None] & (np.abs(r64['pre']).max(-1) < 4 * cfg.grid)      # boxes that can render, within a few grids of the SDC
    dev = float(np.abs(r32['pre'].astype(np.float64) - r64['pre'])[near].max())
    print(f'{name}: largest pre-rounding deviation {dev:.3e} px (eps / 4 = {AMBIGUITY_EPS / 4:.3e})')
    assert dev < AMBIGUITY_EPS / 4
    # ---- caps, on the reference alone
    n_set = int(o64['ogm'].sum())
    n_free = int(r64['free'].sum())
    flow_px = o64['flow'].any(-1) | r64['flow_sure']
    n_touched = int((r64['flow_touched'] & flow_px).sum())
    print(f'{name}: free {n_free} of {n_set} set ({100 * n_free / n_set:.3f} %), touched flow pixels {n_touched} of {int(flow_px.sum())} '
          f'({100 * n_touched / max(1, flow_px.sum()):.2f} %)')
    assert n_free <= 0.003 * n_set
    assert n_touched <= 0.15 * flow_px.sum()
    # ---- flow: bitwise on clean pixels, inside the candidates' bounds elsewhere
    f32, f64 = o32['flow'], o64['flow'].astype(np.float32)
    clean = ~r64['flow_touched']
    assert np.array_equal(f32[clean], f64[clean])
    check_flow_bounds(f32, r64)
    # ---- actors: the same agents in the same order
    for k in ('in_box', 'occu_mask', 'obs_src', 'occ_src', 'obs_listed', 'occ_listed'):
        assert np.array_equal(r32[k], r64[k]), k
    assert (o64['ok'] == o32['ok']).all()
    if name == 'full':
        assert o64['ok'].tolist() == [1, 0, 1] and not o64['ogm'][1].any() and not o64['obs'][1].any()
        assert (r64['obs_src'][0] >= 0).sum() > 10 and (r64['occ_src'][0] >= 0).sum() > 2


def check_flow_bounds(flow, rep):
    """On a touched pixel the value lies within the least and the greatest candidate displacement of the points that may land there (or
    is zero where no unambiguous point lands)."""
    t = rep['flow_touched']
    v, lo, hi = flow[t], rep['flow_lo'][t], rep['flow_hi'][t]
    inside = ((v >= lo) & (v <= hi)).all(-1)
    zero_ok = ~rep['flow_sure'][t] & (v == 0).all(-1)
    assert (inside | zero_ok).all()
    assert not flow[~t & ~np.isfinite(rep['flow_lo'][..., 0])].any()            # nothing may land there


@pytest.mark.parametrize('name', ['small', 'full'])
def test_actor_deviation_recorded(name):
    """The float32-to-float64 deviation of obs / occ that _raster_cases.ACTOR_DEVIATION records for the GPU test's tolerance."""
    o64, _ = rc.reference(name)
    o32, _ = rc.reference(name, 'float32')
    dev = max(float(np.abs(o32[k].astype(np.float64) - o64[k]).max()) for k in ('obs', 'occ'))
    print(f'{name}: obs / occ float32 deviation {dev:.3e} (recorded {rc.ACTOR_DEVIATION[name]:.3e})')
    assert rc.ACTOR_DEVIATION[name] / 2 <= dev <= rc.ACTOR_DEVIATION[name]


_HOST_PROGRAM = r'''
#include <stdio.h>
#include "%s"
int main() {
  const rst_frame_t f = rst_frame(1234.5f, -987.25f, 0.75f);
  // the SDC's own 4.8 x 2.0 box, yaw equal to the SDC's: every point's pixel on the 128 grid (SDC at (64, 80), 3.2 px/m)
  const rst_box_t b = rst_box(f, 1234.5f, -987.25f, 0.75f, 4.8f, 2.0f, 3.f, 4.f, 1, 1.f);
  int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1, n = 0;
  for (int i = 0; i < 48; ++i)
    for (int j = 0; j < 16; ++j) {
      float x, y, px, py;
      rst_point(b, i, j, 48, 16, &x, &y);
      rst_pixel(x, y, 3.2f, 64.f, 80.f, &px, &py);
      if (!rst_in_grid(px, py, 128, 0)) continue;
      ++n;
      x0 = px < x0 ? (int)px : x0; x1 = px > x1 ? (int)px : x1; y0 = py < y0 ? (int)py : y0; y1 = py > y1 ? (int)py : y1;
    }
  printf("rect %%d %%d %%d %%d %%d\n", x0, x1, y0, y1, n);
  int q[4];
  rst_aabb(b, 3.2f, 64.f, 80.f, 128, q);
  printf("aabb %%d\n", q[0] <= x0 && q[1] <= y0 && q[2] >= x1 && q[3] >= y1 && q[0] >= x0 - 2 && q[2] <= x1 + 2);
  float px, py;
  const float halves[5] = {0.25f, 0.75f, 1.25f, -0.25f, -0.75f};
  printf("half");
  for (int k = 0; k < 5; ++k) { rst_pixel(halves[k], halves[k], 2.f, 64.f, 80.f, &px, &py); printf(" %%d %%d", (int)px, (int)py); }
  printf("\nplanes %%u %%u %%u %%u\n", rst_plane_mask(0, 0), rst_plane_mask(3, 1), rst_plane_mask(10, 1), rst_plane_mask(4, -1));
  printf("class %%d %%d %%d %%d %%d\n", rst_class(0), rst_class(1), rst_class(2), rst_class(3), rst_class(4));
  printf("speed %%.3f yaw %%.2f\n", (double)(b.vx * b.vx + b.vy * b.vy), (double)b.yaw);
  printf("ws");
  for (int p = 0; p <= RST_WS_PARTS; ++p) printf(" %%lld", rst_ws_offset(3, 128, p));
  printf("\n");
  return 0;
}
'''


def test_header_rules_compile_on_the_host(tmp_path):
    """csrc/raster.h as a host program compiles it: the frame, point and pixel rules give the hand-worked rectangle, halves round to even,
    the plane table routes (step, class) to bit 2 t + c, and the workspace layout is the one the library reports."""
    import os
    import subprocess
    from strajnet_amd import _lib, build
    src = tmp_path / 'raster_host.cpp'
    src.write_text(_HOST_PROGRAM % os.path.join(build.CSRC, 'raster.h'))
    exe = tmp_path / 'raster_host'
    r = subprocess.run([build._hipcc(), '-x', 'c++', '-std=c++17', '-O1', str(src), '-o', str(exe)], capture_output=True, text=True)      # host only
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(line.split(' ', 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split('\n'))
    assert got['rect'] == '61 67 72 88 768' and got['aabb'] == '1'
    assert got['half'] == '64 80 66 78 66 78 64 80 62 82'
    assert got['planes'] == f'{1 << 0} {1 << 7} {1 << 21} 0' and got['class'] == '-1 0 1 1 -1'
    assert got['speed'] == '25.000 yaw 0.75'         # velocities are rotated, not shifted; the yaw stays the world's
    build.build(verbose=False)
    L = _lib.lib()
    want = [L.stj_raster_workspace_offset(3, 128, p) for p in range(7)] + [L.stj_raster_workspace_bytes(3, 128)]
    assert got['ws'] == ' '.join(str(w) for w in want) and L.stj_raster_workspace_offset(3, 128, 7) == -1
