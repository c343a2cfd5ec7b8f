"""The model's inputs from agent tracks: the reference's L0 layer (data_preprocessing.py, grid_utils.py) on the device, without TensorFlow.

    tracks = tracks_from_motion_example(payload)            # or Tracks(...) from a simulator / tracker
    x = rasterize(tracks)                                   # ogm [B,512,512,11,2], flow [B,512,512,2], obs [B,48,11,8], occ [B,16,11,8], ok [B]
    y = model(**model_inputs(x), map_img=map_img)

`raster_reference` states the semantics in NumPy and is the only CPU path (tests check the kernels against it; it is not a fallback).
`map_img` stays the caller's: the reference renders it with matplotlib (data_preprocessing.py:275-337), which has no reproducible definition.
The centre lines and the ground-truth waypoint grids are not built here either.

The semantics (csrc/raster.h holds the same rules for the device and for host programs):
  frame    the SDC is the lowest agent with is_sdc == 1; every position has the SDC's current one subtracted and is rotated by
           angle = pi/2 - sdc_yaw, velocities are rotated only, boxes are sampled with bbox_yaw + angle, the actor rows keep the unrotated
           bbox_yaw (grid_utils.py:63-77, 541-582).  A scene without an SDC has ok = 0 and all-zero outputs.
  points   point (i, j), i < 48, j < 16 of a box: centre + R(yaw) (u_i length, v_j width), u_i = i/47 - 0.5, v_j = j/15 - 0.5.  This is the
           published Waymo renderer's _sample_points_from_agent_boxes WRITTEN FROM MEMORY; the library is not part of the reference's tree,
           so this statement is the contract.  The same holds for "vec_flow is the backward flow at index 0" below.
  pixels   px = rint(x ppm) + sdc_x, py = rint(-y ppm) + sdc_y, round-half-even; a point renders iff 0 <= px, py < grid (grid_utils.py:40-51).
  ogm      ogm[y, x, t, c] = 1 iff a rendered point of an agent of class c that is valid (valid > 0) at step t lands there; class 0 is
           type 1, class 1 is type 2 or 3 (data_preprocessing.py:262-273); t = 0..9 past, 10 current.
  flow     vehicles only; points valid at step 10 AND step 0 and rendered at step 10: the mean, at the step-10 pixel, of
           (px(0) - px(10), py(0) - py(10)); zero where none lands (data_preprocessing.py:360-363, grid_utils.py:398-435).
  actors   grid_utils.py:555-584 and data_preprocessing.py:145-213 on the FOV grid (256, SDC at (128, 192)), see _actors_reference.
"""
import dataclasses

import numpy as np
import torch

from . import data
from ._lib import ENUMS, lib
from .ops import _p, _st, call

STEPS, CUR = 11, 10
MAX_OBS, MAX_OCC, OCC_MARGIN = 48, 16, 64
AMBIGUITY_EPS = 2.0 ** -10          # px: a pre-rounding coordinate this close to a half-integer may round either way in float32
STATE_FIELDS = ('x', 'y', 'bbox_yaw', 'length', 'width', 'velocity_x', 'velocity_y', 'valid')
_PART = ENUMS['stj_raster_part']


@dataclasses.dataclass(frozen=True)
class RasterConfig:
    """The raster configuration (ogm, flow) and the FOV configuration (actor masks) of data_preprocessing.py:65-101."""
    grid: int = 512
    sdc_x: int = 256
    sdc_y: int = 320
    pixels_per_meter: float = 3.2
    points_length: int = 48
    points_width: int = 16
    fov_grid: int = 256
    fov_sdc_x: int = 128
    fov_sdc_y: int = 192


@dataclasses.dataclass
class Tracks:
    """Agent tracks over 10 past + 1 current step.  [B, A, 11] float32: x, y, bbox_yaw, length, width, velocity_x, velocity_y, valid
    (> 0 is valid); [B, A] integers: type (1 vehicle, 2 pedestrian, 3 cyclist) and is_sdc."""
    x: np.ndarray
    y: np.ndarray
    bbox_yaw: np.ndarray
    length: np.ndarray
    width: np.ndarray
    velocity_x: np.ndarray
    velocity_y: np.ndarray
    valid: np.ndarray
    type: np.ndarray
    is_sdc: np.ndarray

    def __post_init__(self):
        for f in STATE_FIELDS:
            setattr(self, f, np.ascontiguousarray(getattr(self, f), np.float32))
        self.type = np.ascontiguousarray(self.type, np.int32)
        self.is_sdc = np.ascontiguousarray(self.is_sdc, np.int32)
        shape = self.x.shape
        if len(shape) != 3 or shape[2] != STEPS:
            raise ValueError(f'Tracks: [B, A, {STEPS}] arrays only, got {shape}')
        for f in STATE_FIELDS:
            if getattr(self, f).shape != shape:
                raise ValueError(f'Tracks.{f}: {getattr(self, f).shape}, expected {shape}')
        if self.type.shape != shape[:2] or self.is_sdc.shape != shape[:2]:
            raise ValueError(f'Tracks: type / is_sdc {self.type.shape} / {self.is_sdc.shape}, expected {shape[:2]}')

    @property
    def B(self):
        return self.x.shape[0]

    @property
    def A(self):
        return self.x.shape[1]

    def state(self):
        """float32 [8, B, A, 11] in STATE_FIELDS order: what stj_raster_boxes reads."""
        return np.stack([getattr(self, f) for f in STATE_FIELDS])

    def scenes(self, idx):
        return Tracks(*(np.array(getattr(self, f.name)[idx]) for f in dataclasses.fields(self)))      # copies


# ---------------------------------------------------------------------------------------------------- the statement
def pixel_rule(x, y, ppm, sdc_x, sdc_y):
    """grid_utils.py:40-42: (x ppm, -y ppm) before rounding, and the pixel (rint(x ppm) + sdc_x, rint(-y ppm) + sdc_y); np.rint rounds
    halves to even like tf.round."""
    qx, qy = x * ppm, -y * ppm
    return qx, qy, np.rint(qx) + sdc_x, np.rint(qy) + sdc_y


def _candidates(pre, eps):
    """The pixel offsets a pre-rounding coordinate may round to: (lo, hi, ambiguous); lo == hi == rint unless it lies within eps of a
    half-integer."""
    fl = np.floor(pre)
    amb = np.abs(pre - fl - 0.5) < eps
    r = np.rint(pre)
    return np.where(amb, fl, r), np.where(amb, fl + 1, r), amb


def _actors_reference(X, Y, VX, VY, yaw, byaw, L, W, valid, typ, cfg, dt):
    """grid_utils.py:555-584 and data_preprocessing.py:145-213 for one scene, as written there.  Two things are ours to say:
    np.argsort leaves ties unspecified -- here they break by agent index (a stable sort); and the reference's `obs` loop indexes
    valid_actor[d] / valid_type[d] (the in_box agents, those without a valid step included) with d, an index into the distance list, which
    skips them (:154-174).  That is restated as written: after an in_box agent without a valid step the rows come from the wrong agent."""
    ppm, G = dt(cfg.pixels_per_meter), cfg.fov_grid

    def to_pix(px, py):
        return px * ppm, -py * ppm

    def in_fov(qx, qy, margin):
        px, py = np.rint(qx) + cfg.fov_sdc_x, np.rint(qy) + cfg.fov_sdc_y
        return (px >= -margin) & (py >= -margin) & (px < G + margin) & (py < G + margin)

    def edge(qx, qy, margin):      # distance of the pre-rounding coordinates to the rounding boundaries of the FOV test
        d = np.inf
        for q, s in ((qx, cfg.fov_sdc_x), (qy, cfg.fov_sdc_y)):
            for bound in (-margin - 0.5, G + margin - 0.5):
                d = np.minimum(d, np.abs(q + s - bound))
        return d

    sin_yaw, cos_yaw, h = np.sin(byaw), np.cos(byaw), dt(0.5)
    in_box = np.zeros(X.shape, bool)
    fov_edge = np.full(X.shape[0], np.inf)
    for sl, sw in ((h, -h), (h, h), (-h, -h), (-h, h)):      # _rotate_box: upper-left, upper-right, lower-left, lower-right
        cx = cos_yaw * L * sl - sin_yaw * W * sw + X
        cy = sin_yaw * L * sl + cos_yaw * W * sw + Y
        qx, qy = to_pix(cx, cy)
        in_box |= in_fov(qx, qy, 0)                          # no validity check (grid_utils.py:562-575)
        fov_edge = np.minimum(fov_edge, edge(qx, qy, 0).min(-1))
    in_box = in_box.any(-1)
    qx, qy = to_pix(X[:, CUR], Y[:, CUR])
    occu = in_fov(qx, qy, OCC_MARGIN) & ~in_box
    fov_edge = np.minimum(fov_edge, edge(qx, qy, OCC_MARGIN))
    traj = valid[..., None].astype(dt) * np.stack([X, Y, VX, VY, yaw], -1)      # actor_traj [A, 11, 5]
    emb = np.eye(3)
    A = X.shape[0]
    dist_last, dist_first = np.zeros(A, np.float32), np.zeros(A, np.float32)
    for a in range(A):
        w = np.where(valid[a])[0]
        if w.shape[0]:
            dist_first[a] = np.float32(np.linalg.norm(traj[a, w[0], :2]))
            dist_last[a] = np.float32(np.linalg.norm(traj[a, w[-1], :2]))

    def onehot(t):
        return emb[int(t) - 1] if int(t) in (1, 2, 3) else np.zeros(3)

    # ---- obs (actor_traj_process, first half)
    traj_m = np.where(in_box)[0]
    dist = [dist_last[a] for a in traj_m if valid[a].any()]
    order = np.argsort(np.asarray(dist, np.float32), kind='stable')[:MAX_OBS]
    obs, obs_src = np.zeros((MAX_OBS, STEPS, 8), dt), np.full(MAX_OBS, -1, np.int64)
    for i, d in enumerate(order):
        a = traj_m[d]                                        # valid_actor[d]: the uncompacted list (the reference's mix-up)
        obs[i] = np.concatenate((traj[a], np.tile(onehot(typ[a]), (STEPS, 1))), -1)
        obs_src[i] = a
    # ---- occ (second half): the lists are compacted together, so d means the same agent everywhere
    kept = [a for a in np.where(occu)[0] if valid[a].any() and not dist_first[a] <= dist_last[a]]
    order = np.argsort(np.asarray([dist_last[a] for a in kept], np.float32), kind='stable')[:MAX_OCC]
    occ, occ_src = np.zeros((MAX_OCC, STEPS, 8), dt), np.full(MAX_OCC, -1, np.int64)
    for i, d in enumerate(order):
        a = kept[d]
        occ[i] = np.concatenate((traj[a], np.tile(onehot(typ[a]), (STEPS, 1))), -1)
        occ_src[i] = a
    rep = dict(in_box=in_box, occu_mask=occu, obs_src=obs_src, occ_src=occ_src, dist_last=dist_last, dist_first=dist_first, fov_edge=fov_edge,
               obs_listed=in_box & valid.any(-1), occ_listed=np.isin(np.arange(A), kept))
    return obs, occ, rep


def _grids_reference(b, out, rep, X, Y, byaw, f, valid, cls, cfg, dt, eps):
    """ogm, flow and their ambiguity report of scene b (written into out / rep) from the frame-relative state [A, 11]."""
    A, G, P = X.shape[0], cfg.grid, cfg.points_length * cfg.points_width
    nl, nw, ppm = cfg.points_length, cfg.points_width, dt(cfg.pixels_per_meter)
    u = (np.arange(nl, dtype=dt) / dt(nl - 1) - dt(0.5))[:, None]
    v = (np.arange(nw, dtype=dt) / dt(nw - 1) - dt(0.5))[None, :]
    # ---- points [A, 11, nl, nw] and their pixel coordinates before rounding
    cb, sb = np.cos(byaw)[..., None, None], np.sin(byaw)[..., None, None]
    ul, vw = u * f['length'][..., None, None], v * f['width'][..., None, None]
    qx, qy, px, py = (q.reshape(A, STEPS, P) for q in pixel_rule(X[..., None, None] + ul * cb - vw * sb, Y[..., None, None] + ul * sb + vw * cb,
                                                               ppm, cfg.sdc_x, cfg.sdc_y))
    rep['pre'][b, ..., 0], rep['pre'][b, ..., 1] = qx, qy
    draw = valid & (cls >= 0)[:, None]
    rep['drawable'][b] = draw
    xlo, xhi, xamb = _candidates(qx, eps)
    ylo, yhi, yamb = _candidates(qy, eps)
    amb = xamb | yamb

    def inside(ax, ay):
        return (ax >= 0) & (ay >= 0) & (ax < G) & (ay < G)

    T = np.broadcast_to(np.arange(STEPS)[None, :, None], qx.shape)
    C = np.broadcast_to(cls[:, None, None], qx.shape)
    m = draw[..., None] & inside(px, py)
    out['ogm'][b][py[m].astype(np.int64), px[m].astype(np.int64), T[m], C[m]] = 1
    sure = np.zeros((G, G, STEPS, 2), bool)
    ms = m & ~amb
    sure[py[ms].astype(np.int64), px[ms].astype(np.int64), T[ms], C[ms]] = True
    maybe = np.zeros((G, G, STEPS, 2), bool)
    ma = draw[..., None] & amb
    for cx in (xlo, xhi):
        for cy in (ylo, yhi):
            ax, ay = cx + cfg.sdc_x, cy + cfg.sdc_y
            k = ma & inside(ax, ay)
            maybe[ay[k].astype(np.int64), ax[k].astype(np.int64), T[k], C[k]] = True
    rep['free'][b] = maybe & ~sure
    # ---- vec_flow: vehicles valid at step 10 and step 0, rendered at step 10
    fa = (cls == 0) & valid[:, CUR] & valid[:, 0]
    m10 = fa[:, None] & inside(px[:, CUR], py[:, CUR])
    iy, ix = py[:, CUR][m10].astype(np.int64), px[:, CUR][m10].astype(np.int64)
    ssum, cnt = np.zeros((G, G, 2), dt), np.zeros((G, G), dt)
    np.add.at(cnt, (iy, ix), 1)
    np.add.at(ssum[..., 0], (iy, ix), (px[:, 0] - px[:, CUR])[m10])
    np.add.at(ssum[..., 1], (iy, ix), (py[:, 0] - py[:, CUR])[m10])
    out['flow'][b] = np.where(cnt[..., None] > 0, ssum / np.maximum(cnt, 1)[..., None], 0)
    famb = fa[:, None] & (amb[:, CUR] | amb[:, 0])
    for cx in (xlo[:, CUR], xhi[:, CUR]):
        for cy in (ylo[:, CUR], yhi[:, CUR]):
            ax, ay = cx + cfg.sdc_x, cy + cfg.sdc_y
            k = fa[:, None] & inside(ax, ay)
            jy, jx = ay[k].astype(np.int64), ax[k].astype(np.int64)
            np.minimum.at(rep['flow_lo'][b, ..., 0], (jy, jx), (xlo[:, 0] - cx)[k])
            np.maximum.at(rep['flow_hi'][b, ..., 0], (jy, jx), (xhi[:, 0] - cx)[k])
            np.minimum.at(rep['flow_lo'][b, ..., 1], (jy, jx), (ylo[:, 0] - cy)[k])
            np.maximum.at(rep['flow_hi'][b, ..., 1], (jy, jx), (yhi[:, 0] - cy)[k])
            k = famb & inside(ax, ay)
            rep['flow_touched'][b][ay[k].astype(np.int64), ax[k].astype(np.int64)] = True
    k = m10 & ~amb[:, CUR]
    rep['flow_sure'][b][py[:, CUR][k].astype(np.int64), px[:, CUR][k].astype(np.int64)] = True


def raster_reference(tracks, cfg=None, dtype=np.float64, eps=AMBIGUITY_EPS, grids=True):
    """The four outputs and `ok` in NumPy, computed in `dtype` from the tracks' float32 values (np.float32: the same statement in the
    device's precision), plus an ambiguity report: ({'ogm', 'flow', 'obs', 'occ', 'ok'}, report).

    A point is AMBIGUOUS when a pixel coordinate before rounding lies within eps px of a half-integer: its CANDIDATES are the (up to four)
    pixels it may round to.  report:
      free          bool [B,G,G,11,2]  a candidate of an ambiguous point that no unambiguous point sets: 0 or 1 are both right there
      flow_touched  bool [B,G,G]       a candidate step-10 pixel of a flow point that is ambiguous at step 0 or step 10
      flow_sure     bool [B,G,G]       a flow point that is unambiguous at step 10 lands here
      flow_lo/_hi   dtype [B,G,G,2]    the least / greatest candidate displacement over the flow points that may land here (+-inf: none)
      pre           dtype [B,A,11,P,2] every point's pixel coordinates before rounding (without the SDC offset); drawable bool [B,A,11]
                                       marks the boxes that can render (valid, class 0 or 1)
      in_box, occu_mask, obs_listed, occ_listed bool [B,A]; obs_src [B,48], occ_src [B,16] the agent of each row (-1: padding);
      dist_last, dist_first float32 [B,A]; fov_edge [B,A] the least distance (px) of a pre-rounding corner / current centre to a
      rounding boundary of the FOV tests.
    grids=False leaves ogm, flow and their report at zero (the actor outputs alone: cheap)."""
    cfg = cfg or RasterConfig()
    dt = np.dtype(dtype).type
    B, A, G = tracks.B, tracks.A, cfg.grid
    nl, nw = cfg.points_length, cfg.points_width
    P = nl * nw
    out = dict(ogm=np.zeros((B, G, G, STEPS, 2), dt), flow=np.zeros((B, G, G, 2), dt), obs=np.zeros((B, MAX_OBS, STEPS, 8), dt),
               occ=np.zeros((B, MAX_OCC, STEPS, 8), dt), ok=np.zeros(B, dt))
    rep = dict(free=np.zeros((B, G, G, STEPS, 2), bool), flow_touched=np.zeros((B, G, G), bool), flow_sure=np.zeros((B, G, G), bool),
               flow_lo=np.full((B, G, G, 2), np.inf, dt), flow_hi=np.full((B, G, G, 2), -np.inf, dt),
               pre=np.zeros((B, A, STEPS, P, 2), dt), drawable=np.zeros((B, A, STEPS), bool),
               in_box=np.zeros((B, A), bool), occu_mask=np.zeros((B, A), bool), obs_listed=np.zeros((B, A), bool),
               occ_listed=np.zeros((B, A), bool), obs_src=np.full((B, MAX_OBS), -1, np.int64), occ_src=np.full((B, MAX_OCC), -1, np.int64),
               dist_last=np.zeros((B, A), np.float32), dist_first=np.zeros((B, A), np.float32), fov_edge=np.full((B, A), np.inf))
    for b in range(B):
        sdc = np.flatnonzero(tracks.is_sdc[b] == 1)
        if sdc.size == 0:
            continue                                         # ok = 0, everything stays zero; never clamped
        s = sdc[0]
        out['ok'][b] = 1
        f = {k: getattr(tracks, k)[b].astype(dt) for k in STATE_FIELDS}
        angle = dt(np.pi / 2) - f['bbox_yaw'][s, CUR]
        c, sn = np.cos(angle), np.sin(angle)
        dx, dy = f['x'] - f['x'][s, CUR], f['y'] - f['y'][s, CUR]
        X, Y = c * dx - sn * dy, sn * dx + c * dy
        VX, VY = c * f['velocity_x'] - sn * f['velocity_y'], sn * f['velocity_x'] + c * f['velocity_y']
        byaw = f['bbox_yaw'] + angle
        valid = tracks.valid[b] > 0
        typ = tracks.type[b]
        cls = np.where(typ == 1, 0, np.where((typ == 2) | (typ == 3), 1, -1))
        if grids:
            _grids_reference(b, out, rep, X, Y, byaw, f, valid, cls, cfg, dt, eps)
        # ---- actors
        out['obs'][b], out['occ'][b], arep = _actors_reference(X, Y, VX, VY, f['bbox_yaw'], byaw, f['length'], f['width'], valid, typ, cfg, dt)
        for k2, val in arep.items():
            rep[k2][b] = val
    return out, rep


# ---------------------------------------------------------------------------------------------------- the device path
def _shapes(B, cfg):
    return {'ogm': (B, cfg.grid, cfg.grid, STEPS, 2), 'flow': (B, cfg.grid, cfg.grid, 2), 'obs': (B, MAX_OBS, STEPS, 8),
            'occ': (B, MAX_OCC, STEPS, 8), 'ok': (B,)}


class Rasterizer:
    """stj_raster_boxes / _grids / _actors for batches of B scenes of A agents: the inputs' device copies, the workspace and the outputs are
    allocated once.  load(tracks) uploads; run() is three launches and one cast on the current stream -- static shapes, no sync, no
    allocation: it can be captured into a graph and replayed after the next load().  __call__(tracks) = load + run."""

    def __init__(self, B, cfg=None, A=128, device='cuda', out=None):
        self.cfg = cfg = cfg or RasterConfig()
        self.B, self.A = int(B), int(A)
        self.device = dev = data._hip_device('Rasterizer', device)
        nbytes = lib().stj_raster_workspace_bytes(self.B, self.A)
        if nbytes < 0:
            raise ValueError(f'Rasterizer: B {B}, A {A}')
        self.ws = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        self.state = torch.zeros((len(STATE_FIELDS), self.B, self.A, STEPS), dtype=torch.float32, device=dev)
        self.meta = torch.zeros((2, self.B, self.A), dtype=torch.int32, device=dev)          # type, is_sdc
        self.out = {}
        for name, shape in _shapes(self.B, cfg).items():
            t = None if out is None else out.get(name)
            if t is None:
                t = torch.empty(shape, dtype=torch.float32, device=dev)
            elif tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != self.ws.device or not t.is_contiguous():
                raise ValueError(f'Rasterizer: out[{name!r}] must be a contiguous float32 {shape} tensor on {self.ws.device}')
            self.out[name] = t
        self._ok = self.part('OK')

    def part(self, name):
        """A workspace part (include/strajnet_hip.h, enum stj_raster_part) as a tensor view: BOX, AABB, FRAME, OK, MASK, DIST, RANK."""
        B, A = self.B, self.A
        dtype, shape = {'BOX': (torch.float32, (B, A, STEPS, 12)), 'AABB': (torch.int32, (B, A, STEPS, 4)), 'FRAME': (torch.float32, (B, 8)),
                        'OK': (torch.int32, (B,)), 'MASK': (torch.int32, (B, A)), 'DIST': (torch.float32, (B, A, 2)),
                        'RANK': (torch.int32, (B, A, 2))}[name]
        off = int(lib().stj_raster_workspace_offset(B, A, _PART['STJ_RASTER_' + name]))
        n = int(np.prod(shape)) * 4
        return self.ws[off:off + n].view(dtype).view(shape)

    def load(self, tracks):
        if (tracks.B, tracks.A) != (self.B, self.A):
            raise ValueError(f'Rasterizer: tracks of [{tracks.B}, {tracks.A}], built for [{self.B}, {self.A}]')
        self.state.copy_(torch.from_numpy(tracks.state()))
        self.meta.copy_(torch.from_numpy(np.stack([tracks.type, tracks.is_sdc])))

    def run(self):
        cfg, B, A, o = self.cfg, self.B, self.A, self.out
        ppm = float(cfg.pixels_per_meter)
        call('stj_raster_boxes', _p(self.state), _p(self.meta[0]), _p(self.meta[1]), _p(self.ws), B, A, cfg.grid, ppm, float(cfg.sdc_x),
             float(cfg.sdc_y), _st())
        call('stj_raster_grids', _p(self.ws), _p(o['ogm']), _p(o['flow']), B, A, cfg.grid, ppm, float(cfg.sdc_x), float(cfg.sdc_y),
             cfg.points_length, cfg.points_width, _st())
        call('stj_raster_actors', _p(self.ws), _p(self.meta[0]), _p(o['obs']), _p(o['occ']), B, A, cfg.fov_grid, ppm, float(cfg.fov_sdc_x),
             float(cfg.fov_sdc_y), _st())
        o['ok'].copy_(self._ok)
        return o

    def __call__(self, tracks):
        self.load(tracks)
        return self.run()


def rasterize(tracks, cfg=None, device='cuda', out=None):
    """Tracks -> {'ogm' [B,G,G,11,2], 'flow' [B,G,G,2], 'obs' [B,48,11,8], 'occ' [B,16,11,8], 'ok' [B]}, float32 tensors on `device`.
    out: a dict of tensors to write into (those named are reused, not reallocated)."""
    return Rasterizer(tracks.B, cfg, tracks.A, device, out)(tracks)


def model_inputs(outputs):
    """The keyword arguments of STrajNet.__call__ among rasterize's outputs (everything but 'ok')."""
    return {k: outputs[k] for k in ('ogm', 'flow', 'obs', 'occ')}


# ---------------------------------------------------------------------------------------------------- records in, records out
_MOTION = {'x': 'x', 'y': 'y', 'bbox_yaw': 'bbox_yaw', 'length': 'length', 'width': 'width', 'velocity_x': 'velocity_x',
           'velocity_y': 'velocity_y', 'valid': 'valid'}


def tracks_from_motion_example(payload):
    """A Waymo motion tf.Example (bytes) -> Tracks of one scene from its state/past/* [A, 10], state/current/* [A, 1], state/type and
    state/is_sdc features (FloatList / Int64List: data.parse_example_lists)."""
    feats = data.parse_example_lists(payload)
    try:
        A = feats['state/type'].size
        cols = {}
        for f, name in _MOTION.items():
            past, cur = feats[f'state/past/{name}'], feats[f'state/current/{name}']
            if past.size != A * (STEPS - 1) or cur.size != A:
                raise ValueError(f'state/*/{name}: {past.size} past and {cur.size} current values for {A} agents')
            cols[f] = np.concatenate([past.reshape(A, STEPS - 1), cur.reshape(A, 1)], 1).astype(np.float32)[None]
        return Tracks(type=feats['state/type'].reshape(1, A), is_sdc=feats['state/is_sdc'].reshape(1, A), **cols)
    except KeyError as e:
        raise ValueError(f'tracks_from_motion_example: feature {e.args[0]!r} is missing') from None


def motion_example(tracks, b=0):
    """The writer that matches tracks_from_motion_example (tests, synthetic records): scene b as a motion tf.Example."""
    feats = {'state/type': tracks.type[b].astype(np.float32), 'state/is_sdc': tracks.is_sdc[b].astype(np.int64)}      # state/type is a FloatList there
    for f, name in _MOTION.items():
        a = getattr(tracks, f)[b]
        a = a.astype(np.int64) if f == 'valid' else a                                                                # the valid flags are Int64Lists
        feats[f'state/past/{name}'], feats[f'state/current/{name}'] = a[:, :CUR].reshape(-1), a[:, CUR:].reshape(-1)
    return data.serialize_example_lists(feats)


def raster_example(outputs, b, map_image, centerlines, scenario_id):
    """Scene b of rasterize's outputs (tensors or arrays) as the {feature: bytes} of a reference TEST record (inference.py:67-96): ogm as
    bool bytes, vec_flow as float32, actors / occl_actors / centerlines as float64, map_image as the caller's int8 [256,256,3] bytes.
    data.decode_batch(..., test=True) and data.pack_example take it like any other record."""
    def host(name):
        t = outputs[name][b]
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    mi = np.asarray(map_image)
    if mi.dtype.itemsize != 1:
        raise ValueError(f'raster_example: map_image must hold one byte per element, got {mi.dtype}')
    return {'ogm': (host('ogm') != 0).astype(np.bool_).tobytes(), 'vec_flow': host('flow').astype('<f4').tobytes(),
            'actors': host('obs').astype('<f8').tobytes(), 'occl_actors': host('occ').astype('<f8').tobytes(),
            'map_image': mi.tobytes(), 'centerlines': np.asarray(centerlines, '<f8').tobytes(),
            'scenario/id': scenario_id if isinstance(scenario_id, bytes) else str(scenario_id).encode()}
