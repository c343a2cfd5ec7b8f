#!/usr/bin/env python
"""What rasterising agent tracks on the device costs (strajnet_amd/raster.py: Rasterizer.run = stj_raster_boxes + stj_raster_grids +
stj_raster_actors), at B = 8 and 32 scenes of A = 128 agents, the default 512 grid.

Per batch size one JSON line on stdout and in profiles/raster_<date>.jsonl:
  ms_per_batch, scenes_per_s   HIP events around --steps runs after --warmup runs, the inputs already on the device (median of --rounds)
  ms_boxes / ms_grids / ms_actors   the three launches timed one by one the same way
  write_gb_s, write_floor_share     the bytes the kernels MUST write (ogm + flow + obs + occ in float32; nothing else is large) over the
                                    time of the run / of stj_raster_grids alone, and that rate as a share of --hbm-write-gb-s (the
                                    streaming-store rate of the device: plain coalesced stores stream at about 6000 GB/s on an MI355X, the default)
  host_reference_scenes_per_s       raster_reference (NumPy, float32) on --host-scenes of the same tracks, the report included
Scenes: random agents within +-95 m of the SDC, speeds up to 15 m/s, lengths 0.5 .. 12 m, widths 0.4 .. 3 m, world offsets of km."""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from strajnet_amd.ops import _p, _st, call
from strajnet_amd.raster import CUR, STEPS, RasterConfig, Rasterizer, Tracks, raster_reference

ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='8,32')
ap.add_argument('--agents', type=int, default=128)
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--host-scenes', type=int, default=2)
ap.add_argument('--hbm-write-gb-s', type=float, default=6000.0)
ap.add_argument('--out', default=None)
a = ap.parse_args()


def random_tracks(B, A, seed):
    rng = np.random.default_rng(seed)
    yaw0 = rng.uniform(-np.pi, np.pi, (B, 1, 1))
    ang = -(np.pi / 2 - yaw0)
    p10 = rng.uniform(-95, 95, (B, A, 1, 2))
    vel = rng.uniform(-15, 15, (B, A, 1, 2))
    p10[:, 0], vel[:, 0] = 0.0, (0.0, 6.0)                       # agent 0 is the SDC, driving ahead
    w = np.linspace(-1.0, 0.0, STEPS)[None, None, :, None]
    p = p10 + vel * w
    c, s = np.cos(ang), np.sin(ang)
    off = rng.uniform(-8000, 8000, (B, 1, 1, 2)).round(2)
    x, y = c * p[..., 0] - s * p[..., 1] + off[..., 0], s * p[..., 0] + c * p[..., 1] + off[..., 1]
    vx, vy = c * vel[..., 0] - s * vel[..., 1], s * vel[..., 0] + c * vel[..., 1]
    yaw = rng.uniform(-np.pi, np.pi, (B, A, 1)) + np.zeros((B, A, STEPS))
    yaw[:, 0] = yaw0[:, 0]
    one = np.ones((B, A, STEPS))
    valid = (rng.random((B, A, STEPS)) > 0.05).astype(np.float32)
    valid[:, 0] = 1
    typ = rng.choice([1, 1, 1, 1, 2, 3], (B, A))
    typ[:, 0] = 1
    sdc = np.zeros((B, A), np.int32)
    sdc[:, 0] = 1
    return Tracks(x=x, y=y, bbox_yaw=yaw, length=one * rng.uniform(0.5, 12.0, (B, A, 1)), width=one * rng.uniform(0.4, 3.0, (B, A, 1)),
                  velocity_x=one * vx, velocity_y=one * vy, valid=valid, type=typ, is_sdc=sdc)


def timed(fn, steps, warmup, rounds):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms))


assert torch.cuda.is_available(), 'bench_raster.py needs a GPU'
cfg = RasterConfig()
date = datetime.date.today().strftime('%Y%m%d')
path = a.out or os.path.join(ROOT, 'profiles', f'raster_{date}.jsonl')
os.makedirs(os.path.dirname(path), exist_ok=True)
host_rate = None
for B in (int(b) for b in a.batches.split(',')):
    tracks = random_tracks(B, a.agents, B)
    r = Rasterizer(B, cfg, a.agents)
    r.load(tracks)
    ppm, sx, sy = float(cfg.pixels_per_meter), float(cfg.sdc_x), float(cfg.sdc_y)
    parts = {
        'boxes': lambda: call('stj_raster_boxes', _p(r.state), _p(r.meta[0]), _p(r.meta[1]), _p(r.ws), B, a.agents, cfg.grid, ppm, sx, sy, _st()),
        'grids': lambda: call('stj_raster_grids', _p(r.ws), _p(r.out['ogm']), _p(r.out['flow']), B, a.agents, cfg.grid, ppm, sx, sy,
                              cfg.points_length, cfg.points_width, _st()),
        'actors': lambda: call('stj_raster_actors', _p(r.ws), _p(r.meta[0]), _p(r.out['obs']), _p(r.out['occ']), B, a.agents, cfg.fov_grid, ppm,
                               float(cfg.fov_sdc_x), float(cfg.fov_sdc_y), _st()),
    }
    ms_all = timed(r.run, a.steps, a.warmup, a.rounds)
    ms = {k: timed(f, a.steps, a.warmup, a.rounds) for k, f in parts.items()}
    nbytes = sum(r.out[k].numel() * 4 for k in ('ogm', 'flow', 'obs', 'occ'))
    grid_bytes = sum(r.out[k].numel() * 4 for k in ('ogm', 'flow'))
    if host_rate is None and a.host_scenes > 0:
        sub = tracks.scenes(slice(0, min(B, a.host_scenes)))
        t0 = time.perf_counter()
        raster_reference(sub, cfg, np.float32)
        host_rate = sub.B / (time.perf_counter() - t0)
    line = {'tool': 'bench_raster', 'date': date, 'B': B, 'A': a.agents, 'grid': cfg.grid, 'steps': a.steps, 'rounds': a.rounds,
            'ms_per_batch': round(ms_all, 4), 'scenes_per_s': round(B / ms_all * 1e3, 1),
            'ms_boxes': round(ms['boxes'], 4), 'ms_grids': round(ms['grids'], 4), 'ms_actors': round(ms['actors'], 4),
            'bytes_written': nbytes, 'write_gb_s': round(nbytes / ms_all / 1e6, 1), 'grids_write_gb_s': round(grid_bytes / ms['grids'] / 1e6, 1),
            'hbm_write_gb_s_assumed': a.hbm_write_gb_s, 'write_floor_share': round(nbytes / ms_all / 1e6 / a.hbm_write_gb_s, 3),
            'grids_write_floor_share': round(grid_bytes / ms['grids'] / 1e6 / a.hbm_write_gb_s, 3),
            'set_ogm_cells': int(r.out['ogm'].sum().item()), 'host_reference_scenes_per_s': None if host_rate is None else round(host_rate, 3),
            'device': torch.cuda.get_device_name(0)}
    print(json.dumps(line), flush=True)
    with open(path, 'a') as f:
        f.write(json.dumps(line) + '\n')
