#!/usr/bin/env python
"""What feeding a captured step from host memory costs, by host format.

  --config train   the B = 8 bf16 train step (GraphedTrainStep + Nadam), as bench.py's headline
  --config infer   the B = 32 fp16 GraphedForward with the agent pipeline, as bench.py --infer

Feed modes, all on the SAME captured graph in one process: `resident` (inputs stay in HBM, no feed), `f32` (HostFeed, decoded float32
tensors), `raw` (HostFeed, the record's own bytes: bool grids and the int8 map one byte per element, float32 flows), `packed`
(PackedFeed: bool grids one bit per element, flows as mask + non-zero words, int8 map), `pool` (ResidentFeed, DESIGN 4u: --pool-scenes x B
blob scenes packed the same way stay in HBM, every step gathers a freshly sampled batch by device index, nothing is uploaded).  Per visit
every mode is timed TWICE in a row,
the modes alternating, --pairs visits: the spread of repeated runs of one mode is measured in the same call.  One JSON line per run:
scenes/s, bytes uploaded per scene, the density of the synthetic scene.

  --all            runs both configs as child processes, each under its own `timeout`; --out FILE collects their lines
  --trace          a few PackedFeed and ResidentFeed landings at the config's shapes and nothing else (no model): the workload of a
                   `rocprofv3 --kernel-trace --stats` run; prints the bytes each unpack / gather kernel reads and writes per landing

The scenes are synthetic: --blobs rectangular vehicles per scene on a zero background, occupancy in every time step, flow non-zero only
inside them (random-normal flow would be dense, and `sparse` then larger than raw).  Real Waymo densities are not available here.
Every timing is a host clock around --steps steps that end in a device synchronise, after --warmup steps, profiler off."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='train', choices=['train', 'infer'])
ap.add_argument('--modes', default='resident,f32,raw,packed,pool')
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--pairs', type=int, default=2)
ap.add_argument('--batch', type=int, default=None)
ap.add_argument('--blobs', type=int, default=24, help='vehicles per scene')
ap.add_argument('--seed', type=int, default=1234)
ap.add_argument('--pool-scenes', type=int, default=8, help='mode pool: the pool holds this many batches of scenes')
ap.add_argument('--all', action='store_true')
ap.add_argument('--trace', action='store_true')
ap.add_argument('--timeout', type=int, default=420, help='--all: seconds per child')
ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
a = ap.parse_args()


def emit(d):
    line = json.dumps(d)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if a.all:
    rc = 0
    for cfg in ('train', 'infer'):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--config', cfg, '--modes', a.modes,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--pairs', str(a.pairs), '--blobs', str(a.blobs), '--seed', str(a.seed),
               '--pool-scenes', str(a.pool_scenes)]
        if a.out:
            cmd += ['--out', a.out]
        r = subprocess.run(cmd)
        if r.returncode != 0:            # a fault, an abort or a time limit: nothing more is started on the GPU
            print(f'bench_feed.py: --config {cfg} ended with status {r.returncode}; stopping', file=sys.stderr)
            sys.exit(r.returncode)
    sys.exit(rc)

import numpy as np
import torch

import bench
from strajnet_amd.data import (HostFeed, PackedFeed, PoolLayout, ResidentFeed, ResidentPool, SparseHost, bits_host, pack_bits,
                               pack_sparse)

assert torch.cuda.is_available(), 'bench_feed.py needs a GPU'
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
B = a.batch or (8 if a.config == 'train' else 32)


def blob_scenes(B, seed, blobs, grid=256, H=256):
    """Host tensors with bench.synth_batch's keys and shapes; the rasters are `blobs` rectangles per scene on zero: each vehicle
    occupies its rectangle in all 11 input time steps (drifting a cell per step) and in the 8 future waypoints, and carries one
    (dx, dy) -- the flow planes are non-zero only inside the rectangles."""
    x = {k: v.cpu() for k, v in bench.synth_batch(B, seed, 'cpu', grid).items()}
    rng = np.random.default_rng(seed)
    ogm = np.zeros((B, grid, grid, 11, 2), np.float32)
    flow = np.zeros((B, grid, grid, 2), np.float32)
    gt_obs, gt_occ = np.zeros((B, 8, H, H, 1), np.float32), np.zeros((B, 8, H, H, 1), np.float32)
    gt_flow, origin = np.zeros((B, 8, H, H, 2), np.float32), np.zeros((B, 8, H, H, 1), np.float32)
    for b in range(B):
        for v in range(blobs):
            h, w = rng.integers(4, 14, 2)
            y, x0 = rng.integers(12, grid - 40), rng.integers(12, grid - 40)
            d = rng.normal(size=2).astype(np.float32) * 2
            ch = int(v % 4 == 0)                                           # every fourth vehicle is a pedestrian / cyclist channel
            for t in range(11):
                ogm[b, y + t // 3:y + t // 3 + h, x0 + t // 4:x0 + t // 4 + w, t, ch] = 1
            flow[b, y + 3:y + 3 + h, x0 + 2:x0 + 2 + w] = d
            occluded = v % 5 == 0
            for k in range(8):
                yy, xx = y + 3 + k, x0 + 2 + k
                (gt_occ if occluded else gt_obs)[b, k, yy:yy + h, xx:xx + w] = 1
                gt_flow[b, k, yy:yy + h, xx:xx + w] = d * (k + 1)
                origin[b, k, yy:yy + h, xx:xx + w] = 0.9
    for k, v in dict(ogm=ogm, flow=flow, gt_obs=gt_obs, gt_occ=gt_occ, gt_flow=gt_flow, origin_flow=origin).items():
        x[k] = torch.from_numpy(v)
    return x


BITS, SPARSE, INT8 = ('ogm', 'gt_obs', 'gt_occ'), ('flow', 'gt_flow', 'origin_flow'), ('map_img',)


def make_feed(mode, static, xh):
    """-> (feed, bytes uploaded per batch)."""
    host, raw, packed = {}, {}, {}
    for k, v in xh.items():
        if k not in static:
            continue
        if mode in ('raw', 'packed') and k in INT8:
            host[k], raw[k] = torch.round(v * 256.0).to(torch.int8).view(torch.uint8).contiguous().pin_memory(), 'int8'
        elif mode == 'raw' and k in BITS:
            host[k], raw[k] = (v != 0).to(torch.uint8).contiguous().pin_memory(), 'bool'
        elif mode == 'packed' and k in BITS:
            host[k], packed[k] = bits_host((v != 0).numpy()), 'bits'
        elif mode == 'packed' and k in SPARSE:
            host[k], packed[k] = SparseHost(v.shape[0], v[0].numel()).fill(v), 'sparse'
        else:
            host[k] = v.float().contiguous().pin_memory()
    if mode == 'packed':
        feed = PackedFeed(static, host, packed=packed, raw=raw)
        return feed, feed.upload_bytes()
    return HostFeed(static, host, raw), sum(h.numel() * h.element_size() for h in host.values())


def make_pool_feed(static):
    """-> (ResidentFeed over a pool of --pool-scenes x B blob scenes under the keys of `static`, 0 bytes uploaded per batch).  The scenes
    are drawn B at a time, so the host never holds more than one batch decoded."""
    cols = {k: [] for k in xh if k in static}
    for j in range(a.pool_scenes):
        xj = blob_scenes(B, a.seed + 1 + j, a.blobs)
        for k, col in cols.items():
            v = xj[k].float().numpy()
            if k in BITS:
                col += [pack_bits(s) for s in v]
            elif k in SPARSE:
                col += [pack_sparse(s) for s in v]
            elif k in INT8:
                col += list(np.round(v * 256.0).astype(np.int8))
            else:
                col += list(v.view(np.uint32))
    lay = PoolLayout()
    for k, col in cols.items():
        shape = tuple(static[k].shape[1:])
        if k in BITS:
            lay.add_bits(k, col, shape)
        elif k in SPARSE:
            lay.add_sparse(k, col, int(np.prod(shape)), shape)
        elif k in INT8:
            lay.add_raw(k, col, 'int8', 1.0 / 256.0, shape)
        else:
            lay.add_raw(k, col, 'float32', 1.0, shape)
    pool = ResidentPool(lay, dev)
    pool.wait()
    return ResidentFeed(static, pool, pool.sampler(B, seed=a.seed)), 0


def pool_bytes(feed):
    """Per key: the kernel and the bytes the last landing read and wrote (the index, 4 B per scene, on top of every read)."""
    idx = feed.idx.cpu().numpy()
    per = {}
    for k, e in feed.pool.layout.entries.items():
        if k not in feed.static:
            continue
        n = e['n']
        if e['kind'] == 'bits':
            kernel, read = 'gather_bits_kernel', B * n // 8
        elif e['kind'] == 'sparse':
            present = int((e['val_base'][idx + 1] - e['val_base'][idx]).sum())
            kernel, read = 'gather_sparse_kernel', B * (e['mask'].shape[1] + e['offs'].shape[1] + 2) * 4 + 4 * present
        else:
            kernel, read = 'gather_raw_kernel', B * n * e['data'].itemsize
        per[k] = {'kernel': kernel, 'written_bytes': B * n * 4, 'read_bytes': read + 4 * B}
    return per


xh = blob_scenes(B, a.seed, a.blobs)
density = {k: round(float((xh[k] != 0).float().mean()), 5) for k in BITS + SPARSE}

if a.trace:
    keys = ('ogm', 'map_img', 'obs', 'occ', 'flow') if a.config == 'infer' else tuple(xh)
    static = {k: torch.zeros(xh[k].shape, device=dev) for k in keys}
    feed, nbytes = make_feed('packed', static, xh)
    feed.start()
    for _ in range(10):
        feed.land()
    torch.cuda.synchronize()
    feed.wait_uploaded()
    feed.close()
    per = {k: {'kernel': 'unpack_bits_kernel' if k in BITS else 'unpack_sparse_kernel', 'written_bytes': static[k].numel() * 4,
               'read_bytes': (static[k].numel() // 8 if k in BITS else feed.sparse[k].nbytes)} for k in keys if k in BITS + SPARSE}
    emit({'mode': 'trace', 'config': a.config, 'batch': B, 'landings': 10, 'blobs': a.blobs, 'density': density,
          'upload_bytes_per_scene': nbytes / B, 'per_landing': per})
    feed, _ = make_pool_feed(static)
    for _ in range(10):
        feed.land()
    torch.cuda.synchronize()
    emit({'mode': 'trace', 'feed': 'pool', 'config': a.config, 'batch': B, 'landings': 10, 'blobs': a.blobs, 'pool_scenes': feed.pool.N,
          'pool_bytes_per_scene': feed.pool.nbytes / feed.pool.N, 'per_landing': pool_bytes(feed)})
    sys.exit(0)

from strajnet_amd import STrajNet

if a.config == 'train':
    from strajnet_amd import Nadam, OGMFlow_loss, OccupancyFlowTaskConfig
    from strajnet_amd.graph import GraphedTrainStep
    model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.bfloat16, device=dev, seed=0, dropout_seed=0)
    loss_fn = OGMFlow_loss(OccupancyFlowTaskConfig(256, 256, 8), ogm_weight=1000.0, occ_weight=1000.0, flow_weight=1.0, replica=1.0,
                           flow_origin_weight=1000.0, no_use_warp=False, use_pred=False, use_focal_loss=False, use_gt=True)
    opt = Nadam.for_model(model, lr=1e-4)
    graphed = GraphedTrainStep(model, loss_fn, {k: v.to(dev) for k, v in xh.items()})

    def step():
        graphed()
        opt.step()
else:
    from strajnet_amd.graph import GraphedForward
    model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float16, device=dev, seed=0)
    graphed = GraphedForward(model, {k: v.to(dev) for k, v in xh.items()}, pipeline_agents=True)

    def step():
        graphed()
        graphed.prefetch_agents()        # the agent branch of the batch that has just landed runs under this replay


def timed(feed):
    def one():
        if feed is not None:
            feed.land()
        step()
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


modes = a.modes.split(',')
feeds = {}
for m in modes:
    feeds[m] = (None, 0) if m == 'resident' else make_pool_feed(graphed.static) if m == 'pool' else make_feed(m, graphed.static, xh)
    if feeds[m][0] is not None:
        feeds[m][0].start()
for visit in range(a.pairs):
    for m in modes:
        feed, nbytes = feeds[m]
        for rep in range(2):
            dt = timed(feed)
            emit({'config': a.config, 'mode': m, 'visit': visit, 'rep': rep, 'batch': B, 'steps': a.steps, 'warmup': a.warmup,
                  'scenes_per_s': round(B * a.steps / dt, 1), 'ms_per_step': round(dt / a.steps * 1e3, 4),
                  'upload_bytes_per_scene': round(nbytes / B), 'blobs': a.blobs, 'density': density,
                  **({'pool_scenes': feed.pool.N, 'pool_bytes_per_scene': round(feed.pool.nbytes / feed.pool.N)} if m == 'pool' else {})})
for feed, _ in feeds.values():
    if feed is not None:
        feed.wait_uploaded()
        feed.close()
