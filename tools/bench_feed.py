#!/usr/bin/env python
"""What feeding a captured step from host memory costs, by host format.

  --config train   the B = 8 bf16 train step (GraphedTrainStep + Nadam), as bench.py's headline
  --config infer   the B = 32 fp16 GraphedForward with the agent pipeline, as bench.py --infer

Feed modes, all on the SAME captured graph in one process: `resident` (inputs stay in HBM, no feed), `f32` (HostFeed, decoded float32
tensors), `raw` (HostFeed, the record's own bytes: bool grids and the int8 map one byte per element, float32 flows), `packed`
(PackedFeed: bool grids one bit per element, flows as mask + non-zero words, int8 map), `pool` (ResidentFeed, DESIGN 4u: --pool-scenes x B
blob scenes packed the same way stay in HBM, every step gathers a freshly sampled batch by device index, nothing is uploaded), `replace`
(opt-in through --modes: the same pool built by ResidentPool.empty and filled by a PoolWriter from raw records; every
--replace-every steps one put() of B raw records replaces B slots in front of the landing), `window` / `window-raw` (opt-in
through --modes: WindowFeed over a ShuffleWindow of --pool-scenes x B slots whose source cycles over the same records, packed by
pack_example / raw; consumed slots are refilled by the window's worker on its own stream; `window@K` sets the lag, --lag the default).  Per visit
every mode is timed TWICE in a row,
the modes alternating, --pairs visits: the spread of repeated runs of one mode is measured in the same call.  One JSON line per run:
scenes/s, bytes uploaded per scene, the density of the synthetic scene.

  --all            runs both configs as child processes, each under its own `timeout`; --out FILE collects their lines
  --trace          a few PackedFeed and ResidentFeed landings at the config's shapes and nothing else (no model): the workload of a
                   `rocprofv3 --kernel-trace --stats` run; prints the bytes each unpack / gather kernel reads and writes per landing
  --trace-replace  the same for the writer: 10 commits of B raw records and 10 gathers of the slots they went to, no model
  --replace-put    what one PoolWriter.put of B raw records costs at --put-grid / --put-out (default the real 512 / 256 geometry), no model:
                   host copy into pinned staging, H2D alone (events on the copy stream), commit alone (events on the main stream), the
                   whole put (host clock to a device synchronise), and the host's pack_example over the same records

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
ap.add_argument('--trace-replace', action='store_true')
ap.add_argument('--replace-put', action='store_true')
ap.add_argument('--replace-every', type=int, default=8, help='mode replace: one put of B records every this many steps')
ap.add_argument('--lag', type=int, default=4, help='modes window / window-raw: steps between the draw of a group and its admission')
ap.add_argument('--put-grid', type=int, default=512)
ap.add_argument('--put-out', type=int, default=256)
ap.add_argument('--put-reps', type=int, default=10)
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
               '--pool-scenes', str(a.pool_scenes), '--replace-every', str(a.replace_every), '--lag', str(a.lag)]
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
from strajnet_amd.data import (POOL_NAMES, HostFeed, PackedFeed, PoolLayout, ResidentFeed, ResidentPool, SparseHost, WindowFeed, bits_host,
                               feature_spec, pack_bits, pack_example, pack_sparse)

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


def blob_records(B, seed, blobs, grid=256, out=256):
    """B raw records ({feature: bytes}, as parse_example gives them for the reference's own files) of blob scenes at (grid, out): the
    ground truth at the full grid, centre-cropped to `out` by whoever decodes it."""
    x = blob_scenes(B, seed, blobs, grid, grid)
    as_bytes = {'bool': lambda v: (v != 0).to(torch.uint8), 'int8': lambda v: torch.round(v * 256.0).to(torch.int8),
                'float32': lambda v: v.float(), 'float64': lambda v: v.double()}
    recs = []
    for b in range(B):
        rec = {}
        for name, (dtype, shape, crop, scale) in feature_spec(grid, out).items():
            v = as_bytes[dtype](x[POOL_NAMES[name]][b]).contiguous().numpy()
            assert v.shape == tuple(shape), (name, v.shape, shape)
            rec[name] = v.tobytes()
        recs.append(rec)
    return recs


def record_capacity(batches, grid, out):
    """{key: value words per slot}: the largest present-word count of any sparse feature over the records, rounded up to 1024."""
    spec = feature_spec(grid, out)
    cap = {}
    for name in ('vec_flow', 'gt_flow', 'origin_flow'):
        dtype, shape, crop, _ = spec[name]
        most = 0
        for recs in batches:
            for r in recs:
                v = np.frombuffer(r[name], '<u4').reshape(shape)
                if crop is not None:
                    v = v[:, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
                most = max(most, int(np.count_nonzero(v)))
        cap[POOL_NAMES[name]] = -(-max(most, 1) // 1024) * 1024
    return cap


class ReplaceFeed(ResidentFeed):
    """ResidentFeed over a pool that a PoolWriter refills: every `every` landings one put() of B raw records replaces B slots (walking
    round the pool) in front of the gathers, on the same stream."""

    def __init__(self, static, pool, sampler, batches, every):
        super().__init__(static, pool, sampler)
        self.writer, self.batches, self.every, self.count, self.puts = pool.writer(self.B), batches, max(1, every), 0, 0

    def land(self, idx=None):
        if self.count % self.every == 0:
            first = (self.puts * self.B) % self.pool.N
            self.writer.put(list(range(first, first + self.B)), self.batches[self.puts % len(self.batches)])
            self.puts += 1
        self.count += 1
        super().land(idx)


def make_replace_feed(static):
    """-> (ReplaceFeed over ResidentPool.empty of --pool-scenes x B slots, every slot filled by the writer; raw bytes uploaded per batch,
    averaged over --replace-every steps)."""
    batches = [blob_records(B, a.seed + 1 + j, a.blobs) for j in range(a.pool_scenes)]
    pool = ResidentPool.empty(a.pool_scenes * B, dev, 256, 256, capacity=record_capacity(batches, 256, 256))
    feed = ReplaceFeed(static, pool, pool.sampler(B, seed=a.seed), batches, a.replace_every)
    for j, recs in enumerate(batches):
        ok = feed.writer.put(list(range(j * B, (j + 1) * B)), recs)
        assert ok.cpu().tolist() == [1] * B
    return feed, sum(len(v) for v in batches[0][0].values()) * B / feed.every


_WINDOW_RECORDS = {}


def make_window_feed(static, mode):
    """-> (WindowFeed over a ShuffleWindow of --pool-scenes x B slots, bytes uploaded per batch).  mode: window[-raw][@lag]; the source
    cycles for ever over --pool-scenes x B blob records, already parsed (and, for `window`, already packed): what a loader thread hands
    over.  The window's worker validates every record again on each pass."""
    import itertools
    kind, _, lag = mode.partition('@')
    packed, lag = kind == 'window', int(lag or a.lag)
    if 'raw' not in _WINDOW_RECORDS:
        batches = [blob_records(B, a.seed + 1 + j, a.blobs) for j in range(a.pool_scenes)]
        _WINDOW_RECORDS['capacity'] = record_capacity(batches, 256, 256)
        _WINDOW_RECORDS['raw'] = [r for recs in batches for r in recs]
    if packed and 'packed' not in _WINDOW_RECORDS:
        _WINDOW_RECORDS['packed'] = [pack_example(r, 256, 256) for r in _WINDOW_RECORDS['raw']]
    recs = _WINDOW_RECORDS['packed' if packed else 'raw']
    pool = ResidentPool.empty(a.pool_scenes * B, dev, 256, 256, capacity=_WINDOW_RECORDS['capacity'])
    feed = WindowFeed(static, pool.window(B, itertools.cycle(recs), packed=packed, lag=lag, seed=a.seed))
    return feed, sum(len(v) for r in recs for v in r.values()) * B / len(recs)


def writer_bytes(writer):
    """Per key: the kernels of one commit and the bytes they read and write (the source is read twice for a sparse key: count + commit)."""
    per = {}
    nb = writer.B
    for name, key, e, nbytes, geom in writer.features:
        n = e['n']
        if e['kind'] == 'bits':
            per[key] = {'kernel': 'pack_bits_kernel', 'read_bytes': nb * n, 'written_bytes': nb * n // 8}
        elif e['kind'] == 'sparse':
            stage = writer.offs_stage[key].cpu().numpy().view(np.uint32)
            present = int(stage[:, -1].sum())
            per[key] = {'kernel': 'pack_count_kernel + pack_commit_kernel', 'count_read_bytes': nb * n * 4,
                        'commit_read_bytes': nb * n * 4, 'commit_written_bytes': nb * (n // 8 + 4 * stage.shape[1]) + 4 * present}
        else:
            per[key] = {'kernel': 'put_raw_kernel', 'read_bytes': nb * nbytes, 'written_bytes': nb * nbytes}
    return per


if a.replace_put:
    grid, out, reps = a.put_grid, a.put_out, a.put_reps
    batches = [blob_records(B, a.seed + j, a.blobs, grid, out) for j in range(2)]
    raw_bytes = sum(len(v) for v in batches[0][0].values())
    t0 = time.perf_counter()
    packed = [pack_example(r, grid, out) for r in batches[0]]
    t_pack = time.perf_counter() - t0
    pool = ResidentPool.empty(2 * B, dev, grid, out, capacity=record_capacity(batches, grid, out))
    w = pool.writer(B)
    slots = [list(range(B)), list(range(B, 2 * B))]
    for j in range(2):                                                   # warm-up: code objects, pinned pages
        assert w.put(slots[j], batches[j]).cpu().tolist() == [1] * B
    torch.cuda.synchronize()
    main = torch.cuda.current_stream(dev)
    t_put, t_stage_host, t_h2d, t_commit = [], [], [], []
    for r in range(reps):
        t0 = time.perf_counter()
        w._set_slots(slots[r % 2])
        w.stage(batches[r % 2])
        t1 = time.perf_counter()
        w.commit()
        torch.cuda.synchronize()
        t_put.append(time.perf_counter() - t0)
        t_stage_host.append(t1 - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(w.copy):                                  # the H2D copies of stage() again, without its host-side fill
            e0.record(w.copy)
            w.unpacked.upload(B)
            e1.record(w.copy)
        torch.cuda.synchronize()
        t_h2d.append(e0.elapsed_time(e1) * 1e-3)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(main)
        w.commit()
        c1.record(main)
        torch.cuda.synchronize()
        t_commit.append(c0.elapsed_time(c1) * 1e-3)
    ms = lambda v: {'mean': round(1e3 * float(np.mean(v)), 3), 'min': round(1e3 * min(v), 3), 'max': round(1e3 * max(v), 3)}
    emit({'mode': 'replace-put', 'grid': grid, 'out': out, 'batch': B, 'reps': reps, 'blobs': a.blobs, 'raw_bytes_per_scene': raw_bytes,
          'pool_bytes_per_scene': round(pool.nbytes / pool.N), 'put_ms': ms(t_put), 'stage_host_ms': ms(t_stage_host), 'h2d_ms': ms(t_h2d),
          'h2d_GBps': round(raw_bytes * B / float(np.mean(t_h2d)) / 1e9, 2), 'commit_ms': ms(t_commit),
          'host_pack_example_ms': round(1e3 * t_pack, 1), 'launches_per_commit': 2 * 3 + 10})
    sys.exit(0)

if a.trace_replace:
    batches = [blob_records(B, a.seed + j, a.blobs) for j in range(2)]
    pool = ResidentPool.empty(2 * B, dev, 256, 256, capacity=record_capacity(batches, 256, 256))
    pool.wait()
    w = pool.writer(B)
    static = {k: torch.zeros((B,) + e['shape'], device=dev) for k, e in pool.layout.entries.items()}
    for j in range(2):
        assert w.put(list(range(j * B, (j + 1) * B)), batches[j]).cpu().tolist() == [1] * B
    for _ in range(10):
        w.commit()
    idx = torch.arange(B, 2 * B, dtype=torch.int32, device=dev)
    for _ in range(10):
        pool.gather_into(static, idx)
    torch.cuda.synchronize()
    emit({'mode': 'trace', 'feed': 'replace', 'config': 'train', 'batch': B, 'commits': 12, 'gathers': 10, 'blobs': a.blobs,
          'pool_scenes': pool.N, 'pool_bytes_per_scene': pool.nbytes / pool.N, 'per_commit': writer_bytes(w)})
    sys.exit(0)

xh = blob_scenes(B, a.seed, a.blobs)
density ={k: round(float((xh[k] != 0).float().mean()), 5) for k in BITS + SPARSE}

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
    feeds[m] = ((None, 0) if m == 'resident' else make_pool_feed(graphed.static) if m == 'pool' else make_replace_feed(graphed.static)
                if m == 'replace' else make_window_feed(graphed.static, m) if m.startswith('window') else make_feed(m, graphed.static, xh))
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
                  **({'pool_scenes': feed.pool.N, 'pool_bytes_per_scene': round(feed.pool.nbytes / feed.pool.N)}
                     if m in ('pool', 'replace') or m.startswith('window') else {}),
                  **({'lag': feed.window.lag, 'draws': feed.window.steps, 'stalls': feed.window.stalls, 'skipped': len(feed.window.skipped),
                      'bad': int(feed.window.bad.item())} if m.startswith('window') else {}),
                  **({'replace_every': feed.every, 'puts': feed.puts} if m == 'replace' else {})})
for feed, _ in feeds.values():
    if feed is not None:
        feed.wait_uploaded()
        feed.close()
