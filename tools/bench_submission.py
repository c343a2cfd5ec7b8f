#!/usr/bin/env python
"""What bringing the inference result to the host costs (config 4: B = 32 fp16, GraphedForward under replay, agent pipeline on).

  --mode rows   scenes/s for (a) no read-back (bench.py --infer's figure), (b) the float32 output copied to pinned memory each step,
                (c) quantised output + ResultDrain, (d) as (c) plus zlib compression of every scene on 16 threads, (e) the graph that
                also compresses on the device (GraphedForward(quantized=True, compressed=True, compress_level=--level)) + ResultDrain,
                no host zlib; bytes per scene of (d) and (e) side by side; (f) the graph that also frames the streams on the device
                (framed=True) + ResultDrain + SubmissionWriter into a BytesIO (rewound per batch): a submission file's bytes; (g) as
                (e), each scene framed on the host with frame_reference and written the same way.  --rows picks a subset.
  --mode ab     GraphedForward(quantized=True) with the quantising gather (stj_outconv_pair_gather_q) against the same graph built from
                stj_outconv_pair_gather + stj_quantize_waypoints, alternating, --pairs times; each build is timed TWICE in a row per
                visit, so the spread of repeated runs of the same build is measured in the same call
  --mode trace  a few replays of both quantised graphs and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run
  --sparse      (instead of a mode) random weights give noise-like planes, which the device-side compressor mostly stores; this fills a
                static quantised buffer ONCE with synthetic sparse planes (seeded blobs on a zero background) and times
                stj_compress_waypoints at --level (captured) + ResultDrain alone against host compress_batch of the same bytes on --threads threads.
                With --trace-only: a few replays of the captured compression, unframed then framed, and nothing else, for a kernel
                trace.  With --mode ab: the device entry pair, stj_compress_waypoints_framed against stj_compress_waypoints_level on
                the same Q and level, each captured; device events around --steps replays; per round the framed chain once and the
                unframed one twice, --pairs rounds alternating.

Every timing is a host clock around `--steps` replays that end in a device synchronise, after `--warmup` replays, profiler off.
One JSON line per mode on stdout."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--mode', default='rows', choices=['rows', 'ab', 'trace'])
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--warmup', type=int, default=20)
ap.add_argument('--pairs', type=int, default=3)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--threads', type=int, default=16)
ap.add_argument('--chunk-bytes', type=int, default=3 << 19)
ap.add_argument('--sparse', action='store_true')
ap.add_argument('--noise', action='store_true', help='with --sparse: uniformly random planes instead (the stored fallback everywhere)')
ap.add_argument('--trace-only', action='store_true')
ap.add_argument('--rows', default='abcdefg', help='--mode rows: the rows to measure')
ap.add_argument('--level', type=int, default=1, choices=[1, 2], help='compression level of row (e) and of --sparse: 1 fixed, 2 dynamic Huffman code')
a = ap.parse_args()

import bench
import io
from strajnet_amd import (STrajNet, ResultDrain, compress_batch, compression_pool, QuantizedWaypoints, CompressedWaypoints,
                          compress_waypoints, FramedWaypoints, SubmissionWriter, frame_reference)
from strajnet_amd.submission import _scene_prefix
from strajnet_amd.graph import GraphedForward

assert torch.cuda.is_available(), 'bench_submission.py needs a GPU'
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
B = a.batch


def sparse_planes(B, H, W, seed, noise=False):
    """[B, 32*H*W] uint8 in QuantizedWaypoints' layout: per plane a zero background with a dozen rectangular blobs -- occupancy: a
    plateau of one value with a one-cell rim of half of it; flow: one (dx, dy) per blob."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if noise:
        return torch.from_numpy(rng.integers(0, 256, (B, 32 * H * W), dtype=np.uint8))
    buf = np.zeros((B, 24, 2 * H * W), np.uint8)
    for b in range(B):
        for p in range(24):
            img = np.zeros((H, W, 2 if p >= 16 else 1), np.uint8)
            for _ in range(12):
                h, w = rng.integers(4, 28, 2)
                y, x0 = rng.integers(0, H - h), rng.integers(0, W - w)
                if p >= 16:
                    img[y:y + h, x0:x0 + w] = rng.integers(0, 256, 2, dtype=np.uint8)
                else:
                    v = rng.integers(32, 256)
                    img[y:y + h, x0:x0 + w] = v // 2
                    img[y + 1:y + h - 1, x0 + 1:x0 + w - 1] = v
            buf[b, p, :img.size] = img.reshape(-1)
    n = H * W
    out = np.concatenate([buf[:, :16, :n].reshape(B, -1), buf[:, 16:].reshape(B, -1)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(out))


if a.sparse:
    H = 256
    host_q = QuantizedWaypoints(sparse_planes(B, H, H, 1234, a.noise), H, H)
    qw = QuantizedWaypoints(host_q.buf.to(dev), H, H)
    cw = CompressedWaypoints.empty(B, H, H, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        compress_waypoints(qw, out=cw, level=a.level)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        compress_waypoints(qw, out=cw, level=a.level)
    if a.trace_only or a.mode == 'ab':
        fw = FramedWaypoints.empty(B, H, H, dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            compress_waypoints(qw, out=fw, level=a.level, framed=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gfr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gfr):
            compress_waypoints(qw, out=fw, level=a.level, framed=True)
    if a.trace_only:
        for gr in (g, gfr):
            for _ in range(10):
                gr.replay()
            torch.cuda.synchronize()
        print(json.dumps({'mode': 'sparse-trace', 'batch': B, 'level': a.level, 'replays_per_graph': 10 + 1, 'noise': a.noise,
                          'input_bytes': qw.buf.numel(), 'stream_bytes': cw.nbytes, 'framed_bytes': fw.nbytes}), flush=True)
        sys.exit(0)
    if a.mode == 'ab':
        def ms(gr):
            for _ in range(a.warmup):
                gr.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps
        assert fw.streams(B - 1) == cw.streams(B - 1)
        rounds = [{'framed': [round(ms(gfr), 5)], 'unframed': [round(ms(g), 5) for _ in range(2)]} for _ in range(a.pairs)]
        un = sorted(t for r in rounds for t in r['unframed'])
        fr = sorted(t for r in rounds for t in r['framed'])
        med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        spread = (un[-1] - un[0]) / un[0]
        ratio = med(fr) / med(un)
        print(json.dumps({'mode': 'sparse-ab', 'noise': a.noise, 'batch': B, 'level': a.level, 'steps': a.steps, 'warmup': a.warmup,
                          'unit': 'ms per captured chain', 'rounds': rounds, 'framed_median': round(med(fr), 5),
                          'unframed_median': round(med(un), 5), 'unframed_spread': round(spread, 4), 'ratio': round(ratio, 4),
                          'gate': '<= 1.02 + spread', 'within_gate': ratio <= 1.02 + spread, 'stream_bytes': cw.nbytes,
                          'framed_bytes': fw.nbytes}), flush=True)
        sys.exit(0)
    drain = ResultDrain(cw, depth=3, chunk_bytes=a.chunk_bytes)
    pending = [0]

    def step():
        g.replay()
        drain.submit()
        pending[0] += 1
        if pending[0] > 1:
            drain.take()
            pending[0] -= 1

    def finish():
        while pending[0]:
            drain.take()
            pending[0] -= 1
    for _ in range(a.warmup):
        step()
    finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    finish()
    torch.cuda.synchronize()
    dev_rate = B * a.steps / (time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    drain.close()
    pool = compression_pool(a.threads)
    compress_batch(host_q, pool)
    reps = max(1, min(5, a.steps))
    t0 = time.perf_counter()
    for _ in range(reps):
        comp = compress_batch(host_q, pool)
    host_rate = B * reps / (time.perf_counter() - t0)
    pool.shutdown()
    zl = sum(len(s) for scene in comp for wp in scene for s in wp)
    print(json.dumps({'mode': 'sparse', 'noise': a.noise, 'batch': B, 'level': a.level, 'stream_bytes': cw.nbytes, 'steps': a.steps, 'warmup': a.warmup, 'threads': a.threads,
                      'device_compress_drain_scenes_per_s': round(dev_rate, 1), 'host_zlib_scenes_per_s': round(host_rate, 1),
                      'compress_ms_per_batch': round(e0.elapsed_time(e1) / 20, 4),
                      'raw_bytes_per_scene': qw.buf.shape[1], 'device_stream_bytes_per_scene': cw.nbytes / B,
                      'zlib_bytes_per_scene': zl / B}), flush=True)
    sys.exit(0)

model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float16, device=dev, seed=0)
x = bench.synth_batch(B, 1234, dev, 256)


def graph(quantized, fused=True, compressed=False, level=1, framed=False):
    model.fused_quantize = fused
    try:
        return GraphedForward(model, x, pipeline_agents=True, quantized=quantized, compressed=compressed, compress_level=level,
                              framed=framed)
    finally:
        model.fused_quantize = True


def timed(step, finish=None):
    for _ in range(a.warmup):
        step()
    if finish:
        finish()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    if finish:
        finish()
    torch.cuda.synchronize()
    return B * a.steps / (time.perf_counter() - t0)


def replay(gf):
    def step():
        gf()
        gf.prefetch_agents()
    return step


if a.mode == 'rows':
    res = {}
    if set('ab') & set(a.rows):
        gf = graph(False)
        res['a_no_readback'] = timed(replay(gf))
        # (b) the float32 output, stream-ordered into one pinned buffer, each step (what a user of the float output does)
        host = torch.empty(gf.out.shape, dtype=torch.float32).pin_memory()

        def step_b():
            gf()
            gf.prefetch_agents()
            host.copy_(gf.out, non_blocking=True)
        res['b_f32_to_pinned'] = timed(step_b)
        res['b_bytes_per_scene'] = gf.out[0].numel() * 4
        res['a_again'] = timed(replay(gf))
        del gf, host
    if set('cd') & set(a.rows):
        gq = graph(True)
        res['q_no_readback'] = timed(replay(gq))
        for with_zlib in (False, True):
            drain = ResultDrain(gq.out, depth=3, chunk_bytes=a.chunk_bytes)
            pool = compression_pool(a.threads) if with_zlib else None
            pending = [0]
            sizes = []

            def consume():
                q = drain.take()
                pending[0] -= 1
                if pool is not None:
                    comp = compress_batch(q, pool)
                    sizes.append(sum(len(s) for scene in comp for wp in scene for s in wp))

            def step_c():
                gq()
                gq.prefetch_agents()
                drain.submit()
                pending[0] += 1
                if pending[0] > 1:                  # the previous batch arrives (and is compressed) under this replay
                    consume()

            def finish():
                while pending[0]:
                    consume()
            res['d_quantized_drain_zlib' if with_zlib else 'c_quantized_drain'] = timed(step_c, finish)
            if with_zlib:
                res['d_compressed_bytes_per_scene'] = sum(sizes) / len(sizes) / B
                pool.shutdown()
            drain.close()
        res['c_bytes_per_scene'] = gq.out.buf.shape[1]
        del gq
    def drained(key, framed, write):
        """Rows (e), (f), (g): a compressing graph + ResultDrain; write(host batch) is the host work per arrived batch."""
        ge = graph(True, compressed=True, level=a.level, framed=framed)
        drain = ResultDrain(ge.out, depth=3, chunk_bytes=a.chunk_bytes)
        pending, sizes = [0], []

        def consume_e():
            h = drain.take()
            sizes.append(h.buf.numel())
            if write is not None:
                write(h)
            pending[0] -= 1

        def step_e():
            ge()
            ge.prefetch_agents()
            drain.submit()
            pending[0] += 1
            if pending[0] > 1:
                consume_e()

        def finish_e():
            while pending[0]:
                consume_e()
        res[key] = timed(step_e, finish_e)
        res[key[0] + '_bytes_per_scene'] = sum(sizes) / len(sizes) / B
        drain.close()
        return ge.out.nbytes

    ids = ['%016x' % (0x637f20cafde22ff8 + i) for i in range(B)]
    sink = io.BytesIO()

    def write_framed(h):                        # (f): the writer's one slice per scene
        sink.seek(0)
        w = SubmissionWriter(sink)
        w.add_batch(h, ids)
        w.close()

    def write_host_framed(h):                   # (g): 24 slices, their headers and a join per scene, on this thread
        sink.seek(0)
        w = SubmissionWriter(sink)
        for b, sid in enumerate(ids):
            blk = frame_reference(h.streams(b))
            sink.write(_scene_prefix(sid, len(blk)))
            sink.write(blk)
        w.close()
    if 'e' in a.rows:
        res['stream_bytes'] = drained('e_compressed_drain', False, None)
        res['e_compressed_bytes_per_scene'] = res.pop('e_bytes_per_scene')
    if 'f' in a.rows:
        res['framed_bytes'] = drained('f_framed_drain_writer', True, write_framed)
        res['f_file_bytes_per_batch'] = sink.tell()
    if 'g' in a.rows:
        drained('g_compressed_drain_host_framing', False, write_host_framed)
        res['g_file_bytes_per_batch'] = sink.tell()
    print(json.dumps({'mode': 'rows', 'batch': B, 'level': a.level, 'steps': a.steps, 'warmup': a.warmup, 'unit': 'scenes/s',
                      **{k: round(v, 1) for k, v in res.items()}}), flush=True)
elif a.mode == 'ab':
    g_f, g_u = graph(True, True), graph(True, False)
    assert torch.equal(g_f().buf, g_u().buf)
    rows = []
    for _ in range(a.pairs):
        rows.append({'fused': [round(timed(replay(g_f)), 1) for _ in range(2)], 'unfused': [round(timed(replay(g_u)), 1) for _ in range(2)]})
    print(json.dumps({'mode': 'ab', 'batch': B, 'steps': a.steps, 'warmup': a.warmup, 'unit': 'scenes/s', 'pairs': rows}), flush=True)
else:
    for g in (graph(True, True), graph(True, False)):
        for _ in range(10):
            g()
            g.prefetch_agents()
        torch.cuda.synchronize()
    print(json.dumps({'mode': 'trace', 'batch': B, 'replays_per_graph': 10 + 1}), flush=True)
