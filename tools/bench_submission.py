#!/usr/bin/env python
"""What bringing the inference result to the host costs (config 4: B = 32 fp16, GraphedForward under replay, agent pipeline on).

  --mode rows   scenes/s for (a) no read-back (bench.py --infer's figure), (b) the float32 output copied to pinned memory each step,
                (c) quantised output + ResultDrain, (d) as (c) plus zlib compression of every scene on 16 threads
  --mode ab     GraphedForward(quantized=True) with the quantising gather (stj_outconv_pair_gather_q) against the same graph built from
                stj_outconv_pair_gather + stj_quantize_waypoints, alternating, --pairs times; each build is timed TWICE in a row per
                visit, so the spread of repeated runs of the same build is measured in the same call
  --mode trace  a few replays of both quantised graphs and nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run

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
a = ap.parse_args()

import bench
from strajnet_amd import STrajNet, ResultDrain, compress_batch, compression_pool
from strajnet_amd.graph import GraphedForward

assert torch.cuda.is_available(), 'bench_submission.py needs a GPU'
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
B = a.batch
model = STrajNet(bench.CFG256, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float16, device=dev, seed=0)
x = bench.synth_batch(B, 1234, dev, 256)


def graph(quantized, fused=True):
    model.fused_quantize = fused
    try:
        return GraphedForward(model, x, pipeline_agents=True, quantized=quantized)
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
    print(json.dumps({'mode': 'rows', 'batch': B, 'steps': a.steps, 'warmup': a.warmup, 'unit': 'scenes/s',
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
