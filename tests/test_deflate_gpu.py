"""GPU side of the device-side compression: stj_compress_waypoints on planted planes -- every stream must pass zlib.decompress to the
plane's bytes (the independent gate) and equal compress_reference byte for byte -- its refusal of shapes it does not take, determinism,
capture in a graph, and the paths above it: STrajNet.predict_compressed, GraphedForward(quantized=True, compressed=True), ResultDrain."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deflate import SHAPES, planted_batch, planes_of                     # noqa: E402

pytestmark = pytest.mark.gpu

CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
_REFS = {}


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


def _planted(shape):
    """(the batch's bytes, the reference stream of every plane in stream order), computed once per shape."""
    from strajnet_amd.submission import compress_reference, DEFLATE_SEGMENT
    if shape not in _REFS:
        B, H, W = shape
        buf = planted_batch(B, H, W, DEFLATE_SEGMENT)
        _REFS[shape] = (buf, [compress_reference(raw, d) for _, _, _, d, raw in planes_of(buf, H, W)])
    return _REFS[shape]


def _check_against_quantized(cw, qw, what=''):
    """Every stream of a HOST CompressedWaypoints decompresses to the plane of the quantised buffer; the offsets are monotone and end at
    the sum of the lengths.  Returns the streams in stream order."""
    off = cw.offsets.numpy().view(np.uint32).astype(np.int64)
    assert off[0] == 0 and (np.diff(off) > 0).all(), what
    flat = []
    for b in range(qw.batch):
        scene = cw.streams(b)
        assert len(scene) == qw.Tn and b''.join(s for wp in scene for s in wp) == cw.scene_bytes(b)
        for k in range(qw.Tn):
            raw = qw.waypoint_bytes(b, k)
            for i in range(3):
                assert zlib.decompress(scene[k][i]) == raw[i], (what, b, k, i)
                flat.append(scene[k][i])
    assert off[-1] == sum(len(s) for s in flat) == cw.nbytes == cw.buf.numel(), what
    assert [len(s) for s in flat] == list(np.diff(off)), what
    return flat


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d_%dx%d' % s)
def test_streams_decompress_and_equal_the_reference(shape):
    """16x16: a plane shorter than a segment; 64x64: at most one segment; 128x64: exactly one (occupancy) and two (flow); 256x256: 8 and
    16 segments, the 131072-byte flow planes.  The planted planes: tests/test_deflate.py."""
    from strajnet_amd import QuantizedWaypoints, CompressedWaypoints, compress_waypoints
    B, H, W = shape
    buf, refs = _planted(shape)
    qw = QuantizedWaypoints(torch.from_numpy(buf).cuda(), H, W)
    cw = compress_waypoints(qw)
    torch.cuda.synchronize()
    assert isinstance(cw, CompressedWaypoints) and cw.buf.is_cuda
    host = cw.cpu()
    assert not host.buf.is_cuda and host.cpu() is host
    flat = _check_against_quantized(host, qw.cpu(), what=str(shape))
    assert len(flat) == len(refs) == 24 * B
    for s, (got, ref) in enumerate(zip(flat, refs)):
        assert got == ref, (shape, s, len(got), len(ref))
    assert cw.streams(B - 1) == host.streams(B - 1) and cw.scene_bytes(0) == host.scene_bytes(0)      # the device object answers the same


def test_unsupported_shape_and_host_input():
    from strajnet_amd import QuantizedWaypoints, compress_waypoints
    from strajnet_amd._lib import StjError
    with pytest.raises(StjError):
        compress_waypoints(QuantizedWaypoints(torch.zeros((1, 32 * 64), dtype=torch.uint8, device='cuda'), 8, 8))     # H * W = 64
    with pytest.raises(RuntimeError):
        compress_waypoints(QuantizedWaypoints(torch.zeros((1, 32 * 256), dtype=torch.uint8), 16, 16))                 # host memory: no fallback


def test_two_calls_give_identical_buffers():
    from strajnet_amd import QuantizedWaypoints, compress_waypoints
    B, H, W = SHAPES[1]
    qw = QuantizedWaypoints(torch.from_numpy(_planted(SHAPES[1])[0]).cuda(), H, W)
    a, b = compress_waypoints(qw), compress_waypoints(qw)
    torch.cuda.synchronize()
    n = a.nbytes
    assert n == b.nbytes and torch.equal(a.offsets, b.offsets) and torch.equal(a.buf[:n], b.buf[:n])


def test_compress_captured_in_a_graph():
    """compress_waypoints(qw, out=static) captured once (a single chain of three launches), replayed over two different inputs == eager."""
    from strajnet_amd import QuantizedWaypoints, CompressedWaypoints, compress_waypoints
    from strajnet_amd.submission import DEFLATE_SEGMENT
    B, H, W = SHAPES[1]
    inputs = [torch.from_numpy(_planted(SHAPES[1])[0]).cuda(), torch.from_numpy(planted_batch(B, H, W, DEFLATE_SEGMENT, seed=7)).cuda().flip(0)]
    assert not torch.equal(inputs[0], inputs[1])
    eager = []
    for x in inputs:
        c = compress_waypoints(QuantizedWaypoints(x, H, W)).cpu()
        eager.append((c.buf.clone(), c.offsets.clone()))
    static_q = QuantizedWaypoints(inputs[0].clone(), H, W)
    static_c = CompressedWaypoints.empty(B, H, W, static_q.buf.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        compress_waypoints(static_q, out=static_c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert compress_waypoints(static_q, out=static_c) is static_c
    for i in (1, 0, 1):
        static_q.buf.copy_(inputs[i])
        g.replay()
        torch.cuda.synchronize()
        c = static_c.cpu()
        assert torch.equal(c.offsets, eager[i][1]) and torch.equal(c.buf, eager[i][0]), i
    with pytest.raises(ValueError):
        compress_waypoints(QuantizedWaypoints(inputs[0][:1].clone(), H, W), out=static_c)             # another batch size
    del g


@pytest.fixture(scope='module')
def model_setup():
    """CFG128, B = 2, fp16 (the setup of tests/test_submission_gpu.py): the model, three batches, and their quantised bytes."""
    from strajnet_amd import STrajNet
    from oracle import np_ref
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float16)
    model.load_weights(np_ref.make_weights(CFG128, 0))
    keys = ('ogm', 'map_img', 'obs', 'occ', 'flow')
    batches = []
    for s in (None, 77, 99):
        xs = np_ref.make_inputs(CFG128, 2) if s is None else np_ref.make_inputs(CFG128, 2, seed=s)
        batches.append({k: torch.as_tensor(xs[k]).cuda() for k in keys})
    exp = [model.predict_quantized(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow']).cpu() for b in batches]
    assert not torch.equal(exp[0].buf, exp[1].buf) and not torch.equal(exp[1].buf, exp[2].buf)
    return model, batches, exp


def test_predict_compressed_decompresses_to_predict_quantized(model_setup):
    from strajnet_amd import CompressedWaypoints
    from strajnet_amd.submission import compress_reference
    model, batches, exp = model_setup
    b = batches[0]
    cw = model.predict_compressed(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow'])
    torch.cuda.synchronize()
    assert isinstance(cw, CompressedWaypoints) and cw.B == 2
    flat = _check_against_quantized(cw.cpu(), exp[0], what='predict_compressed')
    raw = exp[0].waypoint_bytes(1, 3)
    assert flat[24 + 3 * 3 + 2] == compress_reference(raw[2], 2) and flat[24 + 3 * 3] == compress_reference(raw[0], 1)
    zl = sum(len(s) for wp in exp[0].compressed(0) for s in wp)
    print(f'predict_compressed, CFG128 fp16 random weights: {cw.nbytes // 2} bytes per scene; zlib.compress of scene 0: {zl}')


def test_graphed_forward_compressed_and_result_drain(model_setup):
    """GraphedForward(quantized=True, compressed=True) over three batches decompresses to eager predict_quantized's bytes; ResultDrain
    over five replays of alternating batches delivers each batch's streams in order, equal to synchronous .cpu() copies."""
    from strajnet_amd import CompressedWaypoints, ResultDrain
    from strajnet_amd.graph import GraphedForward
    model, batches, exp = model_setup
    with pytest.raises(ValueError):
        GraphedForward(model, batches[0], compressed=True)
    gf = GraphedForward(model, batches[0], quantized=True, compressed=True)
    assert isinstance(gf.out, CompressedWaypoints)
    for i in (1, 0, 2):
        o = gf(batches[i])
        torch.cuda.synchronize()
        assert o is gf.out
        _check_against_quantized(o.cpu(), exp[i], what=f'graph batch {i}')
    order = [0, 1, 0, 2, 1]
    drain = ResultDrain(gf.out, depth=2, chunk_bytes=1 << 18)
    got = []
    try:
        for n, i in enumerate(order):
            gf(batches[i])
            drain.submit()
            if n >= 1:                                   # one batch in flight behind the replay
                h = drain.take()
                got.append((h.buf.clone(), h.offsets.clone()))
        h = drain.take()
        got.append((h.buf.clone(), h.offsets.clone()))
        assert isinstance(h, CompressedWaypoints) and not h.buf.is_cuda
        with pytest.raises(RuntimeError):
            drain.take()
    finally:
        drain.close()
    assert len(got) == 5
    for n, i in enumerate(order):
        gf(batches[i])
        torch.cuda.synchronize()
        s = gf.out.cpu()                                 # the second run: synchronous copies
        assert torch.equal(got[n][1], s.offsets) and torch.equal(got[n][0], s.buf), n
    _check_against_quantized(CompressedWaypoints(got[3][0], got[3][1], 2), exp[2], what='drained batch 2')
    del gf, drain
