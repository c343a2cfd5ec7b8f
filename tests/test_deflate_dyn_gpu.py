"""GPU side of level 2 of the device-side compression: stj_compress_waypoints_level on the planted planes plus one segment per match
distance whose literal code needs the 15-bit limit -- every stream equal to compress_reference(level=2) byte for byte and decompressing
to its plane --, level 1 through the new argument, determinism, capture in a graph, the refusals, and the paths above it:
STrajNet.predict_compressed(level=2) and GraphedForward(compressed=True, compress_level=2)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deflate import planted_batch, planes_of                              # noqa: E402
from test_deflate_dyn import deep_plane                                        # noqa: E402
from test_deflate_gpu import _check_against_quantized, model_setup             # noqa: E402,F401

pytestmark = pytest.mark.gpu

DYN_SHAPES = [(1, 16, 16), (2, 64, 64), (1, 128, 64)]      # plane < segment; one short segment; exactly one (occupancy) and two (flow)
_REFS = {}


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


def _planted(shape):
    """(the batch's bytes, the level-2 reference stream of every plane in stream order), once per shape.  (1, 128, 64): occupancy plane 5
    of the scene is the 15-bit plane at d = 1 (exactly one segment); (2, 64, 64): flow plane 3 of scene 1 is the one at d = 2."""
    from strajnet_amd.submission import compress_reference, DEFLATE_SEGMENT
    if shape not in _REFS:
        B, H, W = shape
        buf = planted_batch(B, H, W, DEFLATE_SEGMENT)
        n = H * W
        if shape == (1, 128, 64):
            buf[0, 5 * n:6 * n] = deep_plane(1)[0]
        if shape == (2, 64, 64):
            buf[1, (16 + 2 * 3) * n:(16 + 2 * 3 + 2) * n] = deep_plane(2)[0]
        _REFS[shape] = (buf, [compress_reference(raw, d, level=2) for _, _, _, d, raw in planes_of(buf, H, W)])
    return _REFS[shape]


@pytest.mark.parametrize('shape', DYN_SHAPES, ids=lambda s: 'B%d_%dx%d' % s)
def test_level2_streams_equal_the_reference_and_decompress(shape):
    from strajnet_amd import QuantizedWaypoints, compress_waypoints
    B, H, W = shape
    buf, refs = _planted(shape)
    qw = QuantizedWaypoints(torch.from_numpy(buf).cuda(), H, W)
    cw = compress_waypoints(qw, level=2)
    torch.cuda.synchronize()
    host = cw.cpu()
    flat = _check_against_quantized(host, qw.cpu(), what=str(shape))            # offsets = prefix sums; every stream decompresses
    assert len(flat) == len(refs) == 24 * B
    for s, (got, ref) in enumerate(zip(flat, refs)):
        assert got == ref, (shape, s, len(got), len(ref))


def test_level1_through_the_argument_and_two_level2_calls():
    from strajnet_amd import QuantizedWaypoints, CompressedWaypoints, compress_waypoints
    B, H, W = DYN_SHAPES[2]
    qw = QuantizedWaypoints(torch.from_numpy(_planted(DYN_SHAPES[2])[0]).cuda(), H, W)
    a, b = compress_waypoints(qw), compress_waypoints(qw, level=1)
    torch.cuda.synchronize()
    n = a.nbytes
    assert n == b.nbytes and torch.equal(a.offsets, b.offsets) and torch.equal(a.buf[:n], b.buf[:n])
    out = CompressedWaypoints.empty(B, H, W, qw.buf.device)
    first = compress_waypoints(qw, out=out, level=2).cpu()
    first = (first.buf.clone(), first.offsets.clone())
    second = compress_waypoints(qw, out=out, level=2).cpu()
    assert torch.equal(first[1], second.offsets) and torch.equal(first[0], second.buf)
    assert second.buf.numel() < n


def test_level2_captured_in_a_graph():
    from strajnet_amd import QuantizedWaypoints, CompressedWaypoints, compress_waypoints
    B, H, W = DYN_SHAPES[1]
    x = torch.from_numpy(_planted(DYN_SHAPES[1])[0]).cuda()
    eager = compress_waypoints(QuantizedWaypoints(x, H, W), level=2).cpu()
    static_q = QuantizedWaypoints(x.clone(), H, W)
    static_c = CompressedWaypoints.empty(B, H, W, x.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        compress_waypoints(static_q, out=static_c, level=2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert compress_waypoints(static_q, out=static_c, level=2) is static_c
    for _ in range(2):
        static_c.buf.zero_()
        g.replay()
        torch.cuda.synchronize()
        c = static_c.cpu()
        assert torch.equal(c.offsets, eager.offsets) and torch.equal(c.buf, eager.buf)
    del g


def test_level2_refusals():
    from strajnet_amd import QuantizedWaypoints, compress_waypoints
    from strajnet_amd._lib import StjError
    qw = QuantizedWaypoints(torch.zeros((1, 32 * 256), dtype=torch.uint8, device='cuda'), 16, 16)
    for level in (0, 3):
        with pytest.raises(ValueError):
            compress_waypoints(qw, level=level)
    with pytest.raises(RuntimeError):
        compress_waypoints(QuantizedWaypoints(torch.zeros((1, 32 * 256), dtype=torch.uint8), 16, 16), level=2)        # host memory: no fallback
    with pytest.raises(StjError):
        compress_waypoints(QuantizedWaypoints(torch.zeros((1, 32 * 64), dtype=torch.uint8, device='cuda'), 8, 8), level=2)   # H * W = 64


def test_predict_compressed_and_graphed_forward_at_level2(model_setup):          # noqa: F811
    from strajnet_amd.graph import GraphedForward
    from strajnet_amd.submission import compress_reference
    model, batches, exp = model_setup
    b = batches[0]
    with pytest.raises(ValueError):
        model.predict_compressed(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow'], level=3)
    cw = model.predict_compressed(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow'], level=2)
    torch.cuda.synchronize()
    flat = _check_against_quantized(cw.cpu(), exp[0], what='predict_compressed level 2')
    raw = exp[0].waypoint_bytes(1, 3)
    assert flat[24 + 3 * 3 + 2] == compress_reference(raw[2], 2, level=2) and flat[24 + 3 * 3] == compress_reference(raw[0], 1, level=2)
    with pytest.raises(ValueError):
        GraphedForward(model, b, quantized=True, compressed=True, compress_level=0)
    gf = GraphedForward(model, b, quantized=True, compressed=True, compress_level=2)
    o = gf(b)
    torch.cuda.synchronize()
    assert _check_against_quantized(o.cpu(), exp[0], what='graph level 2') == flat
    del gf
