"""GPU side of the submission files: stj_compress_waypoints_framed on the cases of tests/_framing_cases.py -- every scene's block must
equal frame_reference(compress_reference(...)) byte for byte, the embedded streams the unframed call's, which the framed call leaves as
it was -- its sizes and refusals through the raw C ABI, and the path above it: GraphedForward(quantized=True, compressed=True,
framed=True) -> ResultDrain -> SubmissionWriter -> parse_submission."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _framing_cases as FC                                                   # noqa: E402

pytestmark = pytest.mark.gpu

CFG128 = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])


@pytest.fixture(scope='module', autouse=True)
def _lib(lib_built):
    assert torch.cuda.is_available()


@pytest.mark.parametrize('level', FC.LEVELS)
@pytest.mark.parametrize('name', ('small', 'mid', 'long', 'many43', 'many', 'sparse'))
def test_framed_blocks_equal_the_reference(name, level):
    """small / mid / long: stream and waypoint-body lengths on both sides of 128 and 16384 (one-, two- and three-byte varints); many43 /
    many: 1032 and 3096 streams, beyond one and three of the scan's chunks of 1008; sparse: 256x256, also through SubmissionWriter."""
    from strajnet_amd import QuantizedWaypoints, FramedWaypoints, SubmissionWriter, compress_waypoints, frame_reference, parse_submission
    from strajnet_amd.submission import compress_framed_sizes
    ref = FC.check_boundaries(name, level)
    buf, H, W = FC.batch(name)
    B = buf.shape[0]
    qw = QuantizedWaypoints(torch.from_numpy(buf).cuda(), H, W)
    before = compress_waypoints(qw, level=level).cpu()
    fw = compress_waypoints(qw, level=level, framed=True)
    after = compress_waypoints(qw, level=level).cpu()
    torch.cuda.synchronize()
    assert isinstance(fw, FramedWaypoints) and fw.buf.is_cuda and fw.batch == B
    assert torch.equal(before.offsets, after.offsets) and torch.equal(before.buf, after.buf)      # the unframed entry: untouched
    host = fw.cpu()
    assert not host.buf.is_cuda and host.cpu() is host
    t = host.table.numpy().view(np.uint32).astype(np.int64)
    n = 24 * B
    starts, lens, scene = t[:n], t[n:2 * n], t[2 * n:]
    blocks = [frame_reference(s) for s in ref]
    assert scene[0] == 0 and list(np.diff(scene)) == [len(x) for x in blocks]
    assert scene[-1] == host.nbytes == host.buf.numel() == fw.nbytes <= compress_framed_sizes(B, H, W)[1] == fw.buf.numel()
    assert list(lens) == [len(s) for sc in ref for wp in sc for s in wp] == list(np.diff(before.offsets.numpy().view(np.uint32).astype(np.int64)))
    assert (np.diff(starts) > lens[:-1]).all() and starts[-1] + lens[-1] == scene[-1]
    for b in range(B):
        assert host.scene_message(b) == blocks[b], (name, level, b)
        assert host.streams(b) == before.streams(b) == ref[b], (name, level, b)
    assert fw.scene_message(B - 1) == blocks[B - 1] and fw.streams(0) == ref[0]                   # the device object answers the same
    if name == 'sparse':
        ids = [f'scene-{b}' for b in range(B)]
        f = io.BytesIO()
        with SubmissionWriter(f, authors=('x', 'y')) as w:
            w.add_batch(host, ids)
        header, got, scenes = parse_submission(f.getvalue())
        assert header['authors'] == ['x', 'y'] and got == ids and scenes == ref
        cpu = qw.cpu()
        for b in range(B):
            for k in range(8):
                assert tuple(zlib.decompress(s) for s in scenes[b][k]) == cpu.waypoint_bytes(b, k)


def test_out_is_written_in_place_and_checked():
    from strajnet_amd import QuantizedWaypoints, FramedWaypoints, CompressedWaypoints, compress_waypoints, frame_reference
    buf, H, W = FC.batch('small')
    qw = QuantizedWaypoints(torch.from_numpy(buf).cuda(), H, W)
    out = FramedWaypoints.empty(3, H, W, qw.buf.device)
    for level in FC.LEVELS:
        assert compress_waypoints(qw, out=out, level=level, framed=True) is out
        torch.cuda.synchronize()
        assert [out.scene_message(b) for b in range(3)] == [frame_reference(s) for s in FC.reference_streams('small', level)]
    with pytest.raises(ValueError):
        compress_waypoints(qw, out=CompressedWaypoints.empty(3, H, W, qw.buf.device), framed=True)
    with pytest.raises(ValueError):
        compress_waypoints(qw, out=FramedWaypoints.empty(2, H, W, qw.buf.device), framed=True)
    with pytest.raises(RuntimeError):
        compress_waypoints(qw.cpu(), framed=True)                                                     # host memory: no fallback


def test_sizes_and_refused_arguments():
    """The documented codes through the raw C ABI: a misaligned buffer, Tn != 8 and a shape it does not take -> STJ_EUNSUPPORTED, a
    level other than 1 or 2 -> STJ_EINVAL; nothing is launched."""
    from strajnet_amd import _lib
    from strajnet_amd.submission import compress_framed_sizes, frame_tags
    L = _lib.lib()
    st = _lib.ENUMS['stj_status']
    vp = ctypes.c_void_p
    B, H, W = 2, 16, 16
    work, cap, words = compress_framed_sizes(B, H, W)
    q = torch.zeros(B * 32 * H * W, dtype=torch.uint8, device='cuda')
    wk, out = torch.zeros(work, dtype=torch.uint8, device='cuda'), torch.zeros(cap + 16, dtype=torch.uint8, device='cuda')
    tab = torch.full((words + 4,), -1, dtype=torch.int32, device='cuda')
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def run(qp=None, wp=None, op=None, tp=None, B=B, Tn=8, H=H, W=W, level=1):
        return L.stj_compress_waypoints_framed(vp(qp or q.data_ptr()), vp(wp or wk.data_ptr()), vp(op or out.data_ptr()),
                                               vp(tp or tab.data_ptr()), B, Tn, H, W, level, frame_tags(), stream)
    assert run() == st['STJ_OK']
    torch.cuda.synchronize()
    t = tab.cpu().numpy().view(np.uint32)
    assert t[words - 1] <= cap and (t[words:] == 0xffffffff).all() and not out[cap:].any()          # nothing behind the table or the capacity
    for kw in (dict(op=out.data_ptr() + 1), dict(tp=tab.data_ptr() + 4), dict(qp=q.data_ptr() + 8), dict(wp=wk.data_ptr() + 2)):
        assert run(**kw) == st['STJ_EUNSUPPORTED'] and b'16-byte aligned' in L.stj_last_error(), kw
    assert run(Tn=7) == st['STJ_EUNSUPPORTED']
    assert run(H=8, W=8) == st['STJ_EUNSUPPORTED']                                                   # H * W = 64
    assert run(B=0) == st['STJ_EINVAL']
    for level in (0, 3):
        assert run(level=level) == st['STJ_EINVAL'] and b'level' in L.stj_last_error()
    sizes = [ctypes.c_longlong(0) for _ in range(3)]
    ptrs = [vp(ctypes.addressof(x)) for x in sizes]
    assert L.stj_compress_framed_sizes(1, 7, 16, 16, *ptrs) == st['STJ_EUNSUPPORTED']
    assert L.stj_compress_framed_sizes(1, 8, 8, 8, *ptrs) == st['STJ_EUNSUPPORTED']
    assert L.stj_compress_framed_sizes(40, 8, 2048, 2048, *ptrs) == st['STJ_EUNSUPPORTED']           # beyond 32-bit offsets
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def model_setup():
    """CFG128, B = 2, fp16 (the setup of tests/test_deflate_gpu.py): the model, two batches, and their quantised bytes."""
    from strajnet_amd import STrajNet
    from oracle import np_ref
    model = STrajNet(CFG128, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float16)
    model.load_weights(np_ref.make_weights(CFG128, 0))
    keys = ('ogm', 'map_img', 'obs', 'occ', 'flow')
    batches = []
    for s in (None, 77):
        xs = np_ref.make_inputs(CFG128, 2) if s is None else np_ref.make_inputs(CFG128, 2, seed=s)
        batches.append({k: torch.as_tensor(xs[k]).cuda() for k in keys})
    exp = [model.predict_quantized(b['ogm'], b['map_img'], obs=b['obs'], occ=b['occ'], flow=b['flow']).cpu() for b in batches]
    assert not torch.equal(exp[0].buf, exp[1].buf)
    return model, batches, exp


@pytest.mark.parametrize('level', FC.LEVELS)
def test_graphed_forward_framed_drain_and_writer(model_setup, level):
    """The captured path: two replays over different inputs, drained by ResultDrain, written by SubmissionWriter, parsed back -- the ids
    in order, every stream decompressing to predict_quantized's plane."""
    from strajnet_amd import FramedWaypoints, ResultDrain, SubmissionWriter, parse_submission
    from strajnet_amd.graph import GraphedForward
    model, batches, exp = model_setup
    with pytest.raises(ValueError):
        GraphedForward(model, batches[0], quantized=True, framed=True)
    gf = GraphedForward(model, batches[0], quantized=True, compressed=True, compress_level=level, framed=True)
    assert isinstance(gf.out, FramedWaypoints)
    order = [1, 0]
    ids = [[f'b{i}s{b}' for b in range(2)] for i in order]
    drain = ResultDrain(gf.out, depth=2, chunk_bytes=1 << 18)
    f = io.BytesIO()
    w = SubmissionWriter(f)
    try:
        for i in order:
            assert gf(batches[i]) is gf.out
            drain.submit()
        for n in range(2):
            h = drain.take()
            assert isinstance(h, FramedWaypoints) and not h.buf.is_cuda and h.buf.numel() == h.nbytes
            w.add_batch(h, ids[n])
        with pytest.raises(RuntimeError):
            drain.take()
    finally:
        drain.close()
    w.close()
    header, got, scenes = parse_submission(f.getvalue())
    assert header == dict(account_name='', unique_method_name='', authors=[''], description='', method_link='')
    assert got == ids[0] + ids[1] and len(scenes) == 4
    for n, i in enumerate(order):
        for b in range(2):
            for k in range(8):
                assert tuple(zlib.decompress(s) for s in scenes[2 * n + b][k]) == exp[i].waypoint_bytes(b, k), (n, b, k)
    del gf, drain
