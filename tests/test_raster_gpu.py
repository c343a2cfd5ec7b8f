"""stj_raster_boxes / stj_raster_grids / stj_raster_actors (strajnet_amd/raster.py: rasterize, Rasterizer) against the float64 statement
raster_reference on the two cases of _raster_cases.py.  What the ambiguity report excuses, and how little that is, is asserted on the
reference alone in test_raster_ref.py."""
import functools

import numpy as np
import pytest
import torch

import _raster_cases as rc
from strajnet_amd.raster import Rasterizer, model_inputs, rasterize
from test_raster_ref import check_flow_bounds

pytestmark = pytest.mark.gpu
CASES = {'small': rc.small_case, 'full': rc.full_case}


@functools.lru_cache(maxsize=None)
def device_run(name):
    """One rasterize of a case, its outputs and workspace parts on the host; shared, left unchanged."""
    tracks, cfg = CASES[name]()
    r = Rasterizer(tracks.B, cfg, tracks.A)
    out = {k: v.cpu().numpy() for k, v in r(tracks).items()}
    parts = {k: r.part(k).cpu().numpy() for k in ('MASK', 'DIST', 'RANK', 'FRAME', 'OK', 'AABB')}
    return out, parts


@pytest.mark.parametrize('name', list(CASES))
def test_ogm(lib_built, name):
    """Equal on every pixel that is not free; a free pixel may be 0 or 1."""
    out, _ = device_run(name)
    ref, rep = rc.reference(name)
    got = out['ogm']
    assert got.dtype == np.float32 and got.shape == ref['ogm'].shape and np.isin(got, (0.0, 1.0)).all()
    diff = got != ref['ogm']
    print(f'{name}: {int(diff.sum())} of {int(ref["ogm"].sum())} set pixels differ, {int(rep["free"].sum())} are free')
    assert not (diff & ~rep['free']).any()


@pytest.mark.parametrize('name', list(CASES))
def test_flow(lib_built, name):
    """Bitwise the correctly rounded quotient on clean pixels; within the candidates' bounds on touched ones."""
    out, _ = device_run(name)
    ref, rep = rc.reference(name)
    want = ref['flow'].astype(np.float32)
    clean = ~rep['flow_touched']
    assert np.array_equal(out['flow'][clean].view(np.uint32), want[clean].view(np.uint32))
    assert np.count_nonzero(want[clean]) > 1000 * (name == 'full')
    check_flow_bounds(out['flow'], rep)


@pytest.mark.parametrize('name', list(CASES))
def test_ok_and_actors(lib_built, name):
    """ok; the masks; the same agents in the same order; values within 4x the float32 statement's own deviation from float64."""
    tracks, _ = CASES[name]()
    out, parts = device_run(name)
    ref, rep = rc.reference(name)
    assert np.array_equal(out['ok'], ref['ok'].astype(np.float32)) and np.array_equal(parts['OK'], ref['ok'].astype(np.int32))
    for b in np.flatnonzero(ref['ok'] == 0):
        assert not any(out[k][b].any() for k in ('ogm', 'flow', 'obs', 'occ'))
        assert not parts['MASK'][b].any() and (parts['RANK'][b] == -1).all()
    m = parts['MASK']
    assert np.array_equal((m & 1) != 0, rep['in_box']) and np.array_equal((m & 2) != 0, rep['occu_mask'])
    assert np.array_equal((m & 4) != 0, (tracks.valid > 0).any(-1) & (ref['ok'] != 0)[:, None])
    tol = 4 * rc.ACTOR_DEVIATION[name]
    for key, src, col, listed in (('obs', 'obs_src', 0, 'obs_listed'), ('occ', 'occ_src', 1, 'occ_listed')):
        rows = rep[src]
        for b in range(tracks.B):
            # the agent whose distance earned row r: the listed agents sorted by the float64 statement's last distance
            idx = np.flatnonzero(rep[listed][b])
            order = idx[np.argsort(rep['dist_last'][b][idx], kind='stable')][:rows.shape[1]]
            want_rank = np.full(tracks.A, -1)
            want_rank[order] = np.arange(order.size)
            assert np.array_equal(parts['RANK'][b, :, col], want_rank), (key, b)
            # the same rows: an agent's row is recognised by its type one-hot and values, zero padding past the list
            n = int((rows[b] >= 0).sum())
            assert not out[key][b, n:].any()
        dev = float(np.abs(out[key].astype(np.float64) - ref[key]).max())
        print(f'{name}: {key} deviates by {dev:.3e} from the float64 statement (allowed {tol:.3e})')
        assert dev <= tol


@pytest.mark.parametrize('name', list(CASES))
def test_two_runs_are_bitwise_identical(lib_built, name):
    tracks, cfg = CASES[name]()
    first, _ = device_run(name)
    again = rasterize(tracks, cfg)
    for k, v in again.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint32), first[k].view(np.uint32)), k


def test_out_buffers_are_reused(lib_built):
    tracks, cfg = rc.small_case()
    first, _ = device_run('small')
    bufs = {k: torch.full(first[k].shape, float('nan'), device='cuda') for k in ('ogm', 'flow', 'obs')}
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    res = rasterize(tracks, cfg, out=bufs)
    for k in bufs:
        assert res[k] is bufs[k] and res[k].data_ptr() == ptrs[k]
    for k, v in res.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint32), first[k].view(np.uint32)), k
    with pytest.raises(ValueError, match='ogm'):
        rasterize(tracks, cfg, out={'ogm': torch.zeros(3, device='cuda')})


def test_captured_graph_replays_on_a_second_batch(lib_built):
    """Rasterizer.run captured into one linear graph (one stream, no branches); a second batch is loaded into the same buffers and the
    replay equals the eager call."""
    tracks, cfg = rc.small_case()
    second = tracks.scenes([1, 0])
    r = Rasterizer(tracks.B, cfg, tracks.A)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r(tracks)                                       # warm up off the default stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.run()
    r.load(second)
    for t in r.out.values():
        t.fill_(float('nan'))
    g.replay()
    torch.cuda.synchronize()
    want = rasterize(second, cfg)
    first, _ = device_run('small')
    for k, v in r.out.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint32), want[k].cpu().numpy().view(np.uint32)), k
        assert np.array_equal(v.cpu().numpy()[::-1].view(np.uint32), first[k].view(np.uint32)), k      # the scenes swapped places
    del g


def test_refusals_at_the_abi(lib_built):
    from strajnet_amd._lib import StjError
    tracks, cfg = rc.small_case()
    with pytest.raises(StjError, match='at most 1024'):
        Rasterizer(1, cfg, 1025).run()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rasterize(tracks, cfg, device='cpu')
    with pytest.raises(ValueError, match='built for'):
        Rasterizer(1, cfg, tracks.A).load(tracks)


def test_model_takes_the_rasterised_scene(lib_built):
    """End to end at B = 1 on the 128 geometry: model(**rasterize(...), map_img=...) gives finite outputs."""
    from oracle import np_ref
    from strajnet_amd import STrajNet
    tracks, cfg = rc.small_case()
    mcfg = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])
    model = STrajNet(mcfg, fg_msa=True, fg=True, large_ogm=False, dtype=torch.float32, device='cuda:0')
    model.load_weights(np_ref.make_weights(mcfg, 0))
    x = rasterize(tracks.scenes([0]), cfg, device='cuda:0')
    assert float(x['ok'][0]) == 1.0 and float(x['ogm'].sum()) > 1000
    map_img = torch.as_tensor(np_ref.make_inputs(mcfg, 1)['map_img']).to('cuda:0')
    y = model(**model_inputs(x), map_img=map_img, training=False)
    torch.cuda.synchronize()
    assert y.shape[0] == 1 and bool(torch.isfinite(y).all())
