"""Scenes resident in HBM on the device (csrc/pool.hip through strajnet_amd/data.py): stj_gather_bits / stj_gather_sparse / stj_gather_raw
against PoolLayout.reference_gather and stj_decode_raw, ResidentPool against decode_batch_packed, ResidentFeed on a static dict, graph
capture with a persistent index tensor, and the refusals of the C ABI.  Every comparison is bitwise."""
import numpy as np
import pytest
import torch

from strajnet_amd import data as D
from test_packed import SIZES, planted, u32, _raw_example

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


def dev_idx(idx):
    return torch.tensor(list(idx), dtype=torch.int32).cuda()


def bits_eq(t, want):
    return np.array_equal(u32(t.cpu().numpy()), u32(np.ascontiguousarray(want, np.float32)))


def planted_layout(n, names):
    """The planted planes `names` as the scenes of a pool: sparse as they are, and the bits of their non-zero words."""
    planes = planted(n)
    scenes = [planes[k] for k in names]
    lay = D.PoolLayout()
    lay.add_sparse('sparse', [D.pack_sparse(x) for x in scenes], n)
    lay.add_bits('bits', [D.pack_bits(u32(x)) for x in scenes])
    return lay


# zero sits next to full, and special (-0.0, NaN payloads, denormals) is scene 3; between them the two sets hold every planted plane
POOLS = {1: [['rand0.5']], 5: [['run8192', 'zero', 'full', 'special', 'rand0.02'], ['last', 'run32', 'first', 'special', 'rand0.5']]}


@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('n', SIZES)
def test_kernels_match_reference_gather(lib_built, n, N):
    for names in POOLS[N]:
        lay = planted_layout(n, names)
        pool = D.ResidentPool(lay, 'cuda')
        for B in (1, 3, 7):
            patterns = {'identity': [b % N for b in range(B)], 'reversed': [N - 1 - b % N for b in range(B)], 'repeated': [N * 3 // 5] * B,
                        'out of range': [(-1, N, INT_MAX)[b % 3] for b in range(B)]}
            for what, idx in patterns.items():
                static = {k: torch.full((B, n), float('nan'), device='cuda') for k in lay.entries}          # an unwritten element shows
                pool.gather_into(static, dev_idx(idx))
                want = lay.reference_gather(idx)
                for k in lay.entries:
                    got = u32(static[k].cpu().numpy())
                    assert np.array_equal(got, u32(want[k])), (names, B, what, k, np.argwhere(got != u32(want[k]))[:8])


def _raw_scenes(kind, N, n, rng):
    if kind == 'bool':
        return ((rng.random((N, n)) < 0.4) * rng.integers(1, 256, (N, n))).astype(np.uint8)
    if kind == 'int8':
        return rng.integers(-128, 128, (N, n)).astype(np.int8)
    if kind == 'float32':
        a = rng.normal(size=(N, n)).astype(np.float32).view(np.uint32)
        a[:, ::3] = np.array([0x80000000, 0x7fc00123, 0x00000001, 0x7f800001], np.uint32)[np.arange(a[:, ::3].shape[1]) % 4]
        return a
    a = rng.normal(size=(N, n)) * 40
    a[:, ::4] = np.array([1e300, -1e-300, -0.0, np.nan])[np.arange(a[:, ::4].shape[1]) % 4]
    return a


@pytest.mark.parametrize('kind', ['bool', 'int8', 'float32', 'float64'])
def test_gather_raw_equals_decode_raw(lib_built, kind):
    """Against stj_decode_raw (no crop) run on the selected rows copied back to back.  B * n is odd for most n, so rows start at every
    alignment; two of the four indices are out of range and clamp."""
    from strajnet_amd.ops import _p, _st, call
    rng = np.random.default_rng(11)
    N, idx = 5, [4, 1, -7, 99]
    rows = [4, 1, 0, 4]
    B = len(idx)
    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        host = _raw_scenes(kind, N, n, rng)
        as_bytes = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        pool, picked = as_bytes(host), as_bytes(host[rows])
        for scale in (1.0, 1.0 / 256.0):
            got, want = torch.full((B, n), 12345.0, device='cuda'), torch.full((B, n), 12345.0, device='cuda')     # no element's value
            call('stj_gather_raw', _p(pool), D.KIND[kind], _p(dev_idx(idx)), N, _p(got), B, n, scale, _st())
            call('stj_decode_raw', _p(picked), D.KIND[kind], _p(want), 1, 1, B * n, 1, 0, 0, 1, B * n, scale, _st())
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, n, scale)


def _pool_vs_decode_batch_packed(grid, out, test, N, idx, seed):
    rng = np.random.default_rng(seed)
    packed = [D.pack_example(_raw_example(rng, grid, out, test), grid, out, test) for _ in range(N)]
    pool = D.ResidentPool.from_examples(packed, 'cuda', grid, out, test)
    got = pool.gather(idx)
    want = D.decode_batch_packed([packed[i] for i in idx], 'cuda', grid, out, test)
    assert set(got) == {D.POOL_NAMES[name] for name in want}
    for name in want:
        g = got[D.POOL_NAMES[name]]
        assert g.shape == want[name].shape and g.dtype == torch.float32, name
        assert torch.equal(g.view(torch.int32), want[name].view(torch.int32)), name
    return pool, got


@pytest.mark.parametrize('test', [False, True])
def test_resident_pool_equals_decode_batch_packed(lib_built, test):
    pool, got = _pool_vs_decode_batch_packed(64, 32, test, 5, [3, 0, 3], 5)
    assert got['ogm'].shape == (3, 64, 64, 11, 2) and (test or got['gt_flow'].shape == (3, 8, 32, 32, 2))
    assert pool.nbytes == pool.layout.nbytes > 0
    again = pool.gather(dev_idx([3, 0, 3]))                                     # a device index gives the same
    assert all(torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)) for k in got)
    with pytest.raises(ValueError):
        pool.gather([0, 5])                                                     # a host list is range-checked


def test_resident_pool_real_geometry(lib_built):
    """(512, 256), N = 2, B = 1, test records: ogm is 704 blocks per scene, vec_flow 64."""
    pool, got = _pool_vs_decode_batch_packed(512, 256, True, 2, [1], 6)
    assert got['ogm'].shape == (1, 512, 512, 11, 2) and pool.layout.entries['ogm']['n'] == 704 * 8192
    assert pool.layout.entries['flow']['n'] == 64 * 8192


def _feed_pool(N, B, seed):
    """A pool of N scenes under the keys of a static dict shaped like test_packed_feed_lands_every_batch's, and that dict."""
    rng = np.random.default_rng(seed)
    shapes = {'ogm': (64, 64, 11, 2), 'map_img': (64, 64, 3), 'flow': (64, 64, 2), 'big': (1 << 20,), 'obs': (48, 11, 8)}
    sparse = lambda shape, dens: np.where(rng.random((N,) + shape) < dens, rng.normal(size=(N,) + shape), 0.0).astype(np.float32)
    flow, big = sparse(shapes['flow'], 0.05), sparse(shapes['big'], 0.02)
    big.view(np.uint32)[:, 7] = 0x80000000                                      # -0.0 is present
    big[1] = 0                                                                  # a scene without a present word
    lay = D.PoolLayout()
    lay.add_bits('ogm', [D.pack_bits(x) for x in (rng.random((N,) + shapes['ogm']) < 0.3)], shapes['ogm'])
    lay.add_raw('map_img', list(rng.integers(-128, 128, (N,) + shapes['map_img']).astype(np.int8)), 'int8', 1.0 / 256.0, shapes['map_img'])
    lay.add_sparse('flow', [D.pack_sparse(x) for x in flow], flow[0].size, shapes['flow'])
    lay.add_sparse('big', [D.pack_sparse(x) for x in big], big[0].size, shapes['big'])
    lay.add_raw('obs', list(rng.normal(size=(N,) + shapes['obs'])), 'float64', 1.0, shapes['obs'])
    static = {k: torch.zeros((B,) + s, device='cuda') for k, s in shapes.items()}
    static['extra'] = torch.arange(12, dtype=torch.float32, device='cuda')        # a key the pool does not hold
    return lay, static


def test_resident_feed_lands_every_batch(lib_built):
    lay, static = _feed_pool(4, 2, 1)
    pool = D.ResidentPool(lay, 'cuda')
    feed = D.ResidentFeed(static, pool, sampler=pool.sampler(2, seed=3))
    assert feed.idx.dtype == torch.int32 and feed.idx.shape == (2,) and feed.idx.is_cuda
    feed.start()
    seen = []
    for step, idx in enumerate(([1, 3], dev_idx([3, 0]), None)):
        feed.land(idx)
        feed.wait_uploaded()
        torch.cuda.synchronize()
        used = feed.idx.cpu().tolist()
        assert idx is None or used == (idx.cpu().tolist() if isinstance(idx, torch.Tensor) else idx)
        seen.append(used)
        want = lay.reference_gather(used)
        for k in lay.entries:
            assert bits_eq(static[k], want[k]), (step, k)
        assert static['extra'].cpu().tolist() == list(range(12))
    assert seen[:2] == [[1, 3], [3, 0]] and all(0 <= i < 4 for i in seen[2]) and seen[2][0] != seen[2][1]
    with pytest.raises(ValueError):
        feed.land([0, 1, 2])                                                    # not the static batch
    with pytest.raises(ValueError):
        feed.land([0, 4])                                                       # a host list out of range
    with pytest.raises(ValueError):
        feed.land(next(pool.sampler(3, drop_last=False)))                       # nor a sampler's batch of another length
    with pytest.raises(ValueError):
        D.ResidentFeed({**static, 'flow': torch.zeros((2, 64, 64, 3), device='cuda')}, pool)
    feed.close()


def test_gathers_capture_and_replay(lib_built):
    """The three launches (bits, sparse, raw) once eagerly on a side stream, then in one torch.cuda.graph on a single stream chain, reading
    a persistent index tensor; between replays only its contents change, and the outputs follow."""
    n, N, B = 8224, 5, 3
    lay = planted_layout(n, POOLS[5][0])
    lay.add_raw('raw', list(np.random.default_rng(2).integers(-128, 128, (N, n)).astype(np.int8)), 'int8', 1.0 / 256.0)
    pool = D.ResidentPool(lay, 'cuda')
    pool.wait()
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    static = {k: torch.zeros((B, n), device='cuda') for k in lay.entries}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.gather_into(static, idx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool.gather_into(static, idx)
    for new in ([3, 1, 2], [4, 4, 0], [-1, 7, 3]):
        idx.copy_(dev_idx(new))
        for t in static.values():
            t.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        want = lay.reference_gather(new)
        for k in lay.entries:
            assert bits_eq(static[k], want[k]), (new, k)


def test_refusals_at_the_abi(lib_built):
    from strajnet_amd._lib import StjError
    from strajnet_amd.ops import _p, _st, call
    w = torch.zeros(64, dtype=torch.int32, device='cuda')
    vb = torch.zeros(4, dtype=torch.int64, device='cuda')
    idx = torch.zeros(4, dtype=torch.int32, device='cuda')
    dst = torch.full((256,), 5.0, device='cuda')
    bits = lambda N, d, B, n: call('stj_gather_bits', _p(w), _p(idx), N, _p(d), B, n, _st())
    sparse = lambda N, d, B, n: call('stj_gather_sparse', _p(w), _p(w), _p(vb), _p(w), 0, _p(idx), N, _p(d), B, n, _st())
    raw = lambda N, d, B, n: call('stj_gather_raw', _p(w), 1, _p(idx), N, _p(d), B, n, 1.0, _st())
    for fn in (bits, sparse):
        with pytest.raises(StjError, match='-3'):
            fn(1, dst, 1, 40)                                                   # n no multiple of 32
    for fn in (bits, sparse, raw):
        with pytest.raises(StjError, match='-3'):
            fn(1, dst[1:], 1, 32)                                               # dst off by 4 bytes
        with pytest.raises(StjError, match='-3'):
            fn(0, dst, 1, 32)                                                   # an empty pool
        with pytest.raises(StjError, match='-3'):
            fn(1, dst, 1, 1 << 32)
        fn(1, dst, 0, 32)                                                       # B = 0: STJ_OK, nothing launched
        fn(0, dst, 0, 32)
    with pytest.raises(StjError, match='-3'):
        call('stj_gather_sparse', _p(w), _p(w), vb.data_ptr() + 4, _p(w), 0, _p(idx), 1, _p(dst), 1, 32, _st())       # val_base off by 4
    with pytest.raises(StjError, match='-3'):
        call('stj_gather_bits', _p(w), idx.data_ptr() + 2, 1, _p(dst), 1, 32, _st())
    torch.cuda.synchronize()
    assert (dst == 5.0).all()
