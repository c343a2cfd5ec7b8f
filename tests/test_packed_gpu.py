"""Packed record features on the device (csrc/unpack.hip through strajnet_amd/data.py): stj_unpack_bits / stj_unpack_sparse against
data.unpack_reference, decode_batch_packed against decode_batch of the unpacked records, the packed feed of a captured step, graph
capture, and the refusal of sizes that are no multiple of 32.  Every comparison is bitwise."""
import os

import numpy as np
import pytest
import torch

from strajnet_amd import data as D
from test_packed import SIZES, planted, u32, _raw_example

pytestmark = pytest.mark.gpu


def dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def run_sparse(scenes, n):
    """scenes: list of float32 [n] -> the kernel's [B, n] as uint32 (host)."""
    from strajnet_amd.ops import _p, _st, call
    B = len(scenes)
    packs = [D.pack_sparse(x) for x in scenes]
    base = np.zeros(B + 1, np.uint32)
    base[1:] = np.cumsum([p[2].size for p in packs])
    mask, offs = dev_words(np.concatenate([p[0] for p in packs])), dev_words(np.concatenate([p[1] for p in packs]))
    vals = dev_words(np.concatenate([p[2] for p in packs] + [np.zeros(1, np.uint32)]))              # never empty: a real pointer
    dst = torch.full((B, n), float('nan'), device='cuda')
    call('stj_unpack_sparse', _p(mask), _p(offs), _p(dev_words(base)), _p(vals), int(base[-1]), _p(dst), B, n, _st())
    return u32(dst.cpu().numpy())


def run_bits(scenes, n):
    from strajnet_amd.ops import _p, _st, call
    B = len(scenes)
    bits = dev_words(np.concatenate([D.pack_bits(x) for x in scenes]))
    dst = torch.full((B, n), float('nan'), device='cuda')
    call('stj_unpack_bits', _p(bits), _p(dst), B * n, _st())
    return dst.cpu().numpy()


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n', SIZES)
def test_kernels_match_reference(lib_built, n, B):
    """Every planted plane as scene 0, with two other planes behind it when B = 3 (so that the scenes' val_base differ).  The expected
    result is unpack_reference of the packed streams, which test_packed.py shows to be the input."""
    planes = planted(n)
    names = list(planes)
    for i, name in enumerate(names):
        scenes = [planes[names[(i + 4 * j) % len(names)]] for j in range(B)]
        want = np.stack([D.unpack_reference('sparse', *D.pack_sparse(x), n) for x in scenes])
        got = run_sparse(scenes, n)
        assert np.array_equal(got, u32(want)), (name, np.flatnonzero(got != u32(want))[:8])
        bytes_ = [(u32(x) != 0).astype(np.uint8) * 5 for x in scenes]
        want = np.stack([D.unpack_reference('bits', D.pack_bits(x), n) for x in bytes_])
        got = run_bits(bytes_, n)
        assert np.array_equal(u32(got), u32(want)), (name, np.flatnonzero(got != want)[:8])


def _decode_both(tmp_path, grid, out, test, B, seed):
    rng = np.random.default_rng(seed)
    exs = [_raw_example(rng, grid, out, test) for _ in range(B)]
    if test:
        for i, e in enumerate(exs):
            e['scenario/id'] = f'scn{i}'.encode()
    p = os.path.join(tmp_path, 'p.tfrecords')
    D.write_tfrecord(p, [D.serialize_example(D.pack_example(e, grid, out, test)) for e in exs])
    got = None
    for batch in D.batches(D.read_tfrecord(p), B):
        got = D.decode_batch_packed(batch, 'cuda', grid, out, test)
    want = D.decode_batch(exs, 'cuda', grid, out, test)
    assert set(got) == set(want)
    for name in want:
        if name == 'scenario/id':
            assert got[name] == want[name]
            continue
        assert got[name].shape == want[name].shape and got[name].dtype == torch.float32, name
        assert torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)), name           # bitwise: NaN payloads, -0.0
    return got


@pytest.mark.parametrize('test', [False, True])
def test_decode_batch_packed_equals_decode_batch(lib_built, tmp_path, test):
    got = _decode_both(tmp_path, 64, 32, test, 3, 5)
    assert got['ogm'].shape == (3, 64, 64, 11, 2) and (test or got['gt_flow'].shape == (3, 8, 32, 32, 2))


def test_decode_batch_packed_real_geometry(lib_built, tmp_path):
    """(512, 256), B = 1, test records: ogm is 5.7 M elements in 704 workgroups, vec_flow 64 blocks."""
    got = _decode_both(tmp_path, 512, 256, True, 1, 6)
    assert got['ogm'].shape == (1, 512, 512, 11, 2) and got['scenario/id'] == [b'scn0']


def test_packed_feed_lands_every_batch(lib_built):
    """data.PackedFeed at the shapes of test_host_feed_lands_every_batch: three consecutive batches arrive bit-exactly in the static
    inputs, each landing while the next is uploaded; the sparse keys carry a different number of present words per batch (none in the
    third), 'big' spans several upload pieces."""
    from strajnet_amd.data import PackedFeed, SparseHost, bits_host
    g = torch.Generator().manual_seed(0)
    static = {'ogm': torch.zeros((2, 64, 64, 11, 2), device='cuda'), 'map_img': torch.zeros((2, 64, 64, 3), device='cuda'),
              'flow': torch.zeros((2, 64, 64, 2), device='cuda'), 'big': torch.zeros((3, 1 << 20), device='cuda'),
              'obs': torch.zeros((2, 48, 11, 8), device='cuda')}
    host = {'ogm': bits_host(np.zeros((2, 64 * 64 * 22), np.uint8)), 'map_img': torch.zeros((2, 64, 64, 3), dtype=torch.uint8).pin_memory(),
            'flow': SparseHost(2, 64 * 64 * 2), 'big': SparseHost(3, 1 << 20), 'obs': torch.zeros((2, 48, 11, 8)).pin_memory(),
            'ignored': torch.zeros(4).pin_memory()}
    feed = PackedFeed(static, host, packed={'ogm': 'bits', 'flow': 'sparse', 'big': 'sparse'}, raw={'map_img': 'int8'})
    counts = []

    def fill(seed, density):
        g.manual_seed(seed)
        ogm = (torch.rand(static['ogm'].shape, generator=g) < 0.3).to(torch.uint8) * 7
        host['ogm'].copy_(torch.from_numpy(D.pack_bits(ogm.numpy()).view(np.int32)))
        host['map_img'].copy_(torch.randint(-128, 128, host['map_img'].shape, generator=g, dtype=torch.int16).to(torch.int8).view(torch.uint8))
        sparse = lambda shape: torch.where(torch.rand(shape, generator=g) < density, torch.randn(shape, generator=g), torch.zeros(()))
        flow, big = sparse(static['flow'].shape), sparse(static['big'].shape)
        big.view(torch.int32)[:, 7] = -2 ** 31                                                    # -0.0 is present
        if density == 0:
            big.zero_()
        host['flow'].fill(flow); host['big'].fill(big)
        host['obs'].copy_(torch.randn(host['obs'].shape, generator=g))
        counts.append((host['flow'].count, host['big'].count))
        return {'ogm': (ogm != 0).float(), 'map_img': host['map_img'].view(torch.int8).float() / 256.0, 'flow': flow, 'big': big,
                'obs': host['obs'].clone()}
    dens = [0.05, 0.6, 0.0, 0.01]                    # landed: the first three
    want = fill(1, dens[0])
    feed.start()
    for step in range(3):
        feed.wait_uploaded()              # the batch in flight has left the host buffers: refill them with the next one
        nxt = fill(2 + step, dens[1 + step])
        feed.land()                       # lands `want`, starts uploading `nxt`
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(static[k].cpu().view(torch.int32), want[k].view(torch.int32)), (step, k)
        want = nxt
    feed.wait_uploaded()
    assert feed.upload_bytes() == (host['ogm'].numel() * 4 + host['map_img'].numel() + host['obs'].numel() * 4 + host['flow'].nbytes + host['big'].nbytes)
    feed.close()
    assert len(set(counts)) == 4 and counts[2] == (0, 0) and counts[1][1] > (3 << 19) // 4              # distinct lengths; several pieces


def test_kernels_capture_and_replay(lib_built):
    """Both kernels in one torch.cuda.graph, replayed with different packed contents in the same buffers (n_vals = the capacity of the
    value buffer: the clamp bound, fixed at capture)."""
    from strajnet_amd.ops import _p, _st, call
    B, n = 3, 8224
    nw, nb1 = n // 32, 3
    mask, offs = torch.zeros(B * nw, dtype=torch.int32, device='cuda'), torch.zeros(B * nb1, dtype=torch.int32, device='cuda')
    vb, vals = torch.zeros(B + 1, dtype=torch.int32, device='cuda'), torch.zeros(B * n, dtype=torch.int32, device='cuda')
    bits = torch.zeros(B * nw, dtype=torch.int32, device='cuda')
    out_s, out_b = torch.zeros((B, n), device='cuda'), torch.zeros((B, n), device='cuda')

    def launch():
        call('stj_unpack_sparse', _p(mask), _p(offs), _p(vb), _p(vals), B * n, _p(out_s), B, n, _st())
        call('stj_unpack_bits', _p(bits), _p(out_b), B * n, _st())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    planes = planted(n)
    for names in (('rand0.5', 'special', 'run8192'), ('last', 'rand0.02', 'full')):
        scenes = [planes[k] for k in names]
        packs = [D.pack_sparse(x) for x in scenes]
        base = np.zeros(B + 1, np.uint32)
        base[1:] = np.cumsum([p[2].size for p in packs])
        v = np.concatenate([p[2] for p in packs])
        mask.copy_(dev_words(np.concatenate([p[0] for p in packs]))); offs.copy_(dev_words(np.concatenate([p[1] for p in packs])))
        vb.copy_(dev_words(base)); vals[:v.size].copy_(dev_words(v))
        bits.copy_(mask)
        out_s.fill_(float('nan')); out_b.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        want = np.stack([D.unpack_reference('sparse', *p, n) for p in packs])
        assert np.array_equal(u32(out_s.cpu().numpy()), u32(want)), names
        assert np.array_equal(out_b.cpu().numpy(), (u32(want) != 0).astype(np.float32)), names


def test_unsupported_sizes_raise(lib_built):
    from strajnet_amd._lib import StjError
    from strajnet_amd.ops import _p, _st, call
    w = torch.zeros(64, dtype=torch.int32, device='cuda')
    dst = torch.zeros(256, device='cuda')
    with pytest.raises(StjError, match='-3'):
        call('stj_unpack_bits', _p(w), _p(dst), 40, _st())
    with pytest.raises(StjError, match='-3'):
        call('stj_unpack_sparse', _p(w), _p(w), _p(w), _p(w), 0, _p(dst), 1, 40, _st())
    with pytest.raises(StjError, match='-3'):
        call('stj_unpack_bits', _p(w), _p(dst[1:]), 32, _st())                                     # dst not 16-byte aligned
    with pytest.raises(StjError, match='-3'):
        call('stj_unpack_sparse', _p(w), _p(w), _p(w), _p(w), 0, _p(dst), 1, 1 << 32, _st())
    call('stj_unpack_bits', _p(w), _p(dst), 0, _st())                                              # zero sizes: STJ_OK, nothing launched
    call('stj_unpack_sparse', _p(w), _p(w), _p(w), _p(w), 0, _p(dst), 0, 64, _st())
    call('stj_unpack_sparse', _p(w), _p(w), _p(w), None, 0, _p(dst), 2, 64, _st())                 # no values at all: zeros, no gather
    torch.cuda.synchronize()
    assert not dst[:128].any()
