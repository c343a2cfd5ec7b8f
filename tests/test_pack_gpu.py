"""Raw records packed on the device into pool slots (csrc/pack.hip through strajnet_amd/data.py): stj_pack_bits / stj_pack_sparse_count /
stj_pool_admit / stj_pack_sparse_commit / stj_pool_put_raw against the host packers (pack_bits, pack_sparse, _decoded), PoolWriter against
decode_batch and PoolLayout.replace_reference, all-or-nothing admission, skipped slots, graph capture and the refusals of the C ABI.
Every comparison is bitwise."""
import numpy as np
import pytest
import torch

from strajnet_amd import data as D
from test_packed import SIZES, planted, u32, _raw_example

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
SENT = -559038737                                                               # 0xdeadbeef as int32: no word any packer writes here
G, O = 64, 32


def _abi():
    from strajnet_amd.ops import _p, _st, call
    return _p, _st, call


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device='cuda')


def host(t):
    return t.cpu().numpy().view(np.uint32)


class Slots:
    """The arrays of one bits key and one sparse key of a pool of N slots of n elements, pre-filled with the sentinel, and the four launches."""

    def __init__(self, N, B, n, cap=None):
        self.N, self.B, self.n, self.nw, self.nblk = N, B, n, n // 32, -(-n // D.SPARSE_BLOCK)
        self.cap = n if cap is None else cap
        self.words, self.mask, self.offs = sent(N, self.nw), sent(N, self.nw), sent(N, self.nblk + 1)
        self.vals = sent(max(N * self.cap, 1))
        self.val_base = torch.arange(N + 1, dtype=torch.int64, device='cuda') * self.cap
        self.stage, self.ok = sent(B, self.nblk + 1), torch.full((B,), 77, dtype=torch.int32, device='cuda')

    def run(self, src_words, src_bytes, slots, geom):
        """src_words uint32 [B, S], src_bytes uint8 [B, S] (host arrays): the float32 and the bool source of the same geometry."""
        _p, _st, call = _abi()
        fw = torch.from_numpy(np.ascontiguousarray(src_words).view(np.int32)).cuda()
        fb = torch.from_numpy(np.ascontiguousarray(src_bytes)).cuda()
        sl = dev_i32(slots)
        call('stj_pack_sparse_count', _p(fw), _p(self.stage), self.B, *geom, _st())
        call('stj_pool_admit', _p(self.stage), self.nblk, _p(self.val_base), _p(sl), self.N, _p(self.ok), self.B, 1, _st())
        call('stj_pack_bits', _p(fb), _p(self.ok), _p(sl), self.N, _p(self.words), self.B, *geom, _st())
        call('stj_pack_sparse_commit', _p(fw), _p(self.stage), _p(self.ok), _p(sl), self.N, _p(self.mask), _p(self.offs), _p(self.val_base),
             _p(self.vals), self.N * self.cap, self.B, *geom, _st())
        torch.cuda.synchronize()

    def check(self, slots, bits_want, sparse_want, what):
        """bits_want[b]: pack_bits words, sparse_want[b]: pack_sparse's triple.  A scene in range within the capacity landed, with ok 1; every
        other slot, and the tail of every slot behind its value words, still holds the sentinel."""
        ok, words, mask, offs, vals, stage = (host(t) for t in (self.ok, self.words, self.mask, self.offs, self.vals, self.stage))
        named = {}
        for b, s in enumerate(slots):
            m, o, v = sparse_want[b]
            want = 0 <= s < self.N and v.size <= self.cap
            assert ok[b] == int(want), (what, b, s, ok[b])
            assert np.array_equal(stage[b], o), (what, b, 'staged prefix')
            if want:
                named[s] = b
                assert np.array_equal(words[s], bits_want[b]), (what, b, 'bits words', np.flatnonzero(words[s] != bits_want[b])[:8])
                assert np.array_equal(mask[s], m), (what, b, 'mask', np.flatnonzero(mask[s] != m)[:8])
                assert np.array_equal(offs[s], o), (what, b, 'offs')
                lo = s * self.cap
                assert np.array_equal(vals[lo:lo + v.size], v), (what, b, 'vals')
                assert (vals[lo + v.size:lo + self.cap] == np.uint32(SENT & 0xffffffff)).all(), (what, b, 'tail of the slot')
        for s in range(self.N):
            if s not in named:
                for part, a in (('words', words[s]), ('mask', mask[s]), ('offs', offs[s]), ('vals', vals[s * self.cap:(s + 1) * self.cap])):
                    assert (a == np.uint32(SENT & 0xffffffff)).all(), (what, 'slot not named but written', s, part)


def _bool_bytes(w):
    """uint8 source of a bool plane with the non-zero pattern of the words w, values 1 .. 255."""
    return ((w != 0) * ((np.arange(w.size, dtype=np.int64) % 255) + 1).reshape(w.shape)).astype(np.uint8)


@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('n', SIZES)
def test_kernels_match_the_host_packers(lib_built, n, N):
    planes = planted(n)
    names = list(planes)
    geom = (1, 1, n, 1, 0, 0, 1, n)
    for B in (1, 3):
        for g0 in range(0, len(names), B):
            group = (names + names)[g0:g0 + B]
            slots = [N * 3 // 5] if B == 1 else ([4, 0, 2] if N == 5 else [N, 0, -1])       # N = 1: one scene lands, two are skipped
            src = np.stack([u32(planes[k]) for k in group])
            pool = Slots(N, B, n)
            pool.run(src, _bool_bytes(src), slots, geom)
            pool.check(slots, [D.pack_bits(src[b]) for b in range(B)], [D.pack_sparse(src[b]) for b in range(B)], (n, N, B, group))


@pytest.mark.parametrize('crop,C', [((4, 4, 8, 8), 1), ((4, 4, 8, 8), 2), ((4, 2, 8, 12), 1)])
def test_crop_matches_decoded_plus_packers(lib_built, crop, C):
    """T = 2, H = W = 16; the third geometry has rows of 12 elements: a mask word straddles source rows."""
    T, H, W = 2, 16, 16
    rng = np.random.default_rng(31)
    N, B, slots = 3, 2, [2, 0]
    shape = (T, H, W, C)
    n = T * crop[2] * crop[3] * C
    assert n % 32 == 0
    for dens in (0.0, 0.3, 1.0):
        src = np.where(rng.random((B,) + shape) < dens, rng.normal(size=(B,) + shape), 0.0).astype(np.float32)
        src.reshape(B, -1).view(np.uint32)[:, 5::17] = 0x80000000                                    # -0.0 is present, inside and outside the crop
        words = u32(src).reshape(B, -1)
        byts = _bool_bytes(words)
        dec_w = [np.ascontiguousarray(D._decoded(words[b].tobytes(), 'float32', shape, crop)) for b in range(B)]
        dec_b = [np.ascontiguousarray(D._decoded(byts[b].tobytes(), 'bool', shape, crop)) for b in range(B)]
        assert dec_w[0].size == n
        pool = Slots(N, B, n)
        pool.run(words, byts, slots, (T, H, W, C) + crop)
        pool.check(slots, [D.pack_bits(a) for a in dec_b], [D.pack_sparse(a) for a in dec_w], (crop, C, dens))


def _records(seed, count, test=False, grid=G, out=O):
    rng = np.random.default_rng(seed)
    return [_raw_example(rng, grid, out, test) for _ in range(count)]


def _gather_equals_decode_batch(pool, slots, exs, test, grid=G, out=O):
    got = pool.gather(slots)
    want = D.decode_batch(exs, 'cuda', grid, out, test)
    assert set(got) == {D.POOL_NAMES[name] for name in want}
    for name in want:
        g = got[D.POOL_NAMES[name]]
        assert g.shape == want[name].shape and g.dtype == torch.float32, name
        assert torch.equal(g.view(torch.int32), want[name].view(torch.int32)), name


def _device_equals_layout(pool, lay):
    """Every device array of the pool is, byte for byte, the array of the layout (on which replace_reference ran the same replacements)."""
    torch.cuda.synchronize()
    for key in lay.entries:
        for part, a in lay.arrays(key).items():
            got = pool.dev_arrays[key][part].cpu().numpy()[:a.nbytes]
            assert got.tobytes() == np.ascontiguousarray(a).tobytes(), (key, part)


@pytest.mark.parametrize('test', [False, True])
def test_round_trip_equals_decode_batch(lib_built, test):
    exs = _records(41, 5, test)
    pool = D.ResidentPool.empty(5, 'cuda', G, O, test)
    twin_lay = D.PoolLayout.empty(5, G, O, test)
    twin = D.ResidentPool(twin_lay, 'cuda')                                       # ResidentPool(PoolLayout.empty(...)) is the same pool
    assert pool.nbytes == twin.nbytes == twin_lay.nbytes > 0 and set(pool.dev_arrays) == set(twin.dev_arrays)
    _device_equals_layout(pool, twin_lay)
    _device_equals_layout(twin, twin_lay)
    zero = pool.gather([0, 4])
    assert all(not t.view(torch.int32).any() for t in zero.values())
    writers = [p.writer(3) for p in (pool, twin)]
    assert writers[0].ok.dtype == torch.int32 and writers[0].slots.shape == (3,) and writers[0].raw['ogm'].shape == (3, G * G * 22)
    for slots, batch in (([3, 0, 4], exs[:3]), ([4, 3, 1], [exs[3], exs[4], exs[0]])):   # the second put replaces slots 3 and 4
        for w in writers:
            ok = w.put(slots, batch)
            assert ok is w.ok and ok.cpu().tolist() == [1, 1, 1]
        assert twin_lay.replace_reference(slots, batch, G, O, test) == [1, 1, 1]
        for p in (pool, twin):
            _gather_equals_decode_batch(p, slots, batch, test)
            _device_equals_layout(p, twin_lay)
    _gather_equals_decode_batch(pool, [0], [exs[1]], test)                               # slot 0 kept the first put's scene
    assert all(not t.view(torch.int32).any() for t in pool.gather([2]).values())         # slot 2 was never named
    # the feed works on such a pool unchanged
    static = {k: torch.zeros((2,) + e['shape'], device='cuda') for k, e in pool.layout.entries.items()}
    feed = D.ResidentFeed(static, pool, sampler=pool.sampler(2, seed=1))
    feed.land(dev_i32([4, 1]))
    want = D.decode_batch([exs[3], exs[0]], 'cuda', G, O, test)
    for name in want:
        assert torch.equal(static[D.POOL_NAMES[name]].view(torch.int32), want[name].view(torch.int32)), name


def _present(ex, name):
    dt, shape, crop, _ = D.feature_spec(G, O)[name]
    return int(np.count_nonzero(D._decoded(ex[name], dt, shape, crop)))


def test_admission_is_all_or_nothing(lib_built):
    exs = _records(42, 3)
    counts = [_present(ex, 'gt_flow') for ex in exs]
    big = int(np.argmax(counts))                                                  # the scene of the batch that will not fit
    assert counts[big] - 1 >= max(counts[b] for b in range(3) if b != big), counts
    for cap, landed in ((counts[big] - 1, False), (counts[big], True)):
        lay = D.PoolLayout.empty(4, G, O, capacity={'gt_flow': cap})
        pool = D.ResidentPool(lay, 'cuda')
        fill = [exs[(big + 1) % 3]] * 4                                            # something to keep in every slot: a scene that fits
        assert pool.writer(4).put([0, 1, 2, 3], fill).cpu().tolist() == [1, 1, 1, 1]
        lay.replace_reference([0, 1, 2, 3], fill, G, O)
        before = {(k, p): t.clone() for k, d in pool.dev_arrays.items() for p, t in d.items()}
        slots = [2, 0, 3]
        want_ok = [int(landed or b != big) for b in range(3)]
        ok = pool.writer(3).put(slots, exs[:3])
        assert ok.cpu().tolist() == want_ok, (cap, counts)
        assert lay.replace_reference(slots, exs[:3], G, O) == want_ok
        _device_equals_layout(pool, lay)                                           # the neighbours landed, as the NumPy statement says
        if not landed:
            s = slots[big]
            for (k, p), old in before.items():
                e = lay.entries[k]
                a, new = lay.arrays(k)[p], pool.dev_arrays[k][p]
                if p == 'vals':
                    lo, hi = 4 * int(e['val_base'][s]), 4 * int(e['val_base'][s + 1])
                elif p == 'val_base':
                    lo, hi = 0, a.nbytes
                else:
                    lo, hi = s * a[0].nbytes, (s + 1) * a[0].nbytes
                assert torch.equal(old[lo:hi], new[lo:hi]), ('a rejected scene changed its slot', k, p)
            _gather_equals_decode_batch(pool, [s], fill[:1], False)
        _gather_equals_decode_batch(pool, [slots[b] for b in range(3) if want_ok[b]], [exs[b] for b in range(3) if want_ok[b]], False)


def test_zero_capacity_and_empty_batch(lib_built):
    """A zero-size `vals` and B = 0 are tolerated: an all-zero flow plane lands in a slot of no value words, anything else is rejected."""
    caps = {'flow': 0, 'gt_flow': 0, 'origin_flow': 0}
    pool = D.ResidentPool.empty(2, 'cuda', G, O, capacity=caps)
    ex = _records(43, 1)[0]
    flat = dict(ex, **{name: bytes(len(ex[name])) for name in ('vec_flow', 'gt_flow', 'origin_flow')})
    assert pool.writer(2).put([1, 0], [flat, ex]).cpu().tolist() == [1, 0]
    _gather_equals_decode_batch(pool, [1], [flat], False)
    assert all(not t.view(torch.int32).any() for t in pool.gather([0]).values())
    w0 = pool.writer(0)
    assert w0.put([], []).shape == (0,) and w0.commit().shape == (0,)
    torch.cuda.synchronize()
    _gather_equals_decode_batch(pool, [1], [flat], False)


def test_slots_outside_the_pool_are_skipped(lib_built):
    N = 3
    exs = _records(44, 3, True)
    pool = D.ResidentPool.empty(N, 'cuda', G, O, True)
    w = pool.writer(3)
    assert w.put([1, 2, 0], [exs[2], exs[0], exs[1]]).cpu().tolist() == [1, 1, 1]
    torch.cuda.synchronize()
    before = {(k, p): t.clone() for k, d in pool.dev_arrays.items() for p, t in d.items()}
    ok = w.put(dev_i32([-1, N, INT_MAX]), exs)                                     # a device tensor is trusted: skipped, never clamped
    assert ok.cpu().tolist() == [0, 0, 0]
    for (k, p), old in before.items():
        assert torch.equal(old, pool.dev_arrays[k][p]), (k, p)
    assert w.put(dev_i32([-1, 1, N]), exs).cpu().tolist() == [0, 1, 0]             # and the neighbour of two skipped scenes lands
    _gather_equals_decode_batch(pool, [1, 2, 0], [exs[1], exs[0], exs[1]], True)
    for bad in ([-1, 0, 1], [0, 1, N], [0, 1, INT_MAX], [0, 1, 1], [0, 1]):         # a host list: range, duplicates, length
        with pytest.raises(ValueError):
            w.put(bad, exs)
    with pytest.raises(ValueError):
        w.put([0, 1, 2], [exs[0], exs[1], dict(exs[2], ogm=exs[2]['ogm'][:-1])])   # a record of the wrong length
    with pytest.raises(ValueError):
        w.put(torch.zeros(3, dtype=torch.int64, device='cuda'), exs)
    torch.cuda.synchronize()
    _gather_equals_decode_batch(pool, [1, 2, 0], [exs[1], exs[0], exs[1]], True)     # a refused put changed nothing


def _fill_raw(writer, exs):
    for name, t in writer.raw.items():
        t.copy_(torch.from_numpy(np.stack([np.frombuffer(ex[name], np.uint8) for ex in exs])))


def test_commit_captures_and_replays(lib_built):
    """About 16 launches once eagerly on a side stream, then in one torch.cuda.graph; between replays only the contents of writer.raw and
    writer.slots change, and the pool follows."""
    exs = _records(45, 6)
    pool = D.ResidentPool.empty(4, 'cuda', G, O)
    pool.wait()
    w = pool.writer(2)
    _fill_raw(w, exs[:2])
    w.slots.copy_(dev_i32([0, 1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w.commit()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.commit()
    held = {0: exs[0], 1: exs[1]}
    for slots, batch, want_ok in (([3, 1], exs[2:4], [1, 1]), ([0, 7], exs[4:6], [1, 0]), ([2, 3], [exs[1], exs[0]], [1, 1])):
        _fill_raw(w, batch)
        w.slots.copy_(dev_i32(slots))
        g.replay()
        torch.cuda.synchronize()
        assert w.ok.cpu().tolist() == want_ok, slots
        held.update({s: ex for s, ex, k in zip(slots, batch, want_ok) if k})
        _gather_equals_decode_batch(pool, sorted(held), [held[s] for s in sorted(held)], False)


def test_real_geometry(lib_built):
    """(512, 256), N = 2, B = 1, a training record: ogm is 704 blocks per scene, gt_flow 128, vec_flow 64."""
    ex = _records(46, 1, False, 512, 256)
    pool = D.ResidentPool.empty(2, 'cuda', 512, 256)
    e = pool.layout.entries
    assert e['ogm']['n'] == 704 * 8192 and e['gt_flow']['n'] == 128 * 8192 and e['flow']['n'] == 64 * 8192
    assert pool.writer(1).put([1], ex).cpu().tolist() == [1]
    _gather_equals_decode_batch(pool, [1], ex, False, 512, 256)
    assert all(not t.view(torch.int32).any() for t in pool.gather([0]).values())


def test_refusals_at_the_abi(lib_built):
    from strajnet_amd._lib import StjError
    _p, _st, call = _abi()
    src = torch.zeros(256, dtype=torch.int32, device='cuda')
    w = sent(64)
    vb = torch.zeros(4, dtype=torch.int64, device='cuda')
    ok, sl = torch.ones(4, dtype=torch.int32, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda')
    un = lambda n: (1, 1, n, 1, 0, 0, 1, n)
    bits = lambda g, B=1, N=1, src=src, ok=ok, sl=sl, pool=w: call('stj_pack_bits', _p(src), _p(ok), _p(sl), N, _p(pool), B, *g, _st())
    count = lambda g, B=1, src=src, stage=w: call('stj_pack_sparse_count', _p(src), _p(stage), B, *g, _st())
    commit = lambda g, B=1, N=1, ok=ok, sl=sl, vb=vb, n_vals=64, mask=w: call('stj_pack_sparse_commit', _p(src), _p(w), _p(ok), _p(sl), N, _p(mask),
                                                                              _p(w), _p(vb), _p(w), n_vals, B, *g, _st())
    admit = lambda B=1, N=1, nblk=1, ok=ok, sl=sl, vb=vb, stage=w: call('stj_pool_admit', _p(stage), nblk, _p(vb), _p(sl), N, _p(ok), B, 1, _st())
    raw = lambda n, item=1, B=1, N=1, ok=ok, sl=sl, src=src, pool=w: call('stj_pool_put_raw', _p(src), item, _p(ok), _p(sl), N, _p(pool), B, n, _st())
    off = lambda t, k: t.data_ptr() + k
    from ctypes import c_void_p as vp
    for fn in (bits, count, commit):
        with pytest.raises(StjError, match='-3'):
            fn(un(40))                                                          # n no multiple of 32
        with pytest.raises(StjError, match='-3'):
            fn((2, 8, 8, 1, 2, 2, 4, 5))                                        # a crop of 40 elements
        with pytest.raises(StjError, match='-3'):
            fn((4, 1, 1 << 30, 1, 0, 0, 1, 1 << 30))                            # n = 2^32
        with pytest.raises(StjError, match='-3'):
            fn((2, 1, 1 << 30, 1, 0, 0, 1, 1 << 30), B=1 << 14)                  # 2^32 workgroups
        with pytest.raises(StjError, match='-1'):
            fn((1, 1, -32, 1, 0, 0, 1, 32))                                     # a negative size
        with pytest.raises(StjError, match='-1'):
            fn(un(32), B=-1)
        with pytest.raises(StjError, match='-1'):
            fn((2, 8, 8, 1, 6, 0, 4, 8))                                        # the crop leaves the source
        fn(un(32), B=0)                                                         # B = 0: STJ_OK, nothing launched
    with pytest.raises(StjError, match='-3'):
        bits(un(32), sl=vp(off(sl, 2)))                                         # slots off by 2 bytes
    with pytest.raises(StjError, match='-3'):
        bits(un(32), ok=vp(off(ok, 2)))
    with pytest.raises(StjError, match='-3'):
        bits(un(32), pool=vp(off(w, 1)))
    with pytest.raises(StjError, match='-1'):
        bits(un(32), pool=None)
    with pytest.raises(StjError, match='-1'):
        bits(un(32), src=None)
    with pytest.raises(StjError, match='-3'):
        count(un(32), src=vp(off(src, 2)))                                      # a 4-byte stream off by 2
    with pytest.raises(StjError, match='-1'):
        count(un(32), stage=None)
    with pytest.raises(StjError, match='-3'):
        commit(un(32), vb=vp(off(vb, 4)))                                       # val_base off by 4
    with pytest.raises(StjError, match='-3'):
        commit(un(32), mask=vp(off(w, 2)))
    with pytest.raises(StjError, match='-1'):
        commit(un(32), n_vals=-1)
    with pytest.raises(StjError, match='-1'):
        commit(un(32), ok=None)
    with pytest.raises(StjError, match='-3'):
        admit(vb=vp(off(vb, 4)))
    with pytest.raises(StjError, match='-3'):
        admit(sl=vp(off(sl, 2)))
    with pytest.raises(StjError, match='-1'):
        admit(ok=None)
    with pytest.raises(StjError, match='-1'):
        admit(nblk=-1)
    with pytest.raises(StjError, match='-1'):
        admit(vb=None)                                                          # a stage without a val_base
    admit(B=0)
    with pytest.raises(StjError, match='-3'):
        raw(1 << 32)
    with pytest.raises(StjError, match='-3'):
        raw(8, item=4, pool=vp(off(w, 2)))                                      # a pool not aligned to its elements
    with pytest.raises(StjError, match='-3'):
        raw(8, ok=vp(off(ok, 2)))
    with pytest.raises(StjError, match='-1'):
        raw(8, item=3)
    with pytest.raises(StjError, match='-1'):
        raw(-1)
    with pytest.raises(StjError, match='-1'):
        raw(8, pool=None)
    raw(8, B=0)
    raw(0)
    torch.cuda.synchronize()
    assert (w == SENT).all() and (ok == 1).all() and not vb.any()              # nothing was written on a refusal
