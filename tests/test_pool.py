"""Scenes resident in HBM, host side (strajnet_amd/data.py PoolLayout, PoolSampler): the pool's format by a hand-written known answer,
from_examples against unpack_example_reference, the refusals, and the sampler on the CPU device.  All comparisons are bitwise."""
import numpy as np
import pytest
import torch

from strajnet_amd import data as D
from test_packed import u32, _raw_example


def _three_scenes():
    """Three scenes of 64 elements; scene 1 has no present word."""
    x = np.zeros((3, 64), np.float32)
    x[0, [0, 9, 31, 32, 63]] = [1.0, 2.0, -0.0, 4.0, 5.0]
    x[2, [1, 40]] = [7.0, -8.0]
    return x


def test_known_answer():
    x = _three_scenes()
    lay = D.PoolLayout()
    lay.add_sparse('flow', [D.pack_sparse(s) for s in x], 64)
    lay.add_bits('ogm', [D.pack_bits(u32(s)) for s in x])
    lay.add_raw('map_img', [np.arange(4 * i, 4 * i + 4, dtype=np.int8) for i in range(3)], 'int8', 1.0 / 256.0)
    e = lay.entries['flow']
    assert lay.N == 3 and e['val_base'].dtype == np.int64 and e['val_base'].tolist() == [0, 5, 5, 7]      # the running total; 1 is empty
    assert (np.diff(e['val_base']) >= 0).all() and e['val_base'][1] == e['val_base'][2]
    assert e['mask'].shape == (3, 2) and e['offs'].tolist() == [[0, 5], [0, 0], [0, 2]] and e['vals'].size == 7
    assert e['mask'][0].tobytes() == bytes.fromhex('01020080' '01000080') and lay.entries['ogm']['words'].tobytes() == e['mask'].tobytes()
    assert lay.nbytes == 2 * 24 + 24 + 32 + 28 + 12
    got = lay.reference_gather([2, 0, 2, -1, 5])                                                           # clamped: 2, 0, 2, 0, 2
    want = x[[2, 0, 2, 0, 2]]
    assert got['flow'].dtype == np.float32 and got['flow'].shape == (5, 64) and np.array_equal(u32(got['flow']), u32(want))
    assert np.array_equal(u32(got['ogm']), u32((u32(want) != 0).astype(np.float32)))
    assert got['map_img'].tolist() == [[8 / 256, 9 / 256, 10 / 256, 11 / 256], [0, 1 / 256, 2 / 256, 3 / 256]] * 2 + [[8 / 256, 9 / 256, 10 / 256, 11 / 256]]
    assert lay.reference_gather([])['flow'].shape == (0, 64)


@pytest.mark.parametrize('test', [False, True])
def test_from_examples_matches_unpack_example_reference(test):
    rng = np.random.default_rng(7)
    raw = [_raw_example(rng, 64, 32, test) for _ in range(4)]
    packed = [D.pack_example(e, 64, 32, test) for e in raw]
    lay = D.PoolLayout.from_examples(packed, 64, 32, test)
    spec = D.feature_spec(64, 32, test)
    assert set(lay.entries) == {D.POOL_NAMES[name] for name in spec} and lay.N == 4
    assert lay.entries['ogm']['kind'] == 'bits' and lay.entries['flow']['kind'] == 'sparse' and lay.entries['map_img']['dtype'] == 'int8'
    assert lay.entries['obs']['dtype'] == 'float64' and lay.entries['map_img']['scale'] == 1.0 / 256.0
    want = [D.unpack_example_reference(p, 64, 32, test) for p in packed]
    for idx in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 2, 0, 2, 2], [1]):
        got = lay.reference_gather(idx)
        for name in spec:
            g = got[D.POOL_NAMES[name]]
            assert g.dtype == np.float32 and g.shape == (len(idx),) + want[0][name].shape, name
            for b, i in enumerate(idx):
                assert np.array_equal(u32(g[b]), u32(want[i][name])), (name, b, i)
    # records that are not packed at all are stored raw (ground truth after its crop) and give the same tensors
    lay_raw = D.PoolLayout.from_examples(raw, 64, 32, test)
    assert all(e['kind'] == 'raw' for e in lay_raw.entries.values()) and lay_raw.nbytes > lay.nbytes
    got, got_raw = lay.reference_gather([3, 0]), lay_raw.reference_gather([3, 0])
    for key in got:
        assert np.array_equal(u32(got[key]), u32(got_raw[key])), key
    # names: record name -> key
    lay_id = D.PoolLayout.from_examples(packed, 64, 32, test, names={})
    assert set(lay_id.entries) == set(spec)


def test_refusals_name_key_and_scene():
    x = _three_scenes()
    packs = [D.pack_sparse(s) for s in x]
    bad = list(packs)
    bad[1] = (packs[1][0], np.array([0, 3], np.uint32), packs[1][2])                    # offs[-1] = 3 but no value words
    with pytest.raises(ValueError, match=r"'flow'.* scene 1"):
        D.PoolLayout().add_sparse('flow', bad, 64)
    bad[1] = (packs[1][0], np.array([2, 1], np.uint32), packs[1][2])                    # not a prefix from 0
    with pytest.raises(ValueError, match=r"'flow'.* scene 1"):
        D.PoolLayout().add_sparse('flow', bad, 64)
    with pytest.raises(ValueError, match=r"'flow'.* scene 2"):                          # a scene of another size
        D.PoolLayout().add_sparse('flow', packs[:2] + [D.pack_sparse(np.zeros(96, np.float32))], 64)
    with pytest.raises(ValueError, match=r"'ogm'.* scene 1"):
        D.PoolLayout().add_bits('ogm', [np.zeros(2, np.uint32), np.zeros(3, np.uint32)])
    with pytest.raises(ValueError, match=r"'m'.* scene 2"):
        D.PoolLayout().add_raw('m', [np.zeros(8, np.int8), np.zeros(8, np.int8), np.zeros(9, np.int8)], 'int8')
    lay = D.PoolLayout().add_sparse('flow', packs, 64)
    with pytest.raises(ValueError, match=r"'flow'.*twice"):                             # a key twice
        lay.add_sparse('flow', packs, 64)
    with pytest.raises(ValueError, match=r"'ogm'.* scene 2"):                           # differing scene counts: scene 2 is missing
        lay.add_bits('ogm', [D.pack_bits(u32(s)) for s in x[:2]])
    assert set(lay.entries) == {'flow'}
    for idx in ([0, 3], [-1], [1, 2, 1 << 31]):                                         # a host index list out of range
        with pytest.raises(ValueError, match='outside the 3 scenes'):
            lay.check_index(idx)
    assert lay.check_index([2, 0, 2]).tolist() == [2, 0, 2]
    with pytest.raises(RuntimeError):                                                   # device only, as the neighbouring classes
        D.ResidentPool(lay, 'cpu')


def test_sampler_on_the_cpu_device():
    N, B = 10, 3
    s = D.PoolSampler(N, B, 'cpu', shuffle=True, seed=5)
    e0, e1 = s.epoch(), s.epoch()
    assert len(s) == 3 and len(e0) == 3 and all(t.dtype == torch.int32 and t.shape == (B,) for t in e0)
    full = D.PoolSampler(N, B, 'cpu', shuffle=True, seed=5, drop_last=False)
    f0, f1 = full.epoch(), full.epoch()
    assert len(full) == 4 and [t.numel() for t in f0] == [3, 3, 3, 1]
    assert sorted(torch.cat(f0).tolist()) == list(range(N)) == sorted(torch.cat(f1).tolist())          # every index exactly once
    assert torch.cat(f0).tolist() != torch.cat(f1).tolist()                                           # two epochs differ
    assert torch.cat(e0).tolist() == torch.cat(f0).tolist()[:9] and torch.cat(e1).tolist() == torch.cat(f1).tolist()[:9]   # same seed
    assert len(set(torch.cat(e0).tolist())) == 9
    other = D.PoolSampler(N, B, 'cpu', shuffle=True, seed=6)
    assert torch.cat(other.epoch()).tolist() != torch.cat(e0).tolist()
    # the iterator runs through the epochs without an end
    it = D.PoolSampler(N, B, 'cpu', shuffle=True, seed=5)
    seq = [next(it) for _ in range(6)]
    assert torch.cat(seq).tolist() == torch.cat(e0 + e1).tolist()
    order = D.PoolSampler(N, B, 'cpu', shuffle=False, drop_last=False)
    assert torch.cat([next(order) for _ in range(5)]).tolist() == list(range(N)) + [0, 1, 2]
    assert torch.cat(D.PoolSampler(N, B, 'cpu', shuffle=False).epoch()).tolist() == list(range(9))
    with pytest.raises(ValueError):
        D.PoolSampler(2, 3, 'cpu')


@pytest.mark.parametrize('test', [False, True])
def test_feature_table_is_the_layouts_keys_and_refuses_another_layout(test):
    """The one walk from record features to pool keys: over PoolLayout.empty it yields exactly the layout's keys with their kind and n, and
    a key of another kind, size or dtype raises ValueError naming the key."""
    lay = D.PoolLayout.empty(1, 64, 32, test)
    spec = D.feature_spec(64, 32, test)
    rows = list(D._feature_table(lay.geometry, lay.entries))
    assert [f.name for f in rows] == list(spec) and [f.key for f in rows] == list(lay.entries)
    for f in rows:
        e = lay.entries[f.key]
        assert f.entry is e and (f.kind, f.n) == (e['kind'], e['n']) and f.key == D.POOL_NAMES[f.name], f.name
        assert (f.dtype, f.shape, f.crop, f.scale) == spec[f.name] and f.n == int(np.prod(D.decoded_shape(f.shape, f.crop))), f.name
        assert f.kind == D.PACKED_KIND.get(f.name, 'raw') and (f.kind != 'raw' or e['dtype'] == f.dtype), f.name
    free = list(D._feature_table(lay.geometry))                                        # without entries: the same rows, nothing checked
    assert [(f.name, f.key, f.kind, f.n) for f in free] == [(f.name, f.key, f.kind, f.n) for f in rows] and all(f.entry is None for f in free)
    n = lay.entries['flow']['n']
    zero = np.zeros(n, np.float32)
    others = {'bits': D.PoolLayout().add_bits('flow', [D.pack_bits(zero)]),
              'another n': D.PoolLayout().add_sparse('flow', [D.pack_sparse(zero[:n // 2])], n // 2),
              'raw float64': D.PoolLayout().add_raw('flow', [zero.astype(np.float64)], 'float64'),
              'missing': D.PoolLayout()}
    for what, other in others.items():
        entries = {k: e for k, e in lay.entries.items() if k != 'flow'}
        entries.update(other.entries)
        with pytest.raises(ValueError, match="'flow'"):
            list(D._feature_table(lay.geometry, entries))
    wrong = dict(lay.entries, map_img=D.PoolLayout().add_raw('map_img', [np.zeros(lay.entries['map_img']['n'], np.uint8)], 'bool').entries['map_img'])
    with pytest.raises(ValueError, match="'map_img'"):                                  # a raw key of the right size and another dtype
        list(D._feature_table(lay.geometry, wrong))
