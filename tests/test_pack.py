"""Replacing pool scenes in place, host side (strajnet_amd/data.py PoolLayout.empty / add_sparse(capacity=) / replace_reference): the
NumPy statement of what PoolWriter and csrc/pack.hip do.  Replaced slots against unpack_example_reference, the all-or-nothing capacity
rule, out-of-range and duplicate slots, and tight layouts unchanged by the slack-aware reference_gather.  All comparisons are bitwise."""
import copy

import numpy as np
import pytest

from strajnet_amd import data as D
from test_packed import u32, _raw_example

G, O = 64, 32
SPARSE_KEYS = {'vec_flow': 'flow', 'gt_flow': 'gt_flow', 'origin_flow': 'origin_flow'}


def _arrays(lay):
    return {(key, part): a.copy() for key in lay.entries for part, a in lay.arrays(key).items()}


def _same(before, lay, slot=None):
    """Every array of the layout (slot: only that slot's rows, and the slot's value words) is byte-identical to the copy `before`."""
    for key in lay.entries:
        e = lay.entries[key]
        for part, a in lay.arrays(key).items():
            old = before[(key, part)]
            if slot is None or part == 'val_base':
                assert np.array_equal(old, a), (key, part)
            elif part == 'vals':
                lo, hi = int(e['val_base'][slot]), int(e['val_base'][slot + 1])
                assert np.array_equal(old[lo:hi], a[lo:hi]), (key, part)
            else:
                assert old[slot].tobytes() == a[slot].tobytes(), (key, part)


def _present(ex, name, test=False):
    dt, shape, crop, _ = D.feature_spec(G, O, test)[name]
    return int(np.count_nonzero(D._decoded(ex[name], dt, shape, crop)))


@pytest.mark.parametrize('test', [False, True])
def test_replaced_slots_gather_as_the_packed_record(test):
    rng = np.random.default_rng(21)
    exs = [_raw_example(rng, G, O, test) for _ in range(4)]
    lay = D.PoolLayout.empty(5, G, O, test)
    spec = D.feature_spec(G, O, test)
    assert set(lay.entries) == {D.POOL_NAMES[name] for name in spec} and lay.N == 5
    assert lay.entries['ogm']['kind'] == 'bits' and lay.entries['flow']['kind'] == 'sparse' and lay.entries['obs']['dtype'] == 'float64'
    n = lay.entries['flow']['n']
    assert lay.entries['flow']['val_base'].tolist() == [i * n for i in range(6)]           # the default capacity: n, which never rejects
    zero = lay.reference_gather([0, 4])
    assert all(not u32(v).any() for v in zero.values())
    assert lay.replace_reference([3, 0, 4], exs[:3], G, O, test) == [1, 1, 1]
    want = [D.unpack_example_reference(D.pack_example(ex, G, O, test), G, O, test) for ex in exs]
    got = lay.reference_gather([3, 0, 4, 1, 2])
    for name in spec:
        g = got[D.POOL_NAMES[name]]
        for b in range(3):
            assert np.array_equal(u32(g[b]), u32(want[b][name])), (name, b)
        assert not u32(g[3:]).any(), name                                                   # slots 1 and 2 were never named
    # a second replacement of the same slots by other records
    assert lay.replace_reference([0, 3], [exs[3], exs[1]], G, O, test) == [1, 1]
    got = lay.reference_gather([0, 3, 4])
    for name in spec:
        for b, i in enumerate((3, 1, 2)):
            assert np.array_equal(u32(got[D.POOL_NAMES[name]][b]), u32(want[i][name])), (name, b)


def test_capacity_is_all_or_nothing():
    rng = np.random.default_rng(22)
    exs = [_raw_example(rng, G, O) for _ in range(3)]
    count = _present(exs[1], 'gt_flow')
    assert count > 1
    # exact fit: lands
    lay = D.PoolLayout.empty(3, G, O, capacity={'gt_flow': count})
    assert lay.entries['gt_flow']['val_base'].tolist() == [0, count, 2 * count, 3 * count] and lay.entries['gt_flow']['vals'].size == 3 * count
    assert lay.replace_reference([2], [exs[1]], G, O) == [1]
    want = D.unpack_example_reference(D.pack_example(exs[1], G, O), G, O)
    got = lay.reference_gather([2])
    for name in want:
        assert np.array_equal(u32(got[D.POOL_NAMES[name]][0]), u32(want[name])), name
    # one word over: rejected, and ALL keys of that slot (and of every other) stay as they were; the batch neighbour lands
    small = copy.deepcopy(exs[0])
    flow = np.frombuffer(small['gt_flow'], np.float32).copy()
    flow[:] = 0                                                                             # a neighbour that fits any slot
    small['gt_flow'] = flow.tobytes()
    lay = D.PoolLayout.empty(3, G, O, capacity={'gt_flow': count - 1})
    assert lay.replace_reference([1, 0], [small, small], G, O) == [1, 1]                    # something to keep in slot 1
    before = _arrays(lay)
    assert lay.replace_reference([1, 2], [exs[1], small], G, O) == [0, 1]
    _same(before, lay, slot=1)
    _same(before, lay, slot=0)
    got = lay.reference_gather([2])
    want = D.unpack_example_reference(D.pack_example(small, G, O), G, O)
    for name in want:
        assert np.array_equal(u32(got[D.POOL_NAMES[name]][0]), u32(want[name])), name
    with pytest.raises(ValueError, match='capacity'):
        D.PoolLayout.empty(3, G, O, capacity={'ogm': 5})                                    # not a sparse key


def test_out_of_range_and_duplicate_slots():
    rng = np.random.default_rng(23)
    exs = [_raw_example(rng, G, O, True) for _ in range(3)]
    lay = D.PoolLayout.empty(2, G, O, True)
    lay.replace_reference([1], [exs[2]], G, O, True)
    before = _arrays(lay)
    assert lay.replace_reference([-1, 2, 2 ** 31 - 1], exs, G, O, True) == [0, 0, 0]
    _same(before, lay)
    assert lay.replace_reference([-1, 0], exs[:2], G, O, True) == [0, 1]
    _same(before, lay, slot=1)
    with pytest.raises(ValueError, match='duplicate'):
        lay.replace_reference([1, 1], exs[:2], G, O, True)
    with pytest.raises(ValueError):
        lay.replace_reference([0], exs[:2], G, O, True)                                     # one slot, two scenes
    short = dict(exs[0], ogm=exs[0]['ogm'][:-1])
    with pytest.raises(ValueError, match="'ogm'.* scene 0"):
        lay.replace_reference([0], [short], G, O, True)
    with pytest.raises(ValueError):
        D.PoolLayout.empty(0, G, O, True)


def test_add_sparse_capacity_and_its_refusal():
    x = np.zeros((3, 64), np.float32)
    x[0, [0, 9, 31, 32, 63]] = [1.0, 2.0, -0.0, 4.0, 5.0]
    x[2, [1, 40]] = [7.0, -8.0]
    packs = [D.pack_sparse(s) for s in x]
    lay = D.PoolLayout().add_sparse('flow', packs, 64, capacity=6)
    e = lay.entries['flow']
    assert e['val_base'].dtype == np.int64 and e['val_base'].tolist() == [0, 6, 12, 18] and e['vals'].size == 18
    assert e['vals'][:5].tobytes() == packs[0][2].tobytes() and not e['vals'][5:12].any()    # the unused tail of a slot is zero
    assert e['vals'][12:14].tobytes() == packs[2][2].tobytes() and not e['vals'][14:].any()
    assert np.array_equal(u32(lay.reference_gather([2, 0, 1])['flow']), u32(x[[2, 0, 1]]))
    assert D.PoolLayout().add_sparse('flow', packs, 64, capacity=5).entries['flow']['val_base'].tolist() == [0, 5, 10, 15]
    with pytest.raises(ValueError, match=r"'flow'.* scene 0"):
        D.PoolLayout().add_sparse('flow', packs, 64, capacity=4)
    tight = D.PoolLayout().add_sparse('flow', packs, 64)
    assert tight.entries['flow']['val_base'].tolist() == [0, 5, 5, 7] and tight.entries['flow']['vals'].size == 7


@pytest.mark.parametrize('test', [False, True])
def test_tight_layouts_gather_as_before(test):
    """reference_gather slices a slot's values by offs[s][-1]; for a tight layout that is the slice up to val_base[s + 1] it took before."""
    rng = np.random.default_rng(24)
    packed = [D.pack_example(_raw_example(rng, G, O, test), G, O, test) for _ in range(3)]
    lay = D.PoolLayout.from_examples(packed, G, O, test)
    for key, e in lay.entries.items():
        if e['kind'] == 'sparse':
            assert np.array_equal(e['val_base'][:-1] + e['offs'][:, -1], e['val_base'][1:]), key
    got = lay.reference_gather([2, 0, 1, 2])
    for name in D.feature_spec(G, O, test):
        for b, i in enumerate((2, 0, 1, 2)):
            want = D.unpack_example_reference(packed[i], G, O, test)[name]
            assert np.array_equal(u32(got[D.POOL_NAMES[name]][b]), u32(want)), (name, b)
    # and a layout built by empty + replace_reference gathers the same scenes as the tight one
    raw_rng = np.random.default_rng(24)
    raws = [_raw_example(raw_rng, G, O, test) for _ in range(3)]
    slack = D.PoolLayout.empty(3, G, O, test)
    assert slack.replace_reference([0, 1, 2], raws, G, O, test) == [1, 1, 1]
    again = slack.reference_gather([2, 0, 1, 2])
    for key in got:
        assert np.array_equal(u32(got[key]), u32(again[key])), key
