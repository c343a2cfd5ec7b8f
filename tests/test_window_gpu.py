"""The shuffle window on the device (csrc/window.hip through strajnet_amd/data.py): stj_pool_draw / stj_pool_admit_packed / stj_pool_put_vals
against the NumPy statements of test_window.py, PoolWriter.put_packed against decode_batch_packed and PoolLayout.replace_packed_reference,
the threaded ShuffleWindow against ShuffleWindow.reference (every scene carries its source ordinal in the raw key `obs`), WindowFeed in
front of a captured graph, skipped records, a worker's exception, and the refusals of the C ABI.  Every comparison is bitwise; the
protocol is tested by what the batches contain."""
import numpy as np
import pytest
import torch

from strajnet_amd import data as D
from test_window import G, O, SPARSE, SENT, record, present, draw_cases, admit_cases, put_cases, put_vals_reference, u_rows
from test_pack_gpu import dev_i32, _device_equals_layout

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


def _abi():
    from strajnet_amd.ops import _p, _st, call
    return _p, _st, call


def dev_u32(v):
    return torch.from_numpy(np.asarray(v, np.uint64).astype(np.uint32).view(np.int32)).cuda()


def dev_i64(v):
    return torch.tensor([int(x) for x in v], dtype=torch.int64).cuda()


# ------------------------------------------------------------------------------------------------------------------ kernels vs NumPy
def test_draw_kernel_matches_numpy(lib_built):
    """The 16 consecutive draws of 2 out of 8 (tail wraps twice; words 0 and 0xffffffff planted) carry perm from one launch to the next;
    the garbage-perm cases start from their own."""
    _p, _st, call = _abi()
    carried = None
    for t, (N, tail, n_live, perm, u) in enumerate(draw_cases()):
        d_perm = carried if t and t < 16 else torch.from_numpy(perm.copy()).cuda()
        idx = torch.full((len(u),), -77, dtype=torch.int32, device='cuda')
        d_u = dev_u32(u)
        call('stj_pool_draw', _p(d_perm), N, tail, n_live, _p(d_u), _p(idx), len(u), _st())
        want = D.ShuffleWindow.draw_reference(perm, tail, n_live, u)
        assert d_perm.cpu().numpy().tolist() == perm.tolist(), (t, 'perm')
        assert idx.cpu().numpy().tolist() == want.tolist(), (t, 'idx')
        carried = d_perm


def test_admit_and_put_vals_kernels_match_numpy(lib_built):
    _p, _st, call = _abi()
    for c, (nblk, n, N, first, ok, slots, rows, src_base, val_base, ok_want) in enumerate(admit_cases()):
        d_ok, d_offs, d_sb, d_vb, d_sl = dev_i32(ok), dev_u32(sum(rows, [])), dev_i64(src_base), dev_i64(val_base), dev_i32(slots)
        call('stj_pool_admit_packed', _p(d_offs), nblk, n, _p(d_sb), _p(d_vb), _p(d_sl), N, _p(d_ok), len(rows), first, _st())
        assert d_ok.cpu().tolist() == ok_want, (c, 'admit')
    for c, (N, n_vals, ok, slots, sb, vb, vals_src, shift) in enumerate(put_cases()):
        vals = torch.full((n_vals,), SENT - (1 << 32), dtype=torch.int32, device='cuda')          # exact size, the sentinel everywhere
        src = torch.zeros(vals_src.size + shift, dtype=torch.int32, device='cuda')
        src[shift:] = dev_u32(vals_src)
        d_src, d_sb, d_ok, d_sl, d_vb = src[shift:], dev_i64(sb), dev_i32(ok), dev_i32(slots), dev_i64(vb)
        call('stj_pool_put_vals', _p(d_src), _p(d_sb), _p(d_ok), _p(d_sl), N, _p(d_vb), _p(vals), n_vals, len(ok), _st())
        want = put_vals_reference(ok, slots, sb, vb, vals_src, n_vals, N)
        got = vals.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), (c, np.flatnonzero(got != want)[:8])


# ------------------------------------------------------------------------------------------------------------------ put_packed
def _records(seed, count, dens=0.05, first_ordinal=0):
    rng = np.random.default_rng(seed)
    return [record(rng, dens, ordinal=first_ordinal + i) for i in range(count)]


def _gather_equals_packed(pool, slots, packed):
    """The pool's gather of `slots` equals decode_batch_packed of the records and, scene by scene, unpack_example_reference."""
    got = pool.gather(slots)
    want = D.decode_batch_packed(packed, 'cuda', G, O)
    assert set(got) == {D.POOL_NAMES[name] for name in want}
    for name in want:
        g = got[D.POOL_NAMES[name]]
        assert g.shape == want[name].shape and torch.equal(g.view(torch.int32), want[name].view(torch.int32)), name
    for b, ex in enumerate(packed):
        ref = D.unpack_example_reference(ex, G, O)
        for name, a in ref.items():
            assert np.array_equal(got[D.POOL_NAMES[name]][b].cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), (name, b)


def test_put_packed_round_trip(lib_built):
    raws = _records(51, 5)
    packed = [D.pack_example(e, G, O) for e in raws]
    pool = D.ResidentPool.empty(5, 'cuda', G, O)
    lay = D.PoolLayout.empty(5, G, O)
    w = pool.writer(3)
    for slots, batch in (([3, 0, 4], packed[:3]), ([4, 3, 1], [packed[3], packed[4], packed[0]])):
        ok = w.put_packed(slots, batch)
        assert ok is w.ok and ok.cpu().tolist() == [1, 1, 1]
        assert lay.replace_packed_reference(slots, batch, G, O) == [1, 1, 1]
        _gather_equals_packed(pool, slots, batch)
        _device_equals_layout(pool, lay)
    # the same pool filled from the raw records by put() holds the same bytes
    twin = D.ResidentPool.empty(5, 'cuda', G, O)
    tw = twin.writer(3)
    tw.put([3, 0, 4], raws[:3]); tw.put([4, 3, 1], [raws[3], raws[4], raws[0]])
    _device_equals_layout(twin, lay)
    assert all(not t.view(torch.int32).any() for t in pool.gather([2]).values())         # slot 2 was never named
    # malformed records are refused on the host, before anything is launched
    offs = np.frombuffer(packed[1]['gt_flow/offs'], '<u4').copy()
    offs[0] = 1
    for bad in (dict(packed[1], **{'gt_flow/offs': offs.tobytes()}), dict(packed[1], **{'vec_flow/vals': packed[1]['vec_flow/vals'][:-4]}),
                dict(packed[1], **{'ogm/bits': packed[1]['ogm/bits'][:-4]})):
        with pytest.raises(ValueError, match='scene 1'):
            w.put_packed([0, 1, 2], [packed[0], bad, packed[2]])
    with pytest.raises(ValueError):
        w.put_packed([0, 1], packed[:2])
    _device_equals_layout(pool, lay)


def test_put_packed_is_all_or_nothing_and_skips_slots_outside(lib_built):
    raws = _records(52, 3)
    counts = [present(e, 'gt_flow') for e in raws]
    big = int(np.argmax(counts))
    assert counts[big] - 1 >= max(c for b, c in enumerate(counts) if b != big), counts
    packed = [D.pack_example(e, G, O) for e in raws]
    for cap, landed in ((counts[big] - 1, False), (counts[big], True)):
        lay = D.PoolLayout.empty(4, G, O, capacity={'gt_flow': cap})
        pool = D.ResidentPool(lay, 'cuda')
        fill = [packed[(big + 1) % 3]] * 4
        assert pool.writer(4).put_packed([0, 1, 2, 3], fill).cpu().tolist() == [1, 1, 1, 1]
        lay.replace_packed_reference([0, 1, 2, 3], fill, G, O)
        want_ok = [int(landed or b != big) for b in range(3)]
        assert pool.writer(3).put_packed([2, 0, 3], packed).cpu().tolist() == want_ok, (cap, counts)
        assert lay.replace_packed_reference([2, 0, 3], packed, G, O) == want_ok
        _device_equals_layout(pool, lay)                             # the rejected scene changed no key of its slot, the neighbours landed
    N = 3
    pool = D.ResidentPool.empty(N, 'cuda', G, O)
    lay = D.PoolLayout.empty(N, G, O)
    w = pool.writer(3)
    assert w.put_packed(dev_i32([-1, N, INT_MAX]), packed).cpu().tolist() == [0, 0, 0]   # a device tensor is trusted: skipped, never clamped
    _device_equals_layout(pool, lay)
    assert w.put_packed(dev_i32([-1, 1, N]), packed).cpu().tolist() == [0, 1, 0]
    lay.replace_packed_reference([-1, 1, N], packed, G, O)
    _device_equals_layout(pool, lay)
    for bad in ([-1, 0, 1], [0, 1, N], [0, 1, 1]):
        with pytest.raises(ValueError):
            w.put_packed(bad, packed)


def test_commit_packed_captures_and_replays(lib_built):
    packed = [D.pack_example(e, G, O) for e in _records(53, 6)]
    pool = D.ResidentPool.empty(4, 'cuda', G, O)
    pool.wait()
    w = pool.writer(2)
    check = lambda exs: [w.packed_stage().check(ex, b) for b, ex in enumerate(exs)]
    w.stage_packed(check(packed[:2]))
    w.slots.copy_(dev_i32([0, 1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        w.commit_packed()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.commit_packed()
    held = {0: packed[0], 1: packed[1]}
    for slots, batch, want_ok in (([3, 1], packed[2:4], [1, 1]), ([0, 7], packed[4:6], [1, 0]), ([2, 3], [packed[1], packed[0]], [1, 1])):
        w.stage_packed(check(batch))                                 # between replays only the contents of the staging and of writer.slots change
        w.slots.copy_(dev_i32(slots))
        g.replay()
        torch.cuda.synchronize()
        assert w.ok.cpu().tolist() == want_ok, slots
        held.update({s: ex for s, ex, k in zip(slots, batch, want_ok) if k})
        _gather_equals_packed(pool, sorted(held), [held[s] for s in sorted(held)])


# ------------------------------------------------------------------------------------------------------------------ the threaded window
N_W, B_W, K_W = 8, 2, 2
_SOURCE = {}


def source(M=41):
    """M raw records carrying their ordinal, their packed form and what every key decodes to; built once, never changed."""
    if 'raw' not in _SOURCE:
        _SOURCE['raw'] = _records(60, M)
        _SOURCE['packed'] = [D.pack_example(e, G, O) for e in _SOURCE['raw']]
        _SOURCE['decoded'] = [D.unpack_example_reference(p, G, O) for p in _SOURCE['packed']]
    return _SOURCE


def run_window(packed, M, drop_last, rows, records=None, capacity=None, lag=K_W):
    """-> (the batches as lists of ordinals read back from the gathered `obs`, the window after close()).  Every gathered scene is
    compared with its record, key by key, bit for bit."""
    src = source()
    recs = (src['packed'] if packed else src['raw'])[:M] if records is None else records
    pool = D.ResidentPool.empty(N_W, 'cuda', G, O, capacity=capacity)
    win = pool.window(B_W, iter(recs), packed=packed, lag=lag, drop_last=drop_last)
    assert isinstance(win, D.ShuffleWindow)
    win.start()
    got = []
    try:
        for t in range(len(rows) + 1):
            try:
                idx = win.next_batch(rows[t] if t < len(rows) else None)
            except StopIteration:
                break
            assert idx.dtype == torch.int32 and idx.is_cuda
            batch = pool.gather(idx)
            win.release()
            ords = batch['obs'][:, 0, 0, 0].cpu().tolist()
            assert all(float(o).is_integer() for o in ords)
            got.append([int(o) for o in ords])
            for b, o in enumerate(got[-1]):
                for name, a in src['decoded'][o].items():
                    have = batch[D.POOL_NAMES[name]][b].cpu().numpy().view(np.uint32)
                    assert np.array_equal(have, np.ascontiguousarray(a).view(np.uint32)), (t, b, o, name)
    finally:
        win.close()
    return got, win


@pytest.mark.parametrize('packed,M,drop_last', [(True, 40, True), (False, 40, True), (True, 37, False), (False, 37, True)])
def test_window_batches_are_the_reference_sequence(lib_built, packed, M, drop_last):
    rows = u_rows(61, M, B_W)
    rows[0], rows[1] = [0, 0xffffffff], [0xffffffff, 0]
    want = D.ShuffleWindow.reference(N_W, B_W, K_W, rows, M, drop_last)
    runs = [run_window(packed, M, drop_last, rows) for _ in range(2)]                   # twice: the sequence is a function of its inputs
    for got, win in runs:
        assert got == want
        seen = sorted(o for b in got for o in b)
        assert len(set(seen)) == len(seen) == (M - M % B_W if drop_last else M) and set(seen) <= set(range(M))      # every scene once
        assert win.consumed == len(seen) and win.steps == len(got) and 0 <= win.stalls <= win.steps
        assert win.skipped == [] and int(win.bad.item()) == 0
        assert win.n_live == (M % B_W if drop_last else 0)


def test_window_feed_in_front_of_a_captured_graph(lib_built):
    src = source()
    M = 24
    rows = u_rows(62, M, B_W)
    want = D.ShuffleWindow.reference(N_W, B_W, K_W, rows, M)
    pool = D.ResidentPool.empty(N_W, 'cuda', G, O)
    static = {k: torch.zeros((B_W,) + e['shape'], device='cuda') for k, e in pool.layout.entries.items()}
    feed = D.WindowFeed(static, pool.window(B_W, iter(src['packed'][:M]), lag=K_W))
    feed.start()
    out = torch.zeros(B_W + 1, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out[:B_W].copy_(static['obs'][:, 0, 0, 0])
        out[B_W:].copy_(static['ogm'].sum().reshape(1))
    got = []
    for t in range(len(want)):
        feed.land(rows[t])
        g.replay()
        o = out.cpu()
        got.append([int(x) for x in o[:B_W].tolist()])
        assert float(o[B_W]) == sum(float(src['decoded'][i]['ogm'].sum()) for i in got[-1]), t
    assert got == want
    with pytest.raises(StopIteration):
        feed.land()
    feed.wait_uploaded()
    feed.close()
    assert feed.window.consumed == M and feed.idx is feed.window.idx


@pytest.mark.parametrize('packed', [True, False])
def test_a_record_over_capacity_is_skipped_and_logged(lib_built, packed):
    src = source()
    M = 16
    cap = {key: max(present(e, name) for e in src['raw'][:M]) for name, key in SPARSE.items()}
    dense = record(np.random.default_rng(63), 1.0, ordinal=1000)                          # every flow word present: no slot holds it
    broken = dict(src['packed'][0], **{'gt_flow/offs': src['packed'][0]['gt_flow/offs'][:-4]}) if packed else dict(src['raw'][0], ogm=b'\x00')
    recs = list((src['packed'] if packed else src['raw'])[:M])
    recs.insert(11, D.pack_example(dense, G, O) if packed else dense)
    recs.insert(3, broken)
    rows = u_rows(64, M, B_W)
    got, win = run_window(packed, M, True, rows, records=recs, capacity=cap)
    assert got == D.ShuffleWindow.reference(N_W, B_W, K_W, rows, M)                        # the next record took the place of each skipped one
    assert [o for o, _ in win.skipped] == [3, 12] and 'value words' in win.skipped[1][1] and win.skipped[0][1]
    assert win.consumed == M and int(win.bad.item()) == 0


def test_a_worker_exception_reaches_land(lib_built):
    src = source()

    def failing():
        yield from src['packed'][:12]
        raise RuntimeError('boom: the source broke')
    pool = D.ResidentPool.empty(N_W, 'cuda', G, O)
    static = {k: torch.zeros((B_W,) + e['shape'], device='cuda') for k, e in pool.layout.entries.items()}
    feed = D.WindowFeed(static, D.ShuffleWindow(pool, B_W, failing(), lag=K_W))
    feed.start()
    with pytest.raises(RuntimeError, match='boom'):
        for _ in range(12):
            feed.land()
    feed.close()                                                       # the error was delivered once; close() joins the worker
    assert not feed.window._thread.is_alive()
    with pytest.raises(ValueError):
        D.ShuffleWindow(pool, 3, iter([]))                             # N % B
    with pytest.raises(ValueError):
        D.ShuffleWindow(pool, 2, iter([]), lag=4)                      # N < (lag + 1) B


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_refusals_at_the_abi(lib_built):
    from ctypes import c_void_p as vp
    from strajnet_amd._lib import StjError
    _p, _st, call = _abi()
    perm = torch.arange(8, dtype=torch.int32, device='cuda')
    u = torch.zeros(8, dtype=torch.int32, device='cuda')
    idx = torch.full((8,), -77, dtype=torch.int32, device='cuda')
    w = torch.full((64,), -77, dtype=torch.int32, device='cuda')
    vb = torch.zeros(4, dtype=torch.int64, device='cuda')
    ok, sl = torch.ones(4, dtype=torch.int32, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda')
    off = lambda t, k: vp(t.data_ptr() + k)
    draw = lambda N=8, tail=0, n_live=8, B=2, perm=perm, u=u, idx=idx: call('stj_pool_draw', _p(perm), N, tail, n_live, _p(u), _p(idx), B, _st())
    admit = lambda nblk=1, n=64, N=1, B=1, offs=w, sb=vb, vb=vb, sl=sl, ok=ok: call('stj_pool_admit_packed', _p(offs), nblk, n, _p(sb), _p(vb), _p(sl), N,
                                                                                 _p(ok), B, 1, _st())
    put = lambda n_vals=64, N=1, B=1, src=w, sb=vb, vb=vb, sl=sl, ok=ok, vals=w: call('stj_pool_put_vals', _p(src), _p(sb), _p(ok), _p(sl), N, _p(vb),
                                                                                      _p(vals), n_vals, B, _st())
    for kw in (dict(n_live=1), dict(B=-1), dict(N=0), dict(tail=-1), dict(tail=8), dict(perm=None), dict(u=None), dict(idx=None)):
        with pytest.raises(StjError, match='-1'):
            draw(**kw)
    for kw in (dict(perm=off(perm, 2)), dict(u=off(u, 1)), dict(idx=off(idx, 2))):
        with pytest.raises(StjError, match='-3'):
            draw(**kw)
    draw(B=0)
    draw(B=0, n_live=0)
    for kw in (dict(B=-1), dict(N=-1), dict(nblk=-1), dict(n=-32), dict(offs=None), dict(sb=None), dict(vb=None), dict(sl=None), dict(ok=None)):
        with pytest.raises(StjError, match='-1'):
            admit(**kw)
    for kw in (dict(n=40), dict(n=1 << 32, nblk=1 << 19), dict(nblk=2), dict(offs=off(w, 2)), dict(sb=off(vb, 4)), dict(vb=off(vb, 4)), dict(sl=off(sl, 2)),
               dict(ok=off(ok, 2))):
        with pytest.raises(StjError, match='-3'):
            admit(**kw)
    admit(B=0)
    for kw in (dict(B=-1), dict(N=-1), dict(n_vals=-1), dict(src=None), dict(sb=None), dict(vb=None), dict(sl=None), dict(ok=None), dict(vals=None)):
        with pytest.raises(StjError, match='-1'):
            put(**kw)
    for kw in (dict(src=off(w, 2)), dict(vals=off(w, 1)), dict(sb=off(vb, 4)), dict(vb=off(vb, 4)), dict(sl=off(sl, 2)), dict(ok=off(ok, 2)),
               dict(n_vals=1 << 45), dict(B=1 << 16)):
        with pytest.raises(StjError, match='-3'):
            put(**kw)
    put(B=0)
    put(n_vals=0)
    torch.cuda.synchronize()
    assert (w == -77).all() and (idx == -77).all() and (ok == 1).all() and perm.cpu().tolist() == list(range(8))      # nothing was written on a refusal
