"""The shuffle window over a resident pool, host side (strajnet_amd/data.py): PoolLayout.replace_packed_reference against replace_reference
through pack_example, ShuffleWindow.reference (every scene exactly once, the live count of every draw, FIFO order for u = 0), and the
host build of csrc/window.h -- the draw loop, the admit checks and the bounds of the value copy -- against the NumPy statements.  All
comparisons are bitwise."""
import os
import subprocess

import numpy as np
import pytest

from strajnet_amd import data as D
from test_packed import _raw_example
from test_deflate_dyn import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, O = 64, 32
SPARSE = {'vec_flow': 'flow', 'gt_flow': 'gt_flow', 'origin_flow': 'origin_flow'}
SENT = 0xdeadbeef


def record(rng, dens, test=False, ordinal=None):
    """_raw_example with the flow planes at density `dens` (0: all-zero planes, 1: every word present); ordinal: written into the first
    element of the raw key `actors`, so that a gathered scene says which source scene it is."""
    ex = _raw_example(rng, G, O, test)
    for name in SPARSE:
        if name in ex:
            n = len(ex[name]) // 4
            ex[name] = (np.where(rng.random(n) < dens, rng.normal(size=n) + 8.0, 0.0).astype(np.float32)).tobytes()
    if ordinal is not None:
        a = np.frombuffer(ex['actors'], np.float64).copy()
        a[0] = float(ordinal)
        ex['actors'] = a.tobytes()
    return ex


def present(ex, name, test=False):
    dt, shape, crop, _ = D.feature_spec(G, O, test)[name]
    return int(np.count_nonzero(D._decoded(ex[name], dt, shape, crop)))


def layout_bytes(lay):
    return {(key, part): np.ascontiguousarray(a).tobytes() for key in lay.entries for part, a in lay.arrays(key).items()}


def capacities(exs, which):
    """dense: None; exact: scene 0 just fits every sparse key; short: one word less for gt_flow (an all-zero plane has no word to be
    short of: density 0 has no such case)."""
    if which == 'dense':
        return None
    cap = {key: present(exs[0], name) for name, key in SPARSE.items()}
    if which == 'short':
        cap['gt_flow'] -= 1
    return cap


@pytest.mark.parametrize('dens,which', [(d, w) for d in (0.0, 0.02, 1.0) for w in ('dense', 'exact', 'short') if (d, w) != (0.0, 'short')])
@pytest.mark.parametrize('N,B', [(1, 1), (1, 3), (5, 1), (5, 3)])
def test_replace_packed_reference_equals_replace_reference(N, B, dens, which):
    rng = np.random.default_rng(1000 * N + 10 * B + int(dens * 100))
    exs = [record(rng, dens) for _ in range(B)]
    cap = capacities(exs, which)
    keep = record(rng, 0.0)                                                          # something to keep in every slot: fits any capacity
    lays = [D.PoolLayout.empty(N, G, O, capacity=cap) for _ in range(2)]
    for lay in lays:
        assert lay.replace_reference(list(range(N)), [keep] * N, G, O) == [1] * N
    slot_sets = [[N * 3 // 5], [-1], [N]] if B == 1 else [[4, 0, 2] if N == 5 else [N, 0, -1], [-1, N, N - 1]]
    for slots in slot_sets:
        ok_raw = lays[0].replace_reference(slots, exs, G, O)
        ok_packed = lays[1].replace_packed_reference(slots, [D.pack_example(e, G, O) for e in exs], G, O)
        assert ok_raw == ok_packed, (slots, ok_raw, ok_packed)
        assert layout_bytes(lays[0]) == layout_bytes(lays[1]), slots
        fits = [all(present(e, name) <= (cap or {}).get(key, 1 << 40) for name, key in SPARSE.items()) for e in exs]
        assert ok_raw == [int(0 <= s < N and f) for s, f in zip(slots, fits)], (slots, which)


def test_malformed_packed_records_raise():
    rng = np.random.default_rng(5)
    packed = [D.pack_example(record(rng, 0.02), G, O) for _ in range(2)]
    lay = D.PoolLayout.empty(3, G, O)
    before = layout_bytes(lay)
    offs = np.frombuffer(packed[1]['gt_flow/offs'], '<u4').copy()
    offs[1] = offs[2] + 1                                                             # decreasing
    with pytest.raises(ValueError, match=r"'gt_flow'.* scene 1"):
        lay.replace_packed_reference([0, 1], [packed[0], dict(packed[1], **{'gt_flow/offs': offs.tobytes()})], G, O)
    with pytest.raises(ValueError, match=r"'flow'.* scene 0"):
        lay.replace_packed_reference([2], [dict(packed[0], **{'vec_flow/vals': packed[0]['vec_flow/vals'][:-4]})], G, O)
    with pytest.raises(ValueError, match=r"'ogm'.* scene 0"):
        lay.replace_packed_reference([2], [{k: v for k, v in packed[0].items() if k != 'ogm/bits'}], G, O)
    with pytest.raises(ValueError, match='duplicate'):
        lay.replace_packed_reference([1, 1], packed, G, O)
    assert layout_bytes(lay) == before                                                # a refused call changed nothing


def u_rows(seed, steps, B):
    return np.random.default_rng(seed).integers(0, 1 << 32, (steps, B), dtype=np.uint64)


@pytest.mark.parametrize('N,B,K', [(8, 2, 1), (8, 2, 3), (12, 4, 2)])
def test_reference_visits_every_scene_once(N, B, K):
    for M in (N, 3 * N, 3 * N + B):
        live = []
        got = D.ShuffleWindow.reference(N, B, K, u_rows(N + M, M, B), M, live=live)
        assert all(len(b) == B for b in got)
        assert sorted(x for b in got for x in b) == list(range(M)), (M, got)
        # the live count every draw saw: nothing is admitted before step K; from then on one group per step, a full one while the
        # source lasts -- such a draw finds N - (K - 1) B live scenes and leaves N - K B --, and the drain after
        refills = (M - N) // B                                                        # groups that the source still fills
        assert len(live) == M // B
        for t, n in enumerate(live):
            assert n == N - t * B + min(max(t - K + 1, 0), refills) * B, (M, t, live)
        for t in range(K, min(refills + K, len(live))):
            assert live[t] - B == N - K * B, (M, t, live)
    M = 3 * N + 1
    got = D.ShuffleWindow.reference(N, B, K, u_rows(7, M, B), M, drop_last=True)
    seen = [x for b in got for x in b]
    assert len(set(seen)) == len(seen) and M - (B - 1) <= len(seen) <= M and all(len(b) == B for b in got)
    got = D.ShuffleWindow.reference(N, B, K, u_rows(7, M, B), M, drop_last=False)
    assert sorted(x for b in got for x in b) == list(range(M)) and [len(b) for b in got[:-1]] == [B] * (len(got) - 1)
    assert D.ShuffleWindow.reference(N, B, K, [], 0) == []
    for bad in ((8, 3, 1), (8, 2, 4), (8, 2, 0)):
        with pytest.raises(ValueError):
            D.ShuffleWindow.reference(*bad, [], 8)


def test_reference_with_zero_words_is_fifo():
    zero = [[0, 0]] * 16
    assert D.ShuffleWindow.reference(8, 2, 1, zero, 12) == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]
    assert D.ShuffleWindow.reference(8, 2, 1, zero, 5, drop_last=False) == [[0, 1], [2, 3], [4]]
    assert D.ShuffleWindow.reference(8, 2, 1, zero, 5) == [[0, 1], [2, 3]]
    # the largest word takes the last live slot: step 0 swaps slot 0 with slot 7
    assert D.ShuffleWindow.reference(8, 2, 1, [[0xffffffff, 0]] + zero, 8)[0] == [7, 1]


# ------------------------------------------------------------------------------------------------ csrc/window.h compiled for the host
_HOST_PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "%s"
template <typename T> static T* take(long long n, const char* fmt) {     /* an exact-size heap array read from stdin */
  T* p = (T*)malloc((size_t)(n > 0 ? n : 0) * sizeof(T) + (n > 0 ? 0 : 1));
  for (long long i = 0; i < n; ++i) if (scanf(fmt, &p[i]) != 1) exit(2);
  return p;
}
int main() {
  char kind;
  while (scanf(" %%c", &kind) == 1) {
    if (kind == 'D') {                                   /* one draw */
      int N, tail, n_live, B;
      if (scanf("%%d %%d %%d %%d", &N, &tail, &n_live, &B) != 4) return 3;
      int* perm = take<int>(N, "%%d");
      uint32_t* u = take<uint32_t>(B, "%%u");
      int* idx = (int*)malloc(sizeof(int) * (B ? B : 1));
      win_draw(perm, N, tail, n_live, u, idx, B);
      printf("P");
      for (int i = 0; i < N; ++i) printf(" %%d", perm[i]);
      printf("\nI");
      for (int i = 0; i < B; ++i) printf(" %%d", idx[i]);
      printf("\n");
      free(perm); free(u); free(idx);
    } else if (kind == 'A') {                            /* one admit launch: a workgroup per scene, a thread per block and round */
      int B, nblk, N, first;
      long long n;
      if (scanf("%%d %%d %%lld %%d %%d", &B, &nblk, &n, &N, &first) != 5) return 3;
      int* ok = take<int>(B, "%%d");
      int* slots = take<int>(B, "%%d");
      uint32_t* offs = take<uint32_t>((long long)B * (nblk + 1), "%%u");
      long long* src_base = take<long long>(B + 1, "%%lld");
      long long* val_base = take<long long>(N + 1, "%%lld");
      printf("K");
      for (int b = 0; b < B; ++b) {
        const uint32_t* row = offs + (size_t)b * (nblk + 1);
        bool bad = false;
        for (uint32_t tid = 0; tid < WIN_NT; ++tid)
          for (uint32_t k = tid; k < (uint32_t)nblk; k += WIN_NT) bad |= !win_block_ok(row, k, nblk, n);
        ok[b] = win_admit_decide(first, first ? 0 : ok[b], slots[b], N, !bad, row, nblk, src_base, b, val_base);
        printf(" %%d", ok[b]);
      }
      printf("\n");
      free(ok); free(slots); free(offs); free(src_base); free(val_base);
    } else if (kind == 'V') {                            /* one put-vals launch: grid (ceil(n_vals / WIN_PIECE), B) x WIN_NT threads */
      int B, N, shift;
      long long n_vals, n_src;
      if (scanf("%%d %%d %%lld %%lld %%d", &B, &N, &n_vals, &n_src, &shift) != 5) return 3;
      int* ok = take<int>(B, "%%d");
      int* slots = take<int>(B, "%%d");
      long long* src_base = take<long long>(B + 1, "%%lld");
      long long* val_base = take<long long>(N + 1, "%%lld");
      /* `shift` words in front of vals_src move it off the 16-byte grid: the word path instead of the vector path */
      uint32_t* src_all = (uint32_t*)aligned_alloc(16, (size_t)((n_src + shift) * 4 + 15) / 16 * 16 + 16);
      uint32_t* vals_src = src_all + shift;
      for (long long i = 0; i < n_src; ++i) if (scanf("%%u", &vals_src[i]) != 1) return 2;
      uint32_t* vals = (uint32_t*)aligned_alloc(16, (size_t)(n_vals * 4 + 15) / 16 * 16 + 16);
      for (long long i = 0; i < n_vals; ++i) vals[i] = 0xdeadbeefu;
      const long long pieces = (n_vals + WIN_PIECE - 1) / WIN_PIECE;
      for (int b = 0; b < B; ++b)
        for (long long piece = 0; piece < pieces; ++piece) {
          const int s = slots[b];
          if (ok[b] == 0 || s < 0 || s >= N) continue;
          win_span sp;
          if (!win_put_span(src_base, val_base, (uint64_t)n_vals, b, (uint32_t)s, (uint64_t)piece, &sp)) continue;
          if (sp.dst + sp.cnt > (uint64_t)n_vals || sp.src + sp.cnt > (uint64_t)n_src) return 7;      /* a span outside its buffer */
          for (uint32_t tid = 0; tid < WIN_NT; ++tid) win_put_thread(vals_src, vals, sp, tid);
        }
      printf("V");
      for (long long i = 0; i < n_vals; ++i) printf(" %%u", vals[i]);
      printf("\n");
      free(ok); free(slots); free(src_base); free(val_base); free(src_all); free(vals);
    } else return 4;
  }
  return 0;
}
'''


def admit_reference(ok, slots, rows, src_base, val_base, n, N, first):
    """stj_pool_admit_packed in NumPy: check_sparse's rules on the offs row, the staged count and the capacity rule."""
    out = []
    for b, (s, row) in enumerate(zip(slots, rows)):
        v = 0 <= s < N and (first or ok[b] != 0)
        try:
            D.check_sparse(np.zeros(n // 32, np.uint32), np.asarray(row, np.uint32), np.zeros(int(row[-1]), np.uint32), n)
        except ValueError:
            v = False
        v = v and int(src_base[b + 1]) - int(src_base[b]) == int(row[-1])
        v = v and 0 <= int(row[-1]) <= int(val_base[s + 1]) - int(val_base[s])
        out.append(int(v))
    return out


def put_vals_reference(ok, slots, src_base, val_base, vals_src, n_vals, N):
    """stj_pool_put_vals in NumPy: every store inside [val_base[s], min(val_base[s + 1], n_vals))."""
    vals = np.full(n_vals, SENT, np.uint32)
    for b, s in enumerate(slots):
        if not ok[b] or not 0 <= s < N:
            continue
        slo, shi, lo, hi = int(src_base[b]), int(src_base[b + 1]), int(val_base[s]), int(val_base[s + 1])
        end = min(hi, n_vals)
        if slo < 0 or shi < slo or lo < 0 or hi < lo or lo >= end:
            continue
        cnt = min(shi - slo, end - lo)
        vals[lo:lo + cnt] = vals_src[slo:slo + cnt]
    return vals


def draw_cases():
    """[(N, tail, n_live, perm before, u)]: 16 consecutive draws of 2 out of 8, so that tail wraps twice, with planted words 0 and
    0xffffffff; then garbage perm values and a live count beyond N; N = 1."""
    rng = np.random.default_rng(17)
    cases = []
    N, B = 8, 2
    perm, tail = np.arange(N, dtype=np.int32), 0
    planted = [[0, 0], [0xffffffff, 0xffffffff], [0, 0xffffffff], [0x80000000, 1]]
    for t in range(16):
        u = planted[t] if t < len(planted) else rng.integers(0, 1 << 32, B, dtype=np.uint64).tolist()
        n_live = N - 2 * (t % 3)                                                      # 8, 6, 4 live slots
        cases.append((N, tail, n_live, perm.copy(), u))
        D.ShuffleWindow.draw_reference(perm, tail, n_live, u)
        tail = (tail + B) % N
    garbage = np.array([-5, 2 ** 31 - 1, 3, -2 ** 31, 8, 0, 7, 100], np.int32)
    for tail, n_live, u in ((6, 8, [0xffffffff, 0x7fffffff, 5]), (7, 3, [0, 0, 0]), (0, 2 ** 31 - 1, [0xffffffff, 0xffffffff, 0xffffffff])):
        cases.append((N, tail, n_live, garbage.copy(), u))
    cases.append((1, 0, 1, np.zeros(1, np.int32), [0xffffffff]))
    return cases


def admit_cases():
    """[(nblk, n, N, first, ok before, slots, offs rows, src_base, val_base, ok wanted)]"""
    cases = []
    # n = 2 blocks + 32 elements (a partial last block), N = 3 slots of capacity 40
    n, nblk, N = 2 * 8192 + 32, 3, 3
    val_base = [0, 40, 80, 120]
    good = [0, 10, 30, 40]
    rows = {'fits exactly': good, 'one word over': [0, 10, 30, 41], 'starts at 1': [1, 10, 30, 40], 'decreases': [0, 30, 10, 40],
            'last block over its 32 elements': [0, 0, 0, 33], 'a block over 8192': [0, 8193, 8193, 8193], 'empty': [0, 0, 0, 0]}
    for first in (1, 0):
        slots = [(i % 5) - 1 for i in range(len(rows))]                               # -1, 0, 1, 2, 3, -1, 0
        slots[0], slots[1] = 1, 2
        ok = [int(i % 2 == 0) for i in range(len(rows))]
        r = list(rows.values())
        src_base = np.concatenate([[0], np.cumsum([x[-1] for x in r])]).tolist()
        cases.append((nblk, n, N, first, ok, slots, r, src_base, val_base, admit_reference(ok, slots, r, src_base, val_base, n, N, first)))
    assert cases[0][-1] == [1, 0, 0, 0, 0, 0, 1] and cases[1][-1] == [1, 0, 0, 0, 0, 0, 1]
    # a staged count that disagrees with the row; a val_base that decreases or leaves too little room
    cases.append((nblk, n, N, 1, [0, 0], [0, 1], [good, good], [0, 39, 79], val_base, [0, 1]))
    cases.append((nblk, n, N, 1, [0, 0], [0, 1], [good, good], [0, 40, 80], [0, -5, 30, 60], [0, 0]))
    # 300 blocks: more than one round of 256 threads; the planted fault sits in block 280
    row = (np.arange(301) * 3).tolist()
    for fault in (False, True):
        r2 = list(row)
        if fault:
            r2[281] = r2[280] - 1
        cases.append((300, 300 * 8192, 1, 1, [1], [0], [r2], [0, r2[-1]], [0, 1000], [int(not fault)]))
    return cases


def put_cases():
    """[(N, n_vals, ok, slots, src_base, val_base, vals_src, shift)]: N = 4 slots in vals of 20000 words, scene 1 spans two pieces; shift
    moves vals_src one word off the 16-byte grid (the word path instead of the vector path)."""
    rng = np.random.default_rng(18)
    N, n_vals = 4, 20000
    totals = [7, 8192 + 5, 0, 33]
    src_base = np.concatenate([[0], np.cumsum(totals)]).tolist()
    vals_src = rng.integers(1, 1 << 32, src_base[-1], dtype=np.uint64).astype(np.uint32)
    cases = [
        ([1, 1, 1, 1], [3, 1, 0, 2], [0, 100, 9000, 9100, 20000], src_base),          # everything lands; slot 1 holds 8900 words
        ([1, 1, 1, 1], [3, 1, 0, 2], [0, 16, 8208, 8240, 8248], src_base),            # slot 1 has room for 8192 of 8197 words, slot 2 for 32 of 33
        ([1, 0, 1, 1], [0, 1, -1, 4], [0, 100, 9000, 9100, 20000], src_base),         # ok == 0 and slots outside: skipped
        ([1, 1, 1, 1], [0, 1, 2, 3], [0, 100, 50, -7, 30000], src_base),              # val_base decreasing, negative, beyond n_vals
        ([1, 1, 1, 1], [3, 1, 0, 2], [19990, 19995, 25000, 2 ** 40, 2 ** 62], src_base),      # slots that leave vals: clipped at n_vals
        ([1, 1, 1, 1], [3, 1, 0, 2], [0, 100, 9000, 9100, 20000], [0, -3, 8000, 7000, 7033]),  # src_base negative / decreasing: skipped
    ]
    res = [(N, n_vals, ok, slots, sb, vb, vals_src, shift) for shift in (0, 1) for ok, slots, vb, sb in cases]
    # a slot and a source that start 4 and 8 words in: the vector path with a tail of 3 words
    res.append((1, 64, [1], [0], [8, 27], [4, 60], vals_src, 0))
    return res


def window_cases():
    """(input lines, expected output lines) for the host program."""
    lines, want = [], []
    fmt = lambda a: ' '.join(str(int(x)) for x in a)
    for N, tail, n_live, perm, u in draw_cases():
        lines.append(f'D {N} {tail} {n_live} {len(u)} {fmt(perm)} {fmt(u)}')
        idx = D.ShuffleWindow.draw_reference(perm, tail, n_live, u)
        assert ((idx >= 0) & (idx < N)).all()
        want += ['P ' + fmt(perm), 'I ' + fmt(idx)]
    for nblk, n, N, first, ok, slots, rows, src_base, val_base, ok_want in admit_cases():
        lines.append(f'A {len(rows)} {nblk} {n} {N} {first} {fmt(ok)} {fmt(slots)} {fmt(sum(rows, []))} {fmt(src_base)} {fmt(val_base)}')
        want.append('K ' + fmt(ok_want))
    for N, n_vals, ok, slots, sb, vb, vals_src, shift in put_cases():
        lines.append(f'V {len(ok)} {N} {n_vals} {vals_src.size} {shift} {fmt(ok)} {fmt(slots)} {fmt(sb)} {fmt(vb)} {fmt(vals_src)}')
        want.append('V ' + fmt(put_vals_reference(ok, slots, sb, vb, vals_src, n_vals, N)))
    return lines, want


def test_host_build_of_window_h_agrees_with_numpy(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host compiler')
    src, exe = tmp_path / 'window_host.cpp', tmp_path / 'window_host'
    src.write_text(_HOST_PROGRAM % os.path.join(ROOT, 'strajnet_amd', 'csrc', 'window.h'))
    r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', str(src), '-o', str(exe)], capture_output=True, text=True)        # host only
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = window_cases()
    r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split('\n')[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            ga, wa = g.split(), w.split()
            first = next((k for k in range(min(len(ga), len(wa))) if ga[k] != wa[k]), None)
            assert False, (i, g[:1], first, ga[first:first + 6] if first is not None else len(ga), wa[first:first + 6] if first is not None else len(wa))
