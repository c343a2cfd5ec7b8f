"""CPU side of level 2 of the device-side compression (strajnet_amd/submission.py): compress_reference(level=2), the statement of the
format with a dynamic Huffman code per segment -- every stream must pass zlib.decompress and be no longer than its level-1 stream --,
huffman_code_lengths and its two limits, and the host build of csrc/deflate_dyn.h (the rules the kernel runs) against both."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deflate import SHAPES, KINDS, planted_plane, planted_batch, planes_of                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIB_COUNTS = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 2501)


def _bound(n, S):
    return n + 5 * -(-n // S) + 6


def deep_plane(d, seed=11):
    """One 8192-byte segment without a matchable byte whose literal code needs the 15-bit limit: 16 byte values of a seeded permutation;
    A fills the even indices (d = 1) or those with i % 4 < 2 (d = 2), the other 15 the other half, shuffled, with the counts FIB_COUNTS.
    Returns (plane, the 286 symbol counts)."""
    rng = np.random.default_rng(seed + d)
    vals = rng.permutation(256)[:16].astype(np.uint8)
    rest = np.repeat(vals[1:], FIB_COUNTS)
    assert rest.size == 4096
    rng.shuffle(rest)
    x = np.empty(8192, np.uint8)
    half = (np.arange(8192) % 2 == 0) if d == 1 else (np.arange(8192) % 4 < 2)
    x[half] = vals[0]
    x[~half] = rest
    assert not (x[d:] == x[:-d]).any()
    counts = np.bincount(x, minlength=286)
    counts[256] = 1
    return x, counts


@pytest.mark.parametrize('d', [1, 2])
@pytest.mark.parametrize('n', [1, 3, 260, 256, 8192, 16384, 65536])
def test_level2_streams_decompress_and_never_exceed_level1(d, n):
    from strajnet_amd.submission import compress_reference, DEFLATE_SEGMENT as S
    rng = np.random.default_rng(n + d)
    for j, kind in enumerate(KINDS + ('runs', 'runs', 'runs')):
        if kind == 'runs' and n < 16 or kind == 'mixed' and n < 256:
            continue
        x = planted_plane(kind, n, d, S, j, rng)
        z1, z2 = compress_reference(x, d, level=1), compress_reference(x, d, level=2)
        assert compress_reference(x, d) == z1
        assert z2[:2] == b'\x78\x01' and zlib.decompress(z2) == x.tobytes(), (kind, n, d)
        assert len(z2) <= len(z1) and len(z2) <= _bound(n, S), (kind, n, d, len(z2), len(z1))
    with pytest.raises(ValueError):
        compress_reference(b'\x00', 1, level=3)


def test_level2_on_the_planted_batches_takes_all_three_forms():
    from strajnet_amd.submission import compress_reference, DEFLATE_SEGMENT as S
    forms = []
    for B, H, W in SHAPES[:3]:
        buf = planted_batch(B, H, W, S)
        for b, k, i, d, raw in planes_of(buf, H, W):
            z1, z2 = compress_reference(raw, d, level=1), compress_reference(raw, d, level=2, forms=forms)
            assert compress_reference(raw, d) == z1
            assert zlib.decompress(z2) == raw, (H, W, b, k, i)
            assert len(z2) <= len(z1) <= _bound(len(raw), S)
    print('segments stored / fixed / dynamic:', [forms.count(f) for f in (0, 1, 2)])
    assert len(forms) == 24 + 48 + 32 and set(forms) == {0, 1, 2}
    small = []                                      # a 16x16 plane of one value: the dynamic header alone is longer than the fixed block
    for kind in ('zeros', 'const', 'all255'):
        compress_reference(planted_plane(kind, 256, 1, S, 0, None), 1, level=2, forms=small)
    assert small == [1, 1, 1]


@pytest.mark.parametrize('d', [1, 2])
def test_the_15_bit_limit_is_reached(d):
    from strajnet_amd.submission import compress_reference, huffman_code_lengths
    x, counts = deep_plane(d)
    assert max(huffman_code_lengths(counts, 99)) == 16
    ll = huffman_code_lengths(counts, 15)
    assert sorted(l for l in ll if l) == list(range(1, 14)) + [15] * 4
    forms = []
    z1, z2 = compress_reference(x, d), compress_reference(x, d, level=2, forms=forms)
    print(f'd = {d}: level 1 {len(z1)} bytes, level 2 {len(z2)} bytes')
    assert forms == [2] and zlib.decompress(z2) == x.tobytes() and len(z2) < len(z1) // 3


def test_the_7_bit_limit_is_reached(monkeypatch):
    from strajnet_amd import submission
    real, deep = submission.huffman_code_lengths, []

    def spy(counts, limit):
        if limit == 7:
            deep.append(max(real(counts, 99)))
        return real(counts, limit)
    monkeypatch.setattr(submission, 'huffman_code_lengths', spy)
    for B, H, W in SHAPES[:3]:
        for _, _, _, d, raw in planes_of(planted_batch(B, H, W, submission.DEFLATE_SEGMENT), H, W):
            submission.compress_reference(raw, d, level=2)
    print('code-length codes built:', len(deep), 'deeper than 7 before the limit:', sum(x > 7 for x in deep))
    assert sum(x > 7 for x in deep) >= 1


def _count_vectors():
    rng = np.random.default_rng(3)
    out = [list(FIB_COUNTS) + [1], [5] * 19, [7] * 286, [1, 1], [0, 9, 0, 1000], [3]]
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    out.append(fib)
    for n, hi, keep in ((286, 8192, 1.0), (286, 40, 0.3), (19, 288, 0.8), (19, 3, 1.0), (60, 2, 1.0)):
        for _ in range(6):
            c = rng.integers(1, hi + 1, n) * (rng.random(n) < keep)
            out.append([int(v) for v in c])
    return out


@pytest.mark.parametrize('limit', [15, 7])
def test_huffman_code_lengths_properties(limit):
    from strajnet_amd.submission import huffman_code_lengths
    for counts in _count_vectors():
        used = [s for s, c in enumerate(counts) if c]
        if len(used) > 1 << limit:
            continue
        ll = huffman_code_lengths(counts, limit)
        assert len(ll) == len(counts) and all((ll[s] > 0) == (counts[s] > 0) for s in range(len(counts)))
        assert max(ll, default=0) <= limit
        if len(used) >= 2:
            assert sum(2 ** (limit - ll[s]) for s in used) == 2 ** limit, counts
        for a in used:
            for b in used:
                assert not (counts[a] > counts[b] and ll[a] > ll[b]), (counts, a, b)


_HOST_PROGRAM = r'''
#include <stdio.h>
#include <vector>
#include "%s"
struct Bits { std::vector<unsigned char> by; int n = 0;
  void put(uint32_t v, int nb) { for (int i = 0; i < nb; ++i, ++n) { if (n %% 8 == 0) by.push_back(0); by[n / 8] |= ((v >> i) & 1u) << (n %% 8); } } };
int main() {
  char kind;
  while (scanf(" %%c", &kind) == 1) {
    int a, b;
    if (scanf("%%d %%d", &a, &b) != 2) return 2;
    const int nsym = kind == 'K' ? a : DFD_NLIT, limit = kind == 'K' ? b : DFD_LIT_LIMIT;
    if (nsym < 1 || nsym > DFD_NSEQ || limit < 1 || limit > 15) return 3;
    uint32_t cnt[DFD_NSEQ], srt[DFD_NSEQ], iw[DFD_NSEQ], cc[DFD_NCL];
    uint16_t lpar[DFD_NSEQ], ipar[DFD_NSEQ], idep[DFD_NSEQ], code[DFD_NSEQ], ccode[DFD_NCL];
    uint8_t len[DFD_NSEQ], cl[DFD_NCL], rsym[DFD_NSEQ], rext[DFD_NSEQ];
    int lc[16], nx[16];
    for (int s = 0; s < nsym; ++s) if (scanf("%%u", &cnt[s]) != 1) return 4;
    dfd_lengths(cnt, nsym, limit, len, code, srt, iw, lpar, ipar, idep, lc, nx);
    printf("L");
    for (int s = 0; s < nsym; ++s) printf(" %%d", len[s]);
    printf("\nC");
    for (int s = 0; s < nsym; ++s) printf(" %%d", code[s]);
    printf("\n");
    if (kind == 'B') {                                   /* a = d, b = final */
      const int nl = dfd_num_lit(len);
      const int nr = dfd_rle(len, nl, a, rsym, rext, cc);
      dfd_lengths(cc, DFD_NCL, DFD_CL_LIMIT, cl, ccode, srt, iw, lpar, ipar, idep, lc, nx);
      Bits h;
      dfd_put_header(h, b, nl, a, cl, ccode, rsym, rext, nr);
      if (h.n != dfd_header_bits(cc, cl)) return 5;
      printf("H %%d ", h.n);
      for (unsigned char c : h.by) printf("%%02x", c);
      printf("\n");
    }
  }
  return 0;
}
'''


def _host_compiler():
    from strajnet_amd import build
    try:
        return build._hipcc()
    except RuntimeError:
        return shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')


def test_host_build_of_the_kernel_rules_agrees_with_the_reference(tmp_path):
    """csrc/deflate_dyn.h compiled for the host, as a program of its own: the lengths and codes of dfd_lengths == huffman_code_lengths
    and the canonical codes on the count vectors of the property test, and the header bits of dfd_put_header == the reference's on the
    literal/length counts of the planted segments and of the two 15-bit planes."""
    from strajnet_amd import submission
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host compiler')
    src, exe = tmp_path / 'dyn_host.cpp', tmp_path / 'dyn_host'
    src.write_text(_HOST_PROGRAM % os.path.join(ROOT, 'strajnet_amd', 'csrc', 'deflate_dyn.h'))
    r = subprocess.run([cxx, '-x', 'c++', '-std=c++17', '-O1', str(src), '-o', str(exe)], capture_output=True, text=True)        # host only
    assert r.returncode == 0, r.stderr[-3000:]
    lines, want = [], []
    for limit in (15, 7):
        for counts in _count_vectors():
            if sum(c > 0 for c in counts) > 1 << limit:
                continue
            ll = submission.huffman_code_lengths(counts, limit)
            lines.append(f'K {len(counts)} {limit} ' + ' '.join(map(str, counts)))
            want += ['L ' + ' '.join(map(str, ll)), 'C ' + ' '.join(map(str, submission._canonical_codes(ll)))]
    blocks = [(d, 1, deep_plane(d)[1]) for d in (1, 2)]
    real, seen = submission.dynamic_block_header, []

    def spy(counts, d, final):
        seen.append((d, int(final), np.array(counts)))
        return real(counts, d, final)
    submission.dynamic_block_header = spy
    try:
        B, H, W = SHAPES[2]
        for _, _, _, d, raw in planes_of(planted_batch(B, H, W, submission.DEFLATE_SEGMENT), H, W):
            submission.compress_reference(raw, d, level=2)
    finally:
        submission.dynamic_block_header = real
    assert len(seen) == 32 and {f for _, f, _ in seen} == {0, 1}
    for d, final, counts in blocks + seen:
        ll, code, hv, hn = real(counts, d, final)
        bits = int(sum(hn))
        packed = submission._pack_bits(np.array(hv, np.uint64), np.array(hn, np.int64), bits).tobytes()
        lines.append(f'B {d} {final} ' + ' '.join(str(int(c)) for c in counts))
        want += ['L ' + ' '.join(map(str, ll)), 'C ' + ' '.join(map(str, code)), f'H {bits} {packed.hex()}']
    r = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split('\n')[:-1]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:200], w[:200])


def sparse_planes(B, H, W, seed):
    """tools/bench_submission.py's generator: per plane a zero background with a dozen rectangular blobs."""
    rng = np.random.default_rng(seed)
    buf = np.zeros((B, 24, 2 * H * W), np.uint8)
    for b in range(B):
        for p in range(24):
            img = np.zeros((H, W, 2 if p >= 16 else 1), np.uint8)
            for _ in range(12):
                h, w = rng.integers(4, 28, 2)
                y, x0 = rng.integers(0, H - h), rng.integers(0, W - w)
                if p >= 16:
                    img[y:y + h, x0:x0 + w] = rng.integers(0, 256, 2, dtype=np.uint8)
                else:
                    v = rng.integers(32, 256)
                    img[y:y + h, x0:x0 + w] = v // 2
                    img[y + 1:y + h - 1, x0 + 1:x0 + w - 1] = v
            buf[b, p, :img.size] = img.reshape(-1)
    n = H * W
    return np.ascontiguousarray(np.concatenate([buf[:, :16, :n].reshape(B, -1), buf[:, 16:].reshape(B, -1)], axis=1))


def test_level2_sizes():
    """All-zero 256x256 planes: <= 256 (occupancy) and <= 512 bytes (flow).  The sparse scene of the submission benchmark: at most 0.6
    of its level-1 size."""
    from strajnet_amd.submission import compress_reference
    zo, zf = compress_reference(np.zeros(65536, np.uint8), 1, level=2), compress_reference(np.zeros(131072, np.uint8), 2, level=2)
    print(f'all-zero planes at level 2: occupancy {len(zo)} bytes, flow {len(zf)} bytes')
    assert len(zo) <= 256 and len(zf) <= 512
    assert zlib.decompress(zo) == bytes(65536) and zlib.decompress(zf) == bytes(131072)
    t = [0, 0, 0, 0]
    for _, _, _, d, raw in planes_of(sparse_planes(1, 256, 256, 1234), 256, 256):
        z2 = compress_reference(raw, d, level=2)
        assert zlib.decompress(z2) == raw
        for i, n in enumerate((len(compress_reference(raw, d)), len(z2), len(zlib.compress(raw, 1)), len(zlib.compress(raw, 6)))):
            t[i] += n
    print(f'sparse scene, 24 streams: level 1 {t[0]}, level 2 {t[1]}, zlib level 1 {t[2]}, zlib level 6 {t[3]} bytes')
    assert t[1] <= 0.6 * t[0]
