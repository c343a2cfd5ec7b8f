"""TFRecord input path of the reference (train.py:71-103, inference.py:67-96) without TensorFlow.

Host side (pure Python, no TF): TFRecord framing (length, masked CRC-32C, payload, masked CRC-32C) and the tf.Example
protobuf wire format restricted to what the reference's records contain -- one BytesList value per feature.
Device side: `decode_batch` uploads the raw feature bytes of a batch and expands them with one HIP launch per feature
(stj_decode_raw: bool / int8 / float32 / float64 -> float32, centre crop, scale), i.e. `_parse_image_function`.

    for batch in batches(read_tfrecord(path), 8):
        data = decode_batch(batch, 'cuda')          # dict: ogm [B,512,512,11,2], map_image [B,256,256,3], gt_flow [B,8,256,256,2] ...

A writer (`write_tfrecord`, `serialize_example`) exists for tests and synthetic data; it produces the same bytes TF reads.

Packed records (opt-in): most of those bytes carry no information -- a bool needs one bit, a float plane that is zero almost everywhere
one bit per cell plus its non-zero words.  `pack_example` rewrites a parsed record into that lossless form once, on the host
(`pack_bits`, `pack_sparse`; `unpack_reference` states the format and is the only CPU path); `decode_batch_packed` and `PackedFeed` upload
the packed bytes and expand them on the device (stj_unpack_bits / stj_unpack_sparse) into the same float32 tensors, bit for bit, that
`decode_batch` and `HostFeed.land()` give for the original record.

Scenes resident in HBM (opt-in): `PoolLayout` lays N packed scenes out for the device, `ResidentPool` uploads them once, and batches are
gathered from them by a device index vector (stj_gather_bits / stj_gather_sparse / stj_gather_raw) -- `ResidentFeed` has HostFeed's protocol
with no upload per step, `PoolSampler` shuffles on the device.  `PoolLayout.reference_gather` states the semantics in NumPy.
Pool scenes are replaced in place from the reference's own unpacked records: `ResidentPool.empty` allocates zero-filled slots,
`PoolWriter` (pool.writer(B)) uploads the raw bytes and packs them on the device (stj_pack_bits / stj_pack_sparse_count / stj_pool_admit /
stj_pack_sparse_commit / stj_pool_put_raw); `PoolLayout.replace_reference` states that in NumPy.
A shuffle buffer in HBM over a stream of any length: `ShuffleWindow` (pool.window(B, source)) draws batches from the live slots on the device
(stj_pool_draw) and refills consumed slots from packed records on a worker thread and a stream of its own (stj_pool_admit_packed /
stj_pool_put_raw / stj_pool_put_vals); `WindowFeed` has HostFeed's protocol, `PoolWriter.put_packed` is the synchronous form;
`ShuffleWindow.reference` and `PoolLayout.replace_packed_reference` state the semantics.
"""
import collections
import ctypes
import struct

import numpy as np
import torch

from .ops import _p, _st, call

KIND = {'bool': 0, 'int8': 1, 'float32': 2, 'float64': 3}
ITEMSIZE = {'bool': 1, 'int8': 1, 'float32': 4, 'float64': 8}


def feature_spec(grid=512, out=256, test=False):
    """name -> (raw dtype, raw shape, (y0, x0, Ho, Wo) or None, scale).  train.py:87-103 (test=False) / inference.py:84-96."""
    c0 = (grid - out) // 2
    crop = (c0, c0, out, out)
    spec = {
        'centerlines': ('float64', (256, 10, 7), None, 1.0),
        'actors': ('float64', (48, 11, 8), None, 1.0),
        'occl_actors': ('float64', (16, 11, 8), None, 1.0),
        'ogm': ('bool', (grid, grid, 11, 2), None, 1.0),
        'map_image': ('int8', (out, out, 3), None, 1.0 / 256.0),
        'vec_flow': ('float32', (grid, grid, 2), None, 1.0),
    }
    if not test:
        spec.update({
            'gt_flow': ('float32', (8, grid, grid, 2), crop, 1.0),
            'origin_flow': ('float32', (8, grid, grid, 1), crop, 1.0),
            'gt_obs_ogm': ('bool', (8, grid, grid, 1), crop, 1.0),
            'gt_occ_ogm': ('bool', (8, grid, grid, 1), crop, 1.0),
        })
    return spec


# ---------------------------------------------------------------------------------------------------- CRC-32C (Castagnoli)
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


_TABLE = _crc_table()


def _crc32c_py(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


_FAST = None


def crc32c(data, crc=0):
    """CRC-32C of `data` (bytes-like or ndarray), continuing from `crc`.  Uses the host routine of libstrajnet_hip.so
    (`stj_crc32c`, slice-by-8); the byte loop above is what it is tested against and what runs if the library is not built."""
    global _FAST
    if _FAST is None:
        try:
            from . import _lib
            _FAST = _lib.lib().stj_crc32c
        except Exception:
            _FAST = False
    if not _FAST:
        return _crc32c_py(data, crc)
    a = np.ascontiguousarray(data).reshape(-1).view(np.uint8) if isinstance(data, np.ndarray) else np.frombuffer(data, np.uint8)
    c = ctypes.c_uint(crc)
    if _FAST(a.ctypes.data if a.size else None, a.size, ctypes.byref(c)) != 0:
        raise RuntimeError('stj_crc32c failed')
    return c.value


def masked_crc(data):
    c = crc32c(data)
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- TFRecord framing
def read_tfrecord(path, check_data_crc=False):
    """Yield the payload of every record.  The 12-byte header CRC is always verified; the payload CRC (35 MB per example in
    pure Python) only on request."""
    with open(path, 'rb') as f:
        while True:
            head = f.read(12)
            if not head:
                return
            if len(head) != 12:
                raise ValueError('truncated TFRecord header')
            n, hcrc = struct.unpack('<QI', head)
            if masked_crc(head[:8]) != hcrc:
                raise ValueError('corrupt TFRecord length')
            data = f.read(n)
            tail = f.read(4)
            if len(data) != n or len(tail) != 4:
                raise ValueError('truncated TFRecord payload')
            if check_data_crc and masked_crc(data) != struct.unpack('<I', tail)[0]:
                raise ValueError('corrupt TFRecord payload')
            yield data


def write_tfrecord(path, payloads):
    with open(path, 'wb') as f:
        for data in payloads:
            head = struct.pack('<Q', len(data))
            f.write(head + struct.pack('<I', masked_crc(head)) + data + struct.pack('<I', masked_crc(data)))


# ---------------------------------------------------------------------------------------------------- tf.Example (bytes features)
def _varint(buf, i):
    r, s = 0, 0
    while True:
        b = buf[i]
        i += 1
        r |= (b & 0x7F) << s
        if not b & 0x80:
            return r, i
        s += 7


def _fields(buf):
    """(field number, wire type, value) of a protobuf message; value = int (varint) or memoryview (length-delimited)."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        fno, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 2:
            ln, i = _varint(buf, i)
            v = buf[i:i + ln]
            i += ln
        elif wt == 1:
            v = buf[i:i + 8]; i += 8
        elif wt == 5:
            v = buf[i:i + 4]; i += 4
        else:
            raise ValueError(f'unsupported protobuf wire type {wt}')
        yield fno, wt, v


def parse_example(payload):
    """tf.train.Example -> {feature name: bytes} for BytesList features (Example.features=1, Features.feature=1 (map entry:
    key=1, value=2), Feature.bytes_list=1, BytesList.value=1)."""
    buf = memoryview(payload)
    out = {}
    for fno, wt, feats in _fields(buf):
        if fno != 1 or wt != 2:
            continue
        for f2, w2, entry in _fields(feats):
            if f2 != 1 or w2 != 2:
                continue
            name, value = None, None
            for f3, w3, v in _fields(entry):
                if f3 == 1:
                    name = bytes(v).decode()
                elif f3 == 2:
                    for f4, w4, lst in _fields(v):
                        if f4 == 1 and w4 == 2:             # bytes_list
                            for f5, w5, b in _fields(lst):
                                if f5 == 1:
                                    value = b
            if name is not None and value is not None:
                out[name] = value
    return out


def _enc_varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _ld(fno, payload):
    return _enc_varint((fno << 3) | 2) + _enc_varint(len(payload)) + payload


def serialize_example(features):
    """{name: bytes} -> tf.train.Example bytes (what data_preprocessing.py:365-381 writes with tf.train.Example)."""
    entries = b''
    for name in sorted(features):
        feat = _ld(1, _ld(1, bytes(features[name])))                  # Feature{bytes_list{value}}
        entries += _ld(1, _ld(1, name.encode()) + _ld(2, feat))       # map entry
    return _ld(1, entries)


def parse_example_lists(payload):
    """tf.train.Example -> {feature name: float32 array | int64 array} for its FloatList (Feature.float_list=2) and Int64List
    (Feature.int64_list=3) features, packed or not: what a Waymo motion record holds (strajnet_amd/raster.py,
    tracks_from_motion_example).  BytesList features are parse_example's."""
    out = {}
    for fno, wt, feats in _fields(memoryview(payload)):
        if fno != 1 or wt != 2:
            continue
        for f2, w2, entry in _fields(feats):
            if f2 != 1 or w2 != 2:
                continue
            name, value = None, None
            for f3, w3, v in _fields(entry):
                if f3 == 1:
                    name = bytes(v).decode()
                elif f3 == 2:
                    for f4, w4, lst in _fields(v):
                        if f4 == 2 and w4 == 2:             # float_list: value = 1, packed (one length-delimited run) or one fixed32 each
                            parts = [bytes(b) for f5, w5, b in _fields(lst) if f5 == 1 and w5 in (2, 5)]
                            value = np.frombuffer(b''.join(parts), '<f4').astype(np.float32)
                        elif f4 == 3 and w4 == 2:           # int64_list: value = 1, packed varints or one varint each
                            ints = []
                            for f5, w5, b in _fields(lst):
                                if f5 != 1:
                                    continue
                                if w5 == 0:
                                    ints.append(b)
                                elif w5 == 2:
                                    i = 0
                                    while i < len(b):
                                        r, i = _varint(b, i)
                                        ints.append(r)
                            value = np.array([r - (1 << 64) if r >> 63 else r for r in ints], np.int64)
            if name is not None and value is not None:
                out[name] = value
    return out


def serialize_example_lists(features):
    """{name: float array | integer array | bytes} -> tf.train.Example bytes with packed FloatList / Int64List / BytesList features: the
    writer that matches parse_example_lists (and parse_example for the bytes), for tests and synthetic motion records."""
    entries = b''
    for name in sorted(features):
        v = features[name]
        if isinstance(v, (bytes, bytearray, memoryview)):
            feat = _ld(1, _ld(1, bytes(v)))
        else:
            v = np.asarray(v)
            if v.dtype.kind == 'f':
                feat = _ld(2, _ld(1, v.astype('<f4').tobytes()) if v.size else b'')
            elif v.dtype.kind in 'iub':
                feat = _ld(3, _ld(1, b''.join(_enc_varint(int(i) & ((1 << 64) - 1)) for i in v.reshape(-1))) if v.size else b'')
            else:
                raise ValueError(f'feature {name}: no tf.Example list for dtype {v.dtype}')
        entries += _ld(1, _ld(1, name.encode()) + _ld(2, feat))
    return _ld(1, entries)


def batches(examples, batch_size):
    buf = []
    for e in examples:
        buf.append(parse_example(e) if isinstance(e, (bytes, bytearray, memoryview)) else e)
        if len(buf) == batch_size:
            yield buf
            buf = []
    if buf:
        yield buf


# ---------------------------------------------------------------------------------------------------- packed features (host, NumPy)
SPARSE_BLOCK = 8192         # elements per block of a sparse plane's `offs` (csrc/unpack.h: UP_BLOCK)
PACKED_KIND = {'ogm': 'bits', 'gt_obs_ogm': 'bits', 'gt_occ_ogm': 'bits', 'vec_flow': 'sparse', 'gt_flow': 'sparse', 'origin_flow': 'sparse'}
_RAW_DTYPE = {'bool': np.uint8, 'int8': np.int8, 'float32': '<u4', 'float64': '<f8'}


def pack_bits(a):
    """Any array -> uint32 words: element i (C order) is bit i & 7 of byte i >> 3, LSB first, set iff the element is non-zero; zero
    bits pad the stream to a whole number of 32-bit words (little-endian words: bit i & 31 of word i >> 5)."""
    b = np.packbits(np.ascontiguousarray(a).reshape(-1) != 0, bitorder='little')
    b = np.concatenate([b, np.zeros(-b.size % 4, np.uint8)])
    return b.view('<u4')


def _words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize != 4:
        raise ValueError(f'pack_sparse: 32-bit elements only, got {a.dtype}')
    return a.reshape(-1).view(np.uint32)


def pack_sparse(a):
    """float32 (or any 32-bit) array of n elements, n a multiple of 32 -> (mask, offs, vals), all uint32: a word is present iff its
    32-bit pattern is non-zero (-0.0, NaN payloads and denormals are present and survive unchanged); mask [n / 32] in pack_bits' order;
    offs [ceil(n / SPARSE_BLOCK) + 1] the exclusive prefix of the present counts per block, offs[-1] the total; vals the present words
    in element order."""
    w = _words(a)
    n = w.size
    if n % 32:
        raise ValueError(f'pack_sparse: {n} elements, a multiple of 32 only')
    present = w != 0
    nblk = -(-n // SPARSE_BLOCK)
    counts = np.add.reduceat(present.astype(np.int64), np.arange(0, n, SPARSE_BLOCK)) if n else np.zeros(0, np.int64)
    offs = np.zeros(nblk + 1, np.uint32)
    offs[1:] = np.cumsum(counts)
    return pack_bits(present), offs, w[present].copy()


def check_sparse(mask, offs, vals, n, name='sparse'):
    """ValueError unless (mask, offs, vals) -- arrays or the record's bytes -- are a well-formed sparse plane of n elements: byte
    lengths, offs starting at 0 and non-decreasing, no block holding more than its element count, offs[-1] values.  -> uint32 arrays."""
    if n % 32:
        raise ValueError(f'{name}: {n} elements, a multiple of 32 only')
    nblk = -(-n // SPARSE_BLOCK)
    arrs = []
    for part, x, want in (('mask', mask, n // 8), ('offs', offs, 4 * (nblk + 1)), ('vals', vals, None)):
        x = np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        if x.size % 4 or (want is not None and x.size != want):
            raise ValueError(f'{name}/{part}: {x.size} bytes' + (f', expected {want}' if want is not None else ', not whole 32-bit words'))
        arrs.append(x.view('<u4'))
    mask, offs, vals = arrs
    d = np.diff(offs.astype(np.int64))
    if offs[0] != 0 or (d < 0).any():
        raise ValueError(f'{name}/offs: not a non-decreasing prefix from 0')
    cap = np.minimum(SPARSE_BLOCK, n - SPARSE_BLOCK * np.arange(nblk))
    if (d > cap).any():
        raise ValueError(f'{name}/offs: a block holds more present words than elements')
    if int(offs[-1]) != vals.size:
        raise ValueError(f'{name}: offs[-1] = {int(offs[-1])} but vals holds {vals.size} words')
    return mask, offs, vals


def unpack_reference(kind, *args):
    """The format, stated in code: unpack_reference('bits', bits, n) / unpack_reference('sparse', mask, offs, vals, n) -> float32 [n].
    bits: 1.0f where bit i & 7 of byte i >> 3 is set, else 0.0f.  sparse: element i is vals[offs[i // SPARSE_BLOCK] + popcount(mask
    bits of its block below i)] where its mask bit is set, else +0.0f."""
    if kind == 'bits':
        bits, n = args
        by = np.ascontiguousarray(bits).reshape(-1).view(np.uint8)
        if by.size != 4 * -(-n // 32):
            raise ValueError(f'bits: {by.size} bytes, expected {4 * -(-n // 32)} for {n} elements')
        return np.unpackbits(by, bitorder='little')[:n].astype(np.float32)
    if kind != 'sparse':
        raise ValueError(f'unpack_reference: kind {kind!r}')
    mask, offs, vals, n = args
    mask, offs, vals = check_sparse(mask, offs, vals, n)
    bit = np.unpackbits(mask.view(np.uint8), bitorder='little')[:n].astype(np.int64)
    out = np.zeros(n, np.uint32)
    for blk in range(-(-n // SPARSE_BLOCK)):
        lo, hi = blk * SPARSE_BLOCK, min(n, (blk + 1) * SPARSE_BLOCK)
        below = np.cumsum(bit[lo:hi]) - bit[lo:hi]                  # popcount of the block's mask bits below each element
        idx = int(offs[blk]) + below
        sel = bit[lo:hi] != 0
        if sel.any() and int(idx[sel].max()) >= vals.size:
            raise ValueError('sparse: mask and offs disagree')
        out[lo:hi][sel] = vals[idx[sel]]
    return out.view(np.float32)


def _decoded(raw, dtype, shape, crop):
    """The decoded array of a feature: the record's bytes after the reshape and centre crop, before the cast (float32 as uint32 words)."""
    a = np.frombuffer(bytes(raw), _RAW_DTYPE[dtype])
    if a.size != int(np.prod(shape)):
        raise ValueError(f'{a.size * a.itemsize} bytes, expected {int(np.prod(shape)) * ITEMSIZE[dtype]} for {dtype}{list(shape)}')
    a = a.reshape(shape)
    if crop is not None:
        y0, x0, Ho, Wo = crop
        a = a[:, y0:y0 + Ho, x0:x0 + Wo, :]
    return a


def decoded_shape(shape, crop):
    return tuple(shape) if crop is None else (shape[0], crop[2], crop[3], shape[3])


def pack_example(example, grid=512, out=256, test=False):
    """A parsed record ({feature: bytes}) -> {feature: bytes} with the bool features as `<name>/bits` and the float32 planes as
    `<name>/mask`, `<name>/offs`, `<name>/vals` (the ground-truth features already centre-cropped); everything else under its own name.
    serialize_example / write_tfrecord store the result like any record."""
    res = {}
    spec = feature_spec(grid, out, test)
    for name, raw in example.items():
        kind = PACKED_KIND.get(name) if name in spec else None
        if kind is None:
            res[name] = bytes(raw)
            continue
        dtype, shape, crop, _ = spec[name]
        try:
            a = _decoded(raw, dtype, shape, crop)
        except ValueError as e:
            raise ValueError(f'feature {name}: {e}') from None
        if a.size % 32:
            raise ValueError(f'feature {name}: {a.size} elements per scene, a multiple of 32 only')
        if kind == 'bits':
            res[name + '/bits'] = pack_bits(a).tobytes()
        else:
            mask, offs, vals = pack_sparse(a)
            res[name + '/mask'], res[name + '/offs'], res[name + '/vals'] = mask.tobytes(), offs.tobytes(), vals.tobytes()
    return res


def unpack_example_reference(packed, grid=512, out=256, test=False):
    """CPU inverse of pack_example + _parse_image_function, NumPy only: {feature: float32 array}, shaped as decode_batch shapes one
    scene.  What decode_batch_packed is tested against; not a product path."""
    res = {}
    for name, (dtype, shape, crop, scale) in feature_spec(grid, out, test).items():
        dshape = decoded_shape(shape, crop)
        n = int(np.prod(dshape))
        kind = PACKED_KIND.get(name)
        if kind == 'bits' and name + '/bits' in packed:
            res[name] = unpack_reference('bits', np.frombuffer(bytes(packed[name + '/bits']), np.uint8), n).reshape(dshape)
        elif kind == 'sparse' and name + '/mask' in packed:
            res[name] = unpack_reference('sparse', *(bytes(packed[f'{name}/{p}']) for p in ('mask', 'offs', 'vals')), n).reshape(dshape)
        else:
            a = _decoded(packed[name], dtype, shape, crop)
            a = a.view(np.float32) if dtype == 'float32' else (a != 0) if dtype == 'bool' else a
            res[name] = a.astype(np.float32) * np.float32(scale)
    return res


# ---------------------------------------------------------------------------------------------------- device decode
def _hip_device(who, device):
    """torch.device(device); RuntimeError unless it is a GPU."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(f'{who}: CUDA (ROCm) device only: the HIP path has no CPU fallback')
    return dev


def _with_scenario_ids(res, examples, test):
    """'scenario/id' is not a tensor: the test records' ids ride along as a list of bytes."""
    if test and 'scenario/id' in examples[0]:
        res['scenario/id'] = [bytes(ex['scenario/id']) for ex in examples]
    return res


def _decode_raw_feature(examples, name, spec, dev):
    """One feature of a batch from the record's own bytes: pinned upload + stj_decode_raw (crop, cast, scale)."""
    dtype, shape, crop, scale = spec
    B = len(examples)
    nbytes = int(np.prod(shape)) * ITEMSIZE[dtype]
    host = torch.empty((B, nbytes), dtype=torch.uint8).pin_memory()
    for b, ex in enumerate(examples):
        raw = ex[name]
        if len(raw) != nbytes:
            raise ValueError(f'feature {name}: {len(raw)} bytes, expected {nbytes} for {dtype}{list(shape)}')
        host[b] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
    src = host.to(dev, non_blocking=True)
    if crop is None:
        n_outer, H, W, C = B, 1, int(np.prod(shape)), 1
        y0, x0, Ho, Wo = 0, 0, 1, W
    else:
        n_outer, H, W, C = B * shape[0], shape[1], shape[2], shape[3]
        y0, x0, Ho, Wo = crop
    dst = torch.empty((B,) + decoded_shape(shape, crop), dtype=torch.float32, device=dev)
    call('stj_decode_raw', _p(src), KIND[dtype], _p(dst), n_outer, H, W, C, y0, x0, Ho, Wo, float(scale), _st())
    return dst


def decode_batch(examples, device='cuda', grid=512, out=256, test=False):
    """examples: list of {feature: bytes} (parse_example output).  Returns float32 tensors on `device`, leading batch axis,
    shaped and cropped as _parse_image_function does (train.py:87-103): ogm [B,g,g,11,2], map_image [B,o,o,3] (/256),
    vec_flow [B,g,g,2], actors [B,48,11,8], occl_actors [B,16,11,8], centerlines [B,256,10,7] and, unless test,
    gt_flow [B,8,o,o,2], origin_flow / gt_obs_ogm / gt_occ_ogm [B,8,o,o,1]."""
    dev = _hip_device('decode_batch', device)
    res = {name: _decode_raw_feature(examples, name, sp, dev) for name, sp in feature_spec(grid, out, test).items()}
    return _with_scenario_ids(res, examples, test)


def _pinned_words(n):
    return torch.empty((max(int(n), 1),), dtype=torch.int32).pin_memory()


def _put(dst, off, arr):
    """uint32 array -> words off.. of a (pinned) int32 tensor."""
    if arr.size:
        dst.numpy()[off:off + arr.size] = np.ascontiguousarray(arr).view(np.int32)


def _batch_sparse(planes, n):
    """[(mask, offs, vals)] of a batch (checked uint32 arrays) -> pinned int32 tensors mask [B * n/32], offs [B * (nblk + 1)],
    val_base [B + 1], vals [total] and the total."""
    B, nw, nb1 = len(planes), n // 32, -(-n // SPARSE_BLOCK) + 1
    base = np.zeros(B + 1, np.int64)
    base[1:] = np.cumsum([pl[2].size for pl in planes])
    mask, offs, vb, vals = _pinned_words(B * nw), _pinned_words(B * nb1), _pinned_words(B + 1), _pinned_words(base[-1])
    for b, (m, o, v) in enumerate(planes):
        _put(mask, b * nw, m); _put(offs, b * nb1, o); _put(vals, int(base[b]), v)
    _put(vb, 0, base.astype(np.uint32))
    return mask, offs, vb, vals, int(base[-1])


def decode_batch_packed(examples, device='cuda', grid=512, out=256, test=False):
    """decode_batch for records written by pack_example: the same dict, shapes and float32 values, bit for bit.  The packed features
    cross PCIe as they are stored (a sparse plane: only its used words) and are expanded by stj_unpack_bits / stj_unpack_sparse; the
    unpacked ones go through stj_decode_raw as in decode_batch.  Every stream is checked on the host before any launch (ValueError)."""
    dev = _hip_device('decode_batch_packed', device)
    B = len(examples)
    spec = feature_spec(grid, out, test)
    todo = []
    for name, sp in spec.items():                                    # host: check every stream first, NumPy only
        dtype, shape, crop, scale = sp
        dshape = decoded_shape(shape, crop)
        n = int(np.prod(dshape))
        kind = PACKED_KIND.get(name)
        if kind == 'bits' and name + '/bits' in examples[0]:
            if n % 32 or B * n >= 1 << 32:
                raise ValueError(f'feature {name}: {B} x {n} elements, a multiple of 32 per scene and fewer than 2^32 only')
            for ex in examples:
                if len(ex[name + '/bits']) != n // 8:
                    raise ValueError(f"feature {name}/bits: {len(ex[name + '/bits'])} bytes, expected {n // 8} for {n} elements")
            todo.append((name, 'bits', dshape, n, None))
        elif kind == 'sparse' and name + '/mask' in examples[0]:
            if B * n >= 1 << 32:
                raise ValueError(f'feature {name}: {B} x {n} elements, fewer than 2^32 only')
            planes = [check_sparse(*(ex[f'{name}/{p}'] for p in ('mask', 'offs', 'vals')), n, f'feature {name}') for ex in examples]
            todo.append((name, 'sparse', dshape, n, planes))
        else:
            for ex in examples:
                if len(ex[name]) != int(np.prod(shape)) * ITEMSIZE[dtype]:
                    raise ValueError(f'feature {name}: {len(ex[name])} bytes, expected {int(np.prod(shape)) * ITEMSIZE[dtype]} for {dtype}{list(shape)}')
            todo.append((name, 'raw', dshape, n, sp))
    res = {}
    for name, kind, dshape, n, h in todo:
        if kind == 'raw':
            res[name] = _decode_raw_feature(examples, name, h, dev)
            continue
        dst = torch.empty((B,) + dshape, dtype=torch.float32, device=dev)
        if kind == 'bits':
            host = _pinned_words(B * n // 32)
            for b, ex in enumerate(examples):
                _put(host, b * (n // 32), np.frombuffer(bytes(ex[name + '/bits']), '<u4'))
            src = host.to(dev, non_blocking=True)
            call('stj_unpack_bits', _p(src), _p(dst), B * n, _st())
        else:
            mask, offs, vb, vals, total = _batch_sparse(h, n)
            d = [t.to(dev, non_blocking=True) for t in (mask, offs, vb, vals)]
            call('stj_unpack_sparse', _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), total, _p(dst), B, n, _st())
        res[name] = dst
    return _with_scenario_ids(res, examples, test)


# ---------------------------------------------------------------------------------------------------- per-step feed of a captured step
_COPY_STREAMS = {}


def _copy_stream(dev):
    """ONE upload stream per device for every HostFeed (streams are multiplexed on a few hardware queues in creation order; a fresh
    stream per feed lands on a different queue each time, and on the main chain's queue its SDMA barriers hold the step up)."""
    key = str(dev)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(dev)
    return _COPY_STREAMS[key]


def _copy_chunked(dst, src, count, chunk_bytes):
    """dst[:count] <- src[:count] (flat tensors, host to device) in copies of at most chunk_bytes, on the current stream.  The one
    upload loop of this module: HostFeed explains the pieces."""
    step = max(1, chunk_bytes // src.element_size())
    for i in range(0, count, step):
        j = min(count, i + step)
        dst[i:j].copy_(src[i:j], non_blocking=True)


class HostFeed:
    """Feeds the static input tensors of a captured train step (graph.GraphedTrainStep.static) from PINNED host buffers, one batch
    per step (reference train.py:85-103,319: every step consumes a new batch), without stretching the step:

        feed = HostFeed(step.static, host, raw={'ogm': 'bool', ...})
        feed.start()                       # upload of the first batch
        for ...:
            feed.land()                    # device: wait for the upload, staging -> static inputs (copies / stj_decode_raw, ~0.1 ms)
                                           # host: the worker thread starts uploading what host[...] holds NOW (the next batch)
            step(); optimizer.step()
            feed.wait_uploaded()           # (a loader refills host[...] only after this returns)

    host[k]: pinned tensors -- float32, or for the keys of `raw` the TFRecord's own bytes ('bool' / 'int8', expanded on the device).
    Why a worker thread and 1.5 MB pieces (tools/probes/feed_probe.py, feed_probe3.py, feed_trace*.sh; B = 8: 77 MB of raw bytes per step):
      * hipMemcpyAsync of a large pinned buffer BLOCKS its host thread for the duration of the transfer.  Issued from the thread that
        replays the graph, no kernel runs until the last byte has arrived: the step grew by the full PCIe time (6.3 -> 8.4 ms),
        whichever stream / priority / order, also as a memcpy node inside the graph;
      * a kernel reading the pinned buffer over PCIe overlaps, but every kernel that runs beside it slows down 5-15x;
      * from a second thread the SDMA transfer overlaps the step -- except that while ONE call is blocked the replaying thread's
        launches stall too: a 33 MB tensor as one call left the GPU idle for 0.7 ms.  Measured by piece size (raw bytes, ms per step;
        resident inputs 6.28): 32 MB 7.42, 8 MB 7.65, 4 MB 7.49, 2 MB 6.60, 1.5 MB 6.47, 1 MB 6.57, 0.5 MB 6.48, 0.25 MB 6.48 --
        in 1.5 MB pieces the step keeps its resident-input time within 3 % (float32 host tensors, 141 MB: 7.2 ms)."""

    def __init__(self, static, host, raw=None, chunk_bytes=3 << 19):
        import threading
        self.static, self.host, self.raw = static, {k: h for k, h in host.items() if k in static}, dict(raw or {})
        dev = next(iter(static.values())).device
        self.dev = dev
        for k, h in self.host.items():
            if not h.is_pinned():
                raise ValueError(f'HostFeed: host[{k!r}] must be pinned memory')
        for k, kind in self.raw.items():
            if k in self.host and kind not in ('bool', 'int8'):               # one byte per element: what land() hands stj_decode_raw
                raise ValueError(f"HostFeed: raw[{k!r}] is {kind!r}, 'bool' or 'int8' only")
        self.stage = {k: torch.empty(h.shape, dtype=h.dtype, device=dev) for k, h in self.host.items()}
        self._landing = self.stage                      # what land() expands, in launch order
        self.chunk = int(chunk_bytes)
        self.copy = _copy_stream(dev)
        self.up, self.landed = torch.cuda.Event(), torch.cuda.Event()
        self._go, self._enqueued = threading.Event(), threading.Event()
        self._stop = False
        self._err = None
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def _upload(self):
        with torch.cuda.stream(self.copy):
            self.copy.wait_event(self.landed)            # the staging buffers are free once the previous batch has left them
            self._copies()
            self.up.record(self.copy)

    def _copies(self):
        for k, h in self.host.items():
            _copy_chunked(self.stage[k].view(-1), h.view(-1), h.numel(), self.chunk)

    def _run(self):
        torch.cuda.set_device(self.dev)
        while True:
            self._go.wait(); self._go.clear()
            if self._stop:
                return
            try:
                self._upload()
            except Exception as e:       # surfaced by the next land() / wait_uploaded()
                self._err = e
            self._enqueued.set()

    def _check(self):
        if self._err is not None:
            e, self._err = self._err, None
            raise e

    def start(self):
        self.landed.record(torch.cuda.current_stream(self.dev))
        self._go.set()

    def land(self):
        self._enqueued.wait(); self._enqueued.clear()       # the upload has been enqueued: its `up` event is recorded
        self._check()
        main = torch.cuda.current_stream(self.dev)
        main.wait_event(self.up)
        for k, st in self._landing.items():
            self._expand(k, st, self.static[k])
        self.landed.record(main)
        self._go.set()                                       # next batch: whatever host[...] holds now

    def _expand(self, k, st, dst):
        """One staged key into its static tensor, on the current stream."""
        if k in self.raw:
            n = dst.numel()
            call('stj_decode_raw', _p(st), KIND[self.raw[k]], _p(dst), 1, 1, n, 1, 0, 0, 1, n, (1.0 / 256.0) if self.raw[k] == 'int8' else 1.0, _st())
        else:
            dst.copy_(st, non_blocking=True)

    def wait_uploaded(self):
        """Host-side: returns once the upload kicked off by the last land() has left the host buffers (a loader may refill them)."""
        self._enqueued.wait()
        self._check()
        self.up.synchronize()

    def close(self):
        self._stop = True
        self._go.set()
        self._thread.join(timeout=5)


class SparseHost:
    """Pinned host side of one sparse key of a PackedFeed: the packed planes of a batch of B scenes of n elements.  `vals` holds the
    dense worst case (B n words); `count` is how many of them the current batch uses -- the feed uploads only those.  A loader either
    calls fill(x) or writes mask / offs / val_base / vals / count itself (between wait_uploaded() and the next land())."""

    def __init__(self, B, n):
        if n % 32 or B * n >= 1 << 32:
            raise ValueError(f'SparseHost: {B} x {n} elements, a multiple of 32 per scene and fewer than 2^32 only')
        self.B, self.n, self.nblk = B, n, -(-n // SPARSE_BLOCK)
        self.mask, self.offs = _pinned_words(B * n // 32), _pinned_words(B * (self.nblk + 1))
        self.val_base, self.vals = _pinned_words(B + 1), _pinned_words(B * n)
        for t in (self.mask, self.offs, self.val_base):
            t.zero_()
        self.count = 0

    def fill(self, x):
        """x: [B, ...] float32 (array or CPU tensor), n elements per scene -> packed in place."""
        x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        x = np.ascontiguousarray(x).reshape(self.B, self.n)
        base = np.zeros(self.B + 1, np.int64)
        for b in range(self.B):
            m, o, v = pack_sparse(x[b])
            _put(self.mask, b * (self.n // 32), m); _put(self.offs, b * (self.nblk + 1), o); _put(self.vals, int(base[b]), v)
            base[b + 1] = base[b] + v.size
        _put(self.val_base, 0, base.astype(np.uint32))
        self.count = int(base[-1])
        return self

    def parts(self):
        return {'mask': self.mask, 'offs': self.offs, 'val_base': self.val_base, 'vals': self.vals}

    @property
    def nbytes(self):
        """Bytes the feed uploads for the current batch."""
        return 4 * (self.mask.numel() + self.offs.numel() + self.val_base.numel() + self.count)


def bits_host(x):
    """[B, ...] array / CPU tensor (non-zero = True), a multiple of 32 elements per scene -> pinned int32 words for a 'bits' key."""
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if x[0].size % 32:
        raise ValueError(f'bits_host: {x[0].size} elements per scene, a multiple of 32 only')
    w = pack_bits(x)
    h = _pinned_words(w.size)
    _put(h, 0, w)
    return h


class PackedFeed(HostFeed):
    """HostFeed whose host side may be packed: same protocol (start / land / wait_uploaded / close), same worker thread, copy stream
    and 1.5 MB pieces; works on GraphedTrainStep.static and GraphedForward.static alike.

        feed = PackedFeed(step.static, host, packed={'ogm': 'bits', 'flow': 'sparse'}, raw={'map_img': 'int8'})

    host[k] for a 'bits' key: pinned int32 words (bits_host; pack_bits of the batch, static[k].numel() / 32 of them); for a 'sparse' key:
    a SparseHost -- its mask, offs and val_base are uploaded whole and of `vals` only the first `count` words, read when the upload
    starts.  land() expands both into static[k] (stj_unpack_bits / stj_unpack_sparse); the other keys behave as in HostFeed."""

    def __init__(self, static, host, packed=None, raw=None, chunk_bytes=3 << 19):
        self.packed = {k: v for k, v in (packed or {}).items() if k in static and k in host}
        for k, kind in self.packed.items():
            B, numel = static[k].shape[0], static[k].numel()
            if kind == 'bits':
                if (numel // B) % 32 or host[k].numel() * host[k].element_size() * 8 != numel:
                    raise ValueError(f'PackedFeed: host[{k!r}] must hold {numel} bits, a multiple of 32 per scene')
            elif kind == 'sparse':
                if not isinstance(host[k], SparseHost) or (host[k].B, host[k].n) != (B, numel // B):
                    raise ValueError(f'PackedFeed: host[{k!r}] must be a SparseHost({B}, {numel // B})')
            else:
                raise ValueError(f'PackedFeed: packed kind {kind!r}')
        self.sparse = {k: host[k] for k, kind in self.packed.items() if kind == 'sparse'}
        self._n_vals = {k: 0 for k in self.sparse}
        super().__init__(static, {k: h for k, h in host.items() if k not in self.sparse}, raw, chunk_bytes)
        for k, sh in self.sparse.items():
            for part, h in sh.parts().items():
                if not h.is_pinned():
                    raise ValueError(f'PackedFeed: host[{k!r}].{part} must be pinned memory')
        self.sparse_stage = {k: {part: torch.empty(h.shape, dtype=h.dtype, device=self.dev) for part, h in sh.parts().items()}
                             for k, sh in self.sparse.items()}
        self._landing = {**self.stage, **self.sparse_stage}                # the sparse keys land behind the others

    def _copies(self):
        super()._copies()
        for k, sh in self.sparse.items():
            count = min(int(sh.count), sh.vals.numel())
            self._n_vals[k] = count                                        # read by the land() of THIS batch, before the next upload starts
            for part, h in sh.parts().items():
                _copy_chunked(self.sparse_stage[k][part], h, count if part == 'vals' else h.numel(), self.chunk)

    def _expand(self, k, st, dst):
        kind = self.packed.get(k)
        if kind == 'bits':
            call('stj_unpack_bits', _p(st), _p(dst), dst.numel(), _st())
        elif kind == 'sparse':
            B = dst.shape[0]
            call('stj_unpack_sparse', _p(st['mask']), _p(st['offs']), _p(st['val_base']), _p(st['vals']), self._n_vals[k], _p(dst), B, dst.numel() // B, _st())
        else:
            super()._expand(k, st, dst)

    def upload_bytes(self):
        """Bytes the next upload moves, as the host buffers stand."""
        return sum(h.numel() * h.element_size() for h in self.host.values()) + sum(sh.nbytes for sh in self.sparse.values())


# ---------------------------------------------------------------------------------------------------- scenes resident in HBM
_KIND_NAME = {v: k for k, v in KIND.items()}
POOL_NAMES = {'ogm': 'ogm', 'map_image': 'map_img', 'actors': 'obs', 'occl_actors': 'occ', 'centerlines': 'mapt', 'vec_flow': 'flow',
              'gt_obs_ogm': 'gt_obs', 'gt_occ_ogm': 'gt_occ', 'gt_flow': 'gt_flow', 'origin_flow': 'origin_flow'}


def _scene_words(x):
    """uint32 words of an array or of a record's bytes; None unless whole 32-bit words."""
    b = np.ascontiguousarray(x).reshape(-1).view(np.uint8) if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), np.uint8)
    return None if b.size % 4 else b.view('<u4')


_Feature = collections.namedtuple('_Feature', 'name key entry kind n dtype shape crop scale')


def _feature_table(geometry, entries=None):
    """The record features of a geometry (grid, out, test, names) as a pool holds them, one _Feature per row of feature_spec: the record
    name, the pool key, the key's entry in `entries`, the kind PACKED_KIND gives it ('bits' / 'sparse' / 'raw'), n elements per scene after
    the centre crop, and feature_spec's dtype, shape, crop and scale.  With entries: ValueError naming the key unless its entry holds that
    kind and n and, for a raw key, that dtype with no crop (stj_pool_put_raw copies whole rows; no row of feature_spec is raw and
    cropped).  Without: entry is None and nothing is checked -- for the code that builds the entries."""
    grid, out, test, names = geometry
    for name, (dtype, shape, crop, scale) in feature_spec(grid, out, test).items():
        key = names.get(name, name)
        kind = PACKED_KIND.get(name, 'raw')
        n = int(np.prod(decoded_shape(shape, crop)))
        e = None
        if entries is not None:
            e = entries.get(key)
            if e is None or e['kind'] != kind or e['n'] != n or (kind == 'raw' and (e['dtype'] != dtype or crop is not None)):
                raise ValueError(f"PoolLayout[{key!r}]: holds {None if e is None else (e['kind'], e['n'], e.get('dtype'))}, the record feature "
                                 f"{name} gives {(kind, n, dtype if kind == 'raw' else None)}")
        yield _Feature(name, key, e, kind, n, dtype, shape, crop, scale)


def _packed_parts(ex, b, table):
    """The arrays of ONE pack_example record as a pool's keys hold them: [(key, parts)] with parts (words,) for a bits key, check_sparse's
    (mask, offs, vals) for a sparse key and (the record's own elements,) for a raw key; table: the checked _feature_table of the pool.
    ValueError naming key and scene `b` for a missing or malformed feature."""
    res = []
    for name, key, _, want, n, dtype, shape, crop, _ in table:
        try:
            if want == 'bits':
                w = _scene_words(ex[name + '/bits'])
                if w is None or w.size != n // 32:
                    raise ValueError(f"{len(ex[name + '/bits'])} bytes of bits, expected {n // 8}")
                parts = (w,)
            elif want == 'sparse':
                parts = check_sparse(*(ex[f'{name}/{p}'] for p in ('mask', 'offs', 'vals')), n, 'stream')
            else:
                parts = (np.ascontiguousarray(_decoded(ex[name], dtype, shape, crop)).reshape(-1),)
        except KeyError as err:
            raise ValueError(f'PoolLayout[{key!r}] scene {b}: the record lacks the feature {err}') from None
        except (ValueError, TypeError) as err:
            raise ValueError(f'PoolLayout[{key!r}] scene {b}: {err}') from None
        res.append((key, parts))
    return res


class PoolLayout:
    """N packed scenes laid out as stj_gather_bits / stj_gather_sparse / stj_gather_raw read them; NumPy only, no device.

    A key (any string; PackedFeed and ResidentFeed work on the keys of a step's `static` dict) holds one feature of every scene:
      bits    words  uint32 [N, n / 32] in pack_bits' order;
      sparse  mask   uint32 [N, n / 32], offs uint32 [N, ceil(n / SPARSE_BLOCK) + 1] relative to the scene, val_base int64 [N + 1] the running
              total of the scenes' value words (64-bit: a pool's can pass 2^32 although a batch's cannot), vals uint32 [val_base[-1]];
      raw     the record's own elements [N, n] (bool / int8 / float32 / float64) and the scale of feature_spec.
    Every key holds the same number of scenes.  Malformed streams, scenes of differing size, a key added twice and differing scene counts
    raise ValueError naming the key and the scene.  reference_gather states what the kernels compute."""

    def __init__(self):
        self.entries = {}          # key -> {'kind': 'bits' | 'sparse' | 'raw', 'n', 'shape', arrays ...}
        self.N = None
        self.geometry = None       # (grid, out, test, names) of from_examples / empty: what a PoolWriter needs to read raw records
        self.device_only = False   # ResidentPool.empty: the entries hold 'parts' {name: (shape, dtype)} and no arrays

    def _begin(self, key, scenes):
        if key in self.entries:
            raise ValueError(f'PoolLayout[{key!r}]: key added twice')
        scenes = list(scenes)
        if self.N is not None and len(scenes) != self.N:
            raise ValueError(f'PoolLayout[{key!r}]: {len(scenes)} scenes where the other keys hold {self.N}: '
                             f'scene {min(len(scenes), self.N)} is the first without a partner')
        if not scenes:
            raise ValueError(f'PoolLayout[{key!r}]: no scene 0: an empty pool')
        return scenes

    def _end(self, key, N, n, shape, entry):
        shape = (n,) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(shape)) != n:
            raise ValueError(f'PoolLayout[{key!r}]: shape {shape} does not hold the {n} elements of scene 0')
        if n >= 1 << 32:
            raise ValueError(f'PoolLayout[{key!r}]: scene 0 has {n} elements, fewer than 2^32 only')
        self.entries[key] = dict(entry, n=n, shape=shape)
        self.N = N

    def add_bits(self, key, scenes, shape=None):
        """scenes: per scene the pack_bits words (uint32 array) or the record's `<name>/bits` bytes; n = 32 x the words of scene 0."""
        scenes = self._begin(key, scenes)
        words = []
        for i, s in enumerate(scenes):
            w = _scene_words(s)
            if w is None:
                raise ValueError(f'PoolLayout[{key!r}] scene {i}: bits are not whole 32-bit words')
            if words and w.size != words[0].size:
                raise ValueError(f'PoolLayout[{key!r}] scene {i}: {w.size} words, scene 0 has {words[0].size}')
            words.append(w)
        self._end(key, len(words), 32 * words[0].size, shape, {'kind': 'bits', 'words': np.stack(words).astype(np.uint32)})
        return self

    def add_sparse(self, key, scenes, n, shape=None, capacity=None):
        """scenes: per scene (mask, offs, vals) of n elements, arrays or the record's bytes; each checked with check_sparse.  capacity: None
        lays the value words out tight (val_base the running total); an int gives every slot that many value words, val_base =
        arange(N + 1) * capacity, the unused tail of a slot zero -- room for PoolLayout.replace_reference / PoolWriter to put another
        scene there.  ValueError naming key and scene if a scene holds more."""
        scenes = self._begin(key, scenes)
        planes = []
        for i, s in enumerate(scenes):
            try:
                planes.append(check_sparse(*s, n, 'stream'))
            except (ValueError, TypeError) as e:
                raise ValueError(f'PoolLayout[{key!r}] scene {i}: {e}') from None
        if capacity is None:
            base = np.zeros(len(planes) + 1, np.int64)
            base[1:] = np.cumsum([p[2].size for p in planes], dtype=np.int64)
            vals = np.concatenate([p[2] for p in planes]).astype(np.uint32)
        else:
            capacity = int(capacity)
            if capacity < 0:
                raise ValueError(f'PoolLayout[{key!r}]: capacity {capacity}')
            for i, p in enumerate(planes):
                if p[2].size > capacity:
                    raise ValueError(f'PoolLayout[{key!r}] scene {i}: {p[2].size} value words, the slots hold {capacity}')
            base = np.arange(len(planes) + 1, dtype=np.int64) * capacity
            vals = np.zeros(len(planes) * capacity, np.uint32)
            for i, p in enumerate(planes):
                vals[base[i]:base[i] + p[2].size] = p[2]
        self._end(key, len(planes), int(n), shape, {'kind': 'sparse', 'mask': np.stack([p[0] for p in planes]).astype(np.uint32),
                                       'offs': np.stack([p[1] for p in planes]).astype(np.uint32), 'val_base': base, 'vals': vals})
        return self

    def add_raw(self, key, scenes, kind, scale=1.0, shape=None):
        """scenes: per scene the record's own elements, an array or bytes; kind: 'bool' / 'int8' / 'float32' / 'float64' or its code."""
        kind = _KIND_NAME.get(kind, kind)
        if kind not in KIND:
            raise ValueError(f'PoolLayout[{key!r}]: raw kind {kind!r}')
        scenes = self._begin(key, scenes)
        rows = []
        for i, s in enumerate(scenes):
            b = np.ascontiguousarray(s).reshape(-1).view(np.uint8) if isinstance(s, np.ndarray) else np.frombuffer(bytes(s), np.uint8)
            if b.size % ITEMSIZE[kind]:
                raise ValueError(f'PoolLayout[{key!r}] scene {i}: {b.size} bytes are not whole {kind} elements')
            if rows and b.size != rows[0].size:
                raise ValueError(f'PoolLayout[{key!r}] scene {i}: {b.size} bytes, scene 0 has {rows[0].size}')
            rows.append(b)
        data = np.stack(rows).view(_RAW_DTYPE[kind])
        self._end(key, len(rows), data.shape[1], shape, {'kind': 'raw', 'data': data, 'dtype': kind, 'scale': float(scale)})
        return self

    @classmethod
    def from_examples(cls, packed_examples, grid=512, out=256, test=False, names=None):
        """The layout of a list of pack_example records.  The packed features go in as packed, the others as the record's own bytes
        (map_image stays int8 with scale 1/256, the float64 agent arrays stay float64); a record that is not packed at all is accepted and
        stored raw, a ground-truth feature after its centre crop.  names: record name -> key; the default maps to the keys of a step's
        `static` dict (POOL_NAMES).  'scenario/id' is not a tensor and stays with the caller."""
        names = POOL_NAMES if names is None else names
        exs = list(packed_examples)
        self = cls()
        for name, key, _, kind, n, dtype, shape, crop, scale in _feature_table((grid, out, test, names)):
            dshape = decoded_shape(shape, crop)
            try:
                if kind == 'bits' and exs and name + '/bits' in exs[0]:
                    self.add_bits(key, [ex[name + '/bits'] for ex in exs], dshape)
                    if self.entries[key]['n'] != n:
                        raise ValueError(f"PoolLayout[{key!r}] scene 0: {self.entries[key]['n']} bits, expected {n}")
                elif kind == 'sparse' and exs and name + '/mask' in exs[0]:
                    self.add_sparse(key, [tuple(ex[f'{name}/{p}'] for p in ('mask', 'offs', 'vals')) for ex in exs], n, dshape)
                else:
                    rows = []
                    for i, ex in enumerate(exs):
                        try:
                            rows.append(np.ascontiguousarray(_decoded(ex[name], dtype, shape, crop)))
                        except ValueError as e:
                            raise ValueError(f'PoolLayout[{key!r}] scene {i}: {e}') from None
                    self.add_raw(key, rows, dtype, scale, dshape)
            except KeyError as e:
                raise ValueError(f'PoolLayout[{key!r}]: a scene lacks the record feature {e}') from None
        self.geometry = (grid, out, test, dict(names))
        return self

    @staticmethod
    def _empty_plan(N, grid, out, test, names, capacity):
        """What `empty` builds, without the arrays: [(key, entry, {part: (shape, dtype)})]; a sparse entry carries its 'capacity'."""
        names = POOL_NAMES if names is None else names
        capacity = dict(capacity or {})
        N = int(N)
        if N < 1:
            raise ValueError(f'PoolLayout.empty: {N} scenes: an empty pool')
        plan = []
        for name, key, _, kind, n, dtype, shape, crop, scale in _feature_table((grid, out, test, names)):
            dshape = decoded_shape(shape, crop)
            if kind != 'raw' and n % 32:
                raise ValueError(f'PoolLayout[{key!r}]: {n} elements per scene, a multiple of 32 only')
            if n >= 1 << 32:
                raise ValueError(f'PoolLayout[{key!r}]: {n} elements per scene, fewer than 2^32 only')
            if kind == 'bits':
                plan.append((key, {'kind': 'bits', 'n': n, 'shape': dshape}, {'words': ((N, n // 32), np.uint32)}))
            elif kind == 'sparse':
                cap = int(capacity.pop(key, n))
                if cap < 0:
                    raise ValueError(f'PoolLayout[{key!r}]: capacity {cap}')
                plan.append((key, {'kind': 'sparse', 'n': n, 'shape': dshape, 'capacity': cap},
                             {'mask': ((N, n // 32), np.uint32), 'offs': ((N, -(-n // SPARSE_BLOCK) + 1), np.uint32), 'val_base': ((N + 1,), np.int64),
                              'vals': ((N * cap,), np.uint32)}))
            else:
                plan.append((key, {'kind': 'raw', 'n': n, 'shape': dshape, 'dtype': dtype, 'scale': float(scale)},
                             {'data': ((N, n), np.dtype(_RAW_DTYPE[dtype]))}))
        if capacity:
            raise ValueError(f'PoolLayout.empty: capacity names {sorted(capacity)}, which are not sparse keys of the pool')
        return plan

    @classmethod
    def empty(cls, N, grid=512, out=256, test=False, names=None, capacity=None):
        """N all-zero scenes under the standard keys, to be filled by replace_reference (here) or by a PoolWriter (on the device): bits and
        sparse keys as PACKED_KIND says, the rest raw, as from_examples lays out packed records.  capacity: {key: value words per slot} for the
        sparse keys; a key that is not named gets n, the dense worst case, which can never reject a scene."""
        self = cls()
        for key, entry, parts in cls._empty_plan(N, grid, out, test, names, capacity):
            arrs = {p: np.zeros(shape, dt) for p, (shape, dt) in parts.items()}
            if entry['kind'] == 'sparse':
                arrs['val_base'] = np.arange(int(N) + 1, dtype=np.int64) * entry['capacity']
            self.entries[key] = dict(entry, **arrs)
        self.N = int(N)
        self.geometry = (grid, out, test, dict(POOL_NAMES if names is None else names))
        return self

    def replace_reference(self, slots, examples, grid=512, out=256, test=False, names=None):
        """The semantics of PoolWriter.put in NumPy.  examples: parsed, UNPACKED records (parse_example); scene b goes to slot slots[b].
        It is admitted iff 0 <= slots[b] < N and, for every sparse key, its present words fit the slot: count <= val_base[s + 1] -
        val_base[s].  An admitted scene replaces EVERY key of its slot -- bits words; mask, scene-relative offs and the present words
        written from val_base[s] on in element order (the slot's words behind them keep what they held); the raw rows -- and a scene that is
        not admitted changes no key of any slot.  -> [1 | 0] per scene.  Duplicate slots raise ValueError, and so does a record whose
        feature has the wrong length or a key whose kind is not the one `empty` gives it."""
        slots, examples = self._slot_list('replace_reference', slots, examples)
        table = list(_feature_table((grid, out, test, POOL_NAMES if names is None else names), self.entries))
        landed = []
        for b, (s, ex) in enumerate(zip(slots, examples)):
            new = []
            for name, key, _, kind, _, dtype, shape, crop, _ in table:
                try:
                    a = np.ascontiguousarray(_decoded(ex[name], dtype, shape, crop))
                except (ValueError, KeyError) as err:
                    raise ValueError(f'PoolLayout[{key!r}] scene {b}: {err}') from None
                new.append((key, (pack_bits(a),) if kind == 'bits' else pack_sparse(a) if kind == 'sparse' else (a.reshape(-1),)))
            landed.append(self._write_slot(s, new))
        return landed

    @staticmethod
    def _slot_list(who, slots, examples):
        slots, examples = [int(s) for s in slots], list(examples)
        if len(slots) != len(examples):
            raise ValueError(f'{who}: {len(slots)} slots for {len(examples)} scenes')
        if len(set(slots)) != len(slots):
            raise ValueError(f'{who}: duplicate slots in {slots}')
        return slots, examples

    def _write_slot(self, s, new):
        """new: [(key, parts)] of one scene, parts as _packed_parts gives them.  -> 1 with every key of slot s replaced, or 0 with nothing
        changed: a slot outside [0, N), or a sparse key with more value words than the slot holds."""
        if not 0 <= s < self.N:
            return 0
        for key, parts in new:
            e = self.entries[key]
            if e['kind'] == 'sparse' and parts[2].size > int(e['val_base'][s + 1] - e['val_base'][s]):
                return 0
        for key, parts in new:
            e = self.entries[key]
            if e['kind'] == 'bits':
                e['words'][s] = parts[0]
            elif e['kind'] == 'sparse':
                v0 = int(e['val_base'][s])
                e['mask'][s], e['offs'][s] = parts[0], parts[1]
                e['vals'][v0:v0 + parts[2].size] = parts[2]
            else:
                e['data'][s] = parts[0]
        return 1

    def replace_packed_reference(self, slots, packed_examples, grid=512, out=256, test=False, names=None):
        """replace_reference for records that pack_example has already rewritten: the semantics of PoolWriter.put_packed and of a
        ShuffleWindow's refill in NumPy.  Scene b goes to slot slots[b]; it is admitted iff 0 <= slots[b] < N and, for every sparse key,
        offs[-1] <= val_base[s + 1] - val_base[s]; all-or-nothing across keys, and what an admitted scene writes is what replace_reference
        writes, so replace_packed_reference(slots, [pack_example(e)]) leaves the layout byte-identical to replace_reference(slots, [e]).
        Every sparse stream is validated with check_sparse: a malformed record raises ValueError naming key and scene, before any slot
        changes.  -> [1 | 0] per scene."""
        slots, examples = self._slot_list('replace_packed_reference', slots, packed_examples)
        table = list(_feature_table((grid, out, test, POOL_NAMES if names is None else names), self.entries))
        plan = [_packed_parts(ex, b, table) for b, ex in enumerate(examples)]
        return [self._write_slot(s, new) for s, new in zip(slots, plan)]

    def check_index(self, idx):
        """A host index list: ValueError unless every index is in [0, N).  -> int64 array."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        bad = np.flatnonzero((idx < 0) | (idx >= self.N))
        if bad.size:
            raise ValueError(f'pool index {int(idx[bad[0]])} at position {int(bad[0])} is outside the {self.N} scenes')
        return idx

    def reference_gather(self, idx):
        """The semantics of the gather kernels in NumPy, built on unpack_reference: {key: float32 [B, ...]}, scene b of every key being
        pool scene clamp(idx[b], 0, N - 1) -- the kernels clamp, so that no index reads outside the pool."""
        idx = np.clip(np.asarray(idx, np.int64).reshape(-1), 0, self.N - 1)
        res = {}
        for key, e in self.entries.items():
            rows = []
            for s in idx:
                if e['kind'] == 'bits':
                    r = unpack_reference('bits', e['words'][s], e['n'])
                elif e['kind'] == 'sparse':
                    v0 = int(e['val_base'][s])                   # a slot may have slack behind its offs[s][-1] value words
                    r = unpack_reference('sparse', e['mask'][s], e['offs'][s], e['vals'][v0:v0 + int(e['offs'][s][-1])], e['n'])
                else:
                    a = e['data'][s]
                    a = a.view(np.float32) if e['dtype'] == 'float32' else (a != 0) if e['dtype'] == 'bool' else a
                    r = a.astype(np.float32) * np.float32(e['scale'])
                rows.append(r.reshape(e['shape']))
            res[key] = np.stack(rows) if rows else np.zeros((0,) + e['shape'], np.float32)
        return res

    def arrays(self, key):
        """The arrays of a key that go to the device, by name."""
        e = self.entries[key]
        return {p: e[p] for p in {'bits': ('words',), 'sparse': ('mask', 'offs', 'val_base', 'vals'), 'raw': ('data',)}[e['kind']]}

    @property
    def nbytes(self):
        """Bytes the pool occupies on the device."""
        if self.device_only:
            return sum(int(np.prod(shape)) * np.dtype(dt).itemsize for e in self.entries.values() for shape, dt in e['parts'].values())
        return sum(a.nbytes for key in self.entries for a in self.arrays(key).values())


class PoolSampler:
    """Endless iterator over batches of pool indices: int32 tensors on `device`, made there, never synchronising with the host.  With
    shuffle every epoch is torch.randperm(N) of the sampler's own generator cut into batches -- a full permutation of the resident scenes,
    not the reference's 64-scene shuffle buffer (train.py:381); without, the scenes run in order.  drop_last=False keeps the shorter last
    batch of an epoch (ResidentPool.gather takes it, ResidentFeed.land refuses it).  Under data parallelism each rank builds its pool
    from its own share of the records and shuffles within it.  epoch() returns the batches of the next whole epoch."""

    def __init__(self, N, batch_size, device='cuda', shuffle=True, seed=0, drop_last=True):
        if N < 1 or batch_size < 1 or (drop_last and batch_size > N):
            raise ValueError(f'PoolSampler: no batch of {batch_size} out of {N} scenes')
        self.N, self.batch_size, self.shuffle, self.drop_last = int(N), int(batch_size), shuffle, drop_last
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device).manual_seed(int(seed))
        self._order = None if shuffle else torch.arange(self.N, dtype=torch.int32, device=self.device)
        self._todo = []

    def __len__(self):
        return self.N // self.batch_size if self.drop_last else -(-self.N // self.batch_size)

    def epoch(self):
        order = torch.randperm(self.N, dtype=torch.int32, device=self.device, generator=self.gen) if self.shuffle else self._order
        self._todo = []
        return list(order.split(self.batch_size))[:len(self)]

    def __iter__(self):
        return self

    def __next__(self):
        if not self._todo:
            self._todo = self.epoch()[::-1]
        return self._todo.pop()


class ResidentPool:
    """A PoolLayout uploaded once and kept in HBM; batches are gathered from it by an index vector that lives on the device
    (stj_gather_bits / stj_gather_sparse / stj_gather_raw: one launch per key, no upload, no worker thread).

        pool = ResidentPool(PoolLayout.from_examples(packed, grid, out, test), 'cuda')
        batch = pool.gather(idx)                 # the dict decode_batch_packed gives for those scenes (keys: the layout's)
        pool.gather_into(step.static, idx)       # into existing tensors; keys the pool does not hold stay untouched

    The upload goes through pinned staging on the process's one copy stream in pieces of chunk_bytes (HostFeed explains why one large copy
    is wrong while a step is running); an event marks it done and the first gather waits on it.  idx: a device int32 tensor, trusted
    because the kernels clamp it to the pool, or a host list, range-checked (ValueError).
    Scenes are replaced in place from the reference's own unpacked records: ResidentPool.empty(N, ...) allocates zero-filled slots (a sparse
    key's slot holds `capacity` value words), pool.writer(B) returns a PoolWriter whose put(slots, examples) uploads the raw bytes and packs
    them on the device (stj_pack_bits / stj_pack_sparse_* / stj_pool_put_raw) -- a rolling window over a dataset larger than HBM.
    put_packed(slots, packed_examples) does the same from records that are already packed (a scatter copy with no packing), and
    pool.window(B, source) is a ShuffleWindow: consumed slots refilled on a stream of its own while the step runs."""

    def __init__(self, layout, device='cuda', chunk_bytes=3 << 19):
        dev = _hip_device('ResidentPool', device)
        if not layout.entries:
            raise ValueError('ResidentPool: an empty layout')
        self.layout, self.dev, self.N = layout, dev, layout.N
        self.dev_arrays, self._staging = {key: {} for key in layout.entries}, []
        self.up, self._ready = torch.cuda.Event(), False
        if layout.device_only:                       # ResidentPool.empty: no host arrays, zero-filled here
            for key, e in layout.entries.items():
                for part, (shape, dt) in e['parts'].items():
                    nb = int(np.prod(shape)) * np.dtype(dt).itemsize
                    if part == 'val_base':
                        d = (torch.arange(self.N + 1, dtype=torch.int64, device=dev) * e['capacity']).view(torch.uint8)
                    else:
                        d = torch.zeros((max(nb, 8),), dtype=torch.uint8, device=dev)          # never empty: a real pointer
                    self.dev_arrays[key][part] = d
            self.up.record(torch.cuda.current_stream(dev))
        else:
            copy = _copy_stream(dev)
            with torch.cuda.stream(copy):
                for key in layout.entries:
                    for part, a in layout.arrays(key).items():
                        nb = a.nbytes
                        host = torch.empty((max(nb, 8),), dtype=torch.uint8).pin_memory()
                        host.numpy()[:nb] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
                        d = torch.empty((max(nb, 8),), dtype=torch.uint8, device=dev)          # never empty: a real pointer
                        _copy_chunked(d, host, nb, int(chunk_bytes))
                        self._staging.append(host)
                        self.dev_arrays[key][part] = d
                self.up.record(copy)

    @classmethod
    def from_examples(cls, packed_examples, device='cuda', grid=512, out=256, test=False, names=None, chunk_bytes=3 << 19):
        return cls(PoolLayout.from_examples(packed_examples, grid, out, test, names), device, chunk_bytes)

    @classmethod
    def empty(cls, N, device='cuda', grid=512, out=256, test=False, names=None, capacity=None):
        """ResidentPool(PoolLayout.empty(...)) without the host copy: the same arrays allocated on the device, zero-filled there (val_base
        computed there).  pool.layout then describes the keys (kind, n, shape, capacity) and holds no arrays."""
        lay = PoolLayout()
        lay.device_only, lay.N = True, int(N)
        lay.geometry = (grid, out, test, dict(POOL_NAMES if names is None else names))
        for key, entry, parts in PoolLayout._empty_plan(N, grid, out, test, names, capacity):
            lay.entries[key] = dict(entry, parts=parts)
        return cls(lay, device)

    def _n_vals(self, key):
        e = self.layout.entries[key]
        return self.N * e['capacity'] if self.layout.device_only else int(e['val_base'][-1])

    def writer(self, B, chunk_bytes=3 << 19):
        """A PoolWriter for B scenes per put: every buffer it needs, allocated once."""
        return PoolWriter(self, B, chunk_bytes)

    @property
    def nbytes(self):
        return self.layout.nbytes

    def wait(self):
        """Host-side: returns once the upload has finished (call it before capturing gathers in a graph)."""
        self.up.synchronize()
        self._ready, self._staging = True, []

    def _await_upload(self):
        if self._ready:
            return
        if self.up.query():
            self._ready, self._staging = True, []
        elif torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ResidentPool: the upload has not finished; call pool.wait() before capturing a gather')
        else:
            torch.cuda.current_stream(self.dev).wait_event(self.up)

    def index(self, idx):
        """idx as the kernels take it: a device int32 tensor is trusted (the kernels clamp); a host list is range-checked and copied."""
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
                raise ValueError(f'pool index: a contiguous int32 [B] device tensor only, got {idx.dtype} {tuple(idx.shape)}')
            return idx
        host = self.layout.check_index(idx.tolist() if isinstance(idx, torch.Tensor) else idx)
        return torch.from_numpy(host.astype(np.int32)).to(self.dev)

    def _launch(self, key, dst, idx):
        e, d = self.layout.entries[key], self.dev_arrays[key]
        B, n = idx.numel(), e['n']
        if e['kind'] == 'bits':
            call('stj_gather_bits', _p(d['words']), _p(idx), self.N, _p(dst), B, n, _st())
        elif e['kind'] == 'sparse':
            call('stj_gather_sparse', _p(d['mask']), _p(d['offs']), _p(d['val_base']), _p(d['vals']), self._n_vals(key), _p(idx), self.N,
                 _p(dst), B, n, _st())
        else:
            call('stj_gather_raw', _p(d['data']), KIND[e['dtype']], _p(idx), self.N, _p(dst), B, n, e['scale'], _st())

    def gather(self, idx):
        """-> {key: float32 [B, ...]} freshly allocated: what decode_batch_packed returns for the scenes idx."""
        idx = self.index(idx)
        self._await_upload()
        res = {}
        for key, e in self.layout.entries.items():
            res[key] = torch.empty((idx.numel(),) + e['shape'], dtype=torch.float32, device=self.dev)
            self._launch(key, res[key], idx)
        return res

    def gather_into(self, static, idx):
        """The same into the tensors of `static` (float32, contiguous, [B] + the key's shape); keys the pool does not hold are left alone."""
        idx = self.index(idx)
        todo = self.check_static(static, idx.numel())
        self._await_upload()
        for key in todo:
            self._launch(key, static[key], idx)

    def check_static(self, static, B):
        """ValueError unless every tensor of `static` under a key of the pool is what a gather of B scenes writes.  -> those keys."""
        todo = [key for key in self.layout.entries if key in static]
        for key in todo:
            t, want = static[key], (B,) + self.layout.entries[key]['shape']
            if t.dtype != torch.float32 or tuple(t.shape) != want or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f'ResidentPool: static[{key!r}] is {t.dtype} {tuple(t.shape)} on {t.device}, expected contiguous float32 {want} on {self.dev}')
        return todo

    def sampler(self, batch_size, shuffle=True, seed=0, drop_last=True):
        """PoolSampler over this pool's scenes, on its device."""
        return PoolSampler(self.N, batch_size, self.dev, shuffle, seed, drop_last)

    def window(self, batch_size, source, **kw):
        """ShuffleWindow(self, batch_size, source, **kw): this pool as the shuffle buffer of a stream of records."""
        return ShuffleWindow(self, batch_size, source, **kw)


class ResidentFeed:
    """HostFeed's protocol (start / land / wait_uploaded / close) over a ResidentPool: nothing is uploaded per step, so there is no worker
    thread and wait_uploaded() returns at once.  Works on GraphedTrainStep.static, GraphedForward.static and GraphedEvalStep.static.

        feed = ResidentFeed(step.static, pool)
        feed.start()
        for ...:
            feed.land()                    # next batch of the feed's sampler; or feed.land(idx)
            step(); optimizer.step()

    feed.idx is a persistent device int32 [B] tensor: land(idx) copies idx into it on the current stream and launches the gathers, which
    read feed.idx -- so a caller may capture the launches in a graph of their own and change feed.idx between replays.  The landing stays
    in front of the step's replay, as HostFeed's does."""

    def __init__(self, static, pool, sampler=None):
        self.static, self.pool = static, pool
        keys = [k for k in pool.layout.entries if k in static]
        if not keys:
            raise ValueError('ResidentFeed: the pool holds none of the keys of `static`')
        self.B = static[keys[0]].shape[0]
        self.idx = torch.zeros((self.B,), dtype=torch.int32, device=pool.dev)
        self.sampler = sampler
        pool.check_static(static, self.B)

    def start(self):
        pass

    def land(self, idx=None):
        if idx is None:
            if self.sampler is None:
                self.sampler = self.pool.sampler(self.B)
            idx = next(self.sampler)
        idx = self.pool.index(idx)
        if idx.numel() != self.B:
            raise ValueError(f'ResidentFeed: {idx.numel()} indices for a static batch of {self.B}')
        self.idx.copy_(idx, non_blocking=True)
        self.pool.gather_into(self.static, self.idx)

    def wait_uploaded(self):
        return

    def close(self):
        pass


class PoolWriter:
    """Replaces B scenes of a ResidentPool in place from the reference's own UNPACKED records (parse_example output): the raw bytes go up
    once and are centre-cropped, bit-packed or stream-compacted on the device, straight into the pool's slots.

        pool = ResidentPool.empty(N, 'cuda', grid, out, test, capacity={'flow': ..., 'gt_flow': ..., 'origin_flow': ...})
        writer = pool.writer(B)
        ok = writer.put(slots, examples)         # device int32 [B]: 1 = the scene landed in slots[b], 0 = the pool is unchanged for it

    PoolLayout.replace_reference states the semantics: a scene lands with every key or with none (a slot outside [0, N), or a sparse key
    whose present words exceed the slot's capacity, rejects it).  Everything is allocated once: pinned staging and the device buffers
    writer.raw[record name] (uint8 [B, nbytes]), the offs_stage workspace of every sparse key, writer.ok and the persistent writer.slots
    (device int32 [B]).  put() stages the records through pinned memory on the process's copy stream in pieces of chunk_bytes (HostFeed
    explains why), lets the current stream wait for them and calls commit().  commit() only launches, on the CURRENT stream -- so it is
    ordered against that stream's gathers and is capturable in a graph (fill writer.raw[...] and writer.slots between replays): the counts
    of every sparse key, the admits, then the commit of every key.  It never waits for the device.  slots: a host list is range- and
    duplicate-checked (ValueError); a device int32 [B] tensor is trusted -- the kernels skip a slot outside the pool and report ok = 0;
    duplicates in it are the caller's error.  The host arrays of pool.layout, where it has any, are not updated.
    The writer is one upload handshake and the slots / ok tensors over a staging (_Stage): writer.unpacked for put / stage / commit (it owns
    features, raw and offs_stage) and writer.packed for the *_packed twins."""

    def __init__(self, pool, B, chunk_bytes=3 << 19):
        self.pool, self.B, self.dev, self.chunk = pool, int(B), pool.dev, max(1, int(chunk_bytes))
        if self.B < 0:
            raise ValueError(f'PoolWriter: B {B}')
        self.unpacked = _RawStage(pool, self.B, self.chunk)         # the staging of put / stage / commit
        self.packed = None                                          # of put_packed / stage_packed / commit_packed: built on first use
        self.features, self.raw, self.offs_stage = self.unpacked.features, self.unpacked.raw, self.unpacked.offs_stage
        rows = max(self.B, 1)                      # never empty: a real pointer, also with B = 0
        self.ok = torch.zeros((rows,), dtype=torch.int32, device=self.dev)[:self.B]
        self.slots = torch.zeros((rows,), dtype=torch.int32, device=self.dev)[:self.B]
        self.copy = _copy_stream(self.dev)

    def packed_stage(self):
        """writer.packed, built on first use: its check(record, b) gives what stage_packed takes."""
        if self.packed is None:
            self.packed = _PackedStage(self.pool, self.B, self.chunk)
        return self.packed

    def _set_slots(self, slots):
        if isinstance(slots, torch.Tensor) and slots.is_cuda:
            if slots.dtype != torch.int32 or tuple(slots.shape) != (self.B,) or not slots.is_contiguous():
                raise ValueError(f'PoolWriter: slots must be a contiguous int32 [{self.B}] device tensor, got {slots.dtype} {tuple(slots.shape)}')
            if slots.data_ptr() != self.slots.data_ptr():
                self.slots.copy_(slots, non_blocking=True)
            return
        host = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
        if len(host) != self.B:
            raise ValueError(f'PoolWriter: {len(host)} slots for a writer of {self.B} scenes')
        self.pool.layout.check_index(host)
        if len(set(host)) != len(host):
            raise ValueError(f'PoolWriter: duplicate slots in {host}')
        if self.B:
            self.slots.copy_(torch.tensor(host, dtype=torch.int32))

    # ---- the three steps, over either stage
    def _checked(self, st, examples):
        examples = list(examples)
        if len(examples) != self.B:
            raise ValueError(f'PoolWriter: {len(examples)} records for a writer of {self.B} scenes')
        return [st.check(ex, b) for b, ex in enumerate(examples)]

    def _stage(self, st, parsed):
        """The upload handshake: the pinned side of `st` is free once its previous upload has left it (a host wait on the copy alone); the
        copy stream starts behind whatever read the device staging before (the previous commit, on the current stream); the current
        stream waits for the copies (a device-side wait)."""
        if len(parsed) != self.B:
            raise ValueError(f'PoolWriter: {len(parsed)} records for a writer of {self.B} scenes')
        if st.pending:
            st.up.synchronize()
        st.begin()
        for b, p in enumerate(parsed):
            st.fill(b, p)
        main = torch.cuda.current_stream(self.dev)
        st.done.record(main)
        with torch.cuda.stream(self.copy):
            self.copy.wait_event(st.done)
            st.upload(self.B)
            st.up.record(self.copy)
        st.pending = True
        main.wait_event(st.up)

    def _commit(self, st, slots):
        if slots is not None:
            self._set_slots(slots)
        self.pool._await_upload()
        st.launch(_p(self.slots), self.B, _p(self.ok))
        return self.ok

    def _put(self, st, slots, examples):
        parsed = self._checked(st, examples)
        self._set_slots(slots)
        self._stage(st, parsed)
        return self._commit(st, None)

    def put(self, slots, examples):
        """examples: B parsed unpacked records ({feature: bytes}); scene b replaces pool slot slots[b].  -> writer.ok."""
        return self._put(self.unpacked, slots, examples)

    def stage(self, examples):
        """The upload half of put(): the records' bytes into writer.raw through pinned memory on the copy stream; the current stream waits
        for them (a device-side wait), so a commit() issued next on it packs these records."""
        self._stage(self.unpacked, self._checked(self.unpacked, examples))

    def commit(self, slots=None):
        """Packs what writer.raw holds into the slots writer.slots names (slots: copied there first).  Launches only, on the current stream."""
        return self._commit(self.unpacked, slots)

    # ---- records that pack_example has already rewritten: a scatter copy with no packing
    def put_packed(self, slots, packed_examples):
        """put() for B pack_example records: the packed planes go up as they are stored (a sparse plane: only its used words) and are
        copied into the slots -- stj_pool_admit_packed per sparse key, then stj_pool_put_raw for the fixed-length rows and stj_pool_put_vals
        for the value words.  PoolLayout.replace_packed_reference states the semantics.  Every stream is checked on the host first
        (check_sparse; ValueError naming key and scene, nothing launched).  -> writer.ok."""
        return self._put(self.packed_stage(), slots, packed_examples)

    def stage_packed(self, parsed):
        """The upload half of put_packed(): parsed = [writer.packed.check(record, b)] into the device staging writer.packed.dev through
        pinned memory on the copy stream; the current stream waits for it."""
        self._stage(self.packed_stage(), parsed)

    def commit_packed(self, slots=None):
        """Copies what writer.packed.dev holds into the slots writer.slots names.  Launches only, on the current stream: capturable like
        commit() (stage_packed() between replays)."""
        return self._commit(self.packed_stage(), slots)


class _Stage:
    """The staging of up to B records on their way into the slots of a pool, allocated once: what a PoolWriter holds per kind of record and
    a ShuffleWindow twice.  _RawStage takes the reference's unpacked records, _PackedStage those pack_example has rewritten; both have
    check(record, b)       one record validated on the host -> what fill() takes; ValueError naming the feature and scene b;
    misfit(parsed)         None, or why no slot of the pool holds this record: a sparse key with more value words than a slot's capacity;
    begin(), fill(b, parsed)     write the pinned side, scene by scene from 0;
    upload(count)          the first `count` scenes to the device twins, in copies of at most chunk_bytes on the current stream;
    launch(slots, count, ok)     slots, ok: device pointers (int32 [count]); the kernels, on the current stream: every admit runs before
                           anything is written, so ok is final before the pool changes.
    up / done / pending are the PoolWriter's handshake around upload(), one per stage."""

    def __init__(self, pool, B, chunk_bytes):
        lay = pool.layout
        if lay.geometry is None:
            raise ValueError('PoolWriter: a pool laid out by PoolLayout.empty / from_examples (or ResidentPool.empty) only: the keys of a '
                             'hand-built layout do not say which record feature they hold')
        self.pool, self.B, self.dev, self.chunk = pool, int(B), pool.dev, max(1, int(chunk_bytes))
        self.geometry = lay.geometry
        self.feats = list(_feature_table(lay.geometry, lay.entries))
        self.capacity = {f.key: int(f.entry['capacity']) if lay.device_only else int(np.diff(f.entry['val_base']).min())
                         for f in self.feats if f.kind == 'sparse'}
        self.up, self.done, self.pending = torch.cuda.Event(), torch.cuda.Event(), False

    def begin(self):
        pass


class _RawStage(_Stage):
    """_Stage for parse_example records as the reference writes them: pinned rows and their device twins stage.raw[record name]
    (uint8 [B, nbytes]), the offs_stage workspace of every sparse key; the kernels crop, bit-pack and stream-compact on the device."""

    def __init__(self, pool, B, chunk_bytes=3 << 19):
        super().__init__(pool, B, chunk_bytes)
        self.features = []                         # (record name, key, entry, nbytes, (T, H, W, C, y0, x0, Ho, Wo))
        for f in self.feats:
            total = int(np.prod(f.shape))
            geom = (1, 1, total, 1, 0, 0, 1, total) if f.crop is None else tuple(f.shape) + tuple(f.crop)
            self.features.append((f.name, f.key, f.entry, total * ITEMSIZE[f.dtype], geom))
        rows = max(self.B, 1)                      # never empty: a real pointer, also with B = 0
        self.host = {f[0]: torch.empty((rows, f[3]), dtype=torch.uint8).pin_memory() for f in self.features}
        self.raw = {f[0]: torch.zeros((rows, f[3]), dtype=torch.uint8, device=self.dev)[:self.B] for f in self.features}
        self.offs_stage = {key: torch.zeros((rows, -(-e['n'] // SPARSE_BLOCK) + 1), dtype=torch.int32, device=self.dev)
                           for _, key, e, _, _ in self.features if e['kind'] == 'sparse'}

    def check(self, ex, b=0):
        for name, _, _, nbytes, _ in self.features:
            if name not in ex or len(ex[name]) != nbytes:
                raise ValueError(f"feature {name} of scene {b}: {len(ex[name]) if name in ex else 'no'} bytes, expected {nbytes}")
        return ex

    def misfit(self, ex):
        for f in self.feats:
            if f.kind == 'sparse':
                count = int(np.count_nonzero(_decoded(ex[f.name], f.dtype, f.shape, f.crop)))
                if count > self.capacity[f.key]:
                    return f'{f.key}: {count} value words, a slot holds {self.capacity[f.key]}'
        return None

    def fill(self, b, ex):
        for name in self.host:
            self.host[name].numpy()[b] = np.frombuffer(ex[name], np.uint8)

    def upload(self, count):
        for name, _, _, nbytes, _ in self.features:
            _copy_chunked(self.raw[name].view(-1), self.host[name].view(-1), count * nbytes, self.chunk)

    def launch(self, slots, count, ok):
        """The counts of every sparse key, the admits, then the commit of every key."""
        N, st, arrs = self.pool.N, _st(), self.pool.dev_arrays
        sparse = [f for f in self.features if f[2]['kind'] == 'sparse']
        for name, key, e, _, geom in sparse:
            call('stj_pack_sparse_count', _p(self.raw[name]), _p(self.offs_stage[key]), count, *geom, st)
        for i, (name, key, e, _, geom) in enumerate(sparse):
            call('stj_pool_admit', _p(self.offs_stage[key]), -(-e['n'] // SPARSE_BLOCK), _p(arrs[key]['val_base']), slots, N, ok, count, int(i == 0), st)
        if not sparse:
            call('stj_pool_admit', None, 0, None, slots, N, ok, count, 1, st)                # the range check of the slots alone
        for name, key, e, _, geom in self.features:
            d = arrs[key]
            if e['kind'] == 'bits':
                call('stj_pack_bits', _p(self.raw[name]), ok, slots, N, _p(d['words']), count, *geom, st)
            elif e['kind'] == 'sparse':
                call('stj_pack_sparse_commit', _p(self.raw[name]), _p(self.offs_stage[key]), ok, slots, N, _p(d['mask']), _p(d['offs']),
                     _p(d['val_base']), _p(d['vals']), self.pool._n_vals(key), count, *geom, st)
            else:
                call('stj_pool_put_raw', _p(self.raw[name]), ITEMSIZE[e['dtype']], ok, slots, N, _p(d['data']), count, e['n'], st)


class _PackedStage(_Stage):
    """_Stage for pack_example records: per record feature pinned host arrays and their device twins in the batch format of SparseHost
    and decode_batch_packed -- bits words [B][n / 32]; a sparse key's mask [B][n / 32], scene-relative offs [B][nblk + 1], src_base int64
    [B + 1] and vals, the scenes' value words back to back; the raw rows [B][nbytes].  vals holds B x the slot capacity: a record that no
    slot can hold is never staged.  launch() is a scatter copy with no packing: the admits, then the puts."""

    def __init__(self, pool, B, chunk_bytes=3 << 19):
        super().__init__(pool, B, chunk_bytes)
        rows = max(self.B, 1)
        self.host, self.dev_bufs = {}, {}
        for name, key, e, kind, n, dtype, *_ in self.feats:
            if kind == 'bits':
                sizes = {'bits': (rows * (n // 32), torch.int32)}
            elif kind == 'sparse':
                sizes = {'mask': (rows * (n // 32), torch.int32), 'offs': (rows * (-(-n // SPARSE_BLOCK) + 1), torch.int32),
                         'base': (rows + 1, torch.int64), 'vals': (max(rows * self.capacity[key], 1), torch.int32)}
            else:
                sizes = {'raw': (rows * n * ITEMSIZE[dtype], torch.uint8)}
            for part, (count, dt) in sizes.items():
                self.host[name, part] = torch.zeros((max(count, 1),), dtype=dt).pin_memory()
                self.dev_bufs[name, part] = torch.zeros((max(count, 1),), dtype=dt, device=self.dev)
        self._base = {}

    def check(self, ex, b=0):
        return _packed_parts(ex, b, self.feats)

    def misfit(self, parsed):
        for (name, key, e, kind, *_), (_, parts) in zip(self.feats, parsed):
            if kind == 'sparse' and parts[2].size > self.capacity[key]:
                return f'{key}: {parts[2].size} value words, a slot holds {self.capacity[key]}'
        return None

    def begin(self):
        self._base = {f.name: [0] for f in self.feats if f.kind == 'sparse'}

    def fill(self, b, parsed):
        for (name, key, e, kind, n, *_), (_, parts) in zip(self.feats, parsed):
            if kind == 'bits':
                _put(self.host[name, 'bits'], b * (n // 32), parts[0])
            elif kind == 'sparse':
                base = self._base[name]
                if len(base) != b + 1:
                    raise ValueError(f'packed staging: scene {b} filled out of order')
                vals = parts[2] if parts[2].size <= self.capacity[key] else parts[2][:0]      # no slot holds it: its words stay behind, and
                _put(self.host[name, 'mask'], b * (n // 32), parts[0])                        # the admit refuses it (count and capacity)
                _put(self.host[name, 'offs'], b * (-(-n // SPARSE_BLOCK) + 1), parts[1])
                _put(self.host[name, 'vals'], base[-1], vals)
                base.append(base[-1] + vals.size)
                self.host[name, 'base'].numpy()[:b + 2] = base
            else:
                raw = np.ascontiguousarray(parts[0]).view(np.uint8)
                self.host[name, 'raw'].numpy()[b * raw.size:(b + 1) * raw.size] = raw

    def upload(self, count):
        for (name, part), h in self.host.items():
            k = count + 1 if part == 'base' else self._base[name][count] if part == 'vals' else (h.numel() // max(self.B, 1)) * count
            _copy_chunked(self.dev_bufs[name, part], h, k, self.chunk)

    def launch(self, slots, count, ok):
        N, st, arrs, d = self.pool.N, _st(), self.pool.dev_arrays, self.dev_bufs
        sparse = [f for f in self.feats if f.kind == 'sparse']
        for i, (name, key, e, _, n, *_) in enumerate(sparse):
            call('stj_pool_admit_packed', _p(d[name, 'offs']), -(-n // SPARSE_BLOCK), n, _p(d[name, 'base']), _p(arrs[key]['val_base']), slots, N, ok,
                 count, int(i == 0), st)
        if not sparse:
            call('stj_pool_admit', None, 0, None, slots, N, ok, count, 1, st)
        for name, key, e, kind, n, *_ in self.feats:
            a = arrs[key]
            if kind == 'bits':
                call('stj_pool_put_raw', _p(d[name, 'bits']), 4, ok, slots, N, _p(a['words']), count, n // 32, st)
            elif kind == 'sparse':
                call('stj_pool_put_raw', _p(d[name, 'mask']), 4, ok, slots, N, _p(a['mask']), count, n // 32, st)
                call('stj_pool_put_raw', _p(d[name, 'offs']), 4, ok, slots, N, _p(a['offs']), count, -(-n // SPARSE_BLOCK) + 1, st)
                call('stj_pool_put_vals', _p(d[name, 'vals']), _p(d[name, 'base']), ok, slots, N, _p(a['val_base']), _p(a['vals']),
                     self.pool._n_vals(key), count, st)
            else:
                call('stj_pool_put_raw', _p(d[name, 'raw']), ITEMSIZE[e['dtype']], ok, slots, N, _p(a['data']), count, n, st)


class _Group:
    """One consumed group of a ShuffleWindow on its way round: its position in perm, the event behind the gathers that read it, and what
    the worker reports back -- how many scenes it refilled and the event behind their puts."""
    __slots__ = ('pos', 'after', 'ready', 'count', 'done')

    def __init__(self, pos, after, ready):
        self.pos, self.after, self.ready, self.count, self.done = pos, after, ready, 0, None


class ShuffleWindow:
    """The reference's `dataset.shuffle(N)` (train.py:381) with the buffer in HBM: a rolling window of N scenes over a source of any length,
    every source scene visited exactly once, at the rate of a ResidentPool.

        pool = ResidentPool.empty(N, 'cuda', grid, out, capacity={...})
        window = pool.window(B, source, lag=4)          # source: an iterator of pack_example records (packed=False: of raw records)
        window.start()                                  # fills the N slots with the first N scenes
        idx = window.next_batch()                       # device int32 [B]: B live slots, drawn on the device
        pool.gather_into(step.static, idx); window.release()       # or WindowFeed(step.static, window).land()

    State: perm int32 [N] on the device (initially arange(N)) and the host integers tail, head, n_live.  The live slots are
    perm[tail : tail + n_live), circular mod N; the free ones follow, the oldest consumed group first at head.  N % B == 0 and
    N >= (lag + 1) * B.
    Draw (stj_pool_draw): from random words u uint32 [B], for i = 0 .. B - 1: m = n_live - i, j = (u[i] * m) >> 32, p = (tail + i) % N,
    q = (tail + i + j) % N, swap perm[p] and perm[q], idx[i] = perm[p]; then tail = (tail + B) % N, n_live -= B.  The multiply-shift picks
    j with a bias of at most m / 2^32 per draw (no rejection sampling).  The B consumed slots are the group perm[old tail : old tail + B),
    which never wraps and is not touched again until it is admitted.
    Refill and admission: consumed groups are refilled in FIFO order with the next B scenes of the source, by a worker thread on a stream
    of its own (uploads from two staging sets, stj_pool_admit_packed / stj_pool_put_raw / stj_pool_put_vals reading their slots from
    perm on the device; the host never learns a slot number).  The group consumed at step t is admitted immediately before the draw of
    step t + lag (head += B, n_live += B), never earlier even if its refill is done, and the draw waits for it if it is not -- so the
    sequence of batches is a pure function of (N, B, lag, the u rows, the source order); a steady-state draw finds N - (lag - 1) * B
    live scenes and leaves N - lag * B.  ShuffleWindow.reference states all of it in Python.
    End of the source: consumed groups are no longer refilled, a last partial group of r < B scenes fills the first r slots of its group
    and is admitted with head += r, and the window drains; drop_last=True leaves the final fewer-than-B scenes unvisited (as PoolSampler
    does), drop_last=False returns them as a short last batch; then next_batch() raises StopIteration.
    Records that cannot land: the worker validates every record and checks the sparse keys against the slot capacity before upload; a
    malformed or oversized record is never uploaded, is logged in window.skipped as (source ordinal, reason), and the next record takes
    its place.  A device-side ok == 0 can then only mean corrupt staging: it is counted in window.bad (device int32 [1]) and such a slot
    KEEPS ITS OLD SCENE, which is then visited a second time.
    Counters: consumed (scenes returned), stalls (draws that found their refill unfinished and waited), skipped, bad.  An exception in the
    worker (the source's included) is re-raised by the next next_batch() / release() / close().  close() joins the worker and drains the
    refill stream.  Not built: state_dict (resuming mid-epoch), coordination across ranks (each rank windows its own shard), capture of
    the draw in a graph, any eviction policy but consumed-first FIFO."""

    def __init__(self, pool, batch_size, source, packed=True, lag=4, seed=0, drop_last=True, chunk_bytes=3 << 19):
        import collections
        import queue
        import threading
        N, B, K = pool.N, int(batch_size), int(lag)
        if B < 1 or K < 1 or N % B or N < (K + 1) * B:
            raise ValueError(f'ShuffleWindow: N {N}, B {B}, lag {K}: N a multiple of B and at least (lag + 1) * B, lag >= 1 only')
        self.pool, self.N, self.B, self.lag, self.packed, self.drop_last = pool, N, B, K, bool(packed), bool(drop_last)
        self.dev = pool.dev
        self.source = iter(source)
        self.perm = torch.arange(N, dtype=torch.int32, device=self.dev)
        self.idx = torch.zeros((B,), dtype=torch.int32, device=self.dev)
        self.bad = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.gen = torch.Generator(device=self.dev).manual_seed(int(seed))
        self.refill = torch.cuda.Stream(self.dev)
        self.tail = self.head = self.n_live = 0
        self.consumed = self.stalls = self.steps = 0
        self.skipped = []
        self._sets = [(_PackedStage if self.packed else _RawStage)(pool, B, chunk_bytes) for _ in range(2)]       # two staging sets
        self._ok = [torch.zeros((B,), dtype=torch.int32, device=self.dev) for _ in self._sets]
        self._free = [None for _ in self._sets]               # the event behind the last upload from a set's pinned side
        self._q, self._pending, self._open = queue.Queue(), collections.deque(), None
        self._ordinal, self._dry, self._stop, self._err, self._done = 0, False, False, None, False
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._started = False

    # ---- the NumPy / Python statement
    @staticmethod
    def reference(N, B, lag, u_rows, M, drop_last=True, live=None):
        """The batches of a window of N slots, batch size B and lag `lag` over a source of M scenes, as lists of source ordinals; u_rows[t]
        holds the random words of draw t.  live: a list that receives the live count every draw saw."""
        N, B, K, M = int(N), int(B), int(lag), int(M)
        if B < 1 or K < 1 or N % B or N < (K + 1) * B:
            raise ValueError(f'ShuffleWindow.reference: N {N}, B {B}, lag {K}')
        perm, holds = list(range(N)), [None] * N
        n_live = min(N, M)
        for s in range(n_live):                               # start(): group g takes scenes g * B ..
            holds[s] = s
        nxt, tail, head = n_live, 0, n_live % N
        pending, batches, t = [], [], 0
        while True:
            if len(pending) == K:                             # the group consumed at step t - K
                r = pending.pop(0)
                head, n_live = (head + r) % N, n_live + r
            b = B if n_live >= B else (0 if drop_last else n_live)
            if b == 0:
                return batches
            if live is not None:
                live.append(n_live)
            u = [int(x) & 0xffffffff for x in u_rows[t]]
            out = []
            for i in range(b):
                m = n_live - i
                j = (u[i] * m) >> 32
                p, q = (tail + i) % N, (tail + i + j) % N
                perm[p], perm[q] = perm[q], perm[p]
                out.append(holds[perm[p]])
            batches.append(out)
            if b < B:
                return batches
            r = min(B, M - nxt)                               # the refill: FIFO, the next r scenes into the group's first r slots
            for i in range(r):
                holds[perm[(tail + i) % N]] = nxt + i
            nxt += r
            pending.append(r)
            tail, n_live, t = (tail + B) % N, n_live - B, t + 1

    @staticmethod
    def draw_reference(perm, tail, n_live, u):
        """One draw as stj_pool_draw makes it, in NumPy: perm int32 [N] is permuted in place, -> idx int32 [len(u)].  As in the kernel every
        position is taken mod N and a value read from perm is clamped to [0, N - 1] on its way into idx (perm itself keeps it)."""
        N = perm.size
        idx = np.zeros(len(u), np.int32)
        for i, w in enumerate(u):
            j = (int(w) * (int(n_live) - i)) >> 32
            p, q = (tail + i) % N, (tail + i + j) % N
            perm[p], perm[q] = perm[q], perm[p]
            idx[i] = min(max(int(perm[p]), 0), N - 1)
        return idx

    # ---- the worker
    def _validate(self, ex):
        parsed = self._sets[0].check(ex, 0)
        why = self._sets[0].misfit(parsed)
        if why is not None:
            raise ValueError(why)
        return parsed

    def _pull(self):
        """The next B records of the source that can land (fewer at its end); the others go to window.skipped."""
        recs = []
        while len(recs) < self.B and not self._dry:
            try:
                ex = next(self.source)
            except StopIteration:
                self._dry = True
                break
            ordinal, self._ordinal = self._ordinal, self._ordinal + 1
            try:
                recs.append(self._validate(ex))
            except ValueError as e:
                self.skipped.append((ordinal, str(e)))
        return recs

    def _prepare(self, k):
        recs = self._pull()
        if recs:
            if self._free[k] is not None:
                self._free[k].synchronize()                   # the set's previous upload has left its pinned side
            st = self._sets[k]
            st.begin()
            for b, p in enumerate(recs):
                st.fill(b, p)
        return recs

    def _commit(self, g, k, recs):
        r = len(recs)
        g.count = r
        if not r:
            return
        with torch.cuda.stream(self.refill):
            slots = self.perm[g.pos:g.pos + r]
            st, ok = self._sets[k], self._ok[k]
            st.upload(r)
            self._free[k] = torch.cuda.Event()
            self._free[k].record(self.refill)
            if g.after is not None:
                self.refill.wait_event(g.after)               # the gathers that read these slots are done
            st.launch(_p(slots), r, _p(ok))
            self.bad.add_(r - ok[:r].sum(dtype=torch.int32))
            g.done = torch.cuda.Event()
            g.done.record(self.refill)

    def _run(self):
        g = None
        try:
            torch.cuda.set_device(self.perm.device)           # a tensor's device carries its index
            k, recs = 0, None
            while True:
                if recs is None:
                    recs = self._prepare(k)
                g = self._q.get()
                if g is None:
                    return
                self._commit(g, k, recs)
                g.ready.set()
                g, recs, k = None, None, (k + 1) % len(self._sets)
        except BaseException as e:                            # surfaced by the next next_batch() / release() / close()
            self._err = e
            while True:                                       # nobody waits for a group for ever
                if g is not None:
                    g.ready.set()
                g = self._q.get()
                if g is None:
                    return

    def _check(self):
        if self._err is not None:
            e, self._err = self._err, None
            self._done = True
            raise e

    def _send(self, pos, after):
        import threading
        g = _Group(pos, after, threading.Event())
        self._q.put(g)
        return g

    # ---- the training thread
    def start(self):
        """Fills the N slots with the first N scenes of the source (group g takes scenes g * B ..) and returns when they are there."""
        if self._started:
            raise RuntimeError('ShuffleWindow: started twice')
        self._started = True
        self.pool.wait()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self.refill.wait_event(ev)                            # perm and the pool's arrays exist
        self._thread.start()
        groups = [self._send(pos, None) for pos in range(0, self.N, self.B)]
        for g in groups:
            g.ready.wait()
            self._check()
        self.refill.synchronize()
        self.n_live = sum(g.count for g in groups)
        self.tail, self.head = 0, self.n_live % self.N
        return self

    def release(self):
        """Call after the gathers of the last next_batch(): records the event behind them on the current stream and hands the consumed
        group to the worker.  The next next_batch() does it if nobody has."""
        if self._open is None:
            return
        pos, self._open = self._open, None
        self._check()
        after = torch.cuda.Event()
        after.record(torch.cuda.current_stream(self.dev))
        self._pending.append(self._send(pos, after))

    def next_batch(self, u=None):
        """-> device int32 [B] (the window's persistent idx; a short last batch is a view of it): the slots of the next batch.  u: B random
        words (uint32, host) for a reproducible draw; None draws them on the device from the window's generator, with no host sync."""
        if not self._started:
            raise RuntimeError('ShuffleWindow: start() first')
        self.release()
        self._check()
        if self._done:
            raise StopIteration
        main = torch.cuda.current_stream(self.dev)
        if len(self._pending) == self.lag:                    # the group consumed lag steps ago
            g = self._pending.popleft()
            late = not g.ready.is_set()
            g.ready.wait()
            self._check()
            if g.count:
                if late or not g.done.query():
                    late = True
                    g.done.synchronize()
                main.wait_event(g.done)
                self.head, self.n_live = (self.head + g.count) % self.N, self.n_live + g.count
            self.stalls += int(late)
        b = self.B if self.n_live >= self.B else (0 if self.drop_last else self.n_live)
        if b == 0:
            self._done = True
            raise StopIteration
        if u is None:
            words = (torch.randint(0, 1 << 32, (b,), dtype=torch.int64, device=self.dev, generator=self.gen) - (1 << 31)).to(torch.int32)
        else:
            host = np.asarray(u, dtype=np.uint64).reshape(-1)
            if host.size < b or (host >> 32).any():
                raise ValueError(f'ShuffleWindow: u must hold {b} 32-bit words')
            words = torch.from_numpy((host[:b] & 0xffffffff).astype(np.uint32).view(np.int32)).to(self.dev)
        call('stj_pool_draw', _p(self.perm), self.N, self.tail, self.n_live, _p(words), _p(self.idx), b, _st())
        self._words = words                                   # alive until the stream has read it
        self.consumed += b
        self.steps += 1
        if b == self.B:
            self._open = self.tail
        else:
            self._done = True
        self.tail, self.n_live = (self.tail + b) % self.N, self.n_live - b
        return self.idx[:b]

    def __iter__(self):
        return self

    __next__ = next_batch

    def close(self):
        """Joins the worker, drains the refill stream and re-raises what the worker died of, if anything."""
        if self._thread.is_alive():
            self._stop = True
            self._q.put(None)
            self._thread.join()
        self.refill.synchronize()
        self._done = True
        self._check()


class WindowFeed:
    """HostFeed's protocol (start / land / wait_uploaded / close) over a ShuffleWindow, like ResidentFeed over a pool:

        feed = WindowFeed(step.static, pool.window(B, source))
        feed.start()
        for ...:
            feed.land()                    # draw, the pool's gathers into static, release; StopIteration when the source is used up
            step(); optimizer.step()

    land() draws into the persistent feed.idx (the window's), launches the gathers that read it and records the event that lets the
    worker refill the consumed slots.  The landing stays in front of a captured step's replay; nothing of the window is captured."""

    def __init__(self, static, window):
        self.static, self.window, self.pool = static, window, window.pool
        if not [k for k in self.pool.layout.entries if k in static]:
            raise ValueError('WindowFeed: the pool holds none of the keys of `static`')
        self.B, self.idx = window.B, window.idx
        self.pool.check_static(static, self.B)

    def start(self):
        if not self.window._started:
            self.window.start()

    def land(self, u=None):
        idx = self.window.next_batch(u)
        if idx.numel() != self.B:
            self.window.release()
            raise ValueError(f'WindowFeed: a last batch of {idx.numel()} scenes for a static batch of {self.B} (drop_last=True avoids it)')
        self.pool.gather_into(self.static, self.idx)
        self.window.release()

    def wait_uploaded(self):
        return

    def close(self):
        self.window.close()
