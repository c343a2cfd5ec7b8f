"""The cases of the protobuf framing (tests/test_framing.py on the CPU, tests/test_framing_gpu.py through the kernels): quantised batches
built so that the varints of the framing take every length that can occur at these shapes, each checked HERE, on the CPU with
compress_reference, to land on both sides of the boundary it is there for.  The reference streams are computed once per (plane content,
level) and shared: the batches draw their planes from small pools, and a stream depends on its plane's bytes alone."""
import numpy as np

LEVELS = (1, 2)
_STREAMS = {}
_BATCHES = {}


def _occ_pool(n, rng):
    """Occupancy planes of n bytes whose streams are short, near 128 bytes, and stored."""
    pool = [np.full(n, v, np.uint8) for v in (0, 7, 255)]
    for head in (3, 40, 100, 118, 130, n // 2, n):
        x = np.zeros(n, np.uint8)
        x[:head] = rng.integers(0, 256, head, dtype=np.uint8)
        pool.append(x)
    return pool


def _flow_pool(n, rng):
    pool = [np.resize(np.array(p, np.uint8), n) for p in ((0, 0), (3, 250))]
    for head in (5, 60, 110, 126, n // 2, n):
        x = np.zeros(n, np.uint8)
        x[:head] = rng.integers(0, 256, head, dtype=np.uint8)
        pool.append(x)
    return pool


def _assemble(B, H, W, pick):
    """[B, 32 H W] uint8 in QuantizedWaypoints' layout; pick(b, k, i) -> the plane (i: 0 obs, 1 occ, 2 flow) of scene b, waypoint k."""
    n = H * W
    buf = np.empty((B, 32 * n), np.uint8)
    for b in range(B):
        for k in range(8):
            buf[b, k * n:(k + 1) * n] = pick(b, k, 0)
            buf[b, (8 + k) * n:(9 + k) * n] = pick(b, k, 1)
            buf[b, (16 + 2 * k) * n:(18 + 2 * k) * n] = pick(b, k, 2)
    return buf


def _sparse(H, W, rng, blobs, flow):
    """A model-like plane: zero but for a few soft blobs (occupancy) or constant-velocity patches (flow, int8 pairs as bytes)."""
    if not flow:
        x = np.zeros((H, W), np.float32)
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(blobs):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.uniform(2, 7)
            x = np.maximum(x, 255 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)))
        return np.round(x).astype(np.uint8).reshape(-1)
    x = np.zeros((H, W, 2), np.int8)
    for _ in range(blobs):
        cy, cx = rng.integers(0, H - 12), rng.integers(0, W - 12)
        x[cy:cy + 12, cx:cx + 12] = rng.integers(-20, 20, 2)
        x[cy + 3:cy + 6, cx:cx + 12, 0] += rng.integers(-2, 3, (3, 12)).astype(np.int8)
    return x.reshape(-1).view(np.uint8)


def batch(name):
    """name -> (uint8 [B, 32 H W], H, W).  small: 16x16 B 3, a constant, a random and a mixed scene; mid: 64x64 B 2, all planes random /
    all constant; long: 128x64 B 1, random flow; many: 16x16 B 129, content varying by index (its first 43 scenes: many43); sparse:
    256x256 B 2, model-like planes."""
    if name in _BATCHES:
        return _BATCHES[name]
    rng = np.random.default_rng(20261021)
    if name == 'small':
        H = W = 16
        rnd = [rng.integers(0, 256, (3, 8, 2 * H * W), dtype=np.uint8) for _ in range(2)]

        def pick(b, k, i):
            n = H * W * (2 if i == 2 else 1)
            const = np.full(n, 9 + i, np.uint8)
            if b == 0:
                return const
            if b == 1:
                return rnd[0][i, k, :n]
            return const if (k + i) % 2 else rnd[1][i, k, :n]                # per plane one or the other; waypoint 0: random, const, random
        buf = _assemble(3, H, W, pick)
    elif name == 'mid':
        H = W = 64
        rnd = rng.integers(0, 256, (3, 8, 2 * H * W), dtype=np.uint8)
        buf = _assemble(2, H, W, lambda b, k, i: rnd[i, k, :H * W * (2 if i == 2 else 1)] if b == 0 else np.full(H * W * (2 if i == 2 else 1), 200, np.uint8))
    elif name == 'long':
        H, W = 128, 64
        occ, flo = _sparse(H, W, rng, 3, False), rng.integers(0, 256, (8, 2 * H * W), dtype=np.uint8)
        buf = _assemble(1, H, W, lambda b, k, i: flo[k] if i == 2 else occ)
    elif name in ('many', 'many43'):
        H = W = 16
        if name == 'many43':
            buf = batch('many')[0][:43].copy()
        else:
            po, pf = _occ_pool(H * W, rng), _flow_pool(2 * H * W, rng)
            buf = _assemble(129, H, W, lambda b, k, i: pf[(5 * b + 3 * k) % len(pf)] if i == 2 else po[(7 * b + 3 * k + 4 * i) % len(po)])
    elif name == 'sparse':
        H = W = 256
        po = [_sparse(H, W, rng, nb, False) for nb in (0, 4, 9)]
        pf = [_sparse(H, W, rng, nb, True) for nb in (0, 5)]
        buf = _assemble(2, H, W, lambda b, k, i: pf[(b + k) % 2] if i == 2 else po[(b + k + i) % 3])
    else:
        raise KeyError(name)
    _BATCHES[name] = (buf, H, W)
    return _BATCHES[name]


def reference_streams(name, level):
    """Per scene a streams(b)-shaped list of compress_reference's streams."""
    from strajnet_amd.submission import compress_reference
    buf, H, W = batch(name)
    n = H * W
    out = []
    for b in range(buf.shape[0]):
        scene = []
        for k in range(8):
            wp = []
            for i, (lo, ln, d) in enumerate(((k * n, n, 1), ((8 + k) * n, n, 1), ((16 + 2 * k) * n, 2 * n, 2))):
                raw = buf[b, lo:lo + ln].tobytes()
                key = (raw, d, level)
                if key not in _STREAMS:
                    _STREAMS[key] = compress_reference(raw, d, level=level)
                wp.append(_STREAMS[key])
            scene.append(tuple(wp))
        out.append(scene)
    return out


def host_framed(scenes):
    """A HOST FramedWaypoints built from streams(b)-shaped lists with frame_reference: what the device call must deliver for them."""
    import torch
    from strajnet_amd.submission import FramedWaypoints, frame_reference
    B, n = len(scenes), 24 * len(scenes)
    table, blocks, at = np.zeros(2 * n + B + 1, np.uint32), [], 0
    for b, scene in enumerate(scenes):
        blk = frame_reference(scene)
        table[2 * n + b] = at
        p = 0
        for k, wp in enumerate(scene):
            body = sum(1 + varint_len(len(s)) + len(s) for s in wp)
            p += 1 + varint_len(body)
            for i, s in enumerate(wp):
                p += 1 + varint_len(len(s))
                assert blk[p:p + len(s)] == s
                table[24 * b + 3 * k + i], table[n + 24 * b + 3 * k + i] = at + p, len(s)
                p += len(s)
        assert p == len(blk)
        blocks.append(blk)
        at += len(blk)
    table[-1] = at
    buf = torch.from_numpy(np.frombuffer(b''.join(blocks), np.uint8).copy())
    return FramedWaypoints(buf, torch.from_numpy(table.view(np.int32)), B)


def varint_len(v):
    return 1 if v < 128 else 1 + varint_len(v >> 7)


def lengths(streams):
    """(every stream length, every waypoint body length) of a batch's reference streams."""
    ls = [len(s) for scene in streams for wp in scene for s in wp]
    bodies = [sum(1 + varint_len(len(s)) + len(s) for s in wp) for scene in streams for wp in scene]
    return ls, bodies


def check_boundaries(name, level):
    """What the case is there for, asserted on the reference streams."""
    ref = reference_streams(name, level)
    ls, bodies = lengths(ref)
    if name == 'small':
        assert min(ls) < 128 <= max(ls) and min(bodies) < 128 <= max(bodies) < 16384
        mixed = [len(s) < 128 for s in ref[2][0]]
        assert True in mixed and False in mixed                               # both kinds inside one waypoint
    elif name == 'mid':
        assert min(bodies) < 16384 <= max(bodies) and max(ls) < 16384
        # (the constant scene's bodies: two bytes of varint at level 1, one at level 2, whose streams are shorter)
        assert {varint_len(v) for v in bodies} == ({2, 3} if level == 1 else {1, 3})
    elif name == 'long':
        assert max(ls) >= 16384 and varint_len(max(ls)) == 3
    elif name in ('many', 'many43'):
        B = len(ref)
        assert B * 24 > 1008 and (B == 43 or B * 24 > 3 * 1008)               # streams beyond one / three chunks of the scan
        assert min(ls) < 128 <= max(ls) and min(bodies) < 128 <= max(bodies)
        assert len({tuple(len(s) for wp in scene for s in wp) for scene in ref}) > 20      # the scenes differ
    elif name == 'sparse':
        assert len(ref) == 2 and max(ls) < 16384 * 8
    return ref
