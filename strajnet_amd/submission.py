"""The output side of inference: the model's [B,H,W,32] logits as the byte strings the Occupancy-and-Flow challenge takes
(reference inference.py:160-182, _add_waypoints_to_scenario_prediction):

    obs  = zlib.compress(np.round(sigmoid(obs_logit) * 255).astype(np.uint8).tobytes())     # [H,W,1]
    occ  = zlib.compress(np.round(sigmoid(occ_logit) * 255).astype(np.uint8).tobytes())     # [H,W,1]
    flow = zlib.compress(np.clip(np.round(flow), -128, 127).astype(np.int8).tobytes())      # [H,W,2]

The quantisation runs on the device, in front of the device-to-host copy (4 bytes per cell and waypoint instead of 16): as a kernel of
its own behind any float32 output (stj_quantize_waypoints) or, on the 16-bit inference path, in the epilogue of the kernel that produces
the logits (stj_outconv_pair_gather_q; STrajNet.predict_quantized picks).  ResultDrain brings the bytes to pinned host memory beside the
replaying thread.  Compression: either host work (zlib: QuantizedWaypoints.compressed / compress_batch, zlib's own sizes) or on the
device (compress_waypoints, stj_compress_waypoints: one zlib stream per plane, run-length DEFLATE with the fixed Huffman code, or at
level 2 with a dynamic Huffman code per segment, in the format `compress_reference` states; larger streams than zlib's default, about
zlib level 1's at level 2, no host work, and only the streams cross to the host).  With framed=True the device also
frames the streams as protobuf fields (FramedWaypoints), and SubmissionWriter turns drained batches into the challenge's
ChallengeSubmission file, one slice per scene.  `quantize_reference`, `compress_reference`, `frame_reference`, `submission_reference`
and `parse_submission` are the only CPU code paths here.

dequantize() loses at most 1/510 in probability and 0.5 per flow component (flow beyond [-128, 127] is clipped, as in the format).
"""
import ctypes
import os
import threading
import zlib

import numpy as np
import torch

from .loss import WaypointGrids
from ._lib import call as _host_call
from .ops import _p, _st, call

NUM_WAYPOINTS = 8
DEFLATE_SEGMENT = 8192      # bytes of a plane per DEFLATE block (csrc/deflate.hip: DF_SEG); a power of two in 4096..32768


def quantize_reference(out):
    """The reference's three NumPy lines on a [B,H,W,32] float array -> (obs u8 [B,Tn,H,W], occ u8 [B,Tn,H,W], flow i8 [B,Tn,H,W,2]).
    CPU; for tests and for users without a GPU at hand."""
    out = np.asarray(out)
    B, H, W, C = out.shape
    y = out.reshape(B, H, W, C // 4, 4)
    with np.errstate(over='ignore'):
        obs = np.round(1.0 / (1.0 + np.exp(-y[..., 0])) * 255).astype(np.uint8)
        occ = np.round(1.0 / (1.0 + np.exp(-y[..., 1])) * 255).astype(np.uint8)
    flow = np.clip(np.round(y[..., 2:4]), -128, 127).astype(np.int8)
    return (np.ascontiguousarray(obs.transpose(0, 3, 1, 2)), np.ascontiguousarray(occ.transpose(0, 3, 1, 2)),
            np.ascontiguousarray(flow.transpose(0, 3, 1, 2, 4)))


class QuantizedWaypoints:
    """A [B, 4*Tn*H*W] uint8 buffer (device or host), per scene [ obs u8 [Tn,H,W] | occ u8 [Tn,H,W] | flow i8 [Tn,H,W,2] ]: the
    layout stj_quantize_waypoints writes.  A scene, or the whole batch, is one contiguous copy, and every (scene, waypoint, field)
    slice is contiguous and equal to the reference's `.tobytes()`."""

    def __init__(self, buf, H, W, Tn=NUM_WAYPOINTS):
        if buf.dtype != torch.uint8 or buf.dim() != 2 or buf.shape[1] != 4 * Tn * H * W or not buf.is_contiguous():
            raise ValueError(f'QuantizedWaypoints: expected a contiguous uint8 [B,{4 * Tn * H * W}] buffer, got {buf.dtype} {tuple(buf.shape)}')
        self.buf, self.H, self.W, self.Tn = buf, H, W, Tn

    @property
    def batch(self):
        return self.buf.shape[0]

    @property
    def observed(self):
        n = self.Tn * self.H * self.W
        return self.buf[:, :n].view(-1, self.Tn, self.H, self.W)

    @property
    def occluded(self):
        n = self.Tn * self.H * self.W
        return self.buf[:, n:2 * n].view(-1, self.Tn, self.H, self.W)

    @property
    def flow(self):
        n = self.Tn * self.H * self.W
        return self.buf[:, 2 * n:].view(torch.int8).view(-1, self.Tn, self.H, self.W, 2)

    def cpu(self):
        """Synchronous copy to host memory (one transfer).  A host buffer is returned as it is."""
        return self if not self.buf.is_cuda else QuantizedWaypoints(self.buf.cpu(), self.H, self.W, self.Tn)

    def clone(self):
        return QuantizedWaypoints(self.buf.clone(), self.H, self.W, self.Tn)

    def waypoint_bytes(self, b, k):
        """(obs, occ, flow) of scene b, waypoint k as raw bytes: what the reference hands to zlib.compress."""
        host = self.buf[b].cpu().numpy()
        n = self.H * self.W
        o, c, f = k * n, (self.Tn + k) * n, (2 * self.Tn + 2 * k) * n
        return host[o:o + n].tobytes(), host[c:c + n].tobytes(), host[f:f + 2 * n].tobytes()

    def compressed(self, b):
        """Scene b: a list of Tn (obs, occ, flow) zlib strings (default level, as the reference calls it)."""
        return [tuple(zlib.compress(s) for s in self.waypoint_bytes(b, k)) for k in range(self.Tn)]

    def dequantize(self):
        """WaypointGrids of probabilities (q / 255) and float flow on the buffer's device, in the form compute_occupancy_flow_metrics
        takes for a prediction."""
        B = self.batch
        packed = torch.empty((B, self.H, self.W, self.Tn, 4), dtype=torch.float32, device=self.buf.device)
        packed[..., 0] = self.observed.permute(0, 2, 3, 1).float() / 255.0
        packed[..., 1] = self.occluded.permute(0, 2, 3, 1).float() / 255.0
        packed[..., 2:] = self.flow.permute(0, 2, 3, 1, 4).float()
        packed = packed.view(B, self.H, self.W, 4 * self.Tn)
        g = WaypointGrids()
        for k in range(self.Tn):
            g.vehicles.observed_occupancy.append(packed[..., 4 * k:4 * k + 1])
            g.vehicles.occluded_occupancy.append(packed[..., 4 * k + 1:4 * k + 2])
            g.vehicles.flow.append(packed[..., 4 * k + 2:4 * k + 4])
        g._packed = packed
        return g


def quantize_waypoints(out):
    """Any [B,H,W,32] float32 model output on the device -> QuantizedWaypoints (stj_quantize_waypoints)."""
    if not out.is_cuda:
        raise RuntimeError('quantize_waypoints: CUDA (ROCm) tensors only: the HIP path has no CPU fallback (CPU: quantize_reference)')
    if out.dim() != 4 or out.shape[3] != 4 * NUM_WAYPOINTS or out.dtype != torch.float32:
        raise ValueError(f'quantize_waypoints: expected float32 [B,H,W,{4 * NUM_WAYPOINTS}], got {out.dtype} {tuple(out.shape)}')
    out = out.detach().contiguous()
    B, H, W, _ = out.shape
    q = torch.empty((B, 4 * NUM_WAYPOINTS * H * W), dtype=torch.uint8, device=out.device)
    call('stj_quantize_waypoints', _p(out), _p(q), B, NUM_WAYPOINTS, H, W, _st())
    return QuantizedWaypoints(q, H, W)


def compression_pool(threads=None):
    """A thread pool for `compress_batch`, sized by the CPUs this job was GIVEN (its affinity mask, at most 16), not by the machine's."""
    from concurrent.futures import ThreadPoolExecutor
    if threads is None:
        threads = min(16, len(os.sched_getaffinity(0)))
    return ThreadPoolExecutor(max_workers=max(1, threads))


def compress_batch(qw, pool):
    """Every scene of a HOST QuantizedWaypoints through `compressed`, spread over `pool` (zlib releases the GIL).  Returns a list of B
    lists of Tn (obs, occ, flow)."""
    return list(pool.map(qw.compressed, range(qw.batch)))


# ---------------------------------------------------------------------------------------------------- device-side compression
# The stream of one plane x of n bytes at match distance d (1: occupancy, 2: flow, so that equal consecutive (dx, dy) pairs match):
#   78 01 | one DEFLATE block per segment of DEFLATE_SEGMENT bytes | Adler-32(x), big-endian
# Byte i of the PLANE is matchable if i >= d and x[i] == x[i - d] (history reaches into the previous segment, never in front of the
# plane).  Within a segment, a maximal stretch of L matchable bytes becomes matches of min(258, rest) at distance d while rest >= 3; the
# 1-2 bytes left over, and stretches shorter than 3, are literals.  Fixed Huffman code (BTYPE 01).  A non-final fixed block is followed
# by an empty stored block (bits 000, pad, 00 00 FF FF), so every segment is a whole number of bytes; the final one pads to the byte.
# A segment whose fixed form, flush included, exceeds 5 + len bytes is a stored block (BTYPE 00) instead.  Hence a stream has at most
# n + 5 ceil(n / DEFLATE_SEGMENT) + 6 bytes.

def _rev(v, bits):
    return int(format(v, f'0{bits}b')[::-1], 2)


def _fixed_tables():
    """(literal value, literal bits) per byte, and per match length 3..258 the (value, bits) of length code + extra bits -- RFC 1951
    3.2.5 / 3.2.6; Huffman codes go out most significant bit first, i.e. reversed in the LSB-first bit stream, extra bits as they are."""
    lit_v = np.array([_rev(0x30 + v, 8) if v < 144 else _rev(0x190 + v - 144, 9) for v in range(256)], np.uint64)
    lit_n = np.array([8 if v < 144 else 9 for v in range(256)], np.int64)
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    len_v, len_n = {}, {}
    for m in range(3, 259):
        c = max(i for i in range(29) if base[i] <= m and (i == 28 or m < 258))
        sym = 257 + c
        hv, hn = (_rev(sym - 256, 7), 7) if sym < 280 else (_rev(0xC0 + sym - 280, 8), 8)
        len_v[m], len_n[m] = hv | ((m - base[c]) << hn), hn + extra[c]
    return lit_v, lit_n, len_v, len_n


_LIT_V, _LIT_N, _LEN_V, _LEN_N = _fixed_tables()


def _pack_bits(vals, nbits, total_bits):
    """Tokens (value, bit count <= 25) laid end to end, least significant bit first -> ceil(total_bits / 8) bytes."""
    out = np.zeros((total_bits + 7) // 8 + 4, np.uint8)
    off = np.concatenate([[0], np.cumsum(nbits)[:-1]]).astype(np.int64)
    sh = vals << (off & 7).astype(np.uint64)
    for k in range(4):
        np.bitwise_or.at(out, (off >> 3) + k, ((sh >> np.uint64(8 * k)) & np.uint64(0xff)).astype(np.uint8))
    return out[:(total_bits + 7) // 8]


# Level 2: the same header, segments, tokens, trailer and empty stored block behind every non-final block; each segment takes the
# shortest of three forms.  fixed: level 1's bytes for the segment.  dynamic (BTYPE 10, RFC 1951 3.2.7), flush included as for fixed:
#   literal/length code: the segment's tokens counted per symbol, EOB once -> huffman_code_lengths(counts, 15); HLIT covers up to the
#     highest used symbol (at least 257 codes).
#   distance code: d codes (HDIST = d - 1), code d - 1 of length 1, any other 0 -- also in a segment without a match.  zlib takes this
#     incomplete one-code set; a match writes the single bit 0 for its distance.
#   the code lengths, literal/length [0, HLIT + 257) then the d distance lengths, as one sequence cut into maximal runs of equal values
#     (a run may cross the join); a run of r values v: v == 0: while r >= 11 symbol 18 with min(r, 138); then symbol 17 with r if
#     r >= 3; the rest literal zeros.  v != 0: v once; while the rest >= 3 symbol 16 with min(rest, 6); the rest literal v.
#   code-length code: huffman_code_lengths(counts of the 19 symbols, 7); HCLEN up to the last non-zero length in the order 16, 17, 18,
#     0, 8, 7, ..., at least 4.  At least two of its symbols are always in use (an unused literal symbol gives a zero next to non-zero
#     lengths).
# fixed if len(fixed) <= len(dynamic), else dynamic; if the form taken exceeds 5 + len bytes the segment is stored.  So a level-2 segment
# is never longer than its level-1 segment and the capacity bound holds.
# Resolutions of what the rules above leave open: a code over a single used symbol gives that symbol length 1 (it occurs in neither of
# the two codes of a stream, only through huffman_code_lengths); the depth histogram of step 4 is built even when no depth exceeds the
# limit, so lengths are ALWAYS handed out by sorted order (equal multiset, and equal counts get lengths that never decrease with the
# symbol number).

_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_LEN_CODE = {m: max(i for i in range(29) if _LEN_BASE[i] <= m and (i == 28 or m < 258)) for m in range(3, 259)}


def huffman_code_lengths(counts, limit):
    """Code lengths (0: unused) of the length-limited Huffman code of level 2 over `counts`:
      1. the used symbols sorted ascending by (count, symbol);
      2. the Huffman tree by the two-queue method over that order -- on equal weight a leaf before an internal node, internal nodes in
         creation order;
      3. a symbol's length is the depth of its leaf;
      4. cnt[l]: the histogram of the lengths, those above `limit` counted at `limit`; while sum cnt[l] 2^(limit - l) > 2^limit:
         cnt[limit] -= 1, and with the largest l < limit that has cnt[l] > 0: cnt[l] -= 1, cnt[l + 1] += 2 (each round lowers the sum by 1);
      5. the lengths 1, 2, ... of the histogram go, in increasing order, to the symbols in DESCENDING sorted order."""
    order = sorted((int(c), s) for s, c in enumerate(counts) if c > 0)
    n, out = len(order), [0] * len(counts)
    if n == 0:
        return out
    if n == 1:
        out[order[0][1]] = 1
        return out
    weight = [c for c, _ in order]                      # nodes 0 .. n - 1: the leaves; n .. 2n - 2: internal, in creation order
    parent = [0] * (2 * n - 1)
    li, ii = 0, n
    for k in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= k or weight[li] <= weight[ii]):
                w, parent[li], li = w + weight[li], k, li + 1
            else:
                w, parent[ii], ii = w + weight[ii], k, ii + 1
        weight.append(w)
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    cnt = [0] * (limit + 1)
    for k in range(n):
        cnt[min(depth[k], limit)] += 1
    while sum(cnt[l] << (limit - l) for l in range(1, limit + 1)) > 1 << limit:
        cnt[limit] -= 1
        l = max(l for l in range(1, limit) if cnt[l] > 0)
        cnt[l] -= 1
        cnt[l + 1] += 2
    q = n - 1
    for l in range(1, limit + 1):
        for _ in range(cnt[l]):
            out[order[q][1]] = l
            q -= 1
    return out


def _canonical_codes(lengths):
    """RFC 1951 3.2.2, each code bit-reversed: as it enters the LSB-first bit stream."""
    mx = max(lengths)
    bl = [0] * (mx + 2)
    for l in lengths:
        bl[l] += l > 0
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        out.append(_rev(nxt[l], l) if l else 0)
        nxt[l] += l > 0
    return out


def dynamic_block_header(lit_counts, d, final):
    """The dynamic block's header for the 286 literal/length counts of a segment (EOB included): (literal/length code lengths, their
    codes as they enter the bit stream, the header's tokens as (values, bit counts) from BFINAL up to the last code length)."""
    ll = huffman_code_lengths(lit_counts, 15)
    nl = max(257, max(s for s in range(286) if ll[s]) + 1)
    seq = ll[:nl] + [0] * (d - 1) + [1]
    rle, i = [], 0                                      # (code-length symbol, extra value, extra bits)
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138)
                rle.append((18, t - 11, 7))
                r -= t
            if r >= 3:
                rle.append((17, r - 3, 3))
                r = 0
        else:
            rle.append((v, 0, 0))
            r -= 1
            while r >= 3:
                t = min(r, 6)
                rle.append((16, t - 3, 2))
                r -= t
        rle += [(v, 0, 0)] * r
    cc = [0] * 19
    for s, _, _ in rle:
        cc[s] += 1
    assert sum(c > 0 for c in cc) >= 2
    cl = huffman_code_lengths(cc, 7)
    ccode = _canonical_codes(cl)
    ncl = max(4, max(j for j in range(19) if cl[_CL_ORDER[j]]) + 1)
    vals = [int(final) | 4, nl - 257, d - 1, ncl - 4] + [cl[_CL_ORDER[j]] for j in range(ncl)]
    nbits = [3, 5, 5, 4] + [3] * ncl
    for s, ev, eb in rle:
        vals.append(ccode[s] | ev << cl[s])
        nbits.append(cl[s] + eb)
    return ll, _canonical_codes(ll), vals, nbits


def compress_reference(plane_bytes, d, level=1, forms=None):
    """The zlib stream stj_compress_waypoints (level 1) / stj_compress_waypoints_level writes for one plane (`plane_bytes`: bytes or a
    uint8 array; d = 1 for an occupancy plane, 2 for a flow plane), byte for byte.  CPU; the statement of the format, for tests and for
    users without a GPU at hand.  `forms`: a list that receives, per segment, the form it took (its BTYPE: 0 stored, 1 fixed, 2 dynamic)."""
    x = np.frombuffer(bytes(plane_bytes), np.uint8) if not isinstance(plane_bytes, np.ndarray) else plane_bytes.reshape(-1).view(np.uint8)
    n, S = x.size, DEFLATE_SEGMENT
    if n == 0 or d not in (1, 2):
        raise ValueError('compress_reference: a non-empty plane and d in (1, 2)')
    if level not in (1, 2):
        raise ValueError('compress_reference: level 1 or 2')
    matchable = np.zeros(n, bool)
    matchable[d:] = x[d:] == x[:-d]
    dist_v = _rev(d - 1, 5)
    out = [b'\x78\x01']
    for s0 in range(0, n, S):
        seg, m = x[s0:s0 + S], matchable[s0:s0 + S]
        L, final = seg.size, s0 + S >= n
        vals, nbits = _LIT_V[seg].copy(), _LIT_N[seg].copy()
        mlen = np.zeros(L, np.int64)                                # level 2: the length of the match that starts at a byte
        edge = np.flatnonzero(np.diff(np.concatenate([[False], m, [False]]).astype(np.int8)))
        for a, e in zip(edge[0::2], edge[1::2]):                   # the stretches [a, e) of matchable bytes
            pos, rest = int(a), int(e - a)
            while rest >= 3:
                ml = min(258, rest)
                vals[pos] = _LEN_V[ml] | (dist_v << _LEN_N[ml])
                nbits[pos] = _LEN_N[ml] + 5
                nbits[pos + 1:pos + ml] = 0
                mlen[pos] = ml
                pos, rest = pos + ml, rest - ml
        keep = nbits > 0
        vals = np.concatenate([[np.uint64(int(final) | 2)], vals[keep]]).astype(np.uint64)          # BFINAL, BTYPE 01 in front; EOB = 7 zero bits
        nbits = np.concatenate([[3], nbits[keep]])
        bits = int(nbits.sum()) + 7 + (0 if final else 3)                                         # non-final: + the empty stored block's 000
        block, form = _pack_bits(vals, nbits, bits).tobytes() + (b'' if final else b'\x00\x00\xff\xff'), 1
        if level == 2:
            tok, tml = seg[keep].astype(np.int64), mlen[keep]
            lc = np.array([_LEN_CODE.get(int(ml), 0) for ml in tml], np.int64)
            sym = np.where(tml > 0, 257 + lc, tok)
            counts = np.bincount(sym, minlength=286)
            counts[256] = 1
            ll, code, hv, hn = dynamic_block_header(counts, d, final)
            ll, code = np.array(ll, np.int64), np.array(code, np.uint64)
            eb = np.where(tml > 0, np.array(_LEN_EXTRA, np.int64)[lc], 0)
            ev = np.where(tml > 0, tml - np.array(_LEN_BASE, np.int64)[lc], 0).astype(np.uint64)
            tv = code[sym] | ev << ll[sym].astype(np.uint64)          # a match: + the distance's single bit 0
            tn = ll[sym] + eb + (tml > 0)
            dv = np.concatenate([np.array(hv, np.uint64), tv, [code[256]]]).astype(np.uint64)
            dn = np.concatenate([np.array(hn, np.int64), tn, [ll[256]]])
            dbits = int(dn.sum()) + (0 if final else 3)
            dyn = _pack_bits(dv, dn, dbits).tobytes() + (b'' if final else b'\x00\x00\xff\xff')
            if len(dyn) < len(block):
                block, form = dyn, 2
        if len(block) > 5 + L:
            block, form = bytes([int(final), L & 255, L >> 8, ~L & 255, (~L >> 8) & 255]) + seg.tobytes(), 0
        out.append(block)
        if forms is not None:
            forms.append(form)
    out.append(zlib.adler32(x.tobytes()).to_bytes(4, 'big'))
    return b''.join(out)


def compress_sizes(B, H, W, Tn=NUM_WAYPOINTS):
    """(workspace bytes, capacity of the packed buffer) of stj_compress_waypoints; raises StjError for a shape it does not take."""
    work, cap = ctypes.c_longlong(0), ctypes.c_longlong(0)
    _host_call('stj_compress_sizes', B, Tn, H, W, ctypes.c_void_p(ctypes.addressof(work)), ctypes.c_void_p(ctypes.addressof(cap)))
    return work.value, cap.value


class CompressedWaypoints:
    """The zlib streams of a batch, packed: `buf` uint8 (device or host), `offsets` [B*Tn*3 + 1] (int32 storage, read as uint32): stream
    s = (b*Tn + k)*3 + i, i in (obs, occ, flow), is buf[offsets[s]:offsets[s + 1]] -- the order of QuantizedWaypoints.compressed(b)[k][i],
    so a scene's 3 Tn streams are one contiguous slice.  On the device `buf` has the capacity of the worst case and only the first
    offsets[-1] bytes mean anything; `work` is the kernels' scratch (kept so that the object can be written again: compress_waypoints(out=))."""

    def __init__(self, buf, offsets, B, Tn=NUM_WAYPOINTS, work=None):
        if buf.dtype != torch.uint8 or buf.dim() != 1 or offsets.dim() != 1 or offsets.numel() != 3 * B * Tn + 1 or offsets.dtype != torch.int32:
            raise ValueError(f'CompressedWaypoints: expected a uint8 [n] buffer and int32 [{3 * B * Tn + 1}] offsets, got '
                             f'{buf.dtype} {tuple(buf.shape)}, {offsets.dtype} {tuple(offsets.shape)}')
        self.buf, self.offsets, self.B, self.Tn, self.work = buf, offsets, B, Tn, work

    @classmethod
    def empty(cls, B, H, W, device, Tn=NUM_WAYPOINTS):
        """Device memory for the streams of a [B, 4*Tn*H*W] QuantizedWaypoints."""
        work, cap = compress_sizes(B, H, W, Tn)
        return cls(torch.empty(cap, dtype=torch.uint8, device=device), torch.empty(3 * B * Tn + 1, dtype=torch.int32, device=device), B, Tn,
                   work=torch.empty(work, dtype=torch.uint8, device=device))

    @property
    def batch(self):
        return self.B

    def _host_offsets(self):
        return self.offsets.cpu().numpy().view(np.uint32).astype(np.int64)

    @property
    def nbytes(self):
        """Total size of the streams (a device object is asked: one small synchronous copy)."""
        return int(self._host_offsets()[-1])

    def cpu(self):
        """Synchronous copy to host memory: the offsets table, then the offsets[-1] bytes that are streams."""
        if not self.buf.is_cuda:
            return self
        off = self.offsets.cpu()
        total = int(off.numpy().view(np.uint32)[-1])
        return CompressedWaypoints(self.buf[:total].cpu(), off, self.B, self.Tn)

    def scene_bytes(self, b):
        """The 3 Tn streams of scene b, back to back, as bytes."""
        off = self._host_offsets()
        lo, hi = int(off[3 * self.Tn * b]), int(off[3 * self.Tn * (b + 1)])
        return self.buf[lo:hi].cpu().numpy().tobytes()

    def streams(self, b):
        """Scene b: a list of Tn (obs, occ, flow) zlib strings, the shape of QuantizedWaypoints.compressed(b)."""
        off = self._host_offsets()[3 * self.Tn * b:3 * self.Tn * (b + 1) + 1]
        raw = self.buf[int(off[0]):int(off[-1])].cpu().numpy().tobytes()
        cut = [int(o - off[0]) for o in off]
        return [tuple(raw[cut[3 * k + i]:cut[3 * k + i + 1]] for i in range(3)) for k in range(self.Tn)]


# ---------------------------------------------------------------------------------------------------- submission files
# The reference's inference.py ends in one ChallengeSubmission protobuf per test shard (inference.py:186-252): a few header strings and
# one ScenarioPrediction per scene, its id and eight Waypoint messages of three zlib strings.  Every field here is length-delimited
# (wire type 2): tag byte (field number << 3 | 2), varint(length), payload.
#
# The field numbers, in ONE table; everything (the device call's tag bytes, the references, the parser, the writer, the tests) reads
# them from here.  They are as recalled from the public occupancy_flow_submission.proto of the Waymo Open Dataset; that file was not at
# hand when this was written and the numbers have NOT been checked against it -- a correction is one line here.
SUBMISSION_SCHEMA = {
    'Waypoint': {'observed_vehicles_occupancy': 1, 'occluded_vehicles_occupancy': 2, 'all_vehicles_flow': 3},
    'ScenarioPrediction': {'scenario_id': 1, 'waypoints': 2},
    'ChallengeSubmission': {'account_name': 1, 'unique_method_name': 2, 'authors': 3, 'affiliation': 4, 'description': 5,
                            'method_link': 6, 'scenario_predictions': 7},
}
WAYPOINT_FIELDS = ('observed_vehicles_occupancy', 'occluded_vehicles_occupancy', 'all_vehicles_flow')       # the order (obs, occ, flow)
NUM_SHARDS = 150


def _tag(message, field):
    n = SUBMISSION_SCHEMA[message][field]
    if not 1 <= n <= 15:
        raise ValueError(f'SUBMISSION_SCHEMA: {message}.{field} = {n}: one-byte tags (field numbers 1..15) only')
    return n << 3 | 2


def frame_tags():
    """The four tag bytes of a scene's block as stj_compress_waypoints_framed takes them: tag_wp | tag_obs << 8 | tag_occ << 16 |
    tag_flow << 24."""
    t = [_tag('ScenarioPrediction', 'waypoints')] + [_tag('Waypoint', f) for f in WAYPOINT_FIELDS]
    return t[0] | t[1] << 8 | t[2] << 16 | t[3] << 24


def pb_varint(v):
    """A non-negative integer below 2^64 as a base-128 varint."""
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f'pb_varint: {v} is not a uint64')
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7f | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _field(tag, payload):
    return bytes([tag]) + pb_varint(len(payload)) + payload


def frame_reference(streams):
    """A scene's block -- the wire form of its `repeated Waypoint waypoints` -- from a `streams(b)`-shaped list of (obs, occ, flow) byte
    strings: what stj_compress_waypoints_framed leaves in the packed buffer, byte for byte (the rules for C: csrc/frame.h).  CPU."""
    tw = _tag('ScenarioPrediction', 'waypoints')
    tf = [_tag('Waypoint', f) for f in WAYPOINT_FIELDS]
    return b''.join(_field(tw, b''.join(_field(t, bytes(s)) for t, s in zip(tf, wp))) for wp in streams)


def _as_bytes(s):
    return s.encode('utf-8') if isinstance(s, str) else bytes(s)


def _header_bytes(header):
    """The ChallengeSubmission's string fields in field-number order; a list or tuple is a repeated field, None is left out."""
    out = []
    for name, _ in sorted(SUBMISSION_SCHEMA['ChallengeSubmission'].items(), key=lambda kv: kv[1]):
        v = header.get(name) if name != 'scenario_predictions' else None
        if v is None:
            continue
        for s in (v if isinstance(v, (list, tuple)) else (v,)):
            out.append(_field(_tag('ChallengeSubmission', name), _as_bytes(s)))
    unknown = set(header) - set(SUBMISSION_SCHEMA['ChallengeSubmission']) | ({'scenario_predictions'} & set(header))
    if unknown:
        raise ValueError(f'submission header: unknown fields {sorted(unknown)}')
    return b''.join(out)


def _scene_prefix(sid, block_len):
    """What stands in front of a scene's block: tag7 varint(n) tag1 varint(len(id)) id."""
    idf = _field(_tag('ScenarioPrediction', 'scenario_id'), _as_bytes(sid))
    return bytes([_tag('ChallengeSubmission', 'scenario_predictions')]) + pb_varint(len(idf) + block_len) + idf


def submission_reference(header, ids, scenes):
    """The whole file: `header` a dict of ChallengeSubmission's string fields (authors: a list), ids the scenario ids, scenes a
    `streams(b)`-shaped list per id.  Pure Python, the order protobuf's own serialiser writes.  CPU."""
    if len(ids) != len(scenes):
        raise ValueError('submission_reference: one id per scene')
    out = [_header_bytes(header)]
    for sid, streams in zip(ids, scenes):
        block = frame_reference(streams)
        out += [_scene_prefix(sid, len(block)), block]
    return b''.join(out)


def _pb_fields(buf, lo, hi):
    """(field number, wire type, value) of every field of the message buf[lo:hi]; a length-delimited value is a (lo, hi) pair."""
    def varint(p):
        v = sh = 0
        while True:
            if p >= hi or sh > 63:
                raise ValueError('parse_submission: bad varint')
            c = buf[p]
            p += 1
            v |= (c & 0x7f) << sh
            sh += 7
            if c < 0x80:
                return v, p
    p = lo
    while p < hi:
        key, p = varint(p)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, p = varint(p)
        elif wt == 2:
            n, p = varint(p)
            val, p = (p, p + n), p + n
        elif wt in (1, 5):
            val, p = None, p + (8 if wt == 1 else 4)
        else:
            raise ValueError(f'parse_submission: wire type {wt}')
        if p > hi or num == 0:
            raise ValueError('parse_submission: truncated message')
        yield num, wt, val


def parse_submission(data):
    """A hand-written reader of the wire format: (header, ids, scenes) of a ChallengeSubmission file -- header: the string fields present
    (authors a list), ids: the scenario ids as str, scenes: per id a list of (obs, occ, flow) byte strings per waypoint (a field a
    waypoint lacks is b'').  Fields the schema does not name are skipped.  CPU."""
    buf = bytes(data)
    top = {n: k for k, n in SUBMISSION_SCHEMA['ChallengeSubmission'].items()}
    sp, wf = SUBMISSION_SCHEMA['ScenarioPrediction'], [SUBMISSION_SCHEMA['Waypoint'][f] for f in WAYPOINT_FIELDS]
    header, ids, scenes = {}, [], []
    for num, wt, val in _pb_fields(buf, 0, len(buf)):
        name = top.get(num)
        if name is None or wt != 2:
            continue
        if name != 'scenario_predictions':
            s = buf[val[0]:val[1]].decode('utf-8')
            if name == 'authors':
                header.setdefault(name, []).append(s)
            else:
                header[name] = s
            continue
        sid, wps = '', []
        for n2, w2, v2 in _pb_fields(buf, *val):
            if w2 != 2:
                continue
            if n2 == sp['scenario_id']:
                sid = buf[v2[0]:v2[1]].decode('utf-8')
            elif n2 == sp['waypoints']:
                wp = [b'', b'', b'']
                for n3, w3, v3 in _pb_fields(buf, *v2):
                    if w3 == 2 and n3 in wf:
                        wp[wf.index(n3)] = buf[v3[0]:v3[1]]
                wps.append(tuple(wp))
        ids.append(sid)
        scenes.append(wps)
    return header, ids, scenes


def compress_framed_sizes(B, H, W, Tn=NUM_WAYPOINTS):
    """(workspace bytes, capacity of the packed buffer, words of the table) of stj_compress_waypoints_framed."""
    v = [ctypes.c_longlong(0) for _ in range(3)]
    _host_call('stj_compress_framed_sizes', B, Tn, H, W, *(ctypes.c_void_p(ctypes.addressof(x)) for x in v))
    return tuple(x.value for x in v)


class FramedWaypoints:
    """The zlib streams of a batch inside their protobuf framing, packed: scene b's block, buf[scene[b]:scene[b + 1]], is the wire form of
    its `repeated Waypoint waypoints` (frame_reference), ready to go into a ScenarioPrediction behind the id.  `table` [6*B*Tn + B + 1]
    (int32 storage, read as uint32; one allocation, so that one small copy brings it): the start of every stream's zlib bytes [3*B*Tn],
    every stream's length [3*B*Tn], the scene starts [B + 1] whose last entry is the total.  On the device `buf` has the capacity of the
    worst case; `work` is the kernels' scratch (compress_waypoints(out=, framed=True) writes the object again)."""

    def __init__(self, buf, table, B, Tn=NUM_WAYPOINTS, work=None):
        if buf.dtype != torch.uint8 or buf.dim() != 1 or table.dim() != 1 or table.numel() != 6 * B * Tn + B + 1 or table.dtype != torch.int32:
            raise ValueError(f'FramedWaypoints: expected a uint8 [n] buffer and an int32 [{6 * B * Tn + B + 1}] table, got '
                             f'{buf.dtype} {tuple(buf.shape)}, {table.dtype} {tuple(table.shape)}')
        self.buf, self.table, self.B, self.Tn, self.work = buf, table, B, Tn, work

    @classmethod
    def empty(cls, B, H, W, device, Tn=NUM_WAYPOINTS):
        """Device memory for the framed streams of a [B, 4*Tn*H*W] QuantizedWaypoints."""
        work, cap, words = compress_framed_sizes(B, H, W, Tn)
        return cls(torch.empty(cap, dtype=torch.uint8, device=device), torch.empty(words, dtype=torch.int32, device=device), B, Tn,
                   work=torch.empty(work, dtype=torch.uint8, device=device))

    @property
    def batch(self):
        return self.B

    def _host_table(self):
        return self.table.cpu().numpy().view(np.uint32).astype(np.int64)

    def scene_starts(self):
        """[B + 1] host int64: scene b's block is buf[s[b]:s[b + 1]]."""
        return self._host_table()[6 * self.B * self.Tn:]

    @property
    def nbytes(self):
        """Total size of the framed blocks (a device object is asked: one small synchronous copy)."""
        return int(self._host_table()[-1])

    def cpu(self):
        """Synchronous copy to host memory: the table, then the table[-1] bytes that are blocks."""
        if not self.buf.is_cuda:
            return self
        tab = self.table.cpu()
        total = int(tab.numpy().view(np.uint32)[-1])
        return FramedWaypoints(self.buf[:total].cpu(), tab, self.B, self.Tn)

    def scene_message(self, b):
        """Scene b's framed block as bytes."""
        s = self.scene_starts()
        return self.buf[int(s[b]):int(s[b + 1])].cpu().numpy().tobytes()

    def streams(self, b):
        """Scene b: a list of Tn (obs, occ, flow) zlib strings, the shape of CompressedWaypoints.streams(b)."""
        t, n, m = self._host_table(), 3 * self.B * self.Tn, 3 * self.Tn
        lo, hi = int(t[2 * n + b]), int(t[2 * n + b + 1])
        raw = self.buf[lo:hi].cpu().numpy().tobytes()
        cut = [(int(t[m * b + j]) - lo, int(t[m * b + j]) - lo + int(t[n + m * b + j])) for j in range(m)]
        return [tuple(raw[cut[3 * k + i][0]:cut[3 * k + i][1]] for i in range(3)) for k in range(self.Tn)]


class SubmissionWriter:
    """One shard's ChallengeSubmission file from host FramedWaypoints (what ResultDrain.take() or FramedWaypoints.cpu() gives):

        with open(os.path.join(save_dir, SubmissionWriter.shard_name(test_shard_path)), 'wb') as f:
            w = SubmissionWriter(f)
            for ids in ...:
                w.add_batch(drain.take(), ids)
            w.close()

    The header fields are the ones the reference sets, with its (empty) values as defaults (inference.py:216-226); `affiliation` is in
    the schema, the reference does not set it, and it is not written.  Per scene the writer appends tag7 varint(n) tag1 varint(len(id)) id
    and ONE slice of the batch's buffer -- no per-stream work.  path_or_file: a path (opened and closed here) or a binary file object
    (flushed, not closed)."""

    def __init__(self, path_or_file, account_name='', unique_method_name='', authors=('',), description='', method_link=''):
        self._own = isinstance(path_or_file, (str, os.PathLike))
        self.f = open(path_or_file, 'wb') if self._own else path_or_file
        self.scenes = 0
        self.f.write(_header_bytes(dict(account_name=account_name, unique_method_name=unique_method_name, authors=list(authors),
                                        description=description, method_link=method_link)))

    def add_batch(self, framed, ids):
        """The first len(ids) <= B scenes of a HOST FramedWaypoints under these ids (a last short batch: fewer ids than scenes)."""
        if framed.buf.is_cuda:
            raise ValueError('SubmissionWriter.add_batch: a host FramedWaypoints (ResultDrain.take() or .cpu())')
        if len(ids) > framed.B:
            raise ValueError(f'SubmissionWriter.add_batch: {len(ids)} ids for a batch of {framed.B}')
        s = framed.scene_starts()
        mem = memoryview(framed.buf.numpy())
        for b, sid in enumerate(ids):
            lo, hi = int(s[b]), int(s[b + 1])
            self.f.write(_scene_prefix(sid, hi - lo))
            self.f.write(mem[lo:hi])
        self.scenes += len(ids)

    def close(self):
        if self.f is not None:
            self.f.close() if self._own else self.f.flush()
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def shard_name(test_shard_path):
        """The submission file's name for a test shard (inference.py:240-244): the shard's first five characters are its number."""
        base = os.path.basename(test_shard_path)
        if 'new.tfrecords' not in base:
            raise ValueError(f'SubmissionWriter.shard_name: {base!r} is not a test shard (no "new.tfrecords" in its name)')
        return f'occupancy_flow_submission.binproto-{base[:5]}-of-{NUM_SHARDS:05d}'


def compress_waypoints(qw, out=None, level=1, framed=False):
    """A device QuantizedWaypoints -> CompressedWaypoints (stj_compress_waypoints: no host synchronisation, no allocation with `out`
    given -- a CompressedWaypoints.empty of the same shape, written in place -- so the call can be captured in a graph).  level 1: the
    fixed Huffman code; level 2: per segment the shortest of stored, fixed and a dynamic Huffman code of its own
    (stj_compress_waypoints_level; compress_reference(level=2)): smaller streams from the same three launches' worth of work.
    framed=True: -> FramedWaypoints (stj_compress_waypoints_framed; `out`: a FramedWaypoints.empty): the same streams inside their
    protobuf framing, the same number of launches."""
    if level not in (1, 2):
        raise ValueError(f'compress_waypoints: level 1 or 2, got {level!r}')
    if not qw.buf.is_cuda:
        raise RuntimeError('compress_waypoints: CUDA (ROCm) buffers only: the HIP path has no CPU fallback (CPU: compress_reference, '
                           'or zlib through QuantizedWaypoints.compressed)')
    B = qw.batch
    if framed:
        if out is None:
            out = FramedWaypoints.empty(B, qw.H, qw.W, qw.buf.device, qw.Tn)
        else:
            work, cap, words = compress_framed_sizes(B, qw.H, qw.W, qw.Tn)
            if (not isinstance(out, FramedWaypoints) or out.work is None or not out.buf.is_cuda or out.B != B or out.Tn != qw.Tn
                    or out.buf.numel() < cap or out.work.numel() < work or out.buf.device != qw.buf.device):
                raise ValueError('compress_waypoints: `out` must be a FramedWaypoints.empty() of the same shape on the same device')
        call('stj_compress_waypoints_framed', _p(qw.buf), _p(out.work), _p(out.buf), _p(out.table), B, qw.Tn, qw.H, qw.W, level,
             frame_tags(), _st())
        return out
    if out is None:
        out = CompressedWaypoints.empty(B, qw.H, qw.W, qw.buf.device, qw.Tn)
    else:
        work, cap = compress_sizes(B, qw.H, qw.W, qw.Tn)
        if (out.work is None or not out.buf.is_cuda or out.B != B or out.Tn != qw.Tn or out.buf.numel() < cap or out.work.numel() < work
                or out.buf.device != qw.buf.device):
            raise ValueError('compress_waypoints: `out` must be a CompressedWaypoints.empty() of the same shape on the same device')
    if level == 1:
        call('stj_compress_waypoints', _p(qw.buf), _p(out.work), _p(out.buf), _p(out.offsets), B, qw.Tn, qw.H, qw.W, _st())
    else:
        call('stj_compress_waypoints_level', _p(qw.buf), _p(out.work), _p(out.buf), _p(out.offsets), B, qw.Tn, qw.H, qw.W, level, _st())
    return out


class ResultDrain:
    """The output-side twin of data.HostFeed: brings the static quantised buffer of a GraphedForward(quantized=True) to pinned host
    memory, one batch per replay, without stalling the replaying thread (or the CompressedWaypoints of a GraphedForward(quantized=True,
    compressed=True), or the FramedWaypoints of one with framed=True as well: then the worker brings the offsets table first and only the
    offsets[-1] bytes that are streams):

        drain = ResultDrain(gf.out)
        for batch in batches:
            gf(batch)
            drain.submit()                     # behind the replay: device copy into a staging slot; the worker thread brings it to the host
            ...
            host = drain.take()                # host QuantizedWaypoints of the OLDEST submitted batch (blocks until it has arrived)

    A ring of `depth` slots, each a device staging buffer and a pinned host buffer: at most `depth` batches may be submitted and not yet
    taken, and what take() returns is a view of ring memory, valid until `depth` further submits.  submit() copies the static buffer into
    the slot's staging buffer on the CURRENT stream (behind the replay by stream order, so the next replay may overwrite the static
    buffer at once; 2 MB per scene at HBM speed) after making that stream wait for the event of the slot's previous host copy, so a
    staging buffer that is still being read is not overwritten.  The host copies are issued by a worker thread in pieces, as in HostFeed
    and for its reason: a large pinned hipMemcpyAsync blocks the thread that issues it, and while one call is blocked the replaying
    thread's launches stall too."""

    def __init__(self, qw, depth=3, chunk_bytes=3 << 19):
        from .data import _copy_stream
        if not qw.buf.is_cuda:
            raise ValueError('ResultDrain: the source must be a device buffer')
        self.src = qw
        self.dev = qw.buf.device
        self.depth, self.chunk = int(depth), int(chunk_bytes)
        self.stage = [torch.empty_like(qw.buf) for _ in range(self.depth)]
        self.ring = [torch.empty(qw.buf.shape, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self.framed = isinstance(qw, FramedWaypoints)
        self.compressed = self.framed or isinstance(qw, CompressedWaypoints)
        if self.compressed:       # + the offsets table (framed: the table); the worker reads it first and brings only [-1] bytes of the buffer
            side = self._side()
            self.stage_off = [torch.empty_like(side) for _ in range(self.depth)]
            self.ring_off = [torch.empty(side.shape, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
            self._total = [0] * self.depth
        self.copy = _copy_stream(self.dev)
        self._done = [torch.cuda.Event() for _ in range(self.depth)]      # slot i's host copy has arrived
        self._ready = [torch.cuda.Event() for _ in range(self.depth)]     # slot i's staging buffer holds the batch
        self._enq = [threading.Event() for _ in range(self.depth)]        # slot i's host copy has been enqueued (`_done[i]` is recorded)
        self._jobs = []
        self._cv = threading.Condition()
        self._n_sub = self._n_take = 0
        self._stop = False
        self._err = None
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def _side(self):
        return self.src.table if self.framed else self.src.offsets

    def _run(self):
        torch.cuda.set_device(self.dev)
        while True:
            with self._cv:
                while not self._jobs and not self._stop:
                    self._cv.wait()
                if self._stop:
                    return
                slot = self._jobs.pop(0)
            try:
                with torch.cuda.stream(self.copy):
                    self.copy.wait_event(self._ready[slot])
                    s, d = self.stage[slot].view(-1), self.ring[slot].view(-1)
                    n = s.numel()
                    if self.compressed:
                        self.ring_off[slot].copy_(self.stage_off[slot], non_blocking=True)
                        self.copy.synchronize()              # (this thread's own stream: the replaying thread is not held up)
                        n = self._total[slot] = int(self.ring_off[slot].numpy().view(np.uint32)[-1])
                    for i in range(0, n, self.chunk):
                        d[i:i + self.chunk].copy_(s[i:i + self.chunk], non_blocking=True)
                    self._done[slot].record(self.copy)
            except Exception as e:       # surfaced by the next take()
                self._err = e
            self._enq[slot].set()

    def submit(self):
        """Queue what the static buffer holds once the current stream's work so far is through (i.e. behind the replay)."""
        if self._n_sub - self._n_take >= self.depth:
            raise RuntimeError('ResultDrain: ring full -- take() before submitting more')
        slot = self._n_sub % self.depth
        main = torch.cuda.current_stream(self.dev)
        if self._n_sub >= self.depth:
            main.wait_event(self._done[slot])        # (taken already, so recorded: the slot's previous host copy has left the staging buffer)
        self.stage[slot].copy_(self.src.buf, non_blocking=True)
        if self.compressed:
            self.stage_off[slot].copy_(self._side(), non_blocking=True)
        self._enq[slot].clear()
        self._ready[slot].record(main)
        self._n_sub += 1
        with self._cv:
            self._jobs.append(slot)
            self._cv.notify()

    def take(self):
        """The oldest submitted batch as a host QuantizedWaypoints (CompressedWaypoints, FramedWaypoints for such a source), a view of ring
        memory."""
        if self._n_take >= self._n_sub:
            raise RuntimeError('ResultDrain: nothing submitted')
        slot = self._n_take % self.depth
        self._enq[slot].wait()
        if self._err is not None:
            e, self._err = self._err, None
            raise e
        self._done[slot].synchronize()
        self._n_take += 1
        if self.framed:
            return FramedWaypoints(self.ring[slot][:self._total[slot]], self.ring_off[slot], self.src.B, self.src.Tn)
        if self.compressed:
            return CompressedWaypoints(self.ring[slot][:self._total[slot]], self.ring_off[slot], self.src.B, self.src.Tn)
        return QuantizedWaypoints(self.ring[slot], self.src.H, self.src.W, self.src.Tn)

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join(timeout=5)
