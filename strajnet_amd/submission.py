"""The output side of inference: the model's [B,H,W,32] logits as the byte strings the Occupancy-and-Flow challenge takes
(reference inference.py:160-182, _add_waypoints_to_scenario_prediction):

    obs  = zlib.compress(np.round(sigmoid(obs_logit) * 255).astype(np.uint8).tobytes())     # [H,W,1]
    occ  = zlib.compress(np.round(sigmoid(occ_logit) * 255).astype(np.uint8).tobytes())     # [H,W,1]
    flow = zlib.compress(np.clip(np.round(flow), -128, 127).astype(np.int8).tobytes())      # [H,W,2]

The quantisation runs on the device, in front of the device-to-host copy (4 bytes per cell and waypoint instead of 16): as a kernel of
its own behind any float32 output (stj_quantize_waypoints) or, on the 16-bit inference path, in the epilogue of the kernel that produces
the logits (stj_outconv_pair_gather_q; STrajNet.predict_quantized picks).  ResultDrain brings the bytes to pinned host memory beside the
replaying thread; compression is host work (zlib) on the caller's side.  `quantize_reference` is the only CPU code path here.

dequantize() loses at most 1/510 in probability and 0.5 per flow component (flow beyond [-128, 127] is clipped, as in the format).
"""
import os
import threading
import zlib

import numpy as np
import torch

from .loss import WaypointGrids
from .ops import _p, _st, call

NUM_WAYPOINTS = 8


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


class ResultDrain:
    """The output-side twin of data.HostFeed: brings the static quantised buffer of a GraphedForward(quantized=True) to pinned host
    memory, one batch per replay, without stalling the replaying thread:

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
                    for i in range(0, s.numel(), self.chunk):
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
        self._enq[slot].clear()
        self._ready[slot].record(main)
        self._n_sub += 1
        with self._cv:
            self._jobs.append(slot)
            self._cv.notify()

    def take(self):
        """The oldest submitted batch as a host QuantizedWaypoints (a view of ring memory)."""
        if self._n_take >= self._n_sub:
            raise RuntimeError('ResultDrain: nothing submitted')
        slot = self._n_take % self.depth
        self._enq[slot].wait()
        if self._err is not None:
            e, self._err = self._err, None
            raise e
        self._done[slot].synchronize()
        self._n_take += 1
        return QuantizedWaypoints(self.ring[slot], self.src.H, self.src.W, self.src.Tn)

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._thread.join(timeout=5)
