"""hipGraph capture of the whole train step (forward + OGMFlow_loss + backward into the flat gradient bucket).

The step is ~650 stream-ordered kernel launches with static shapes, no host synchronisation and no allocation outside
torch's graph-private pool (every kernel of libstrajnet_hip.so launches on the current stream and never allocates), so
it is capturable as ONE graph; replaying it removes the Python / launch overhead (~10 ms per step, measured with B=1).
New data is fed by copying into the static input tensors; weights are read in place (the bf16 shadow cast is part of
the graph), gradients land in model.flat_grads().  The data-parallel all-reduce stays outside the graph.
The Dropout / DropPath stream advances inside the graph (stj_rng_advance bumps a device counter), so every replay draws new masks.
"""
import torch

from . import ops
from .loss import get_pred_waypoint_logits, warpped_gt


class GraphedTrainStep:
    """split=False: ONE graph for the whole step.  split=True (data parallel): TWO graphs cut at the raster encoder's outputs
    (model.cut_encoder) -- graph A = forward + loss + backward of everything downstream of the encoder, graph B = the encoder's
    backward; `__call__(between=f)` runs f between the two replays (dp.OverlappedGradSync.tail: the tail bucket's all-reduce then
    overlaps graph B).  Both graphs share one private memory pool: B reads the activations A saved.

    optimizer (an optim.DeviceNadam: its scalar state lives on the device): the update is captured at the end of the step, so one replay
    is the whole of train.py:199-230 -- forward, loss, backward, update, and with optimizer.attach_loss_means the four train-loss means
    (fed by each pass's LossDict.packed).  The warm-up passes do not train: weights, moments, optimizer state and running sums are put
    back afterwards, bit for bit.  Not with split=True: the update must follow the all-reduce, which stays outside the graph."""

    def __init__(self, model, loss_fn, batch, warmup=2, training=True, split=False, keep_graph=False, optimizer=None):
        """keep_graph: leave the captured hipGraph_t un-instantiated (torch.cuda.CUDAGraph(keep_graph=True)) so that a caller can edit it
        (self.graph.raw_cuda_graph(): e.g. kernel-node attributes, tools/probes/graph_node_priority.py) before self.graph.instantiate()."""
        if optimizer is not None and split:
            raise ValueError('GraphedTrainStep: optimizer= cannot be captured with split=True (the update must follow the all-reduce, '
                             'which stays outside the graph): call optimizer.step() after sync.head_and_wait()')
        if optimizer is not None and not getattr(optimizer, 'capturable', False):
            raise ValueError('GraphedTrainStep: optimizer= needs an optimizer whose step() is launches only (optim.DeviceNadam); a '
                             'host-state optimizer\'s coefficients would freeze at capture time')
        self.model, self.loss_fn, self.training, self.split, self.optimizer = model, loss_fn, training, split, optimizer
        self.static = {k: v.clone() for k, v in batch.items()}
        self.graph = self.graph_b = None
        self._side = None
        self.losses = None
        # the gradient `total` is differentiated with: created up front and announced to the loss, which then writes d(total)/d(logits)
        # in its forward pass (OGMFlow_loss.unit_grad, ops.LOSS_FUSED_BWD)
        self._one = torch.ones((), dtype=torch.float32, device=next(iter(batch.values())).device)
        if hasattr(loss_fn, 'unit_grad'):
            loss_fn.unit_grad = self._one
        if split:
            model.cut_encoder = True
        trained = optimizer.tensors() if optimizer is not None else []
        snap = [t.clone() for t in trained]          # the warm-up passes must not train
        side = ops.role_stream(torch.cuda.current_device(), 'warmup')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._eager()
                if split:
                    model.backward_encoder()
            for t, s in zip(trained, snap):
                t.copy_(s)
            if trained:
                model._sync_compute_weights()        # the compute-dtype copy was cast from the warm-up's weights
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        # thread_local: calls that are illegal during capture only count against THIS thread -- a process-group watchdog thread
        # (RCCL, data parallel runs) querying its events must not invalidate the capture
        with torch.cuda.graph(g, capture_error_mode='thread_local'):
            self.losses = self._eager()
        self.graph = g
        if split:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, pool=g.pool(), capture_error_mode='thread_local'):
                model.backward_encoder()
            self.graph_b = gb

    def _eager(self):
        x, m = self.static, self.model
        m.zero_grad()
        tw = warpped_gt(x['gt_obs'], x['gt_occ'], x['gt_flow'], x['origin_flow'])
        main = torch.cuda.current_stream()
        if hasattr(self.loss_fn, 'prepare'):         # the ground-truth-only part of the loss: side stream, under the forward pass --
            if self._side is None:                   # issued from the model's mid-forward hook (behind the encoder's first stage: at the
                self._side = ops.role_stream(torch.cuda.current_device(), 'loss_prep')     # head of the step its two launches delayed the first encoder kernel)

            def prepare():
                self._side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._side):
                    self.loss_fn.prepare(tw)
            m.mid_forward_hook = prepare
        try:
            out = m(x['ogm'], x['map_img'], training=self.training, obs=x['obs'], occ=x['occ'], mapt=x.get('mapt'), flow=x['flow'])
        finally:
            m.mid_forward_hook = None
        if self._side is not None:
            main.wait_stream(self._side)
        d = self.loss_fn(get_pred_waypoint_logits(out), tw, None)
        total = d.total                      # observed_xe + occluded_xe + flow + flow_warp_xe (train.py:221)
        total.backward(self._one)             # (an explicit tensor: backward()'s implicit ones_like is a fill launch on every replay)
        self.total = total.detach()           # the sum the finalize kernel wrote (static across replays, like self.losses)
        if self.optimizer is not None:
            if self.optimizer.loss_scale is not None:
                self.optimizer.attach_loss_means(d.packed, self.optimizer.loss_scale)
            self.optimizer.step()
        return d.packed             # [observed_xe, occluded_xe, flow, flow_warp_xe], detached

    def load(self, batch):
        """Copy a new batch into the static input tensors (stream-ordered device copies)."""
        for k, v in batch.items():
            if k in self.static:
                self.static[k].copy_(v, non_blocking=True)

    def __call__(self, batch=None, between=None):
        if batch is not None:
            self.load(batch)
        self.graph.replay()
        if self.graph_b is not None:
            if between is not None:
                between()
            self.graph_b.replay()
        return self.losses          # [observed_xe, occluded_xe, flow, flow_warp_xe]; gradients in model.flat_grads()


class GraphedForward:
    """hipGraph capture of the inference forward (training=False, no autograd): BASELINE config 4 (batch 32, one MI355X).
    __call__(batch) copies the batch into the static inputs, replays, and returns the static [B,Hg,Hg,32] f32 output.

    quantized=True: the captured forward is model.predict_quantized and the result a submission.QuantizedWaypoints over static memory
    (the challenge format's bytes: 4 per cell and waypoint instead of 16 to bring to the host; submission.ResultDrain does that).
    With compressed=True as well the captured forward is model.predict_compressed and the result a submission.CompressedWaypoints over
    static memory: the zlib strings, of which ResultDrain brings only the bytes they really have (compress_level=2: a dynamic Huffman
    code per segment, streams about half the size on sparse planes).  framed=True on top: a submission.FramedWaypoints, the streams
    inside their protobuf framing, for submission.SubmissionWriter.

    pipeline_agents=True: the agent branch (trajNet: ~30 dependent launches of a few microseconds that a replayed graph starts only when
    the raster encoder is through -- 0.3 of the 6.3 ms B = 32 step with nothing beside them, profiles/r05_c_timeline_infer_b32_f16.txt) is
    taken OUT of the graph and launched on a second stream.  prefetch_agents(next_batch), called right after __call__(batch), runs it for the NEXT batch under
    this batch's raster path; __call__ then waits for it, copies its two small results into the main graph's static inputs and replays the
    main graph, which no longer contains the branch.  Without a prefetch the agent branch runs in front of the main graph (same result).
    (Also tried: a replay that does not re-cast / re-pack / re-fold the constant weights -- one cast + seven side-stream launches less per step --
    measured 1.3 % SLOWER in three same-box pairs, 5333 / 5118 / 5333 vs 5390 / 5206 / 5412 scenes/s: where those launches sit decides when the
    executor starts the other branches, DESIGN 4e.  Not kept.)"""

    def __init__(self, model, batch, warmup=2, pipeline_agents=False, quantized=False, compressed=False, compress_level=1, framed=False):
        if compressed and not quantized:
            raise ValueError('GraphedForward: compressed=True compresses the quantised output: pass quantized=True with it')
        if compress_level not in (1, 2):
            raise ValueError(f'GraphedForward: compress_level 1 or 2, got {compress_level!r}')
        if framed and not compressed:
            raise ValueError('GraphedForward: framed=True frames the compressed streams: pass compressed=True with it')
        self.compress_level = compress_level
        self.framed = framed
        self.model = model
        self.quantized = quantized
        self.compressed = compressed
        self.static = {k: v.clone() for k, v in batch.items() if k in ('ogm', 'map_img', 'obs', 'occ', 'flow')}
        self.pipeline_agents = pipeline_agents
        self._prefetched = False
        self._staged = None
        self._weights_seen = -1
        side = ops.role_stream(torch.cuda.current_device(), 'warmup')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                self._eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if pipeline_agents:
            # the model's own agent-branch stream (idle in a main graph captured without the branch).  NOT one more stream: with a sixth
            # side stream alive in the process a LATER, unrelated graph replay died in hip::Graph::UpdateStreams (ROCm 7.2; tests/test_model_gpu.py
            # run as a whole: bisected to the number of distinct streams in use -- see ops.role_stream)
            self.agent_stream = model._streams[0] if model._streams[0] is not None else ops.role_stream(torch.cuda.current_device(), 'side')
            self.agent_done, self.agent_free = torch.cuda.Event(), torch.cuda.Event()
            # (the branch is launched EAGERLY, ~30 small launches issued by the host while the GPU replays the main graph; as a hipGraph of its
            #  own it ran as fast)
            with torch.no_grad():
                self.agent_next = model.agent_encode(self.static['obs'], self.static['occ'])
            self.agent_cur = tuple(t.clone() for t in self.agent_next)
            torch.cuda.synchronize()
            model.agent_override = self.agent_cur
        try:
            self.graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
                self.out = self._eager()
        finally:
            model.agent_override = None
        if pipeline_agents:
            self.agent_free.record(torch.cuda.current_stream())

    def _eager(self):
        x = self.static
        if self.compressed:
            return self.model.predict_compressed(x['ogm'], x['map_img'], obs=x['obs'], occ=x['occ'], mapt=None, flow=x['flow'],
                                                 level=self.compress_level, framed=self.framed)
        if self.quantized:
            return self.model.predict_quantized(x['ogm'], x['map_img'], obs=x['obs'], occ=x['occ'], mapt=None, flow=x['flow'])
        return self.model(x['ogm'], x['map_img'], training=False, obs=x['obs'], occ=x['occ'], mapt=None, flow=x['flow'])

    def prefetch_agents(self, batch=None, ready=None):
        """Start the agent branch of the NEXT batch (None: the static inputs as they are) on the agent stream, under whatever the main
        stream is running.  `ready`: an event recorded behind whatever produced batch['obs'] / batch['occ'] (e.g. their host-to-device
        copies on a feed stream); the agent stream waits for it.  Without one the agent stream is ordered behind everything the CALLER's
        current stream has been given so far -- always safe, but when that stream is the one replaying the main graph the branch then runs
        after the replay instead of under it: prefer `__call__(batch, next_batch=...)`, which stages the tracks in front of the replay."""
        if not self.pipeline_agents:
            return
        st = self.agent_stream
        st.wait_event(self.agent_free)               # the previous results have been copied out
        if batch is not None:
            if ready is not None:
                st.wait_event(ready)
            else:
                st.wait_stream(torch.cuda.current_stream())
        if self._staged is not None:                 # tracks staged on the main stream in front of the replay (__call__(next_batch=))
            st.wait_event(self._staged)
            self._staged = None
        with torch.cuda.stream(st):
            if batch is not None:
                for k in ('obs', 'occ'):
                    if k in batch:
                        self.static[k].copy_(batch[k], non_blocking=True)
                        batch[k].record_stream(st)
            with torch.no_grad():
                # (no weight cast here: the main graph casts the same buffer at the head of every replay, and two casts of one buffer on two
                #  streams are an unordered write / read pair)
                self.agent_next = self.model.agent_encode(self.static['obs'], self.static['occ'], cast=False)
            self.agent_done.record(st)
        self._prefetched = True
        self._weights_seen = self.model.weights_version

    def __call__(self, batch=None, next_batch=None):
        """next_batch (pipeline_agents only): the batch of the NEXT call; its agent tracks are copied into the static inputs on the
        current stream IN FRONT of this replay (ordered behind whatever produced them on this stream) and the agent branch for them
        starts on the agent stream under the replay."""
        main = torch.cuda.current_stream()
        if self.pipeline_agents and self._prefetched and self._weights_seen != self.model.weights_version:
            self._prefetched = False                 # the prefetched encoding is of the OLD weights (load_weights since): run it again
        if self.pipeline_agents and not self._prefetched:
            self.model._sync_compute_weights()       # (the branch runs in front of the replay: it needs the current compute copy now)
            self.agent_stream.wait_stream(main)
            self.prefetch_agents(batch)
        if batch is not None:
            for k, v in batch.items():
                if k in self.static and not (self.pipeline_agents and k in ('obs', 'occ')):
                    self.static[k].copy_(v, non_blocking=True)
        if self.pipeline_agents:
            main.wait_event(self.agent_done)
            for d, s_ in zip(self.agent_cur, self.agent_next):
                d.copy_(s_, non_blocking=True)
            self.agent_free.record(main)
            self._prefetched = False
            if next_batch is not None:               # the agent branch has read the static tracks (agent_done): they may be overwritten
                for k in ('obs', 'occ'):
                    if k in next_batch:
                        self.static[k].copy_(next_batch[k], non_blocking=True)
                self._staged = torch.cuda.Event()
                self._staged.record(main)
        self.graph.replay()
        if self.pipeline_agents and next_batch is not None:
            self.prefetch_agents()
        return self.out


class GraphedEvalStep:
    """hipGraph capture of the validation step (train.py:252-282): the forward pass with training=False, the fused loss + metrics pass
    (ops.eval_loss_metrics, csrc/eval.hip) and the update of the running means, which that pass's last launch does itself.  The pattern
    is GraphedForward's (warm-up on the role stream, thread-local capture errors, static inputs), and like it this class opens no stream
    of its own: the model's side streams are the only ones inside the graph (see GraphedForward on the number of distinct streams).
    That the step captures at all is the proof that it never waits for the host.

    __call__(batch=None) loads the batch and replays; .logits / .losses / .metrics are static device tensors ([B,H,W,32] f32, the
    four loss terms, the seven metrics in the order of metrics.FIELDS), .result() the means since the last reset() as a dict
    (one host sync): the four losses x loss_fn.replica under the names of evaluate.LOSS_KEYS, the metrics under evaluate.METRIC_KEYS.

    per_scene=True, capacity=N captures the per-scene pass (stj_eval_scenes_fwd) instead: .scores is an evaluate.SceneScores of N rows,
    .scene_rows the static [B,12] rows of the last replay, .live a static device int32[B].  __call__(batch, live=None) then accepts a
    batch of k <= B scenes (live = k, or the batch's own length): the first k static slots are loaded, live = [1] * k + [0] * (B - k) is
    copied in front of the replay, and the stale tail is never read by the pass.  .losses / .metrics / .result() are the pooled numbers
    of the live scenes: a last short batch is pooled over its real scenes only.  Without per_scene nothing changes."""

    KEYS = ('ogm', 'map_img', 'obs', 'occ', 'flow', 'gt_obs', 'gt_occ', 'gt_flow', 'origin_flow')

    def __init__(self, model, loss_fn, batch, warmup=2, no_warp=False, per_scene=False, capacity=0):
        from .evaluate import eval_loss_metrics
        self._pass = eval_loss_metrics
        self.model, self.loss_fn, self.no_warp, self.per_scene = model, loss_fn, no_warp, per_scene
        self.static = {k: v.clone() for k, v in batch.items() if k in self.KEYS}
        dev = self.static['ogm'].device
        self.running = torch.zeros(12, dtype=torch.float64, device=dev)      # count, 4 losses x replica, 7 metrics
        B, H, W = self.static['gt_obs'].shape[0], self.static['gt_obs'].shape[2], self.static['gt_obs'].shape[3]
        self._ws = ops.eval_workspace(B, H, W, dev) if not per_scene else ops.eval_scenes_workspace(B, H, W, dev)
        if per_scene:
            self._scene_state(B, capacity, dev)
        side = ops.role_stream(torch.cuda.current_device(), 'warmup')
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                self._eager()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.running.zero_()                 # the warm-up steps are not part of any mean
        if per_scene:
            self.scores.reset()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
            self.logits, self.losses, self.metrics = self._eager()

    def _scene_state(self, B, capacity, dev):
        from .evaluate import SceneScores
        self.scores = SceneScores(capacity, no_warp=self.no_warp, device=dev)
        self.live = torch.ones(B, dtype=torch.int32, device=dev)
        self.scene_rows = torch.zeros(B, 12, dtype=torch.float32, device=dev)
        # the pooled losses[5] and metrics[7] of a replay, then a constant 1: gathered and scaled into `running`'s layout by two launches
        self._pooled = torch.zeros(13, dtype=torch.float32, device=dev)
        self._pooled[12] = 1.0
        self._pick = torch.tensor([12, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11], device=dev)
        r = float(self.loss_fn.replica)
        self._scale = torch.tensor([1.0] + [r] * 4 + [1.0] * 7, dtype=torch.float64, device=dev)

    def _eager_scenes(self, out):
        from .evaluate import eval_scene_loss_metrics
        x = self.static
        d, m = eval_scene_loss_metrics(self.loss_fn, get_pred_waypoint_logits(out),
                                       warpped_gt(x['gt_obs'], x['gt_occ'], x['gt_flow'], x['origin_flow']), self.scores, live=self.live,
                                       no_warp=self.no_warp, workspace=self._ws, rows=self.scene_rows, pooled_out=self._pooled[:12])
        self.running.addcmul_(self._pooled[self._pick].double(), self._scale)       # count, 4 losses x replica, 7 metrics
        return out, d.packed, m.values

    def _eager(self):
        x = self.static
        out = self.model(x['ogm'], x['map_img'], training=False, obs=x['obs'], occ=x['occ'], mapt=None, flow=x['flow'])
        if self.per_scene:
            return self._eager_scenes(out)
        d, m = self._pass(self.loss_fn, get_pred_waypoint_logits(out), warpped_gt(x['gt_obs'], x['gt_occ'], x['gt_flow'], x['origin_flow']),
                          no_warp=self.no_warp, running=self.running, workspace=self._ws)
        return out, d.packed, m.values

    def load(self, batch):
        """Copy a new batch into the static input tensors (stream-ordered device copies)."""
        for k, v in batch.items():
            if k in self.static:
                self.static[k].copy_(v, non_blocking=True)

    def load_scenes(self, batch, live=None):
        """A batch of k <= B scenes into the first k static slots, live = [1] * k + [0] * (B - k); the tail keeps what it held."""
        B = self.live.numel()
        k = B
        if batch is not None:
            k = min(int(v.shape[0]) for key, v in batch.items() if key in self.static and v is not None)
            for key, v in batch.items():
                if key in self.static and v is not None:
                    self.static[key][:k].copy_(v[:k], non_blocking=True)
        if live is not None:
            k = int(live)
        if not 0 <= k <= B:
            raise ValueError(f'live = {k} scenes in a step captured for {B}')
        self.live.copy_((torch.arange(B, device=self.live.device) < k).to(torch.int32), non_blocking=True)

    def __call__(self, batch=None, live=None):
        if self.per_scene:
            self.load_scenes(batch, live)
        elif live is not None:
            raise ValueError('GraphedEvalStep: live needs per_scene=True')
        elif batch is not None:
            self.load(batch)
        self.graph.replay()
        return self.losses, self.metrics

    def result(self):
        """The means over the replays since the last reset() (0.0 each before the first), as {name: float}: one host sync."""
        from .evaluate import LOSS_KEYS, METRIC_KEYS
        r = self.running.tolist()
        n = r[0]
        keys = LOSS_KEYS + (METRIC_KEYS[:5] if self.no_warp else METRIC_KEYS)
        return {k: (v / n if n else 0.0) for k, v in zip(keys, r[1:])}

    def reset(self):
        self.running.zero_()
        if self.per_scene:
            self.scores.reset()
