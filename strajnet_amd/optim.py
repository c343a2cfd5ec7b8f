"""Fused Keras-Nadam step over the model's flat parameter / gradient buffers.

Reference: train.py:197,224 -- `tf.keras.optimizers.Nadam(learning_rate=1e-4)` applied to all trainable variables after
the cross-replica gradient SUM.  Keras defaults beta_1 .9, beta_2 .999, epsilon 1e-7, momentum-cache schedule
mu_t = beta_1 (1 - 0.5 * 0.96^(0.004 t)).  One HIP launch (stj_nadam_step) updates every tensor: the
parameters are slices of ONE flat f32 buffer and their gradients of another (the all-reduce bucket).

Nadam keeps its step counter and momentum-cache product on the host and hands stj_nadam_step by-value coefficients: a hipGraph would
freeze them at capture time.  DeviceNadam keeps that state on the device (csrc/optim.hip): a one-workgroup launch advances it,
evaluates the learning-rate schedule (CosineDecayRestarts / CustomSchedule: lr_schedule.py) and writes the coefficients the update
launch reads, so step() is launches only and the whole of train.py:199-230 captures as one graph (graph.GraphedTrainStep(optimizer=))."""
import math

import torch

from ._lib import ENUMS
from .ops import _p, _st, call

_OPT = ENUMS['stj_optim']
LOSS_MEAN_KEYS = ('train_loss', 'train_loss_occ', 'train_loss_flow', 'train_loss_wp')      # train.py:159-162, in the order of train.py:226-229


class Nadam:
    def __init__(self, flat_weights, flat_grads, lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        if flat_weights.dtype != torch.float32 or flat_grads.dtype != torch.float32 or flat_weights.shape != flat_grads.shape:
            raise ValueError('Nadam needs matching flat float32 weight and gradient buffers')
        if not flat_weights.is_cuda:
            raise RuntimeError('Nadam: CUDA (ROCm) buffers only: the HIP path has no CPU fallback')
        self.w, self.g = flat_weights, flat_grads
        self.lr, self.b1, self.b2, self.eps = float(lr), float(beta_1), float(beta_2), float(epsilon)
        self.m = torch.zeros_like(flat_weights)
        self.v = torch.zeros_like(flat_weights)
        self.t = 0
        self.m_schedule = 1.0

    @classmethod
    def for_model(cls, model, **kw):
        """Optimizer over every parameter of a strajnet_amd.STrajNet (its flat master / gradient buffers)."""
        return cls(model._flat, model._gflat, **kw)

    def _mu(self, t):
        return self.b1 * (1.0 - 0.5 * 0.96 ** (0.004 * t))

    def step(self, grad_scale=1.0):
        self.t += 1
        mu_t, mu_n = self._mu(self.t), self._mu(self.t + 1)
        sched_t = self.m_schedule * mu_t
        sched_n = sched_t * mu_n
        self.m_schedule = sched_t
        cg = (1.0 - mu_t) / (1.0 - sched_t)
        cm = mu_n / (1.0 - sched_n)
        vs = 1.0 / (1.0 - self.b2 ** self.t)
        call('stj_nadam_step', _p(self.w), _p(self.g), _p(self.m), _p(self.v), self.w.numel(), self.lr, self.b1, self.b2, self.eps,
             cg, cm, vs, float(grad_scale), _st())


class CosineDecayRestarts:
    """lr_schedule.py:19-76 (tf.keras CosineDecayRestarts, SGDR): __call__(step) is the learning rate at the 0-based step, on the host in
    float64; encode() the same schedule as DeviceNadam's `sched` block, which the device evaluates in float64 too.  TensorFlow
    evaluates these formulas in float32: the float64 result here and on the device is the better-rounded one, within float32
    rounding of TensorFlow's -- except right at a restart of a geometric (t_mul != 1) schedule, where floor(log(.) / log(t_mul)) of a
    value within rounding of an integer can fall on either side in any precision."""

    def __init__(self, initial_learning_rate, first_decay_steps, t_mul=2.0, m_mul=1.0, alpha=0.0):
        self.initial_learning_rate, self.first_decay_steps = float(initial_learning_rate), float(first_decay_steps)
        self.t_mul, self.m_mul, self.alpha = float(t_mul), float(m_mul), float(alpha)
        if self.first_decay_steps <= 0 or self.t_mul <= 0:
            raise ValueError('CosineDecayRestarts: first_decay_steps and t_mul must be positive')

    def __call__(self, step):
        frac = float(step) / self.first_decay_steps
        if self.t_mul == 1.0:
            i_restart = math.floor(frac)
            frac -= i_restart
        else:
            i_restart = math.floor(math.log(1.0 - frac * (1.0 - self.t_mul)) / math.log(self.t_mul))
            length = self.t_mul ** i_restart
            frac = (frac - (1.0 - length) / (1.0 - self.t_mul)) / length
        cosine = 0.5 * self.m_mul ** i_restart * (1.0 + math.cos(math.pi * frac))
        return self.initial_learning_rate * ((1.0 - self.alpha) * cosine + self.alpha)

    def encode(self):
        return [_OPT['STJ_SCHED_COSINE_RESTARTS'], self.initial_learning_rate, self.first_decay_steps, self.t_mul, self.m_mul, self.alpha, 0.0, 0.0]


class CustomSchedule:
    """lr_schedule.py:4-17 (the Transformer warm-up): rsqrt(d_model) * min(rsqrt(step), step * warmup_steps^-1.5); 0 at step 0, from
    min(inf, 0).  Host __call__ and device evaluation in float64, as CosineDecayRestarts."""

    def __init__(self, d_model, warmup_steps=4000):
        self.d_model, self.warmup_steps = float(d_model), float(warmup_steps)
        if self.d_model <= 0 or self.warmup_steps <= 0:
            raise ValueError('CustomSchedule: d_model and warmup_steps must be positive')

    def __call__(self, step):
        step = float(step)
        arg1 = math.inf if step == 0.0 else 1.0 / math.sqrt(step)
        return (1.0 / math.sqrt(self.d_model)) * min(arg1, step * self.warmup_steps ** -1.5)

    def encode(self):
        return [_OPT['STJ_SCHED_CUSTOM'], self.d_model, self.warmup_steps, 0.0, 0.0, 0.0, 0.0, 0.0]


class DeviceNadam:
    """Nadam with the same update and every scalar of its state on the device (include/strajnet_hip.h: state, sched, coef, running).

    lr: a float or a schedule object (CosineDecayRestarts, CustomSchedule; evaluated at `iterations`, 0-based, as Keras does).
    global_clipnorm: tf.clip_by_global_norm over the whole flat gradient (after grad_scale); a step whose norm is within it is
    bit-identical to an unclipped one.  skip_nonfinite: a step whose gradient holds a NaN or an infinity changes nothing but the
    `skipped` count (and the loss means) -- decided on the device, so no host sync guards the f32 master weights and moments.
    step() is 2 launches (prepare, apply), 3 with a clip or the skip (the gradient's sum of squares first); it allocates nothing,
    reads nothing back and can be captured into a hipGraph.  iterations / lr / grad_norm / skipped are 0-d views of `state`:
    float(opt.lr) is where the host waits."""

    capturable = True

    def __init__(self, flat_weights, flat_grads, lr=1e-4, beta_1=0.9, beta_2=0.999, epsilon=1e-7, global_clipnorm=None, skip_nonfinite=False):
        if flat_weights.dtype != torch.float32 or flat_grads.dtype != torch.float32 or flat_weights.shape != flat_grads.shape:
            raise ValueError('DeviceNadam needs matching flat float32 weight and gradient buffers')
        if not flat_weights.is_cuda or not flat_grads.is_cuda:
            raise RuntimeError('DeviceNadam: CUDA (ROCm) buffers only: the HIP path has no CPU fallback')
        if flat_weights.device != flat_grads.device or not flat_weights.is_contiguous() or not flat_grads.is_contiguous():
            raise ValueError('DeviceNadam needs contiguous weight and gradient buffers on one device')
        if global_clipnorm is not None and not float(global_clipnorm) > 0.0:
            raise ValueError('DeviceNadam: global_clipnorm must be positive (None: no clipping)')
        self.w, self.g = flat_weights, flat_grads
        self.schedule = lr if hasattr(lr, 'encode') else None
        self.b1, self.b2, self.eps = float(beta_1), float(beta_2), float(epsilon)
        self.clipnorm = 0.0 if global_clipnorm is None else float(global_clipnorm)
        self.skip_nonfinite = bool(skip_nonfinite)
        dev = flat_weights.device
        self.m = torch.zeros_like(flat_weights)
        self.v = torch.zeros_like(flat_weights)
        sched = self.schedule.encode() if self.schedule is not None else [_OPT['STJ_SCHED_CONSTANT'], float(lr)] + [0.0] * 6
        self.state = torch.tensor([0.0, 1.0] + [0.0] * 6, dtype=torch.float64).to(dev)
        self.sched = torch.tensor(sched, dtype=torch.float64).to(dev)
        self.coef = torch.zeros(8, dtype=torch.float32, device=dev)
        self.partials = torch.zeros(_OPT['STJ_GRADNORM_PARTS'], dtype=torch.float64, device=dev)
        self.running = torch.zeros(5, dtype=torch.float64, device=dev)
        self.loss_scale = None           # not None: the loss means are on (attach_loss_means)
        self._losses = None

    @classmethod
    def for_model(cls, model, **kw):
        """Optimizer over every parameter of a strajnet_amd.STrajNet (its flat master / gradient buffers)."""
        return cls(model._flat, model._gflat, **kw)

    iterations = property(lambda self: self.state[0], doc='updates applied (device scalar)')
    skipped = property(lambda self: self.state[2], doc='steps skipped for a non-finite gradient (device scalar)')
    grad_norm = property(lambda self: self.state[3], doc='global gradient norm of the last step, after grad_scale and before clipping; 0 '
                                                         'when neither global_clipnorm nor skip_nonfinite asks for it (device scalar)')
    lr = property(lambda self: self.state[4], doc='learning rate of the last applied step (device scalar)')

    def step(self, grad_scale=1.0):
        st, n = _st(), self.w.numel()
        partials = None
        if self.clipnorm > 0.0 or self.skip_nonfinite:
            partials = self.partials
            call('stj_gradnorm_partials', _p(self.g), n, _p(partials), st)
        means = self.loss_scale is not None
        if means and self._losses is None:
            raise RuntimeError('DeviceNadam: the loss means are on but no loss tensor is attached (attach_loss_means(losses, loss_scale))')
        call('stj_nadam_prepare', _p(self.state), _p(self.sched), _p(partials), _p(self.coef), _p(self._losses if means else None),
             _p(self.running if means else None), self.b1, self.b2, float(grad_scale), self.clipnorm, self.loss_scale if means else 1.0,
             _OPT['STJ_NADAM_SKIP_NONFINITE'] if self.skip_nonfinite else 0, st)
        call('stj_nadam_apply', _p(self.w), _p(self.g), _p(self.m), _p(self.v), n, _p(self.coef), self.b1, self.b2, self.eps, st)

    # ---- the four train-loss means of train.py:159-162,226-229, kept by the prepare launch
    def attach_loss_means(self, losses, loss_scale=1.0):
        """Every later step() adds `losses` (f32[4] on the device: observed_xe, occluded_xe, flow, flow_warp_xe -- LossDict.packed) x
        loss_scale (train.py:226-229 `* REPLICA`) to the running sums, skipped steps included.  losses=None turns the means on and
        leaves the tensor to whoever runs the step (training.train_step, graph.GraphedTrainStep: each pass's LossDict.packed)."""
        if losses is not None:
            if losses.dtype != torch.float32 or losses.numel() != 4 or not losses.is_contiguous() or losses.device != self.w.device:
                raise ValueError('DeviceNadam.attach_loss_means: losses must be a contiguous float32[4] on the optimizer\'s device')
        self._losses, self.loss_scale = losses, float(loss_scale)

    def loss_result(self):
        """The means since the last reset_loss_means() (0.0 each before the first step) under train.py:159-162's names: one host sync."""
        r = self.running.tolist()
        return {k: (v / r[0] if r[0] else 0.0) for k, v in zip(LOSS_MEAN_KEYS, r[1:])}

    def reset_loss_means(self):
        self.running.zero_()

    # ---- checkpointing
    def tensors(self):
        """Everything a step changes: weights, both moments, the scalar state, the running loss sums (graph.GraphedTrainStep snapshots
        them around its warm-up passes)."""
        return [self.w, self.m, self.v, self.state, self.running]

    def state_dict(self):
        """m, v and state on the host (pinned copies behind ONE stream synchronisation)."""
        src = {'m': self.m, 'v': self.v, 'state': self.state}
        out = {k: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for k, t in src.items()}
        for k, t in src.items():
            out[k].copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.w.device).synchronize()
        return out

    def load_state_dict(self, sd):
        dst = {'m': self.m, 'v': self.v, 'state': self.state}
        for k, t in dst.items():
            if k not in sd or tuple(sd[k].shape) != tuple(t.shape) or sd[k].dtype != t.dtype:
                raise ValueError(f'DeviceNadam.load_state_dict: {k} missing or of another shape / dtype')
        for k, t in dst.items():
            t.copy_(sd[k], non_blocking=True)
        torch.cuda.current_stream(self.w.device).synchronize()
