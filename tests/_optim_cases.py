"""Float64 references, in plain Python / NumPy, for the device-state Nadam step (csrc/optim.hip, strajnet_amd/optim.py: DeviceNadam and
the schedules), shared by test_optim_ref.py (the references themselves against hand-derived values, on the CPU) and test_optim_gpu.py.
Nothing here imports the product.

    cosine_restarts / custom_schedule    lr_schedule.py:37-76 / :13-17 at a 0-based step
    schedule_values(sched, step)         the value(s) a step may take: one, except where a geometric CosineDecayRestarts sits on a restart
    RefState                             the scalar bookkeeping of one step (Keras Nadam, SURVEY App. C-8, plus clip / skip) -> coefficients
    RefNadam                             RefState + the element update over float64 arrays
    rel_err                              the measure of tests/test_ops_gpu.py (test_nadam_step_matches_keras_formula's gate is rel_err < 1e-5)

beta_1 and beta_2 cross the C ABI as floats, and the element update multiplies by those float values; the references therefore take the
betas ROUNDED TO FLOAT32 (as Keras, which holds them in float32, does) and compute everything else in float64.
"""
import math

import numpy as np

PARTS = 256                       # STJ_GRADNORM_PARTS
# the scalar tail alone (1, 3); 250 vectors + a tail of 3; the grid-stride loop past the update kernel's 4096-workgroup cap, tail of 1
SIZES = (1, 3, 1003, 4 * 256 * 4096 + 1029)
BOUNDARY_EPS = 1e-9               # a geometric restart whose float64 log-argument is this close to an integer may fall on either side

# (kind, parameters...) -- the `sched` block's contents
CONSTANT = ('constant', 1e-3)
COS_ARITH = ('cosine', 1e-3, 10.0, 1.0, 0.5, 0.1)              # t_mul = 1: restarts every 10 steps, floor() of an exact quotient
COS_GEOM = ('cosine', 1e-3, 10.0, 2.0, 0.9, 0.0)               # restarts at 10, 30, 70
COS_TRAIN = ('cosine', 1e-4, 45657.0, 1.25, 0.99, 0.0)         # train.py:185-186: int(30438 * 1.5); first restart at 45657
CUSTOM = ('custom', 384.0, 4000.0)


def f32(x):
    return float(np.float32(x))


def _cosine_at(i_restart, frac, lr0, t_mul, m_mul, alpha, geometric):
    if geometric:
        length = t_mul ** i_restart
        frac = (frac - (1.0 - length) / (1.0 - t_mul)) / length
    else:
        frac = frac - i_restart
    cosine = 0.5 * m_mul ** i_restart * (1.0 + math.cos(math.pi * frac))
    return lr0 * ((1.0 - alpha) * cosine + alpha)


def _restart_index(step, first, t_mul):
    """-> (i_restart, on_boundary).  Geometric: floor(log(1 - frac (1 - t_mul)) / log(t_mul)); on_boundary when that quotient is within
    BOUNDARY_EPS of an integer >= 1 (the function is discontinuous there and the last bit of a logarithm decides the side; step 0 is no
    restart: log(1) is exactly 0 in any arithmetic)."""
    frac = float(step) / first
    if t_mul == 1.0:
        return math.floor(frac), False
    q = math.log(1.0 - frac * (1.0 - t_mul)) / math.log(t_mul)
    return math.floor(q), round(q) >= 1 and abs(q - round(q)) < BOUNDARY_EPS


def cosine_restarts(step, lr0, first, t_mul=2.0, m_mul=1.0, alpha=0.0):
    i, _ = _restart_index(step, first, t_mul)
    return _cosine_at(i, float(step) / first, lr0, t_mul, m_mul, alpha, t_mul != 1.0)


def custom_schedule(step, d_model, warmup=4000.0):
    step = float(step)
    arg1 = math.inf if step == 0.0 else 1.0 / math.sqrt(step)
    return (1.0 / math.sqrt(d_model)) * min(arg1, step * warmup ** -1.5)


def schedule_values(sched, step):
    """Every value the schedule may take at `step`: one, or the two neighbouring restarts' values on a geometric boundary."""
    if sched[0] == 'constant':
        return [sched[1]]
    if sched[0] == 'custom':
        return [custom_schedule(step, *sched[1:])]
    lr0, first, t_mul, m_mul, alpha = sched[1:]
    i, boundary = _restart_index(step, first, t_mul)
    if not boundary:
        return [_cosine_at(i, float(step) / first, lr0, t_mul, m_mul, alpha, t_mul != 1.0)]
    r = round(math.log(1.0 - float(step) / first * (1.0 - t_mul)) / math.log(t_mul))
    return [_cosine_at(k, float(step) / first, lr0, t_mul, m_mul, alpha, True) for k in (r - 1, r)]


def schedule(sched, step):
    return schedule_values(sched, step)[-1]           # on a boundary: the new restart's value (what exact arithmetic gives)


def encode(sched):
    """The `sched` block (double[8]) of include/strajnet_hip.h."""
    kind = {'constant': 0.0, 'cosine': 1.0, 'custom': 2.0}[sched[0]]
    body = list(sched[1:])
    return np.array([kind] + body + [0.0] * (7 - len(body)), dtype=np.float64)


def mu(t, b1):
    return b1 * (1.0 - 0.5 * 0.96 ** (0.004 * t))


def m_schedule_after(t, b1):
    """prod of mu_1 .. mu_t: the state's [1] after t updates."""
    p = 1.0
    for k in range(1, t + 1):
        p *= mu(k, b1)
    return p


class RefState:
    """state double[8] and one step's bookkeeping, as the header states it."""

    def __init__(self, sched, beta_1=0.9, beta_2=0.999, clipnorm=None, skip_nonfinite=False, iterations=0):
        self.sched, self.b1, self.b2 = sched, f32(beta_1), f32(beta_2)
        self.clipnorm, self.skip_nonfinite = clipnorm, skip_nonfinite
        self.iterations, self.m_schedule = iterations, m_schedule_after(iterations, self.b1)
        self.skipped, self.grad_norm, self.lr = 0, 0.0, 0.0
        self.lr_values = [0.0]

    def state(self):
        return np.array([self.iterations, self.m_schedule, self.skipped, self.grad_norm, self.lr, 0.0, 0.0, 0.0])

    def prepare(self, sumsq=None, gscale=1.0):
        """-> coef (lr, cg, cm, vhat_scale, gscale, apply) in float64.  sumsq None: no norm, no clip, no skip."""
        gscale = f32(gscale)
        if sumsq is None:
            self.grad_norm = 0.0
        else:
            self.grad_norm = math.nan if math.isnan(sumsq) else gscale * math.sqrt(sumsq)
        if sumsq is not None and self.skip_nonfinite and not math.isfinite(sumsq):
            self.skipped += 1
            return (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        if sumsq is not None and self.clipnorm is not None:
            c = f32(self.clipnorm)
            gscale = gscale * (c / (self.grad_norm if self.grad_norm > c else c))       # max(norm, c), a NaN norm giving c
        t = self.iterations + 1
        self.lr_values = schedule_values(self.sched, self.iterations)
        self.lr = self.lr_values[-1]
        mu_t, mu_n = mu(t, self.b1), mu(t + 1, self.b1)
        prod_t = self.m_schedule * mu_t
        prod_n = prod_t * mu_n
        self.iterations, self.m_schedule = t, prod_t
        return (self.lr, (1.0 - mu_t) / (1.0 - prod_t), mu_n / (1.0 - prod_n), 1.0 / (1.0 - self.b2 ** t), gscale, 1.0)


class RefNadam:
    """The full update in float64 over NumPy arrays: w, m, v and a RefState."""

    def __init__(self, w, sched, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, skip_nonfinite=False):
        self.w = np.array(w, dtype=np.float64)
        self.m, self.v = np.zeros_like(self.w), np.zeros_like(self.w)
        self.s = RefState(sched, beta_1, beta_2, clipnorm, skip_nonfinite)
        self.eps = f32(epsilon)
        self.norm = clipnorm is not None or skip_nonfinite

    def step(self, g, gscale=1.0, w=None):
        """g: the float32 gradient the device saw.  w: start this update from these weights instead of the reference's own."""
        g = np.asarray(g, dtype=np.float64)
        if w is not None:
            self.w = np.array(w, dtype=np.float64)
        with np.errstate(all='ignore'):
            lr, cg, cm, vs, gs, apply = self.s.prepare(float(np.sum(g * g)) if self.norm else None, gscale)
            if not apply:
                return self.w
            b1, b2 = self.s.b1, self.s.b2
            gg = g * gs
            self.m = b1 * self.m + (1.0 - b1) * gg
            self.v = b2 * self.v + (1.0 - b2) * gg * gg
            self.w = self.w - lr * (cg * gg + cm * self.m) / (np.sqrt(self.v * vs) + self.eps)
        return self.w


RMS_WEIGHT = 2.5


def rel_err(a, ref):
    """max( max |a - ref| / max |ref| , 2.5 rms(a - ref) / rms(ref) ): tests/test_ops_gpu.py's measure, on NumPy arrays."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = a - ref
    e_max = float(np.abs(d).max() / (np.abs(ref).max() + 1e-12))
    e_rms = float(np.sqrt(np.mean(d * d)) / (np.sqrt(np.mean(ref * ref)) + 1e-12))
    return max(e_max, RMS_WEIGHT * e_rms)


def close(x, want, rel):
    """|x - want| <= rel |want| (want == 0: x == 0)."""
    return abs(x - want) <= rel * abs(want)


def gradient(n, seed):
    """A seeded float32 gradient of n elements, N(0, 1)."""
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)
