"""The float64 references of _optim_cases.py and the host __call__ of optim.CosineDecayRestarts / optim.CustomSchedule against answers
derived by hand from lr_schedule.py:37-76 and :13-17, to 1e-12 relative -- on the CPU.  test_optim_gpu.py judges the kernels by these.

CosineDecayRestarts(1e-3, 10, t_mul=1, m_mul=.5, alpha=.1): lr = 1e-3 (.9 * .5 m_fac (1 + cos(pi frac)) + .1)
    step 0: frac 0, m_fac 1 -> 1e-3;  step 5: frac .5 -> 1e-3 (.45 + .1);  step 10: restart 1, frac 0, m_fac .5 -> the same 5.5e-4;
    step 15: restart 1, frac .5 -> 1e-3 (.9 * .25 + .1) = 3.25e-4.
CosineDecayRestarts(1e-3, 10, t_mul=2, m_mul=.9): periods 10, 20, 40 starting at 0, 10, 30
    step 11: restart 1, frac .05 -> 1e-3 * .45 (1 + cos(.05 pi));  step 20: restart 1, frac .5 -> 4.5e-4;
    step 31: restart 2, frac .025 -> 1e-3 * .405 (1 + cos(.025 pi)).
CustomSchedule(384): 384^-.5 min(step^-.5, step 4000^-1.5): 0 at step 0; the two arguments meet at step 4000.
"""
import math

import pytest

import _optim_cases as OC

REL = 1e-12

HAND = [
    (OC.COS_ARITH, 0, 1e-3), (OC.COS_ARITH, 5, 5.5e-4), (OC.COS_ARITH, 10, 5.5e-4), (OC.COS_ARITH, 15, 3.25e-4),
    (OC.COS_GEOM, 11, 8.944597532678e-4), (OC.COS_GEOM, 20, 4.5e-4), (OC.COS_GEOM, 31, 8.087515201619e-4),
    (OC.COS_TRAIN, 22828, 5.00017202141e-5), (OC.COS_TRAIN, 200000, 7.81523969223e-5),
    (OC.CUSTOM, 0, 0.0), (OC.CUSTOM, 4000, 8.068715304599e-4), (OC.CUSTOM, 100000, 1.613743060920e-4),
]


def _product_schedule(sched):
    from strajnet_amd.optim import CosineDecayRestarts, CustomSchedule
    if sched[0] == 'cosine':
        return CosineDecayRestarts(sched[1], sched[2], t_mul=sched[3], m_mul=sched[4], alpha=sched[5])
    return CustomSchedule(sched[1], warmup_steps=sched[2])


@pytest.mark.parametrize('sched,step,want', HAND)
def test_schedules_match_hand_derived_values(sched, step, want):
    ref = OC.schedule(sched, step)
    host = _product_schedule(sched)(step)
    print(f'{sched} step {step}: reference {ref!r} host {host!r} hand {want!r}')
    assert OC.close(ref, want, REL)
    assert OC.close(host, want, REL)


def test_closed_forms_of_the_hand_values():
    """The decimal constants above are these expressions."""
    assert OC.close(8.944597532678e-4, 1e-3 * 0.45 * (1.0 + math.cos(0.05 * math.pi)), REL)
    assert OC.close(8.087515201619e-4, 1e-3 * 0.405 * (1.0 + math.cos(0.025 * math.pi)), REL)
    assert OC.close(8.068715304599e-4, 1.0 / math.sqrt(384.0 * 4000.0), REL)
    assert OC.close(1.613743060920e-4, 1.0 / math.sqrt(384.0 * 100000.0), REL)


def test_schedule_encoding_is_the_header_layout():
    from strajnet_amd import _lib
    kinds = _lib.ENUMS['stj_optim']
    assert (kinds['STJ_SCHED_CONSTANT'], kinds['STJ_SCHED_COSINE_RESTARTS'], kinds['STJ_SCHED_CUSTOM']) == (0, 1, 2)
    assert kinds['STJ_GRADNORM_PARTS'] == OC.PARTS
    for sched in (OC.COS_ARITH, OC.COS_GEOM, OC.COS_TRAIN, OC.CUSTOM):
        assert _product_schedule(sched).encode() == OC.encode(sched).tolist()


def test_boundaries_are_where_the_issue_says():
    """Either-side acceptance applies at the geometric restarts only: 10, 30, 70 of the t_mul = 2 case, 45657 of train.py's; every step
    of a t_mul = 1 schedule and every other step has ONE value."""
    assert [s for s in range(0, 100) if len(OC.schedule_values(OC.COS_GEOM, s)) == 2] == [10, 30, 70]
    assert [s for s in range(45600, 45700) if len(OC.schedule_values(OC.COS_TRAIN, s)) == 2] == [45657]
    assert all(len(OC.schedule_values(OC.COS_ARITH, s)) == 1 for s in range(0, 100))
    # the two sides at step 30: the old period's end (frac 1: alpha's floor, here 0) and the new one's start (m_fac .81)
    lo, hi = OC.schedule_values(OC.COS_GEOM, 30)
    assert lo == 0.0 and OC.close(hi, 1e-3 * 0.81, REL)


def test_nadam_coefficients_first_steps():
    """t = 1 with beta_1 = .9, beta_2 = .999 as float32: mu_1 = b1 (1 - .5 .96^.004), prod_1 = mu_1, cg = 1 (the first gradient is
    unbiased: (1 - mu_1) / (1 - prod_1)), vhat_scale = 1 / (1 - b2)."""
    s = OC.RefState(OC.CONSTANT)
    lr, cg, cm, vs, gs, apply = s.prepare()
    b1, b2 = OC.f32(0.9), OC.f32(0.999)
    mu1, mu2 = b1 * (1 - 0.5 * 0.96 ** 0.004), b1 * (1 - 0.5 * 0.96 ** 0.008)
    assert (lr, cg, gs, apply) == (1e-3, 1.0, 1.0, 1.0)
    assert OC.close(cm, mu2 / (1 - mu1 * mu2), REL) and OC.close(vs, 1 / (1 - b2), REL)
    assert s.state().tolist()[:5] == [1, mu1, 0, 0.0, 1e-3]
    assert OC.close(OC.m_schedule_after(2, b1), mu1 * mu2, REL)


def test_reference_clip_and_skip():
    import numpy as np
    g = np.array([3.0, 4.0], dtype=np.float32)                 # norm 5
    a = OC.RefNadam([1.0, 1.0], OC.CONSTANT, clipnorm=1.0)
    b = OC.RefNadam([1.0, 1.0], OC.CONSTANT)
    assert np.array_equal(a.step(g), b.step(g / 5.0)) and a.s.grad_norm == 5.0
    c = OC.RefNadam([1.0, 1.0], OC.CONSTANT, clipnorm=10.0)    # within the norm: the unclipped step
    d = OC.RefNadam([1.0, 1.0], OC.CONSTANT)
    assert np.array_equal(c.step(g), d.step(g))
    e = OC.RefNadam([1.0, 1.0], OC.CONSTANT, skip_nonfinite=True)
    w = e.step(np.array([np.nan, 1.0], dtype=np.float32))
    assert w.tolist() == [1.0, 1.0] and e.s.skipped == 1 and e.s.iterations == 0 and math.isnan(e.s.grad_norm)
    e.step(g)
    assert e.s.iterations == 1 and e.s.skipped == 1
