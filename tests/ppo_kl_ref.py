"""fp64 numpy restatement of csrc/vn_ppo_kl.hip (include/vnav.h states the contracts): the
target-KL gate and the two optimiser steps behind its flag, and the generated cases the CPU and GPU
tests share. Pure numpy: no GPU, no library.

Every decision case keeps the fp64 KL at least CLEARANCE (relative to the limit) away from the
limit it is checked against (tests/test_ppo_kl_refs.py checks that on this reference alone): 100
times the 1e-5 the kernel's KL is held to, so the fp32 launch decides as the reference does and no
case has to be left out. The limits are 0.9 and 1.1 times the case's own fp64 KL, rounded to fp32:
one stops, one passes. With one action the KL is exactly 0 and no limit lies below it (a negative
limit is refused), so those cases carry the limit above only; their exact 0 against a limit of 0 is
a case of its own in the GPU test."""
import functools

import numpy as np

import ppo_ref as ref

CLEARANCE = 1e-3
NS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4100)  # one lane, the wave edge, the block edge, a 2nd and 3rd stride
AS = ref.AS
SCALES = ref.SCALES
STEP_NS = (1, 255, 256, 257, 70001)


def kl_terms(out, out_old, actions, A):
    """expm1(d_i) - d_i, d_i = logp_a - logp_old_a: the terms of the k3 estimate (ppo_ref.loss_grad's
    terms[4])."""
    out, out_old = np.asarray(out, np.float64), np.asarray(out_old, np.float64)
    idx, a = np.arange(out.shape[0]), np.asarray(actions)
    d = ref.softmax_stats(out[:, :A])[1][idx, a] - ref.softmax_stats(out_old[:, :A])[1][idx, a]
    return np.expm1(d) - d


def kl(out, out_old, actions, A):
    t = kl_terms(out, out_old, actions, A)
    return float(t.sum() / t.size)


def gate(out, out_old, actions, A, limit, gate2=(0, 0), kl2=(0.0, 0.0)):
    """vn_ppo_kl_gate in fp64: the new ([stopped, steps_allowed], [kl, kl at the stop])."""
    gate2, kl2 = [int(x) for x in gate2], [float(x) for x in kl2]
    if gate2[0] != 0:  # sticky: nothing is written
        return gate2, kl2
    k = kl(out, out_old, actions, A)
    kl2[0] = k
    if k > float(limit):
        gate2[0], kl2[1] = 1, k
    else:
        gate2[1] += 1
    return gate2, kl2


def rmsprop_step(p, g, sq, coef, lr, alpha, eps):
    """One vn_rmsprop_step_dev in fp64: (p, square_avg)."""
    p, g, sq = (np.asarray(x, np.float64) for x in (p, g, sq))
    g = g * float(coef)
    sq = float(alpha) * sq + (1.0 - float(alpha)) * g * g
    return p - float(lr) * g / (np.sqrt(sq) + float(eps)), sq


def rmsprop_step_gated(p, g, sq, coef, lr, alpha, eps, skip):
    if skip:
        return np.asarray(p, np.float64), np.asarray(sq, np.float64)
    return rmsprop_step(p, g, sq, coef, lr, alpha, eps)


def adam_step_gated(p, g, m, v, t, coef, lr, beta1, beta2, eps, skip):
    """One vn_adam_step_gated in fp64: (p, m, v, the step count after the call)."""
    if skip:
        return np.asarray(p, np.float64), np.asarray(m, np.float64), np.asarray(v, np.float64), int(t)
    p, m, v, _ = ref.adam_step(p, g, m, v, t, coef, lr, beta1, beta2, eps)
    return p, m, v, int(t) + 1


@functools.lru_cache(maxsize=None)
def case(n, A, scale):
    """(out, out_old, actions, kl64, mean magnitude of the terms, limits) of one generated case: the
    float32 inputs of ppo_ref's draw (the unused columns poisoned), and the fp32 limits the decision
    is checked at. The KL has no branch per sample, so the draw needs none of ppo_ref.case's margins."""
    out, out_old, actions, _ = ref._draw(n, A, scale, 1000 * n + 10 * A + int(scale))
    for x in (out, out_old, actions):
        x.setflags(write=False)
    t = kl_terms(out, out_old, actions, A)
    k = float(t.sum() / n)
    limits = (np.float32(1.0),) if A == 1 else (np.float32(0.9 * k), np.float32(1.1 * k))
    return out, out_old, actions, k, float(np.abs(t).sum() / n), limits


def all_cases():
    return [(n, A, s) for n in NS for A in AS for s in SCALES]


def decision_cases():
    """Every (n, A, scale, limit) a decision is checked at."""
    return [(n, A, s, lim) for n, A, s in all_cases() for lim in case(n, A, s)[5]]
