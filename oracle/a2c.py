"""A2C update restated in torch fp32 on the CPU (TEST INFRASTRUCTURE ONLY).

PARITY UNPINNED: the reference's trainer math lives in the absent deep-rl==0.2.9
(experiments/thor_cached_auxiliary.py:2-18,26-42 import it). This file states the
standard A2C the engine implements (DESIGN.md "A2C contract"), with the reference's
hyper-parameters (thor_cached_auxiliary.py:29-37):
  returns    R_T = V(s_T);  R_t = r_t + gamma * R_{t+1} * (1 - done_t)
  advantage  A_t = R_t - V(s_t)
  loss       L = value_coef * mean(A^2) - mean(A.detach() * log pi(a_t|s_t))
                 - entropy_coef * mean(H(pi(.|s_t)))
  clip       torch.nn.utils.clip_grad_norm_(params, max_norm)      (max_norm 0.5)
  optimizer  torch.optim.RMSprop(lr, alpha=0.99, eps=1e-5)         (lr 7e-4 -> 0 linear)

The second half (returns64 ... categorical_draw64) restates each A2C step / update kernel
in numpy float64 without autograd: the references of tests/test_a2c_kernels_gpu.py, checked
against the torch restatements above by tests/test_a2c_refs.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import philox


def returns(rewards, dones, values_ext, gamma):
    """rewards, dones [T,E]; values_ext [T+1,E] (last row = bootstrap) -> returns [T,E]."""
    T = rewards.shape[0]
    R = values_ext[T].clone()
    out = torch.empty_like(rewards)
    for t in range(T - 1, -1, -1):
        R = rewards[t] + gamma * R * (1.0 - dones[t].to(rewards.dtype))
        out[t] = R
    return out


def loss(logits, values, actions, rets, value_coef=0.5, entropy_coef=0.01):
    """logits [N,A], values [N], actions [N] long, rets [N] -> (loss, stats dict)."""
    logp_all = F.log_softmax(logits, dim=-1)
    p = logp_all.exp()
    logp = logp_all.gather(1, actions.view(-1, 1)).squeeze(1)
    ent = -(p * logp_all).sum(-1)
    adv = rets - values
    value_loss = adv.pow(2).mean()
    action_loss = -(adv.detach() * logp).mean()
    entropy = ent.mean()
    total = value_coef * value_loss + action_loss - entropy_coef * entropy
    return total, dict(value_loss=value_loss, action_loss=action_loss, entropy=entropy)


def clip_and_rmsprop(params, grads, square_avg, lr, max_norm=0.5, alpha=0.99, eps=1e-5):
    """In-place on lists of tensors; returns the pre-clip total norm."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).float()
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    for p, g, s in zip(params, grads, square_avg):
        g = g * coef
        s.mul_(alpha).addcmul_(g, g, value=1 - alpha)
        p.addcdiv_(g, s.sqrt().add_(eps), value=-lr)
    return total


# ---- float64 restatements of the A2C step / update kernels (numpy, no autograd) ----------
# Every function takes its inputs as the float32 values the kernel reads (gamma, the
# coefficients and scale are cast through np.float32 first) and computes in float64, so the
# only difference to the kernel is the kernel's own fp32 arithmetic.

def _f32(x):
    return float(np.float32(x))


def returns64(rewards, dones, bootstrap_out, num_actions, gamma):
    """rewards, dones [T,E]; bootstrap_out [E,8] (value in column num_actions) -> R [T,E]."""
    r = np.asarray(rewards, dtype=np.float64)
    nd = 1.0 - (np.asarray(dones) != 0).astype(np.float64)
    g = _f32(gamma)
    R = np.asarray(bootstrap_out, dtype=np.float64)[:, num_actions].copy()
    out = np.empty_like(r)
    for t in range(r.shape[0] - 1, -1, -1):
        R = r[t] + g * R * nd[t]
        out[t] = R
    return out


def softmax_stats64(logits):
    """logits [..., A] -> (p, logp, H); p * logp := 0 where p underflows to 0. The log of
    the sum is log1p over the terms other than the (first) maximum, so a saturated
    distribution keeps the relative precision of the dominant action's log-probability
    (log(1 + s) is exactly 0 in float64 from s < 1.1e-16 on, and 1e-4 off at s = 1e-12)."""
    lg = np.asarray(logits, dtype=np.float64)
    z = lg - lg.max(-1, keepdims=True)
    e = np.exp(z)
    first = np.arange(lg.shape[-1]) == np.argmax(lg, -1)[..., None]
    logp = z - np.log1p(np.where(first, 0.0, e).sum(-1, keepdims=True))
    p = np.exp(logp)
    H = -np.where(p > 0.0, p * logp, 0.0).sum(-1)
    return p, logp, H


def loss_grad64(out, actions, returns, num_actions, value_coef, entropy_coef):
    """out [n,8] (logits 0..A-1, value at A), actions [n], returns [n] ->
    (dout [n,8], stats4, abs4): the gradient of L = vc mean(A^2) - mean(A logp_a) - ec mean(H)
    w.r.t. the head outputs, the sums over samples of (A^2, -A logp_a, H, R) and the sums of
    their magnitudes (the scale a summation error is measured against)."""
    A = int(num_actions)
    o = np.asarray(out, dtype=np.float64)
    a = np.asarray(actions, dtype=np.int64)
    R = np.asarray(returns, dtype=np.float64)
    n = o.shape[0]
    vc, ec = _f32(value_coef), _f32(entropy_coef)
    inv_n = float(np.float32(1.0) / np.float32(n))
    p, lp, H = softmax_stats64(o[:, :A])
    adv = R - o[:, A]
    ind = (np.arange(A)[None, :] == a[:, None]).astype(np.float64)
    dout = np.zeros((n, 8), dtype=np.float64)
    dout[:, :A] = (-adv[:, None] * (ind - p) + ec * p * (lp + H[:, None])) * inv_n
    dout[:, A] = vc * (-2.0 * adv) * inv_n
    terms = np.stack([adv * adv, -adv * lp[np.arange(n), a], H, R])
    return dout, terms.sum(1), np.abs(terms).sum(1)


def grad_norm64(grads, scale, max_norm):
    """(norm of scale * grads, clip coefficient): torch's clip_grad_norm_, max_norm /
    (norm + 1e-6) capped at 1; max_norm <= 0 does not clip."""
    v = np.asarray(grads, dtype=np.float64) * _f32(scale)
    norm = float(np.sqrt((v * v).sum()))
    mn = _f32(max_norm)
    coef = min(mn / (norm + _f32(1e-6)), 1.0) if mn > 0.0 else 1.0
    return norm, coef


def rmsprop64(params, grads, square_avg, coef, scale, lr, alpha, eps):
    """One clipped RMSprop step (torch's rule) -> (params', square_avg'); coef is the clip
    coefficient (scalars2[1]) and scale the gradient scale."""
    al, ep, lr = _f32(alpha), _f32(eps), _f32(lr)
    g = np.asarray(grads, dtype=np.float64) * (_f32(coef) * _f32(scale))
    s = np.asarray(square_avg, dtype=np.float64) * al + (1.0 - al) * g * g
    p = np.asarray(params, dtype=np.float64) - lr * (g / (np.sqrt(s) + ep))
    return p, s


def schedule64(state3, lr0, max_time_steps, steps_per_update, T):
    """vn_a2c_schedule: state3 = [next counter base, env-steps so far, this update's base]
    -> (state3', lr as np.float32)."""
    base, total = int(state3[0]), int(state3[1])
    frac = min(total / float(max_time_steps), 1.0) if max_time_steps > 0 else 0.0
    lr = np.float32(float(lr0) * (1.0 - frac))
    return np.array([base + int(T), total + int(steps_per_update), base], dtype=np.int64), lr


def step_post64(actions, rewards, dones, ep_return, ep_length, num_actions):
    """vn_a2c_step_post: (lra [E,A+1] = [one_hot(a) | r] * m, mask m = 1 - done [E], the
    finished episodes' (count, return sum, length sum))."""
    A = int(num_actions)
    a = np.asarray(actions, dtype=np.int64)
    d = np.asarray(dones) != 0
    m = 1.0 - d.astype(np.float64)
    r = np.asarray(rewards, dtype=np.float64)
    lra = np.zeros((a.shape[0], A + 1), dtype=np.float64)
    lra[:, :A] = (np.arange(A)[None, :] == a[:, None]) * m[:, None]
    lra[:, A] = r * m
    stats = np.array([d.sum(), np.asarray(ep_return, dtype=np.float64)[d].sum(),
                      np.asarray(ep_length, dtype=np.float64)[d].sum()], dtype=np.float64)
    return lra, m, stats


def categorical_draw64(logits, num_actions, seed, ctr, i):
    """The policy's inverse-CDF draw of samples i (array) from logits [n, >= A]: u = the top
    24 bits of Philox4x32-10 (i, ctr_lo, ctr_hi, STREAM_POLICY) under key seed; the action is
    the number of CDF boundaries c_j = p_0 + .. + p_j (j < A - 1) at or below u. Returns
    (actions, distance of u to the nearest boundary; inf when A = 1)."""
    A = int(num_actions)
    ctr = int(ctr) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = philox.seed_key(seed)
    i = np.asarray(i, dtype=np.int64)
    rx = philox.philox4x32_10(i, ctr & 0xFFFFFFFF, ctr >> 32, philox.STREAM_POLICY, k0, k1)[0]
    u = (rx >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
    p, _, _ = softmax_stats64(np.asarray(logits, dtype=np.float64).reshape(-1, np.shape(logits)[-1])[:, :A])
    cdf = np.cumsum(p, -1)[:, :A - 1]
    act = (cdf <= u[:, None]).sum(-1).astype(np.int64)
    dist = np.abs(cdf - u[:, None]).min(-1) if A > 1 else np.full(u.shape, np.inf)
    return act, dist
