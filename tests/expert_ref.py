"""numpy float64 restatement of the shortest-path expert term of the A2C update
(vn_a2c_loss_grad_expert, include/vnav.h; DESIGN.md "Expert loss from the navigation tables"):
the annealed weight, the loss gradient with both statistics, and the slot convention of the
trainer's mask history. Shared by test_expert_refs.py (CPU, against torch autograd) and the GPU
expert tests, as nav_ref.py serves the nav tests."""
import numpy as np

from oracle import a2c as oa2c

import nav_ref as nr


def anneal_weight(w0, steps, anneal_steps):
    """The fp32 weight of an update whose learning rate is computed from `steps` env-steps:
    w0 when anneal_steps <= 0, else w0 max(0, 1 - steps / anneal_steps) in fp64, rounded once."""
    w0 = float(np.float32(w0))
    if anneal_steps <= 0:
        return np.float32(w0)
    return np.float32(w0 * max(0.0, 1.0 - float(int(steps)) / float(int(anneal_steps))))


def mask_bits(mask, num_actions):
    """[n, A] bool: bit a of mask[i] for a < A (bits >= A are ignored)."""
    m = np.asarray(mask).astype(np.int64) & ((1 << int(num_actions)) - 1)
    return ((m[:, None] >> np.arange(int(num_actions))[None, :]) & 1).astype(bool)


def log_q64(p, logp, in_mask):
    """log sum_{a in M} p_a per row (0 where M is empty): log1p(-the other actions' mass) once
    they hold less than half, else a log-sum-exp of the mask's log-probabilities. Neither forms
    p / q, so a mask holding 1e-300 of the mass and one holding all of it are both exact to
    fp64 rounding."""
    rest = np.where(in_mask, 0.0, p).sum(1)
    valid = in_mask.any(1)
    neg = np.where(in_mask, logp, -np.inf)
    mx = np.where(valid, neg.max(1, initial=-np.inf), 0.0)
    se = np.where(in_mask, np.exp(np.where(in_mask, logp - mx[:, None], 0.0)), 0.0).sum(1)
    with np.errstate(divide="ignore"):
        lse = mx + np.log(np.where(valid, se, 1.0))
    lq = np.where(rest < 0.5, np.log1p(-np.minimum(rest, 0.5)), lse)
    return np.where(valid, lq, 0.0), valid


def expert_loss_grad64(out, actions, returns, mask, num_actions, value_coef, entropy_coef, pg_coef, w):
    """out [n, 8] (logits 0..A-1, value at A), actions, returns, mask [n], the fp32 weight w ->
    dict(dout [n, 8], stats4, mags4, expert3 = [sum of -log q over the labelled samples, how
    many of them sampled an action of their mask, their number], expert_mag = sum |log q|,
    loss = vc mean(A^2) - pg mean(A logp_a) - ec mean(H) - w mean([M != 0] log q))."""
    A = int(num_actions)
    o = np.asarray(out, dtype=np.float64)
    a = np.asarray(actions, dtype=np.int64)
    R = np.asarray(returns, dtype=np.float64)
    n = o.shape[0]
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    vc, ec, pg, w = f32(value_coef), f32(entropy_coef), f32(pg_coef), f32(w)
    inv_n = float(np.float32(1.0) / np.float32(n))
    p, lp, H = oa2c.softmax_stats64(o[:, :A])
    adv = R - o[:, A]
    ind = (np.arange(A)[None, :] == a[:, None]).astype(np.float64)
    in_mask = mask_bits(mask, A)
    lq, valid = log_q64(p, lp, in_mask)
    dout = np.zeros((n, 8), dtype=np.float64)
    dout[:, :A] = (pg * (-adv[:, None] * (ind - p)) + ec * p * (lp + H[:, None])) * inv_n
    resp = np.where(in_mask, np.exp(np.where(in_mask, lp - lq[:, None], 0.0)), 0.0)
    dout[:, :A] += np.where(valid[:, None], w * inv_n * (p - resp), 0.0)
    dout[:, A] = vc * (-2.0 * adv) * inv_n
    lpa = lp[np.arange(n), a]
    terms = np.stack([adv * adv, -adv * lpa, H, R])
    agree = valid & in_mask[np.arange(n), a]
    expert3 = np.array([-(lq[valid]).sum(), float(agree.sum()), float(valid.sum())])
    loss = (vc * (adv * adv).sum() - pg * (adv * lpa).sum() - ec * H.sum() - w * lq[valid].sum()) * inv_n
    return dict(dout=dout, stats4=terms.sum(1), mags4=np.abs(terms).sum(1), expert3=expert3,
                expert_mag=float(np.abs(lq[valid]).sum()), loss=float(loss))


def observed_masks(graphs, geos, scene, state, goal):
    """uint8 [E]: optimal_mask of every env's (scene, state, goal)."""
    return np.array([nr.distance_mask_action(graphs[int(k)], geos[int(k)], int(s), int(g))[1]
                     for k, s, g in zip(scene, state, goal)], dtype=np.uint8)


def rollout_mask_history(own, masks_after_step):
    """The trainer's slot convention. own: the env's own mask buffer when the rollout begins;
    masks_after_step [T][E]: what the nav launch behind step t writes (the mask of the state
    step t leaves the env in, after an auto-reset the new episode's). Slot 0 is copied from
    `own`, step t < T - 1 writes slot t + 1, the last step writes the env's own buffer.
    Returns (expert_mask [T, E], the env's own buffer after the rollout)."""
    T = len(masks_after_step)
    hist = np.zeros((T, len(own)), dtype=np.uint8)
    hist[0] = own
    own = np.array(own, dtype=np.uint8)
    for t in range(T):
        if t + 1 < T:
            hist[t + 1] = masks_after_step[t]
        else:
            own = np.array(masks_after_step[t], dtype=np.uint8)
    return hist, own
