"""fp64 numpy restatement of csrc/vn_ppo.hip's three kernels (include/vnav.h states the contracts)
and the generated cases the CPU and GPU tests share. Pure numpy: no GPU, no library.

Every generated case keeps each sample at least MARGIN clear of every decision boundary of the
loss (tests/test_ppo_refs.py checks that on this fp64 reference alone), so the fp32 kernel takes
the reference's branch at every sample and no sample has to be left out of a comparison."""
import functools

import numpy as np

OUT_LD = 8
MARGIN = 1e-4  # the clearance tests/test_a2c_refs.py keeps for its draws
CLIP, VALUE_CLIP, VC, EC, ADV_EPS = 0.2, 0.2, 0.5, 0.01, 1e-8

NS = (1, 63, 65, 257, 1025)  # one lane, a ragged wave, a second wave, a second block, a ragged last block
AS = (1, 4, 7)
SCALES = (1.0, 8.0)


def softmax_stats(lg):
    """p, logp, H of logits [n][A]."""
    z = lg - lg.max(axis=1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    return p, logp, -(p * logp).sum(axis=1)


def adv_stats(returns, out_old, A, eps):
    """[mean, 1 / (std + eps)] of returns - V_old, population std."""
    adv = np.asarray(returns, np.float64) - np.asarray(out_old, np.float64)[:, A]
    mean = adv.sum() / adv.size
    std = np.sqrt(((adv - mean) ** 2).sum() / adv.size)
    return np.array([mean, 1.0 / (std + float(eps))])


def loss_grad(out, out_old, actions, returns, stats2, A, clip=CLIP, value_clip=VALUE_CLIP, vc=VC, ec=EC):
    """vn_ppo_loss_grad in fp64. Returns a dict: dout [n][8], stats4, ppo_stats4, their terms
    (``terms`` [8][n]), the per-sample branch flags and the distances to the decision boundaries."""
    out, out_old = np.asarray(out, np.float64), np.asarray(out_old, np.float64)
    R, a = np.asarray(returns, np.float64), np.asarray(actions)
    n = out.shape[0]
    idx = np.arange(n)
    p, logp, H = softmax_stats(out[:, :A])
    _, logp_old, _ = softmax_stats(out_old[:, :A])
    V, Vo = out[:, A], out_old[:, A]
    d = logp[idx, a] - logp_old[idx, a]
    r = np.exp(d)
    adv = R - Vo
    if stats2 is not None:
        adv = (adv - float(stats2[0])) * float(stats2[1])
    rc = np.clip(r, 1.0 - clip, 1.0 + clip)
    s1, s2 = r * adv, rc * adv
    active = s1 <= s2
    g = np.where(active, -adv * r, 0.0)
    ind = np.zeros((n, A))
    ind[idx, a] = 1.0
    dout = np.zeros((n, OUT_LD))
    dout[:, :A] = (g[:, None] * (ind - p) + ec * p * (logp + H[:, None])) / n
    e1 = R - V
    lv, vgrad = e1 ** 2, np.ones(n, bool)
    dv = V - Vo
    vclipped = np.abs(dv) > value_clip if value_clip > 0 else np.zeros(n, bool)
    e2 = e1.copy()
    if value_clip > 0:
        e2 = R - np.where(vclipped, Vo + np.clip(dv, -value_clip, value_clip), V)
        vgrad = e1 ** 2 >= e2 ** 2
        lv = np.maximum(e1 ** 2, e2 ** 2)
    dout[:, A] = np.where(vgrad, vc * (-2.0 * e1) / n, 0.0)
    out_of_range = (r < 1.0 - clip) | (r > 1.0 + clip)
    terms = np.stack([lv, -np.minimum(s1, s2), H, R, np.expm1(d) - d, out_of_range.astype(np.float64), r,
                      (~vgrad).astype(np.float64)])
    big = np.full(n, np.inf)
    margins = {
        "r = 1 - c": np.abs(r - (1.0 - clip)),
        "r = 1 + c": np.abs(r - (1.0 + clip)),
        # inside the range both terms are one number (a tie, the gradient flows); outside, the
        # sign of their difference decides
        "s1 = s2": np.where(out_of_range, np.abs(s1 - s2), big),
        "|V - V_old| = cv": np.abs(np.abs(dv) - value_clip) if value_clip > 0 else big,
        # unclipped, the two squares are one number (a tie, the gradient flows)
        "e1^2 = e2^2": np.where(vclipped, np.abs(e1 ** 2 - e2 ** 2), big),
    }
    branches = {
        "unclipped": ~out_of_range,
        "cut, adv > 0": out_of_range & ~active & (adv > 0),
        "cut, adv < 0": out_of_range & ~active & (adv < 0),
        "clipped, flowing": out_of_range & active,
        "value clipped": ~vgrad,
        "value unclipped": vgrad,
    }
    return dict(dout=dout, stats4=terms[:4].sum(axis=1), ppo_stats4=terms[4:].sum(axis=1), terms=terms,
                margins=margins, branches=branches, adv=adv)


def adam_step(p, g, m, v, t, coef, lr, beta1, beta2, eps):
    """One vn_adam_step_dev in fp64 from fp64 copies of the state; t = the step count before the
    call. Returns (p, m, v, step) with step = the parameter decrement."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    g = g * float(coef)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    t = int(t) + 1
    bc1, bc2 = 1.0 - float(beta1) ** t, 1.0 - float(beta2) ** t
    step = (float(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + float(eps))
    return p - step, m, v, step


def _draw(n, A, scale, seed):
    rng = np.random.RandomState(seed)
    out_old = np.zeros((n, OUT_LD), np.float32)
    out = np.zeros((n, OUT_LD), np.float32)
    out_old[:, :A] = scale * rng.randn(n, A)
    out[:, :A] = out_old[:, :A] + 0.35 * rng.randn(n, A)
    out_old[:, A] = rng.randn(n)
    out[:, A] = out_old[:, A] + 0.3 * rng.randn(n)
    # poison the unused columns: the kernel must not read them
    out[:, A + 1:] = 1e30
    out_old[:, A + 1:] = -1e30
    actions = rng.randint(0, A, size=n).astype(np.int32)
    returns = (1.5 * rng.randn(n)).astype(np.float32)
    return out, out_old, actions, returns


def min_margin(ref):
    return min(float(m.min()) for m in ref["margins"].values())


@functools.lru_cache(maxsize=None)
def case(n, A, scale, normalize=True):
    """(out, out_old, actions, returns, stats2 or None, ref) of one generated case: float32 inputs,
    stats2 the fp32-rounded advantage statistics the kernel reads, ref = loss_grad's dict on
    exactly those inputs. The seed is the first of base, base + 1, ... whose draw is MARGIN clear
    of every boundary at every sample (choosing another seed, never a wider bound)."""
    base = 1000 * n + 10 * A + int(scale)
    for k in range(4096):
        out, out_old, actions, returns = _draw(n, A, scale, base + k)
        stats2 = adv_stats(returns, out_old, A, ADV_EPS).astype(np.float32) if normalize else None
        if normalize and n == 1:
            # one sample's own statistics are std = 0, rstd = 1 / eps = 1e8, which multiplies the
            # single fp32 rounding of R - V_old into O(1): no fp32 launch can follow fp64 there. The
            # loss kernel only reads the two numbers, so the one-lane case reads ordinary ones.
            stats2 = np.array([0.1, 0.7], np.float32)
        ref = loss_grad(out, out_old, actions, returns, stats2, A)
        if min_margin(ref) >= MARGIN and (n < 63 or A < 2 or all(b.any() for b in ref["branches"].values())):
            for x in (out, out_old, actions, returns):
                x.setflags(write=False)
            return out, out_old, actions, returns, stats2, ref
    raise AssertionError("no seed of case n=%d A=%d scale=%g is clear of the boundaries" % (n, A, scale))


def all_cases():
    return [(n, A, s) for n in NS for A in AS for s in SCALES]
