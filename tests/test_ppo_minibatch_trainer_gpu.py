"""A2CTrainer(ppo_clip=..., ppo_minibatches=M): every epoch splits the envs by one device-drawn
permutation into M minibatches of whole sequences (sizes by floor(m E / M), the reference
permutation of tests/ppo_minibatch_ref.py under the update's counter); with learning_rate 0 every
minibatch's re-forward is the rollout's forward at its gathered rows and the size-weighted sum of
the minibatch gradients is the full-batch PPO gradient; with a learning rate every minibatch moves
the parameters and minibatch (0, 1) runs on what (0, 0) left, its loss gradient the fp64
restatement's; the metrics are the final epoch's sums over all of its minibatches; the captured
hipGraph equals eager by bits; a resume follows the same splits; ppo_minibatches=1 is the trainer
as it was. The maze, sizes and time limit of tests/test_ppo_trainer_gpu.py, plus 18 envs x 3 steps
for goal runs."""
import copy

import numpy as np
import pytest
import torch

import ppo_minibatch_ref as mref
import ppo_ref as ref
from test_ppo_trainer_gpu import CASES, PPO_KEYS, E, T, bits_equal, make, tensors, worst_of_scale

pytestmark = pytest.mark.gpu


def key_seed(tr):
    from vnav import dist as vdist
    return vdist.rank_seed(tr.seed, tr.rank)


def rows_of(envs, steps, num_envs):
    """Rollout rows t E + e of the envs, in the minibatch's order (row t Eb + j)."""
    envs = np.asarray(envs, dtype=np.int64)
    return (np.arange(steps)[:, None] * num_envs + envs[None, :]).reshape(-1)


def record(tr, names=("out", "dout", "grads")):
    """on_ppo_minibatch hook that keeps, per (k, m), the minibatch's envs, the compact buffers and
    clones of the named trainer buffers (row buffers cut to the minibatch's T Eb rows)."""
    seen = {}

    def hook(k, m):
        lo, hi = tr.mb_bounds[m], tr.mb_bounds[m + 1]
        nb = tr.num_steps * (hi - lo)
        d = dict(envs=tr.ppo_perm[lo:hi].cpu().numpy(), perm=tr.ppo_perm.cpu().numpy(), nb=nb,
                 params=tr.params.clone())
        for n in names:
            v = getattr(tr, n)
            d[n] = (v if n == "grads" else v[:nb]).clone()
        for n in ("rows_img", "out_old", "actions", "returns"):
            d["mb_" + n] = tr.mb[n][:nb].clone()
        seen[(k, m)] = d

    tr.on_ppo_minibatch = hook
    return seen


@pytest.mark.parametrize("M", [2, 3])
def test_every_epoch_partitions_the_envs_by_the_reference_permutation(M):
    K = 2
    tr = make("goal-lstm", ppo_clip=0.2, ppo_epochs=K, ppo_minibatches=M)
    tr.step()
    seen = record(tr, names=())
    epochs = []
    tr.on_ppo_epoch = epochs.append
    tr.step()
    torch.cuda.synchronize()
    assert sorted(seen) == [(k, m) for k in range(K) for m in range(M)] and epochs == list(range(K))
    ctr = int(tr.sched[2])
    assert ctr == T  # the second update's counter base: updates * num_steps
    lo = mref.bounds(E, M)
    assert tr.mb_bounds == lo
    rows_img = tr.rows_img.cpu().numpy()
    for k in range(K):
        want = mref.permutation(key_seed(tr), ctr, k, E)
        got = np.concatenate([seen[(k, m)]["envs"] for m in range(M)])
        assert np.array_equal(got, want) and sorted(got.tolist()) == list(range(E))
        for m in range(M):
            s = seen[(k, m)]
            assert len(s["envs"]) == lo[m + 1] - lo[m] and np.array_equal(s["perm"], want)
            assert np.array_equal(s["mb_rows_img"].cpu().numpy(), rows_img[rows_of(s["envs"], T, E)])
    assert not np.array_equal(seen[(0, 0)]["perm"], seen[(1, 0)]["perm"])


def _lr0(case, M, K=2, envs=E, steps=T, **kw):
    """learning_rate 0: the minibatch trainer and an M = 1 PPO trainer on one rollout."""
    opts = dict(envs=envs, steps=steps, ppo_clip=0.2, learning_rate=0.0, **kw)
    tr = make(case, ppo_epochs=K, ppo_minibatches=M, **opts)
    full = make(case, ppo_epochs=1, **opts)
    for x in (tr, full):
        x.step()
    assert torch.equal(tr.params, full.params)
    p0 = tr.params.clone()
    for x in (tr, full):
        x.rollout()
    torch.cuda.synchronize()
    for name in ("out", "actions", "rewards", "dones", "rows_img", "rows_goal", "boot_out"):
        assert torch.equal(getattr(tr, name), getattr(full, name)), name
    assert int(tr.dones.sum()) > 0
    A = tr.A
    out_rollout = tr.out.cpu().double().numpy()[:, :A + 1]
    last = tr._hc_all.view(2, steps, envs, 512)[:, -1].clone() if tr.recurrent else None
    want = {}
    full.on_ppo_epoch = lambda k: want.setdefault(k, full.grads.clone())
    full.update()
    seen = record(tr)
    tr.update()
    torch.cuda.synchronize()
    g_full = tensors(full, want[0])
    assert sorted(seen) == [(k, m) for k in range(K) for m in range(M)]
    for k in range(K):
        total = None
        for m in range(M):
            s = seen[(k, m)]
            got = s["out"].cpu().double().numpy()[:, :A + 1]
            ref_rows = out_rollout[rows_of(s["envs"], steps, envs)]
            e_out = np.abs(got - ref_rows).max() / np.abs(out_rollout).max()
            print("PPOMB %s lr=0 (k=%d, m=%d): out vs the rollout's rows %.3e of scale" % (case, k, m, e_out))
            assert e_out <= 1e-5, (k, m, e_out)
            assert torch.equal(s["mb_out_old"], tr.out_old[torch.as_tensor(rows_of(s["envs"], steps, envs)).cuda()])
            part = s["grads"].double() * (len(s["envs"]) / envs)
            total = part if total is None else total + part
        e_g = worst_of_scale(tensors(tr, total.float()), g_full)
        print("PPOMB %s lr=0 epoch %d: sum of (Eb / E) minibatch grads vs the full-batch gradient %.3e of scale"
              % (case, k, e_g))
        assert e_g <= 1e-4, (k, e_g)
    assert torch.equal(tr.params.view(torch.int32), p0.view(torch.int32))
    if tr.recurrent:
        assert torch.equal(tr._hc0, last)
    return tr


@pytest.mark.parametrize("case", list(CASES))
def test_lr0_minibatch_gradients_sum_to_the_full_batch_gradient(case):
    _lr0(case, M=2)


def test_lr0_with_aux_heads():
    tr = _lr0("goal-lstm", M=2, aux=True, aux_weight=0.1)
    assert tr.aux_source == "rollout" and float(tr.aux_stats.abs().sum()) > 0


@pytest.mark.parametrize("M", [4, 2])
def test_lr0_with_goal_runs(M):
    """18 envs x 3 steps. M = 4: minibatches of 12 and 15 rows, at or below the 16 rows from which
    the policy takes goal runs, so they run without (the same outputs). M = 2: 27 rows, the goal
    runs rebuilt per minibatch from its gathered dones."""
    tr = _lr0("goal-lstm", M=M, envs=18, steps=3, dedup_goals=True)
    assert tr.dedup_goals
    assert sorted(tr._mb_goal_runs) == ([9] if M == 2 else [])
    if M == 2:
        assert 0 < int(tr.goal_count[3]) < 3 * 9  # fewer goal frames than the minibatch has samples


def _reforward(tr, params, hc0):
    """The whole stored rollout under ``params``, with the test's own buffers: out [N, 8]."""
    net, N = tr.net, T * E
    acts = net.new_acts(N)
    out = torch.zeros((N, 8), device="cuda")
    frames = tr._frames(tr.rows_img, tr.rows_goal)
    if not tr.recurrent:
        net.forward(params, frames, N, acts, N, 0, out)
        return out
    net.forward(params, frames, N, acts, N, 0, None)
    x5 = net.x5(acts, N)
    f32 = dict(dtype=torch.float32, device="cuda")
    xcat, lacts = torch.zeros((N, net.lstm["xcat"]), **f32), torch.zeros((N, 2048), **f32)
    h, c, gates = torch.zeros((N, 512), **f32), torch.zeros((N, 512), **f32), torch.zeros((E, 2048), **f32)
    for t in range(T):
        sl = slice(t * E, (t + 1) * E)
        hp = hc0[0] if t == 0 else h[(t - 1) * E:t * E]
        cp = hc0[1] if t == 0 else c[(t - 1) * E:t * E]
        net.lstm_step(params, E, x5[sl], tr.lra[t], tr.masks[t], hp, cp, xcat[sl], gates, lacts[sl], c[sl], h[sl])
    net.heads(params, h, N, out)
    return out


def _loss_ref(tr, s):
    return ref.loss_grad(s["out"].cpu().numpy(), s["mb_out_old"].cpu().numpy(), s["mb_actions"].cpu().numpy(),
                         s["mb_returns"].cpu().numpy(), tr.adv_stats.cpu().numpy(), tr.A, clip=0.2, value_clip=0.0,
                         vc=tr.value_coefficient, ec=tr.entropy_coefficient)


@pytest.mark.parametrize("case", list(CASES))
def test_minibatch_1_runs_on_the_parameters_minibatch_0_left(case):
    K, M = 2, 2
    tr = make(case, ppo_clip=0.2, ppo_epochs=K, ppo_minibatches=M)
    tr.step()
    tr.rollout()
    torch.cuda.synchronize()
    A = tr.A
    hc0 = tr._hc0.clone() if tr.recurrent else None
    before = tr.params.clone()
    seen = record(tr)
    tr.update()
    torch.cuda.synchronize()
    order = [(k, m) for k in range(K) for m in range(M)]
    assert sorted(seen) == order
    prev = before
    for km in order:  # every minibatch took a step
        assert not torch.equal(seen[km]["params"], prev), km
        prev = seen[km]["params"]
    assert torch.equal(prev, tr.params)
    s = seen[(0, 1)]
    rows = rows_of(s["envs"], T, E)
    want = _reforward(tr, seen[(0, 0)]["params"], hc0).cpu().double().numpy()[rows, :A + 1]
    torch.cuda.synchronize()
    got = s["out"].cpu().double().numpy()[:, :A + 1]
    old = s["mb_out_old"].cpu().double().numpy()[:, :A + 1]
    assert np.array_equal(old, tr.out_old.cpu().double().numpy()[rows, :A + 1])
    e_out = np.abs(got - want).max() / np.abs(want).max()
    moved = np.abs(got - old).max() / np.abs(want).max()
    print("PPOMB %s minibatch (0, 1) out vs the test's re-forward: %.3e of scale (moved %.3e from the rollout's)"
          % (case, e_out, moved))
    assert e_out <= 1e-5, e_out
    assert moved > 1e-4  # it did not run on the rollout's parameters
    r = _loss_ref(tr, s)
    assert min(float(x.min()) for x in r["margins"].values()) >= ref.MARGIN  # no sample near a branch
    dout = s["dout"].cpu().double().numpy()
    e_d = np.abs(dout[:, :A + 1] - r["dout"][:, :A + 1]).max() / np.abs(r["dout"]).max()
    print("PPOMB %s minibatch (0, 1) dout vs fp64: %.3e of scale" % (case, e_d))
    assert e_d <= 1e-5, e_d
    assert not dout[:, A + 1:].any()
    if tr.recurrent:  # the carried state is the behaviour policy's
        assert not torch.equal(tr._hc0, hc0)


def test_metrics_are_the_final_epochs_sums_over_its_minibatches():
    K, M = 2, 2
    tr = make("goal-lstm", ppo_clip=0.2, ppo_epochs=K, ppo_minibatches=M)
    tr.step()
    tr.rollout()
    seen = record(tr)
    tr.update()
    torch.cuda.synchronize()
    parts = [_loss_ref(tr, seen[(K - 1, m)]) for m in range(M)]
    terms = np.concatenate([p["terms"] for p in parts], axis=1)
    assert terms.shape == (8, T * E)
    sums, mags = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    got = np.concatenate([tr.stats.cpu().double().numpy(), tr.ppo_stats.cpu().double().numpy()])
    err = np.abs(got - sums)  # (a statistic whose terms are all zero, as the value-clip flags here, must be 0)
    print("PPOMB final-epoch sums %s vs fp64 over its minibatches %s: worst %.3e of the terms' magnitudes"
          % (got, sums, (err[mags > 0] / mags[mags > 0]).max()))
    assert (err <= 1e-5 * mags).all(), (err, mags)
    assert mags[:3].all() and mags[4] > 0 and mags[6] > 0
    first = np.concatenate([_loss_ref(tr, seen[(0, m)])["terms"] for m in range(M)], axis=1).sum(axis=1)
    assert np.abs(first[4] - sums[4]) > 1e-5 * mags[4]  # not the first epoch's
    m = tr.step()
    assert PPO_KEYS <= set(m) and 0.0 <= m["clip_fraction"] <= 1.0 and m["ratio_mean"] > 0
    assert tr._metric_layout["ppo"][1] == 4


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_graph_is_bit_identical_to_eager(optimizer):
    runs = {}
    for graph in (False, True):
        tr = make("goal-lstm", ppo_clip=0.2, ppo_epochs=2, ppo_minibatches=2, ppo_value_clip=0.2, optimizer=optimizer,
                  cuda_graph=graph)
        raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        state = [tr.params.clone(), tr.square_avg.clone(), tr._hc0.clone(), tr.out.clone(), tr.ppo_stats.clone(),
                 tr.stats.clone(), tr.ppo_perm.clone()]
        if optimizer == "adam":
            state += [tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.adam_step.clone()]
            assert int(tr.adam_step) == 12 and not tr.square_avg.any()  # one step per minibatch
        runs[graph] = (state, raws)
    for x, y in zip(runs[True][0], runs[False][0]):
        assert bits_equal(x, y)
    for x, y in zip(runs[True][1], runs[False][1]):
        assert bits_equal(x, y)
    assert np.array_equal(tr.ppo_perm.cpu().numpy(), mref.permutation(key_seed(tr), 2 * T, 1, E))
    for name in ("on_ppo_minibatch", "on_ppo_epoch"):
        with pytest.raises(ValueError, match=name):
            setattr(tr, name, lambda *a: None)


def test_resume_follows_the_same_splits():
    kw = dict(ppo_clip=0.2, ppo_epochs=2, ppo_minibatches=2, optimizer="adam")
    a = make("goal-lstm", **kw)
    a.step()
    a.step()
    sd = copy.deepcopy(a.state_dict())
    assert int(sd["adam_step"]) == 8
    a.step()
    b = make("goal-lstm", **kw)
    b.step()  # somewhere else: the load must replace it
    b.load_state_dict(sd)
    b.step()
    torch.cuda.synchronize()
    for name in ("params", "exp_avg", "exp_avg_sq", "adam_step", "returns", "out", "_hc0", "ppo_perm", "ppo_stats"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(b.ppo_perm.cpu().numpy(), mref.permutation(key_seed(b), 2 * T, 1, E))


def test_one_minibatch_is_the_trainer_as_it_was():
    a = make("goal-lstm", ppo_clip=0.2, ppo_epochs=2)
    b = make("goal-lstm", ppo_clip=0.2, ppo_epochs=2, ppo_minibatches=1)
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    for name in ("params", "square_avg", "_hc0", "out", "ppo_stats", "stats"):
        assert bits_equal(getattr(a, name), getattr(b, name)), name
    assert not hasattr(b, "mb") and not hasattr(b, "ppo_perm")  # nothing allocated


def test_refusals():
    for bad in (dict(ppo_clip=0.2, ppo_minibatches=0), dict(ppo_clip=0.2, ppo_minibatches=-1),
                dict(ppo_clip=0.2, ppo_minibatches=E + 1)):
        with pytest.raises(ValueError, match="ppo_minibatches"):
            make("goal-lstm", **bad)
    with pytest.raises(ValueError, match="ppo_clip"):
        make("goal-lstm", ppo_minibatches=2)
    make("goal-lstm", ppo_minibatches=1)  # the default needs no PPO
    tr = make("goal-lstm", ppo_clip=0.2, ppo_minibatches=E)  # one env per minibatch is the limit
    assert tr.mb_bounds == list(range(E + 1))
    # the PPO refusals stand with minibatches too
    with pytest.raises(ValueError, match="unreal"):
        make("bighouse-lstm", unreal=True, ppo_clip=0.2, ppo_minibatches=2)
    with pytest.raises(ValueError):
        make("goal-lstm", ppo_clip=0.2, ppo_minibatches=2, expert_weight=0.3)
