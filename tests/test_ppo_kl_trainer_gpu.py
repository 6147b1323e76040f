"""A2CTrainer(ppo_clip=..., ppo_target_kl=...): a target that never fires leaves the trainer what it
was, bit for bit, and counts every optimiser step; a tiny target stops at epoch 1's check and
leaves the state of a one-epoch trainer; a target set between two recorded KLs stops where the
recording says and leaves the state of a trainer with that many epochs; the captured hipGraph
equals eager by bits across updates that stop; ppo_kl_host_stop ends with the same bits and runs
fewer epochs; a resume across a stopped update is exact; the combinations out of scope are refused.
The maze, steps and time limit of tests/test_ppo_trainer_gpu.py at 16 envs, K = 4 epochs, RMSprop and
Adam, M = 1 and 2 minibatches."""
import copy
import functools
import math

import pytest
import torch

from test_ppo_trainer_gpu import bits_equal, make

pytestmark = pytest.mark.gpu

ENVS, K = 16, 4
OPTIMIZERS = ("rmsprop", "adam")
BOTH = [(o, M) for o in OPTIMIZERS for M in (1, 2)]


def mk(optimizer, M, **kw):
    opts = dict(envs=ENVS, ppo_clip=0.2, ppo_epochs=K, optimizer=optimizer, ppo_minibatches=M)
    opts.update(kw)
    return make("goal-lstm", **opts)


def state(tr):
    s = {"params": tr.params, "square_avg": tr.square_avg, "hc0": tr._hc0}
    if tr.optimizer == "adam":
        s.update(exp_avg=tr.exp_avg, exp_avg_sq=tr.exp_avg_sq, adam_step=tr.adam_step)
    return {k: v.clone() for k, v in s.items()}


def same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert bits_equal(a[k], b[k]), k


@functools.lru_cache(maxsize=None)
def recorded(optimizer, M):
    """The KL of every check of the first update, in order (one per optimiser step), from an eager
    run whose target never fires; and from them (steps allowed, target): the limit 1.5 * target is
    the geometric mean of the first two consecutive KLs a factor above 1.01 apart with every
    earlier one below it. None when no such pair exists."""
    tr = mk(optimizer, M, ppo_target_kl=1e30)
    kls = []
    if M == 1:
        tr.on_ppo_epoch = lambda k: kls.append(float(tr.kl_dev[0]))
    else:
        tr.on_ppo_minibatch = lambda k, m: kls.append(float(tr.kl_dev[0]))
    tr.step()
    assert len(kls) == K * M
    print("PPOKL %s M=%d KL of the first update's checks: %s" % (optimizer, M, " ".join("%.3e" % x for x in kls)))
    for i in range(len(kls) - 1):
        lo, hi = kls[i], kls[i + 1]
        if lo > 0.0 and hi > 1.01 * lo:
            limit = math.sqrt(lo * hi)
            if max(kls[:i + 1]) < limit:
                return tuple(kls), (i + 1, limit / 1.5)
    return tuple(kls), None


def mid_target(optimizer, M):
    kls, pick = recorded(optimizer, M)
    if pick is None:
        pytest.skip("no two consecutive KLs a factor 1.01 apart in %s" % (kls,))
    return pick


@pytest.mark.parametrize("optimizer, M", BOTH)
def test_a_target_that_never_fires_is_the_trainer_without_it(optimizer, M):
    a, b = mk(optimizer, M), mk(optimizer, M, ppo_target_kl=1e30)
    for _ in range(2):
        a.step(sync=False)
        b.step(sync=False)
    ma, mb = a.step(), b.step()
    torch.cuda.synchronize()
    same_state(state(a), state(b))
    for name in ("out", "ppo_stats", "stats"):
        assert bits_equal(getattr(a, name), getattr(b, name)), name
    assert mb["ppo_steps"] == K * M and mb["kl_stopped"] == 0 and mb["kl_at_stop"] == 0
    assert not {"ppo_steps", "kl_stopped", "kl_at_stop"} & set(ma) and not hasattr(a, "kl_gate")
    assert mb["approx_kl"] == ma["approx_kl"] and mb["grad_norm"] == ma["grad_norm"]
    assert list(b._metric_layout)[-1] == "ppo_kl" and "ppo_kl" not in a._metric_layout


@pytest.mark.parametrize("optimizer", OPTIMIZERS)
def test_a_tiny_target_stops_at_epoch_1(optimizer):
    a, one = mk(optimizer, 1, ppo_target_kl=1e-30), mk(optimizer, 1, ppo_epochs=1)
    m = a.step()
    one.step()
    torch.cuda.synchronize()
    same_state(state(a), state(one))
    assert m["ppo_steps"] == 1 and m["kl_stopped"] == 1 and m["kl_at_stop"] > 0
    assert a.kl_gate.tolist() == [1, 1] and float(a.kl_dev[0]) == float(a.kl_dev[1]) == m["kl_at_stop"]
    if optimizer == "adam":
        assert int(a.adam_step) == 1
    # the stop is the update's own: the next update starts open and stops again after its first step
    m = a.step()
    assert m["ppo_steps"] == 1 and m["kl_stopped"] == 1
    if optimizer == "adam":
        assert int(a.adam_step) == 2


@pytest.mark.parametrize("optimizer", OPTIMIZERS)
def test_a_target_between_two_recorded_kls_stops_there(optimizer):
    steps, target = mid_target(optimizer, 1)
    kls = recorded(optimizer, 1)[0]
    assert kls[0] == 0.0  # epoch 0, full batch: r is exactly 1
    a, short = mk(optimizer, 1, ppo_target_kl=target), mk(optimizer, 1, ppo_epochs=steps)
    m = a.step()
    short.step()
    torch.cuda.synchronize()
    assert 1 <= steps < K and m["ppo_steps"] == steps and m["kl_stopped"] == 1
    assert m["kl_at_stop"] == kls[steps]  # the recorded run's KL at that check, by bits
    same_state(state(a), state(short))
    if optimizer == "adam":
        assert int(a.adam_step) == steps


@pytest.mark.parametrize("optimizer, M", BOTH)
def test_graph_is_bit_identical_to_eager(optimizer, M):
    steps, target = mid_target(optimizer, M)
    runs = {}
    for graph in (False, True):
        tr = mk(optimizer, M, ppo_target_kl=target, cuda_graph=graph)
        raws = [tr.step(sync=False)["raw"].clone() for _ in range(3)]
        torch.cuda.synchronize()
        runs[graph] = (state(tr), raws, tr.kl_gate.clone(), tr.kl_dev.clone(), tr.out.clone())
    same_state(runs[True][0], runs[False][0])
    for x, y in zip(runs[True][1], runs[False][1]):
        assert bits_equal(x, y)
    for i in (2, 3, 4):
        assert bits_equal(runs[True][i], runs[False][i])
    o, w = tr._metric_layout["ppo_kl"]
    first = runs[True][1][0][o:o + w].tolist()
    assert first[0] == steps and first[1] == 1 and first[2] > 0  # the first update stopped where recorded
    with pytest.raises(ValueError, match="on_ppo_epoch"):
        tr.on_ppo_epoch = lambda k: None


@pytest.mark.parametrize("optimizer, M", BOTH)
def test_host_stop_ends_with_the_same_bits_and_runs_fewer_epochs(optimizer, M):
    steps, target = mid_target(optimizer, M)
    gated, host = mk(optimizer, M, ppo_target_kl=target), mk(optimizer, M, ppo_target_kl=target, ppo_kl_host_stop=True)
    ran = {id(gated): [], id(host): []}
    for tr in (gated, host):
        tr.on_ppo_epoch = ran[id(tr)].append
    stops = 0
    for _ in range(3):
        mg, mh = gated.step(), host.step()
        torch.cuda.synchronize()
        same_state(state(gated), state(host))
        for key in ("ppo_steps", "kl_stopped", "kl_at_stop"):
            assert mg[key] == mh[key], key
        stops += int(mg["kl_stopped"])
    assert stops >= 1 and len(ran[id(gated)]) == 3 * K
    assert len(ran[id(host)]) < len(ran[id(gated)])
    assert ran[id(host)][:steps // M] == list(range(steps // M))  # the first update's finished epochs


@pytest.mark.parametrize("optimizer, M", BOTH)
def test_resume_across_a_stopped_update_is_exact(optimizer, M):
    _, target = mid_target(optimizer, M)
    kw = dict(ppo_target_kl=target)
    a = mk(optimizer, M, **kw)
    m = a.step()
    assert m["kl_stopped"] == 1
    a.step()
    sd = copy.deepcopy(a.state_dict())
    assert not any("kl" in k for k in sd)  # the gate is the update's own: nothing of it is saved
    ma = a.step()
    b = mk(optimizer, M, **kw)
    b.step()  # somewhere else: the load must replace it
    b.load_state_dict(sd)
    mb = b.step()
    torch.cuda.synchronize()
    same_state(state(a), state(b))
    for name in ("returns", "out", "kl_gate", "kl_dev"):
        assert bits_equal(getattr(a, name), getattr(b, name)), name
    for key in ("ppo_steps", "kl_stopped", "kl_at_stop"):
        assert ma[key] == mb[key], key


def test_refusals():
    with pytest.raises(ValueError, match="ppo_target_kl.*needs ppo_clip"):
        make("goal-lstm", ppo_target_kl=0.01)
    for bad in (0.0, -0.01, float("nan")):
        with pytest.raises(ValueError, match="ppo_target_kl must be > 0"):
            make("goal-lstm", ppo_clip=0.2, ppo_target_kl=bad)
    with pytest.raises(ValueError, match="ppo_kl_host_stop.*needs ppo_target_kl"):
        make("goal-lstm", ppo_clip=0.2, ppo_kl_host_stop=True)
    with pytest.raises(ValueError, match="ppo_kl_host_stop.*captured hipGraph.*cuda_graph=False"):
        make("goal-lstm", ppo_clip=0.2, ppo_target_kl=0.01, ppo_kl_host_stop=True, cuda_graph=True)
    tr = make("goal-lstm", ppo_clip=0.2, ppo_target_kl=0.01, ppo_kl_host_stop=True)  # eager: accepted
    assert tr.ppo_kl_host_stop and abs(tr._kl_limit - 0.015) < 1e-8
    # the PPO refusals stand with a target too
    with pytest.raises(ValueError, match="unreal"):
        make("bighouse-lstm", unreal=True, ppo_clip=0.2, ppo_target_kl=0.01)
