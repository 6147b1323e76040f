"""PolicyNet.lstm_sequence is the loop of lstm_step calls it replaces, by bits: against a hand-written
loop into separate buffers at one step of one env, at an odd size, on both sides of the skinny-row
limit (kSkinnyRows = 16) and at the replayed UNREAL pass's T + 1 steps with its [T + 1, S, A + 1]
and [T + 1, S] inputs; an episode starts at t = 1 (a mask row of zeros). And the trainer's
stored-rollout forward (_forward_stored) on the rollout just sampled gives the rollout's own head
outputs and (h, c), by bits, at 5 envs x 3 steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

A = 4


@pytest.fixture(scope="module")
def net_params():
    from vnav.policy import PolicyNet
    net = PolicyNet((84, 84), A, device="cuda:0", recurrent=True)
    return net, net.init_params(3)


def _buffers(net, n, E):
    kw = dict(dtype=torch.float32, device="cuda")
    return dict(xcat=torch.zeros((n, net.lstm["xcat"]), **kw), gates=torch.zeros((E, 2048), **kw),
                acts=torch.zeros((n, 2048), **kw), c_all=torch.zeros((n, 512), **kw),
                h_all=torch.zeros((n, 512), **kw))


@pytest.mark.parametrize("T,E,flat", [(1, 1, False), (3, 5, True), (2, 16, False), (2, 17, True), (3 + 1, 2, False)])
def test_lstm_sequence_is_the_loop_of_steps(net_params, T, E, flat):
    net, params = net_params
    n = T * E
    g = torch.Generator(device="cuda").manual_seed(100 * T + E)
    rnd = lambda *shape: torch.randn(shape, generator=g, device="cuda")  # noqa: E731
    x5, h0, c0 = rnd(n, 512), rnd(E, 512), rnd(E, 512)
    lra, masks = rnd(T, E, A + 1), torch.ones((T, E), device="cuda")
    if T > 1:
        masks[1] = 0.0  # every env starts an episode at t = 1
    want = _buffers(net, n, E)
    for t in range(T):
        sl = slice(t * E, (t + 1) * E)
        hp = h0 if t == 0 else want["h_all"][(t - 1) * E:t * E]
        cp = c0 if t == 0 else want["c_all"][(t - 1) * E:t * E]
        net.lstm_step(params, E, x5[sl], lra[t], masks[t], hp, cp, want["xcat"][sl], want["gates"], want["acts"][sl],
                      want["c_all"][sl], want["h_all"][sl])
    got = _buffers(net, n, E)
    h0_in, c0_in = h0.clone(), c0.clone()
    # the trainer's rollout feeds [T, E, A + 1] and [T, E], the replayed pass the same at T + 1
    # steps; the minibatches and the autograd functions feed [n, A + 1]: one set of addresses
    lra_in, masks_in = (lra.view(n, A + 1), masks.view(n)) if flat else (lra, masks)
    net.lstm_sequence(params, T, E, x5, lra_in, masks_in, h0, c0, got["xcat"], got["gates"], got["acts"], got["c_all"],
                      got["h_all"])
    torch.cuda.synchronize()
    for k in ("xcat", "acts", "c_all", "h_all"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(h0, h0_in) and torch.equal(c0, c0_in)
    assert float(want["h_all"].abs().sum()) > 0


def test_forward_stored_is_the_rollouts_forward():
    """learning_rate 0 and no optimiser step taken: the stored-rollout forward over the rollout just
    sampled (15 rows in one trunk call, the LSTM from the state the rollout started from) writes
    the head outputs and (h, c) the rollout's own steps wrote."""
    from test_ppo_trainer_gpu import make
    E, T = 5, 3
    tr = make("goal-lstm", envs=E, steps=T, ppo_clip=0.2, ppo_epochs=2, learning_rate=0.0)
    tr.rollout()
    torch.cuda.synchronize()
    want = {k: getattr(tr, k).clone() for k in ("out", "h_all", "c_all")}
    assert float(want["h_all"].abs().sum()) > 0
    tr.out.zero_()
    tr._hc_all.zero_()
    goals = tr._rollout_goal_runs(tr.dones, T, E)
    tr._forward_stored(E, tr._frames(tr.rows_img, tr.rows_goal), tr._seq, goals)
    torch.cuda.synchronize()
    for k, w in want.items():
        assert torch.equal(getattr(tr, k), w), k
