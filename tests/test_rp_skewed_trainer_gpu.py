"""A2CTrainer(rp_sampling="skewed"): the reward-prediction samples drawn from the whole replay ring
(vn_unreal_rp_sample), their frames appended to the replayed UNREAL pass's trunk rows. Off is off;
the trainer's draws equal tests/rp_sample_ref.py on its own ring; the rp gradient against fp64
(oracle/policy.py, oracle/unreal.py); captured graph = eager; resume; the inline pass, the stream
guard, update(None) and the constructor's refusals. BigHouseModel on 84x84 frames where the goal
arch is not needed, thor-cached-auxiliary's 174x174 settings for graph = eager."""
import ctypes
import os

import numpy as np
import pytest
import torch

import rp_sample_ref as rr

pytestmark = pytest.mark.gpu

TOL = 1e-4  # every gradient tensor, of its scale (tests/test_unreal_update_gpu.py)
LOSS_RTOL = 1e-5
T = 5


def _scene():
    import vnav
    from oracle.frames import synth_frames
    from oracle.graph import h5_tables
    graph, spd, _ = h5_tables(np.ones((3, 3), dtype=bool))
    return vnav.scene_from_arrays(graph, spd, synth_frames(3, np.arange(len(graph)), (84, 84, 3)))


def _trainer(E=4, S=4, graph=False, seed=3, env_seed=2, **kw):
    """BigHouseModel, LSTM + UNREAL on replayed sequences, a ring of 3; skewed unless told."""
    import vnav
    env = vnav.VectorEnv([_scene()], E, seed=env_seed, max_episode_steps=30, tasks=[(0, 5)])
    kw.setdefault("rp_sampling", "skewed")
    return vnav.A2CTrainer(env, num_steps=T, seed=seed, max_time_steps=1e9, recurrent=True, arch="bighouse",
                           unreal=True, unreal_envs=S, unreal_source="replay", replay_size=3, cuda_graph=graph, **kw)


def _same_state(a, b):
    assert torch.equal(a.params, b.params) and torch.equal(a.square_avg, b.square_avg)
    assert torch.equal(a.replay_meta, b.replay_meta) and torch.equal(a.replay_rows, b.replay_rows)
    for key in a.ur:
        assert torch.equal(a.ur[key], b.ur[key]), key


def _draws(tr):
    n = (T + 1) * tr.unreal_S
    return [t.cpu().numpy().copy() for t in (tr.ur_rows_ext[0, n:].view(-1, 3), tr.ur_rows_ext[1, n:].view(-1, 3),
                                             tr.rp_label, tr.rp_src, tr.rp_draw_stats)]


@pytest.mark.parametrize("S", [4, 1])
def test_off_is_off(S):
    """rp_sampling='sequence' given explicitly is the default trainer bitwise over 5 updates:
    parameters, RMSprop state, ring, meta, no new buffer, and the raw metric vector. Element 9 of
    that vector, the pixel-control loss, is a sum of per-workgroup partials by float atomics
    (unreal_pc_loss_kernel; a metric only): two runs of the very same trainer differ in its last
    bits as soon as three partials meet, so at S = 4 (7 workgroups) it is held to rtol 1e-5 as
    tests/test_replay_gpu.py holds it, and at S = 1 (2 workgroups: a + b = b + a) the whole vector
    is compared bitwise."""
    import vnav

    def run(**kw):
        env = vnav.VectorEnv([_scene()], 4, seed=2, max_episode_steps=30, tasks=[(0, 5)])
        tr = vnav.A2CTrainer(env, num_steps=T, seed=3, max_time_steps=1e9, recurrent=True, arch="bighouse",
                             unreal=True, unreal_envs=S, unreal_source="replay", replay_size=3, **kw)
        raw = [tr.step(sync=False)["raw"].cpu().numpy() for _ in range(5)]
        torch.cuda.synchronize()
        return tr, raw

    a, ra = run()
    b, rb = run(rp_sampling="sequence")
    _same_state(a, b)
    for x, y in zip(ra, rb):
        assert x.dtype == y.dtype == np.float32 and x.shape == y.shape == (12,)
        if S > 1:
            np.testing.assert_allclose(x[9], y[9], rtol=1e-5)
            x, y = np.delete(x, 9), np.delete(y, 9)
        assert x.tobytes() == y.tobytes()
    for tr in (a, b):
        assert not tr.rp_skewed and "rp_sampling" not in tr._metric_layout
        assert not hasattr(tr, "ur_rows_ext") and not hasattr(tr, "rp_label")
        assert tr.ur_cap == (T + 1) * S and tr.ur_dx4.shape[0] == tr.ur_cap and tr.rp_x.shape[0] == (T - 2) * S


@pytest.mark.parametrize("E,S,rp_batch", [(4, 4, 5), (16, 8, 8)])
def test_draws_equal_the_restatement(E, S, rp_batch):
    """3 rp_batch = 15 and 24 appended frames: one on each side of the trunk's 16-row launch switch.
    After every update the sampled rows, labels, sources and stats4 are the restatement's on the
    trainer's own ring and meta; the metrics decode the same counts."""
    tr = _trainer(E=E, S=S, rp_batch=rp_batch, env_seed=3)  # a seed whose first update falls back, the next are mixed
    assert tr.rp_n == rp_batch and tr.ur_cap == (T + 1) * S + 3 * rp_batch
    both = fell_back = 0
    for k in range(5):
        m = tr.step(sync=True)
        meta = tr.replay_meta.cpu().tolist()
        assert meta[1] == min(k + 1, 3) and meta[2] == k + 1
        u = {key: tr.ur[key].cpu().numpy() for key in ("rewards", "dones", "rows")}
        want = rr.sample(u["rewards"], u["dones"], u["rows"], meta[1], rp_batch, tr.rp_skew, tr._rp_seed, meta[2])
        for got, w, name in zip(_draws(tr), want, ("rows_img", "rows_goal", "label", "src", "stats4")):
            assert got.tobytes() == w.tobytes(), (k, name, got, w)
        st = want[4].tolist()
        print("FIGURE update %d: |Q0| %d |Q1| %d drawn nonzero %d drawn %d" % (k, *st))
        assert [m["rp_candidates_zero"], m["rp_candidates_nonzero"], m["rp_drawn_nonzero"], m["rp_drawn"]] == st
        assert tr.unreal_stats[2].item() == st[3]  # the loss ran on exactly the non-void draws
        both += st[0] > 0 and st[1] > 0
        fell_back += st[0] == 0 or st[1] == 0
    assert both >= 1 and fell_back >= 1, (both, fell_back)  # neither path passes vacuously


def _frames_of(tr, rows):
    """uint8 [n, 84, 84, 3] frames of arena rows."""
    from vnav import _lib
    dst = torch.empty((rows.numel(), 84, 84, 3), dtype=torch.uint8, device="cuda")
    _lib.check(tr.lib.vn_gather_rows(ctypes.c_void_p(tr._arena), int(tr._fb), _lib.ptr(rows.contiguous()), rows.numel(),
                                     _lib.ptr(dst), tr._stream()), "vn_gather_rows")
    torch.cuda.synchronize()
    return dst.cpu()


TIE = 1e-6  # of a layer's largest |pre-activation|: below it the fp32 forward cannot decide a ReLU's sign


def test_rp_gradient_vs_fp64():
    """pc_weight = vr_weight = 0: after an update the rp block of grads and the trunk part of ur_grads
    hold only rp_weight * mean CE over the sampled windows. Its fp64 gradient from BigHouseOracle's
    conv_base layers, bighouse_reward_prediction and oracle.unreal.rp_loss (labels arranged as T = 3,
    S = rp_batch: rewards row 2 carries the class, a done at step 0 an unused draw) on the same
    frames and labels. Loss rtol 1e-5, every gradient tensor 1e-4 of its scale.

    ReLU ties: a pre-activation within TIE of zero has no sign the fp32 forward and the fp64 oracle
    must agree on (this case has two, |z| = 3e-8 at a layer scale of 0.43, in the two copies of one
    frame: with the oracle's own signs conv2's gradient is 1.9e-2 off in that one output channel).
    As GoalNetOracle.forward_masked does for the goal net, the oracle differentiates the function
    the GPU differentiated: every ReLU outside the tie band by the oracle's own sign, the few inside
    it by the one assignment under which all tensors meet the bound (at most 6 such units, else the
    case is unfit)."""
    import itertools

    from oracle import unreal as ou
    from oracle.policy import BigHouseOracle, bighouse_reward_prediction, frames_to_float
    rp_batch, w = 8, 0.7
    # a learning rate that leaves the predictor unsaturated over the two updates that fill the ring,
    # and an env seed whose third update draws both zero- and non-zero-reward windows
    tr = _trainer(E=16, S=8, rp_batch=rp_batch, pc_weight=0.0, vr_weight=0.0, rp_weight=w, learning_rate=1e-6,
                  env_seed=3)
    for _ in range(2):
        tr.step(sync=True)
    p0 = tr.params.detach().clone()
    m = tr.step(sync=True)
    ri, _, lab, _, st = _draws(tr)
    assert st[3] == rp_batch == tr.unreal_stats[2].item() and 0 < st[2] < rp_batch  # both classes in the loss
    ref = {k: v.double() for k, v in tr.net.to_reference(p0).items()}
    x = frames_to_float(_frames_of(tr, torch.as_tensor(ri.reshape(-1)).cuda())).double()
    rew = torch.zeros((3, rp_batch), dtype=torch.float64)
    rew[2] = torch.as_tensor(np.select([lab == 1, lab == 2], [1.0, -1.0], 0.0))
    don = torch.zeros((3, rp_batch), dtype=torch.bool)
    don[0] = torch.as_tensor(lab < 0)

    def oracle(flipped=()):
        """(loss, {name: gradient}, tie units) with the ReLUs of ``flipped`` (layer, flat index) inverted."""
        o = BigHouseOracle().double().load_reference(ref)
        a, ties = x, []
        for i, conv in enumerate((o.conv1, o.conv2, o.conv3)):  # conv_base: three Conv2d + ReLU
            z = conv(a)
            mask = (z > 0).double().contiguous()
            zf = z.detach().abs().reshape(-1)
            ties += [(i, int(j)) for j in torch.nonzero(zf <= TIE * zf.max()).reshape(-1)]
            for layer, j in flipped:
                if layer == i:
                    mask.view(-1)[j] = 1.0 - mask.view(-1)[j]
            a = z * mask
        sd = {k: ref[k].clone().requires_grad_() for k in ("rp.weight", "rp.bias")}
        logits = bighouse_reward_prediction(sd, a.view(rp_batch, 3, 32, 7, 7))
        loss, dlogits, count = ou.rp_loss(logits, rew, don)
        assert count == st[3]
        logits.backward(dlogits * float(np.float32(w)))
        want = {"rp.weight": sd["rp.weight"].grad, "rp.bias": sd["rp.bias"].grad}
        for k, mod in {"conv_base.0.0": o.conv1, "conv_base.0.2": o.conv2, "conv_base.0.4": o.conv3}.items():
            want[k + ".weight"], want[k + ".bias"] = mod.weight.grad, mod.bias.grad
        return float(loss), {k: v.numpy() for k, v in want.items()}, ties

    g_rp, g_ur = tr.net.to_reference(tr.grads), tr.net.to_reference(tr.ur_grads)

    def errors(want):
        return {k: np.abs((g_rp if k.startswith("rp.") else g_ur)[k].double().numpy() - v).max() / np.abs(v).max()
                for k, v in want.items()}

    loss, want, ties = oracle()
    print("FIGURE ReLU ties within %g of a layer's scale: %s" % (TIE, ties))
    assert len(ties) <= 6, "too many undecidable ReLUs: choose another case"
    err = errors(want)
    for r in range(1, len(ties) + 1):
        for sub in itertools.combinations(ties, r):
            if max(err.values()) <= TOL:
                break
            loss2, want2, _ = oracle(sub)
            err2 = errors(want2)
            if max(err2.values()) < max(err.values()):
                loss, want, err = loss2, want2, err2
    got_loss = tr.unreal_stats[1].item()
    print("FIGURE rp loss: %.3g of the bound" % (abs(got_loss - loss) / (LOSS_RTOL * loss)))
    assert abs(got_loss - loss) <= LOSS_RTOL * loss and m["rp_loss"] == got_loss
    for k, e in err.items():
        scale = np.abs(want[k]).max()
        print("FIGURE %s: %.3g of the bound (scale %.3g)" % (k, e / TOL, scale))
        assert scale > 0 and e <= TOL, (k, e)
    # nothing else reached the replayed pass's trunk gradient: conv_merge got zeros
    assert not g_ur["conv_merge.0.1.weight"].any()
    # and in the update's whole gradient of a conv_base weight the rp share is far above the bound
    k = "conv_base.0.4.weight"
    share = np.abs(want[k]).max() / np.abs(g_rp[k].double().numpy()).max()
    print("FIGURE rp share of %s: %.3g" % (k, share))
    assert share >= 10 * TOL


def _ref_trainer(graph, E, S, **kw):
    """thor-cached-auxiliary's settings (tests/test_replay_gpu.py): 174x174, the goal arch, LSTM + aux
    heads + UNREAL, both batches replayed."""
    import vnav
    from test_aux_gpu import _aux_scene
    env = vnav.VectorEnv([_aux_scene(0, (174, 174, 3))], E, seed=5, max_episode_steps=30)
    return vnav.A2CTrainer(env, num_steps=T, seed=3, max_time_steps=1e9, recurrent=True, aux_weight=0.1, unreal=True,
                           unreal_envs=S, aux_source="replay", unreal_source="replay", replay_size=3,
                           cuda_graph=graph, entropy_coefficient=0.001, rp_sampling="skewed", **kw)


@pytest.mark.parametrize("E,S", [(16, 8), (4, 4)])
def test_cuda_graph_is_bit_identical(E, S):
    def run(graph):
        tr = _ref_trainer(graph, E, S)
        ms, draws = [], []
        for _ in range(7):
            ms.append(tr.step(sync=True))
            draws.append(_draws(tr))
        torch.cuda.synchronize()
        return tr, ms, draws

    a, ma, da = run(False)
    b, mb, db = run(True)
    assert b._graph is not None
    _same_state(a, b)
    for x, y in zip(da, db):
        for p, q in zip(x, y):
            assert p.tobytes() == q.tobytes()
    assert any(d[4][3] > 0 for d in da)
    for x, y in zip(ma, mb):
        for k in ("value_loss", "rp_loss", "vr_loss", "grad_norm", "entropy", "rp_candidates_zero",
                  "rp_candidates_nonzero", "rp_drawn_nonzero", "rp_drawn"):
            assert x[k] == y[k], (k, x[k], y[k])


def test_resume_continues_the_draws():
    a = _trainer(rp_batch=5)
    for _ in range(6):
        a.step(sync=True)
    b = _trainer(rp_batch=5)
    for _ in range(3):
        b.step(sync=True)
    sd = b.state_dict()
    assert not [k for k in sd if k.startswith("rp_")]  # no new checkpoint key: the counter is the ring's
    c = _trainer(rp_batch=5)
    c.load_state_dict(sd)
    for _ in range(3):
        c.step(sync=True)
    torch.cuda.synchronize()
    _same_state(a, c)
    for p, q in zip(_draws(a), _draws(c)):
        assert p.tobytes() == q.tobytes()


def test_inline_pass_stream_guard_and_update_without_batch():
    def run(inline=False, debug=False, bare=False):
        if inline:
            os.environ["VN_UNREAL_INLINE"] = "1"
        try:
            tr = _trainer(E=16, S=8, rp_batch=8)
        finally:
            os.environ.pop("VN_UNREAL_INLINE", None)
        assert tr._unreal_inline == inline
        tr.debug_streams = debug
        for _ in range(4):
            if bare:  # update(None): the push and the draws happen inside the update
                tr.rollout()
                tr.update(None)
            else:
                tr.step(sync=True)
        torch.cuda.synchronize()
        return tr

    a = run()
    for other in (run(inline=True), run(debug=True), run(bare=True)):
        _same_state(a, other)
        for p, q in zip(_draws(a), _draws(other)):
            assert p.tobytes() == q.tobytes()
    names = [k for k, _ in a._side_owned()]
    for k in ("ur_rows_ext", "rp_label", "rp_src", "rp_draw_stats", "ur_acts", "ur_dx4"):
        assert k in names


def test_constructor_refusals():
    import vnav
    env = vnav.VectorEnv([_scene()], 4, seed=2, max_episode_steps=30, tasks=[(0, 5)])

    def make(**kw):
        args = dict(num_steps=T, seed=3, recurrent=True, arch="bighouse", unreal=True, unreal_envs=4,
                    unreal_source="replay", replay_size=3, rp_sampling="skewed")
        args.update(kw)
        return vnav.A2CTrainer(env, **args)

    for kw in (dict(unreal=False), dict(unreal_source="rollout"), dict(rp_skew=-0.1), dict(rp_skew=1.5),
               dict(rp_batch=0), dict(rp_batch=-2), dict(rp_sampling="uniform")):
        with pytest.raises(ValueError):
            make(**kw)
    os.environ["VN_REPLAY_MERGED"] = "1"
    try:
        with pytest.raises(ValueError, match="VN_REPLAY_MERGED"):
            make()
    finally:
        os.environ.pop("VN_REPLAY_MERGED", None)
    tr = make(rp_skew=0.0, rp_batch=1)
    assert tr.rp_n == 1 and make().rp_n == 4  # rp_batch defaults to unreal_envs
