"""One A2CTrainer update restated in float64 (TEST INFRASTRUCTURE ONLY — see oracle/__init__.py).

second_update_vs_fp64 runs a trainer's second rollout + update on a small random maze and
restates it on the CPU: the env transitions on the oracle env driven by the same actions, the
sampled actions by the Philox inverse-CDF draw on the rollout's logits, the masked trunk, the
LSTM with the MaskedRNN convention, the heads, the returns, the A2C loss, the aux deconv MSE
and — with unreal=True — the UNREAL terms as A2CTrainer._unreal_head_losses wires them:
  * pixel control (oracle.policy.pixel_control / bighouse_pixel_control, oracle.unreal.pc_loss)
    on h_t of the envs e < S for t < T plus the bootstrap h; the frames of pixel_change are the
    rollout's image rows and, for the observation after the last step, the env's current
    img_row;
  * reward prediction (reward_prediction, rp_loss) on the conv_base maps of frames t..t+2;
  * value replay (vr_loss) on V of the first S envs against the returns.
The oracle's loss functions detach at q / logits / values; their returned gradients are chained
into the graph as the linear term sum(x * dL/dx), so the parameter gradients are those of the
losses. Every ReLU runs with the GPU forward's own mask (a pre-activation within rounding of
zero may sit on the other side there: a tie, not an error). Each loss term's gradient is taken
on its own, so the gradient with one term dropped is the total minus that term's: `visible`
gives, per UNREAL term, its share of a tensor it has in common with the A2C loss, in units of
that tensor's scale in the total — a term below the tolerance could go missing unnoticed.

Above 16 envs the goal net's trainer runs shared_base on a goal frame once per goal run
(vn_goal_runs); the restatement runs it on every sample and takes a sample's goal-map masks
from the start of its run, where the GPU stored them.

Used by tests/test_prod_oracle_gpu.py (the logged run's shape, no UNREAL),
tests/test_unreal_update_gpu.py and tests/test_lstm_regimes_gpu.py (20 and 136 envs).
"""
import dataclasses

import numpy as np
import torch

from oracle import a2c as oa2c
from oracle import envs as oe
from oracle import graph as og
from oracle import philox
from oracle import unreal as ou
from oracle.policy import (BIGHOUSE_UNREAL_PARAM_ORDER, UNREAL_PARAM_ORDER, AuxHeadsOracle, BigHouseOracle,
                           GoalNetOracle, aux_targets, bighouse_pixel_control, bighouse_reward_prediction,
                           frames_to_float, pixel_control, reward_prediction)
from oracle.trunk_checks import (AUX_NAMES, BIGHOUSE_NAMES, LSTM_NAMES, NAMES, _bighouse_forward_masked,
                                 _bighouse_masks, _check_masks_are_signs, _check_outputs, _elementwise, _err,
                                 _gpu_masks, _ties_only)

UNREAL_REWARDS = (1.0, 0.0, -0.1)  # goal, step, collision: the three reward-prediction classes

# The composed-update cases of tests/test_unreal_update_gpu.py. E, S, T of the small ones are the
# smallest that keep S < E (rows t*E + e differ from t*S + e), T - 2 >= 2 reward-prediction
# samples per env and room for a reset inside the rollout; the frame sizes are the smallest the
# kernels are instantiated for (pixel control crops 42 cells of 4 px, BigHouseModel's 20).
# max_steps: the episode limit, short so that dones fall inside the second rollout. visible:
# the tensor each UNREAL term shares with the A2C loss (see second_update_vs_fp64).
UPDATE_CASES = {
    "goal-174-aux": dict(arch="goal", hw=(174, 174), E=5, S=3, T=6, aux_weight=0.1, max_steps=4),
    "goal-174-noaux": dict(arch="goal", hw=(174, 174), E=5, S=3, T=6, aux_weight=0.0, max_steps=4),
    "goal-174-logged": dict(arch="goal", hw=(174, 174), E=4, S=4, T=20, aux_weight=0.1, max_steps=9),
    "bighouse-84": dict(arch="bighouse", hw=(84, 84), E=5, S=3, T=6, aux_weight=0.0, max_steps=4),
}
VISIBLE_IN = {"goal": {"pc": "rnn.inner.weight_hh_l0", "rp": "conv_base.0.0.weight", "vr": "critic.0.weight"},
              "bighouse": {"pc": "rnn.inner.weight_hh_l0", "rp": "conv_base.0.4.weight", "vr": "critic.0.weight"}}


def maze_scene(hw, aux, rewards=None):
    """The logged-run test's scene at frame size hw: a 5 x 6 random maze with random frames
    (and depth / segmentation for the aux heads). -> (scene, graph, spd, frames)."""
    import vnav
    maze = np.random.RandomState(2).rand(5, 6) > 0.2
    graph, spd, _ = og.h5_tables(maze)
    ns = len(graph)
    rng = np.random.RandomState(4)
    h, w = hw
    frames = rng.randint(0, 256, size=(ns, h, w, 3)).astype(np.uint8)
    scene = vnav.scene_from_arrays(graph, spd, frames) if rewards is None else \
        vnav.scene_from_arrays(graph, spd, frames, rewards=tuple(rewards))
    if aux:
        scene = dataclasses.replace(scene, depth=rng.randint(0, 256, size=(ns, h, w, 1)).astype(np.uint8),
                                    segmentation=rng.randint(0, 256, size=(ns, h, w, 3)).astype(np.uint8))
    return scene, graph, spd, frames


def _pc_masks(net, params, h_pc):
    """The pixel-control ReLU masks of the trainer's pc_forward: the same call on the same rows
    (the backward overwrites the trainer's own buffers with gradients)."""
    n, A = h_pc.shape[0], net.num_actions
    pcb, a1, p2, _ = net.pc_buffers(n, with_q=False)
    ws = torch.empty(net.pc_workspace_floats(), dtype=torch.float32, device=h_pc.device)
    net.pc_forward(params, h_pc, n, pcb, a1, p2, None, ws)
    m = {"pc_base": pcb > 0}
    if a1 is None:
        m.update({"pc_value": p2[..., :A] > 0, "pc_action": p2[..., A:A + 1] > 0})
    else:
        m.update({"pc_value.0": a1[..., :32] > 0, "pc_action.0": a1[..., 32:] > 0, "pc_value.2": p2[..., :A] > 0,
                  "pc_action.2": p2[..., A:A + 1] > 0})
    return {k: v.permute(0, 3, 1, 2).cpu() for k, v in m.items()}


def second_update_vs_fp64(scene, graph, spd, frames, E, T, seed, env_seed, max_steps, **trainer_kw):
    """Build VectorEnv + A2CTrainer(recurrent, **trainer_kw), run one full step, then the second
    rollout + update, and restate that update in float64. Asserts the env transitions, the
    sampled actions and the rollout's logits / values / bootstrap values as it goes. Returns a
    dict: errs (every tensor of the total gradient: |gpu - fp64| of the tensor's scale), mine /
    want (the gradients by reference name), stats (gpu, fp64) of the UNREAL losses, info (dones,
    reward-prediction samples and classes), visible (see the module docstring), tr (the trainer)."""
    import vnav
    from vnav import dist as vdist
    env = vnav.VectorEnv([scene], E, seed=env_seed, max_episode_steps=max_steps)
    tr = vnav.A2CTrainer(env, num_steps=T, seed=seed, max_time_steps=1e6, recurrent=True, **trainer_kw)
    net = tr.net
    A, arch, hw = net.num_actions, net.arch, net.frame_hw
    unreal, w = bool(getattr(tr, "unreal", False)), float(tr.aux_weight)
    o = oe.VectorEnvOracle([dict(graph=graph, spd=spd, rewards=scene.rewards)], E, env_seed, max_steps=max_steps)
    tr.step(sync=True)
    a1 = tr.actions.cpu().numpy().reshape(T, E)
    for t in range(T):
        o.step(a1[t])
    h0, c0 = tr.h0.cpu().double(), tr.c0.cpu().double()
    p0 = tr.params.detach().clone()
    tr.rollout()
    N = T * E
    if arch == "bighouse":
        masks, bmasks = _bighouse_masks(net, tr.acts, N), _bighouse_masks(net, tr.boot_acts, E)
    else:
        # above 16 envs the trainer runs shared_base on a goal frame once per goal run (vn_goal_runs): a
        # sample's goal maps, and so their ReLU masks, are those stored at the start of its run
        src = None
        if tr.dedup_goals:
            src = torch.arange(N) + tr.goal_delta.cpu().view(-1).long()
            starts = torch.cat((torch.ones(1, E, dtype=torch.bool), tr.dones.cpu().view(T, E)[:-1].bool())).view(-1)
            assert torch.equal(src == torch.arange(N), starts), "goal runs start at step 0 and after each done"
        masks, bmasks = _gpu_masks(net, tr.acts, N, goal_src=src), _gpu_masks(net, tr.boot_acts, E)
    amasks = None
    if w > 0:  # the aux heads' ReLU masks: the same first layer run on the rollout's X4
        a1buf, predbuf = net.aux_buffers(N)
        net.aux_forward(tr.params, tr.acts, N, N, a1buf, predbuf,
                        torch.empty(net.aux_workspace_floats(), device="cuda"))
        amasks = [(a1buf[..., 16 * h:16 * h + 16] > 0).permute(0, 3, 1, 2).double().cpu() for h in range(3)]
    rows_i, rows_g = tr.rows_img.cpu().numpy(), tr.rows_goal.cpu().numpy()
    brows = (env._info["img_row"].cpu().numpy(), env._info["goal_row"].cpu().numpy())
    actions = tr.actions.cpu().long()
    rewards, dones = tr.rewards.cpu(), tr.dones.cpu()
    out = tr.out.cpu().double()
    boot = tr.boot_out.cpu().double()
    lmask, lra = tr.masks.cpu().double(), tr.lra.cpu().double()
    bmask, blra = tr.boot_mask.cpu().double(), tr.boot_lra.cpu().double()
    if unreal:
        S = tr.unreal_S
        h_pc = torch.cat((tr.h_all[:N].view(T, E, 512)[:, :S].reshape(T * S, 512), tr.boot_h[:S])).contiguous()
        pmasks = _pc_masks(net, tr.params, h_pc)
    tr.update()
    grads = tr.grads.clone()
    torch.cuda.synchronize()
    res = dict(tr=tr, E=E, T=T)
    if unreal:
        assert torch.equal(tr.h_pc, h_pc), "vn_unreal_gather: h rows t*E+e -> t*S+e, bootstrap rows from boot_h"

    # env transitions (index-only vn_step) vs the env oracle on the same actions
    a2 = actions.numpy().reshape(T, E)
    for t in range(T):
        r = o.step(a2[t])
        ri = rows_i[(t + 1) * E:(t + 2) * E] if t + 1 < T else brows[0]
        rg = rows_g[(t + 1) * E:(t + 2) * E] if t + 1 < T else brows[1]
        assert np.array_equal(ri, r["img_row"]) and np.array_equal(rg, r["goal_row"]), t
        assert np.array_equal(rewards[t].numpy().view(np.uint32), r["reward"].view(np.uint32)), t
        assert np.array_equal(dones[t].numpy(), r["done"]), t
    # sampled actions: Philox stream 3 inverse-CDF on the rollout's logits (vn_a2c.hip sample_kernel)
    k = vdist.rank_seed(seed, 0)
    lg = out[:, :A].numpy().astype(np.float32).reshape(T, E, A)
    for t in range(T):
        ctr = T * 1 + t  # updates so far x T + step
        rr = philox.philox4x32_10(np.arange(E), ctr & 0xffffffff, ctr >> 32, philox.STREAM_POLICY,
                                  k & 0xffffffff, k >> 32)[0]
        u = (rr >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)
        p = np.exp(lg[t] - lg[t].max(1, keepdims=True))
        p = p / p.sum(1, keepdims=True)
        cdf = np.cumsum(p, 1)
        want = np.minimum((u[:, None] >= cdf[:, :A - 1]).sum(1), A - 1)
        near = np.abs(u[:, None] - cdf[:, :A - 1]).min(1) < 1e-5
        assert np.array_equal(want[~near], a2[t][~near]), t

    sd = net.to_reference(p0)
    fl = lambda x: frames_to_float(torch.as_tensor(x)).double()  # noqa: E731
    if arch == "bighouse":
        ref = BigHouseOracle(A).load_reference(sd).double()
        lstm = ref.lstm
        x4, f, pre = _bighouse_forward_masked(ref, fl(frames[rows_i]), masks)
        _ties_only(masks, pre, {"m1": "z1", "m2": "z2", "m3": "z3", "m5": "z5"})
        x5 = f.view(T, E, 512)
        _, xb, _ = _bighouse_forward_masked(ref, fl(frames[brows[0]]), bmasks)
        names = BIGHOUSE_NAMES
    else:
        ref = GoalNetOracle(hw, 3, A).load_reference(sd).double()
        lstm = torch.nn.LSTM(512 + A + 1, 512, batch_first=True).double()
        for name in LSTM_NAMES:
            getattr(lstm, name).data.copy_(sd["rnn.inner." + name].double())
        _, _, x4, pre = ref.forward_masked(fl(frames[rows_i]), fl(frames[rows_g]), masks)
        _check_masks_are_signs(masks, pre)
        x5 = (pre["z5"] * masks["m5"]).view(T, E, 512)
        _, _, _, bpre = ref.forward_masked(fl(frames[brows[0]]), fl(frames[brows[1]]), bmasks)
        xb = bpre["z5"] * bmasks["m5"]
        names = NAMES
    h, c = h0[None], c0[None]
    ys = []
    for t in range(T):
        m = lmask[t][None, :, None]
        y, (h, c) = lstm(torch.cat((x5[t], lra[t]), 1)[:, None], (h * m, c * m))
        ys.append(y[:, 0])
    m = bmask[None, :, None]
    yb, _ = lstm(torch.cat((xb, blra), 1)[:, None], (h * m, c * m))
    y = torch.cat(ys)
    logits, value = ref.policy_logits(y), ref.critic(y).view(-1)
    vboot = ref.critic(yb[:, 0]).view(-1)
    _check_outputs(out[:, :A].numpy(), out[:, A].numpy(), logits.detach().numpy(), value.detach().numpy())
    assert _err(boot[:, A].numpy(), vboot.detach().numpy()) <= 1e-5
    assert _elementwise(boot[:, A].numpy(), vboot.detach().numpy()) <= 1.0
    vext = torch.cat([value.detach().view(T, E), vboot.detach().view(1, E)])
    R = oa2c.returns(rewards.double(), dones, vext, 0.99)
    loss, _ = oa2c.loss(logits, value, actions, R.view(-1))
    heads = None
    if w > 0:
        heads = AuxHeadsOracle().load_reference(sd).double()
        preds, apre = heads.forward_masked(x4, amasks)
        dd, ss = scene.depth, scene.segmentation
        ph, pw = net.aux_layout["p_hw"]
        tgt = [t_.double() for t_ in aux_targets(dd[rows_i], ss[rows_i], ss[rows_g], 4, (ph, pw))]
        loss = loss + w * sum(torch.nn.functional.mse_loss(p, t_) for p, t_ in zip(preds, tgt))
    terms = {"a2c": loss}
    usd = None
    if unreal:
        order = BIGHOUSE_UNREAL_PARAM_ORDER if arch == "bighouse" else UNREAL_PARAM_ORDER
        usd = {k_: sd[k_].double().requires_grad_() for k_ in order}
        C = net.pc_side
        # pixel control: rows t*S + e of h_t (t < T) and the bootstrap h
        hp = torch.cat((y.view(T, E, 512)[:, :S].reshape(T * S, 512), yb[:S, 0]))
        q = (bighouse_pixel_control if arch == "bighouse" else pixel_control)(usd, hp, pmasks)
        q5 = q.permute(0, 2, 3, 1).reshape(T + 1, S, C, C, A)
        prow = np.concatenate((rows_i.reshape(T, E)[:, :S], brows[0][None, :S]))
        pc, gq = ou.pc_loss(q5, torch.as_tensor(frames[prow]), actions.view(T, E)[:, :S], dones[:, :S], tr.pc_gamma)
        terms["pc"] = tr.pc_weight * (q5 * gq).sum()
        # reward prediction: the conv_base maps of frames ts-2..ts, ts = 2..T-1, env-minor
        xs = x4.reshape(T, E, *x4.shape[1:])[:, :S]
        feats = torch.stack([xs[k_:k_ + T - 2] for k_ in range(3)], 2).reshape(-1, 3, *x4.shape[1:])
        rl = (bighouse_reward_prediction if arch == "bighouse" else reward_prediction)(usd, feats)
        rp, grl, count = ou.rp_loss(rl, rewards[:, :S], dones[:, :S])
        terms["rp"] = tr.rp_weight * (rl * grl).sum()
        # value replay: V of the first S envs against the returns
        vs = value.view(T, E)[:, :S]
        vr, gv = ou.vr_loss(vs, R.view(T, E)[:, :S])
        terms["vr"] = tr.vr_weight * (vs * gv).sum()
        st = tr.unreal_stats.cpu().double().numpy()
        res["stats"] = ({"pc": st[0] / (T * S * C * C), "rp": st[1], "vr": st[3] / (T * S), "rp_count": int(st[2])},
                        {"pc": pc.item(), "rp": rp.item(), "vr": vr.item(), "rp_count": count})
        ts = torch.arange(2, T).repeat_interleave(S)
        e_ = torch.arange(S).repeat(T - 2)
        used = ~(dones[ts - 2, e_].bool() | dones[ts - 1, e_].bool())
        r_ = rewards[ts, e_][used]
        res["info"] = dict(dones=int(dones[:, :S].sum()), rp_used=int(used.sum()), rp_skipped=int((~used).sum()),
                           classes=sorted({0 if v == 0 else (1 if v > 0 else 2) for v in r_.tolist()}))
    # the gradient of each term on its own: the total is their sum, and the total without one
    # term is the total minus that term's
    plist = {}
    for k_, attr in names.items():
        for kind in ("weight", "bias"):
            plist[k_ + "." + kind] = getattr(getattr(ref, attr), kind)
    for name in LSTM_NAMES:
        plist["rnn.inner." + name] = getattr(lstm, name)
    if heads is not None:
        for hd, name in zip(heads.heads, AUX_NAMES):
            for i, layer in ((1, hd[0]), (3, hd[2])):
                for kind in ("weight", "bias"):
                    plist["%s.0.%d.%s" % (name, i, kind)] = getattr(layer, kind)
    if usd is not None:
        plist.update(usd)
    keys = list(plist)
    per = {}
    for tname, term in terms.items():
        g = torch.autograd.grad(term, [plist[k_] for k_ in keys], retain_graph=True, allow_unused=True)
        per[tname] = {k_: (torch.zeros_like(plist[k_]) if gi is None else gi) for k_, gi in zip(keys, g)}
    want = {k_: sum(per[tname][k_] for tname in per) for k_ in keys}
    mine = net.to_reference(grads)
    res["errs"] = {k_: _err(mine[k_].numpy(), want[k_].numpy()) for k_ in keys}
    res["mine"], res["want"], res["grads"] = mine, want, grads
    res["visible"] = {tname: {k_: float(per[tname][k_].abs().max() / max(float(want[k_].abs().max()), 1e-30))
                              for k_ in keys} for tname in per if tname != "a2c"}
    return res

