"""Production-size kernel paths against the fp64 oracle, directly.

The training update runs its batches through kernels that small test batches never reach:
persistent conv kernels that wrap their grids (conv1 banded forward / weight gradient,
the x6 conv2 / conv3 weight gradients with the two-stage slab reduce, the parity-class
input gradients, the conv2 input gradient), products with enough tiles to skip split-K
(>= 128 tiles: the conv_merge / head / LSTM products at >= 4096 rows) and the LSTM at
thousands of envs. These tests run those paths at batch sizes that take them — 84x84 with
4096 samples, 174x174 with 512 samples through the scene-cache row gather plus the aux
heads' fused loss, the LSTM core at 1024 envs — and compare every output and parameter
gradient with oracle/policy.py evaluated in float64 on the CPU.

ReLU ties: a pre-activation within fp32 rounding of zero can take the other side of its
ReLU on the GPU, and its channel's weight gradient then moves by ~1e-3 of the scale (a
tie, not an error). Instead of shrinking the batch until no tie occurs, the oracle is run
with the GPU forward's own ReLU masks (GoalNetOracle.forward_masked), read from the
activation store the kernels wrote; every mask bit that disagrees with the sign of the
oracle's own pre-activation is asserted to be a tie (|z| <= 1e-5 of the layer's scale).

Tolerances (north star): outputs 1e-5, parameter gradients 1e-4 of each tensor's scale.
Logits and values are also checked element by element: |gpu - fp64| <= 1e-5 |fp64| + a floor
of 1e-6 of the tensor's scale (a logit near zero is a sum of cancelling terms whose fp32
rounding is set by the terms, not by the sum: the floor states that absolute bound).
The checks themselves are oracle/trunk_checks.py, shared with tests/test_few_env_gpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle.policy import AuxHeadsOracle, GoalNetOracle, aux_targets, frames_to_float
from oracle.trunk_checks import (AUX_NAMES, NAMES, _check_masks_are_signs, _check_outputs, _err,
                                 _gpu_masks, _grads_vs_oracle, lstm_core_check)
from oracle.trunk_checks import a2c_loss_grad as _loss_grad

pytestmark = pytest.mark.gpu


def _noisy_policy(hw, seed, aux=False):
    from vnav.policy import GoalNavPolicy
    torch.manual_seed(seed)
    pol = GoalNavPolicy(3, 4, hw, aux=aux)
    with torch.no_grad():
        pol.params.add_(torch.randn_like(pol.params) * 0.01)
        if aux:  # block-diagonal second head layer, zero pad channel (the layout's structure)
            w1, b1, w2, b2 = pol.net.views(pol.params.data)["aux"]
            m = torch.zeros(48, 8, device=w2.device)
            m[0:16, 0] = 1
            m[16:32, 1:4] = 1
            m[32:48, 4:7] = 1
            w2.mul_(m[:, None, None, :])
            b2[7] = 0.0
    return pol


def test_84_batch4096_forward_backward_vs_fp64_oracle():
    """84x84, 4096 samples (the bench's per-step env count): forward outputs, conv_merge
    features and every parameter gradient of the A2C loss vs the fp64 oracle."""
    from vnav.policy import frames_from_batch
    pol = _noisy_policy((84, 84), 21)
    net, params = pol.net, pol.params.data
    n = 4096
    g = torch.Generator(device="cuda").manual_seed(5)
    img = torch.randint(0, 256, (n, 84, 84, 3), dtype=torch.uint8, device="cuda", generator=g)
    gl = torch.randint(0, 256, (n, 84, 84, 3), dtype=torch.uint8, device="cuda", generator=g)
    actions = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda", generator=g)
    rets = torch.randn(n, device="cuda", generator=g)
    acts = net.new_acts(n)
    out = torch.zeros((n, 8), device="cuda")
    frames = frames_from_batch(img, gl)
    net.forward(params, frames, n, acts, n, 0, out)
    masks = _gpu_masks(net, acts, n)
    x5 = net.x5(acts, n).double().cpu()
    dout = _loss_grad(out, actions, rets)
    grads = torch.zeros_like(params)
    ws = torch.empty(net.workspace_floats(n), device="cuda")
    net.backward(params, frames, n, acts, n, dout, grads, ws)
    torch.cuda.synchronize()

    ref = GoalNetOracle((84, 84)).load_reference(pol.reference_state_dict()).double()
    fi, fg = frames_to_float(img.cpu()).double(), frames_to_float(gl.cpu()).double()
    logits, value, _, pre = ref.forward_masked(fi, fg, masks)
    flips = _check_masks_are_signs(masks, pre)
    o = out.cpu().numpy()
    _check_outputs(o[:, :4], o[:, 4], logits.detach().numpy(), value.detach().numpy().ravel())
    assert _err(x5.numpy(), (pre["z5"] * masks["m5"]).detach().numpy()) <= 1e-5
    loss, _ = oa2c.loss(logits, value.view(-1), actions.cpu().long(), rets.cpu().double())
    loss.backward()
    worst = _grads_vs_oracle(net, grads, ref)
    print("84x84 n=4096: worst gradient error %.3g of scale; tie flips %s" % (worst, flips))


def _aux_scene(hw=(174, 174), X=6):
    import vnav
    rng = np.random.RandomState(3)
    Y = X
    h, w = hw
    maze = np.ones((X, Y), dtype=bool)
    obs = rng.randint(0, 256, size=(X, Y, 4, h, w, 3)).astype(np.uint8)
    dep = rng.randint(0, 256, size=(X, Y, 4, h, w, 1)).astype(np.uint8)
    seg = rng.randint(0, 256, size=(X, Y, 4, h, w, 3)).astype(np.uint8)
    return vnav.oriented_scene(maze, obs, [(0, 0, 1)], depths=dep, segmentations=seg)


def _gather(env, rows):
    from vnav import _lib
    arena, fb, _, _ = env.frame_arena()
    dst = torch.empty((rows.numel(),) + tuple(env.frame_shape), dtype=torch.uint8, device=env.device)
    _lib.check(env.lib.vn_gather_rows(ctypes.c_void_p(arena), int(fb), _lib.ptr(rows), rows.numel(), _lib.ptr(dst),
                                      env._stream()), "vn_gather_rows")
    return dst


@pytest.mark.parametrize("hw,n", [((174, 174), 512), ((300, 400), 512)], ids=["174x174", "c5_300x400"])
def test_batch_rows_aux_vs_fp64_oracle(hw, n):
    """174x174 (the reference topology) and config C5's 300x400 (the size-adaptive trunk:
    74x99 -> 36x48 -> 17x23, conv_merge over 12,512 features, heads to 74x98), 512 samples
    gathered from the scene cache by row, as the trainer's update runs them (the C5 leg's
    rollout forward runs 512 envs per step): trunk + heads forward, the aux heads' fused loss
    (vn_aux_forward_loss_grad), the aux backward into dL/dX4 and the trunk backward of the
    A2C loss + 0.1 x the deconv loss — outputs, predictions and every gradient vs fp64, with
    the GPU's ReLU masks (no tie search)."""
    import vnav
    from vnav.policy import AuxTargets, frames_from_rows
    pol = _noisy_policy(hw, 8, aux=True)
    net, params = pol.net, pol.params.data
    env = vnav.VectorEnv([_aux_scene(hw, 6 if hw == (174, 174) else 4)], 8, seed=1)
    arena, fb, rows_total, _ = env.frame_arena()
    w = 0.1
    g = torch.Generator(device="cuda").manual_seed(9)
    rows_i = torch.randint(0, rows_total, (n,), dtype=torch.int32, device="cuda", generator=g)
    rows_g = torch.randint(0, rows_total, (n,), dtype=torch.int32, device="cuda", generator=g)
    actions = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda", generator=g)
    rets = torch.randn(n, device="cuda", generator=g)
    frames = frames_from_rows(arena, fb, rows_i, rows_g)
    acts = net.new_acts(n)
    out = torch.zeros((n, 8), device="cuda")
    net.forward(params, frames, n, acts, n, 0, out)
    masks = _gpu_masks(net, acts, n)
    dout = _loss_grad(out, actions, rets)
    depth, seg = env.aux_arena
    table = net.aux_target_table(depth, seg)
    tg = AuxTargets(table.data_ptr(), rows_i.data_ptr(), rows_g.data_ptr())
    a1, pred = net.aux_buffers(n)
    dpred = torch.empty_like(pred)
    stats = torch.zeros(4, device="cuda")
    aws = torch.empty(net.aux_workspace_floats(), device="cuda")
    net.aux_forward_loss_grad(params, acts, n, n, a1, pred, tg, w, dpred, stats, aws)
    amasks = [(a1[..., 16 * h:16 * h + 16] > 0).permute(0, 3, 1, 2).double().cpu() for h in range(3)]
    grads = torch.zeros_like(params)
    dx4 = torch.empty((n, net.fc_in), device="cuda")
    net.aux_backward(params, acts, n, n, a1, dpred, grads, dx4, aws)
    ws = torch.empty(net.workspace_floats(n), device="cuda")
    net.backward_ex(params, frames, n, acts, n, dout, None, dx4, grads, ws)
    img, gl = _gather(env, rows_i).cpu(), _gather(env, rows_g).cpu()
    ri, rg = rows_i.cpu().numpy(), rows_g.cpu().numpy()
    dd, ss = depth.cpu().numpy(), seg.cpu().numpy()
    torch.cuda.synchronize()

    sd = pol.reference_state_dict()
    ref = GoalNetOracle(hw).load_reference(sd).double()
    heads = AuxHeadsOracle().load_reference(sd).double()
    logits, value, x4, pre = ref.forward_masked(frames_to_float(img).double(), frames_to_float(gl).double(), masks)
    flips = _check_masks_are_signs(masks, pre)
    preds, apre = heads.forward_masked(x4, amasks)
    for m, z in zip(amasks, apre):
        bad = (m > 0) != (z.detach() > 0)
        if bad.any():
            assert float(z.detach()[bad].abs().max() / z.detach().abs().max()) <= 1e-5
    o = out.cpu().numpy()
    _check_outputs(o[:, :4], o[:, 4], logits.detach().numpy(), value.detach().numpy().ravel())
    ph, pw = net.aux_layout["p_hw"]
    tgt = [t.double() for t in aux_targets(dd[ri], ss[ri], ss[rg], 4, (ph, pw))]
    mse = [torch.nn.functional.mse_loss(p, t) for p, t in zip(preds, tgt)]
    numel = np.array([1, 3, 3]) * n * ph * pw
    assert _err(stats[:3].cpu().numpy() / numel, np.array([m.item() for m in mse])) <= 1e-5
    loss, _ = oa2c.loss(logits, value.view(-1), actions.cpu().long(), rets.cpu().double())
    (loss + w * sum(mse)).backward()
    worst = _grads_vs_oracle(net, grads, ref, heads)
    print("%dx%d n=%d + aux: worst gradient error %.3g of scale; tie flips %s" % (hw[0], hw[1], n, worst, flips))


@pytest.mark.parametrize("E", [2048, 1024, 16, 5])
def test_lstm_core_vs_fp64_torch_lstm(E):
    """The recurrent core at 2048 envs x 3 steps (6144 rows: the trunk-feature gradient
    dz5 = dgates x W_ih takes the unsplit 128 x 128 EpiMask product the training update runs at
    >= 4096 rows), at 1024 envs x 3 steps (gates / dh products past the split-K
    threshold, the weight gradient over 3072 rows) and at 16 / 5 envs (the fused VALU
    steps of vn_skinny.h: xcat + gates + cell, dh product + next cell backward): per-step
    (h, c), the heads on h, and the gradients of W_ih, W_hh, both biases, the heads and
    dL/dZ5 (masked by the features' ReLU) vs torch's float64 nn.LSTM with the restated
    MaskedRNN convention."""
    lstm_core_check(E, T=3, A=4)


def test_logged_run_shape_trainer_update_vs_fp64_oracle():
    """The reference's own batch (outputs/output.txt: 174x174, LSTM + deconv heads, aux weight
    0.1, 4 envs x 20 steps): the second rollout + update of A2CTrainer — the small-batch
    split-K products and their epilogues, the per-step LSTM / sampling / index-only env
    step / step_post kernels — restated in float64: the env transitions against the env
    oracle driven by the same actions, the sampled actions against the Philox inverse-CDF
    draw on the rollout's logits, the rollout's logits / values against the masked fp64
    network, and the update's total gradient (A2C + 0.1 x deconv loss through BPTT) against
    the fp64 gradient."""
    from oracle.update_checks import maze_scene, second_update_vs_fp64
    scene, graph, spd, frames = maze_scene((174, 174), aux=True)
    res = second_update_vs_fp64(scene, graph, spd, frames, E=4, T=20, seed=3, env_seed=11, max_steps=25,
                                aux_weight=0.1)
    errs = res["errs"]
    want = {k_ + "." + kind for k_ in NAMES for kind in ("weight", "bias")}
    want |= {"rnn.inner." + name for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}
    want |= {"%s.0.%d.%s" % (name, i, kind) for name in AUX_NAMES for i in (1, 3) for kind in ("weight", "bias")}
    assert set(errs) == want  # every tensor of the trunk, the heads, the LSTM and the aux heads
    bad = {k_: "%.3g" % e for k_, e in errs.items() if e > 1e-4}
    assert not bad, bad
    print("logged-run shape (174x174, LSTM + aux, 4 envs x 20): worst gradient error %.3g" % max(errs.values()))
