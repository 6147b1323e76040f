"""The few-env, float-frame and 1..7-action policy paths against the fp64 oracle.

A rollout step of n <= 16 envs (the reference's own run has 4) runs kernels no training batch
reaches (csrc/vn_skinny.h): conv3 + conv4 in one launch (conv34_small_kernel), conv_merge and
the heads as whole-K VALU columns (skinny_kernel, instantiated for 4 / 8 / 16 rows, K staged
through LDS chunk by chunk), the LSTM step and the BPTT step fused into one launch each. Dense
float frames (the reference wrappers' format) take another conv1 forward, conv1 weight
gradient and conv2 input gradient than u8 frames; an action count other than 4 moves the head
products, the column of h inside xcat and its zero pad. Every one of these is held here to
oracle/policy.py in float64 at the project's bars (oracle/trunk_checks.py): outputs and
activations 1e-5 of the tensor's scale, logits and values also element by element, parameter
gradients 1e-4 of each tensor's scale. The cases and their inputs are oracle/few_env_cases.py
(tests/test_few_env_cases.py checks what they rest on).

ReLU ties as in tests/test_prod_oracle_gpu.py: the oracle runs with the GPU forward's own
masks and every disagreeing bit is asserted to be a tie; no seed is searched.
"""
import numpy as np
import pytest
import torch

from oracle import few_env_cases as fc
from oracle.policy import GoalNetOracle, frames_to_float
from oracle.trunk_checks import (_acts_views, _check_masks_are_signs, _check_outputs, _err, _gpu_masks,
                                 _grads_vs_oracle, lstm_core_check, trunk_heads_u8_vs_oracle)

pytestmark = pytest.mark.gpu


def _noisy_policy(hw, A, seed):
    """init_params + N(0, 0.01) on every parameter (biases included)."""
    from vnav.policy import GoalNavPolicy
    torch.manual_seed(seed)
    pol = GoalNavPolicy(3, A, hw)
    with torch.no_grad():
        pol.params.add_(torch.randn_like(pol.params) * 0.01)
    return pol


@pytest.mark.parametrize("hw,n,A", fc.TRUNK_CASES, ids=fc.TRUNK_IDS)
def test_trunk_and_heads_u8_vs_fp64_oracle(hw, n, A):
    """A: forward + backward of n samples of u8 frames: logits, value, X1 / X2 (the persistent conv1
    and conv2 forwards), X3 / X4 (conv34_small_kernel below 17 samples), X5 (conv_merge:
    skinny_kernel) and all 14 parameter gradients of the A2C loss (oracle/trunk_checks.py
    trunk_heads_u8_vs_oracle). n walks the row instances of launch_skinny on both sides of each
    switch and the switch to the tensor-core path; odd n leaves conv34_small's last workgroup one
    live row; 300x400 runs conv_merge's K = 12512 in several LDS chunks plus a remainder."""
    from vnav.policy import frames_from_batch
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A))
    img, gl = (torch.as_tensor(f) for f in fc.u8_frames(hw, n))
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A))
    img_d, gl_d = img.cuda(), gl.cuda()
    trunk_heads_u8_vs_oracle("few-env A", pol, frames_from_batch(img_d, gl_d), img, gl, n, A, actions, rets)


@pytest.mark.parametrize("hw,n", fc.GUARD_CASES, ids=fc.GUARD_IDS)
def test_forward_keeps_guard_rows(hw, n):
    """B: the forward of n samples into sample slots 1..n of an activation store of n + 2 and
    into rows 1..n of an (n + 2) x 8 output, both prefilled with a NaN bit pattern: slots 0 and
    n + 1 of every section (the conv1 bitmask, X1..X5) and both guard rows of the output keep
    their bits, every value of slots 1..n is finite, and the results equal the same forward at
    offset 0 bit for bit."""
    from vnav.policy import frames_from_batch
    pol = _noisy_policy(hw, 4, fc.weight_seed(hw, n, 4))
    net, params = pol.net, pol.params.data
    img, gl = (torch.as_tensor(f).cuda() for f in fc.u8_frames(hw, n, key=1))
    frames = frames_from_batch(img, gl)

    def run(cap, off):
        acts = net.new_acts(cap)
        acts.view(torch.int32).fill_(fc.GUARD_BITS)
        out = torch.empty((cap, 8), device="cuda")
        out.view(torch.int32).fill_(fc.GUARD_BITS)
        net.forward(params, frames, n, acts, cap, off, out[off:])
        torch.cuda.synchronize()
        return _acts_views(net, acts, cap), out

    base, base_out = run(n, 0)
    v, out = run(n + 2, 1)

    def bits(t):
        return t.contiguous().view(torch.int32)
    for k in ("M1", "X1", "X2", "X3", "X4", "X5"):
        for slot in (0, n + 1):
            assert bool((bits(v[k][slot]) == fc.GUARD_BITS).all()), "%s: guard slot %d written" % (k, slot)
        if k != "M1":
            assert bool(torch.isfinite(v[k][1:n + 1]).all()), "%s: unwritten or non-finite values" % k
            assert bool(torch.isfinite(base[k]).all()), "%s at offset 0: unwritten or non-finite values" % k
        assert torch.equal(bits(v[k][1:n + 1]), bits(base[k])), "%s differs from the forward at offset 0" % k
    for row in (0, n + 1):
        assert bool((bits(out[row]) == fc.GUARD_BITS).all()), "out: guard row %d written" % row
    assert bool(torch.isfinite(out[1:n + 1, :5]).all())
    assert torch.equal(bits(out[1:n + 1, :5]), bits(base_out[:, :5]))


def _linear_loss(logits, value, cot, n, A):
    c = torch.as_tensor(cot, dtype=logits.dtype, device=logits.device)
    return (logits.reshape(n, A) * c[:, :A]).sum() + (value.reshape(n) * c[:, A]).sum()


def _policy_grads(pol, img, gl, cot, n, A):
    pol.params.grad = None
    logits, value, _ = pol(((img[:, None], gl[:, None]), None), None, None)
    _linear_loss(logits, value, cot, n, A).backward()
    torch.cuda.synchronize()
    return logits.detach().reshape(n, A), value.detach().reshape(n), pol.params.grad.clone()


@pytest.mark.parametrize("hw,n", fc.FLOAT_CASES, ids=fc.FLOAT_IDS)
def test_float_frames_vs_fp64_oracle(hw, n):
    """C: dense float frames [n, 3, H, W], uniform in [0, 1) (off the k/255 grid), forward +
    backward through GoalNavPolicy: outputs and all parameter gradients of a linear loss vs the
    fp64 oracle on the same floats. n = 3 takes the few-env rest of the trunk, n = 17 the
    tensor-core one. The masks are those of the same forward run directly (float frames: X1 > 0,
    no bitmask), whose outputs the policy's equal bit for bit."""
    from vnav.policy import frames_from_batch
    A = 4
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A) + 1)
    net, params = pol.net, pol.params.data
    img, gl = (torch.as_tensor(f) for f in fc.float_frames(hw, n))
    img_d, gl_d = img.cuda(), gl.cuda()
    acts = net.new_acts(n)
    out = torch.zeros((n, 8), device="cuda")
    net.forward(params, frames_from_batch(img_d, gl_d), n, acts, n, 0, out)
    masks = _gpu_masks(net, acts, n, float_frames=True)
    cot = fc.out_cotangent(n, A)
    gl_logits, gl_value, grads = _policy_grads(pol, img_d, gl_d, cot, n, A)
    assert torch.equal(gl_logits, out[:, :A]) and torch.equal(gl_value, out[:, A])

    ref = GoalNetOracle(hw, 3, A).load_reference(pol.reference_state_dict()).double()
    logits, value, _, pre = ref.forward_masked(img.double(), gl.double(), masks)
    flips = _check_masks_are_signs(masks, pre)
    o = out.cpu().numpy()
    _check_outputs(o[:, :A], o[:, A], logits.detach().numpy(), value.detach().numpy().ravel())
    _linear_loss(logits, value, cot, n, A).backward()
    worst = _grads_vs_oracle(net, grads, ref)
    print("few-env C %s n=%d float frames: logits %.3g value %.3g, worst gradient error %.3g of scale; tie flips %s"
          % (fc.GEO_IDS[hw], n, _err(o[:, :A], logits.detach().numpy()),
             _err(o[:, A], value.detach().numpy().ravel()), worst, flips))


@pytest.mark.parametrize("hw", fc.GEOMETRIES, ids=[fc.GEO_IDS[hw] for hw in fc.GEOMETRIES])
def test_float_frames_of_u8_match_u8_run(hw):
    """C: float frames that are exactly frames_to_float(u8) against the u8 run of the same
    policy: outputs within 1e-5, every parameter gradient within 1e-5 of its scale (the bar
    test_conv12_small_matches_two_kernels holds two forms of one computation to)."""
    n, A = fc.FLOAT_U8_N, 4
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A) + 2)
    img, gl = (torch.as_tensor(f) for f in fc.u8_frames(hw, n, key=2))
    cot = fc.out_cotangent(n, A)
    ul, uv, ug = _policy_grads(pol, img.cuda(), gl.cuda(), cot, n, A)
    fl, fv, fg = _policy_grads(pol, frames_to_float(img).contiguous().cuda(), frames_to_float(gl).contiguous().cuda(),
                               cot, n, A)
    e = {"logits": _err(fl.cpu().numpy(), ul.cpu().numpy()), "value": _err(fv.cpu().numpy(), uv.cpu().numpy())}
    gu, gf = pol.net.to_reference(ug), pol.net.to_reference(fg)
    for k in gu:
        e[k] = _err(gf[k].numpy(), gu[k].numpy())
    print("few-env C %s float(u8) vs u8: worst %.3g" % (fc.GEO_IDS[hw], max(e.values())))
    bad = {k: "%.3g" % x for k, x in e.items() if not x <= 1e-5}
    assert not bad, bad


@pytest.mark.parametrize("E,T,A,null_args,extra", fc.LSTM_CASES, ids=fc.LSTM_IDS)
def test_recurrent_core_few_envs_vs_fp64_torch_lstm(E, T, A, null_args, extra):
    """D: vn_lstm_forward_step, vn_policy_heads and vn_lstm_backward(_ex) of E envs x T steps
    with placed resets: (h, c) of every step, the stored xcat rows bitwise, the heads on h and
    the gradients of W_ih, W_hh, both biases, both heads and dz5 (oracle/trunk_checks.py
    lstm_core_check, the body of test_lstm_core_vs_fp64_torch_lstm)."""
    e = lstm_core_check(E, T, A, masks=fc.lstm_masks(E, T), null_args=null_args, dh_extra=extra, strict=True)
    print("few-env D %s: %s" % (fc.LSTM_IDS[fc.LSTM_CASES.index((E, T, A, null_args, extra))],
                               " ".join("%s %.3g" % kv for kv in e.items())))
