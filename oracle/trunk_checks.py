"""Shared checks of the policy kernels against the fp64 oracle (TEST INFRASTRUCTURE ONLY — see
oracle/__init__.py).

tests/test_prod_oracle_gpu.py (production-size batches) and tests/test_few_env_gpu.py (a few
envs, float frames, other action counts) hold the kernels to the same bars with the same
code: the error measures, the reading of the activation store the forward wrote, the ReLU
masks of the GPU forward (the oracle is run with them, see GoalNetOracle.forward_masked, and
every disagreeing bit is asserted to be a tie), the comparison of the 14 (+ aux) parameter
gradients, the whole forward + backward of the goal trunk on u8 frames (trunk_heads_u8_vs_oracle,
which tests/test_goal_trunk_regimes_gpu.py runs at every launch regime above 16 rows), and the
recurrent core against torch's float64 nn.LSTM (lstm_core_check, which
tests/test_lstm_regimes_gpu.py runs at every launch regime from 18 to 1030 envs on inputs made
on the CPU). The
BigHouse trunk's twins (_bighouse_masks, _bighouse_forward_masked, _ties_only,
_bighouse_grads_vs_oracle) serve tests/test_bighouse_regimes_gpu.py and oracle/update_checks.py.

Tolerances (north star): outputs and activations 1e-5, parameter gradients 1e-4 of each
tensor's scale. Logits and values are also checked element by element: |gpu - fp64| <= 1e-5
|fp64| + a floor of 1e-6 of the tensor's scale (a logit near zero is a sum of cancelling
terms whose fp32 rounding is set by the terms, not by the sum: the floor states that bound).
"""
import ctypes

import numpy as np
import torch

from oracle import a2c as oa2c
from oracle.policy import GoalNetOracle, frames_to_float, trunk_sizes

NAMES = {"shared_base.0.0": "conv1", "shared_base.0.2": "conv2", "conv_base.0.0": "conv3",
         "conv_base.0.2": "conv4", "conv_merge.0.1": "fc", "policy_logits.0": "policy_logits",
         "critic.0": "critic"}
BIGHOUSE_NAMES = {"conv_base.0.0": "conv1", "conv_base.0.2": "conv2", "conv_base.0.4": "conv3",
                  "conv_merge.0.1": "fc", "policy_logits.0": "policy_logits", "critic.0": "critic"}
AUX_NAMES = ("deconv_depth", "deconv_mask", "deconv_mask_goal")
LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


ELEM_RTOL, ELEM_FLOOR = 1e-5, 1e-6


def _elementwise(a, b, rtol=ELEM_RTOL, floor=ELEM_FLOOR):
    """max over elements of |a - b| / (rtol |b| + floor max|b|): <= 1 passes."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / (rtol * np.abs(b) + floor * max(np.abs(b).max(), 1e-30))).max())


def _check_outputs(o_logits, o_value, logits, value):
    """Logits / values: normwise 1e-5 of scale and the elementwise bound above."""
    assert _err(o_logits, logits) <= 1e-5
    assert _err(o_value, value) <= 1e-5
    e = (_elementwise(o_logits, logits), _elementwise(o_value, value))
    assert max(e) <= 1.0, "elementwise logits / values: %.3g / %.3g of the bound" % e
    return e


def _acts_views(net, acts, n):
    """The activation store the forward wrote (csrc/vn_policy.hip acts_at): [conv1 ReLU
    bitmask | X1 | X2 | X3 | X4 | X5], each sample-contiguous NHWC, frames 2i (image) and
    2i + 1 (goal)."""
    o1, o2, o3 = trunk_sizes(*net.frame_hw)
    msz = 2 * o1[0] * o1[1]
    sz = [2 * o1[0] * o1[1] * 32, 2 * o2[0] * o2[1] * 32, o3[0] * o3[1] * 64, o3[0] * o3[1] * 32, 512]
    assert net.act_floats == msz + sum(sz)
    out = {"M1": acts[:n * msz].view(torch.int32).view(n, 2, o1[0], o1[1])}
    p = n * msz
    shapes = [(n, 2, o1[0], o1[1], 32), (n, 2, o2[0], o2[1], 32), (n, o3[0], o3[1], 64), (n, o3[0], o3[1], 32),
              (n, 512)]
    for i, sh in enumerate(shapes):
        out["X%d" % (i + 1)] = acts[p:p + n * sz[i]].view(sh)
        p += n * sz[i]
    return out


def _gpu_masks(net, acts, n, float_frames=False, goal_src=None):
    """0/1 float64 masks (NCHW) of every trunk ReLU from the GPU's activations; checks that
    conv1's channel bitmask (what conv2's input gradient reads) equals X1 > 0. float_frames:
    the forward ran on dense float frames, whose conv1 (the im2col product) writes no bitmask
    (the conv2 input gradient of that path reads X1 itself), so the mask is X1 > 0 alone. Read
    the masks before the backward runs: it overwrites X1. goal_src: int64 [n], the forward ran
    with goal runs (vn_goal_runs): sample i's goal maps are those stored at sample goal_src[i]
    (the start of its run, i + goal_delta[i]), the goal slots of the other samples are not
    written; the goal masks are read there and the bitmask is checked on the image slots and
    on the run starts' goal slots."""
    v = _acts_views(net, acts, n)
    x1 = v["X1"] > 0
    x2g = v["X2"][:, 1] > 0
    if goal_src is not None:
        goal_src = goal_src.to(acts.device)
    if not float_frames:
        bits = ((v["M1"][..., None] >> torch.arange(32, device=acts.device, dtype=torch.int32)) & 1).bool()
        if goal_src is None:
            assert torch.equal(bits, x1), "conv1 ReLU bitmask != X1 > 0"
        else:
            start = goal_src == torch.arange(n, device=acts.device)
            assert bool(start.any()) and bool(start[goal_src].all()) and int(goal_src.min()) >= 0
            assert torch.equal(bits[:, 0], x1[:, 0]), "conv1 ReLU bitmask != X1 > 0 (image frames)"
            assert torch.equal(bits[start, 1], x1[start, 1]), "conv1 ReLU bitmask != X1 > 0 (goal frames of run starts)"
    x1g = x1[:, 1]
    if goal_src is not None:
        x1g, x2g = x1g[goal_src], x2g[goal_src]

    def nchw(t):
        return t.permute(0, 3, 1, 2).double().cpu()
    return {"m1i": nchw(x1[:, 0]), "m1g": nchw(x1g), "m2i": nchw(v["X2"][:, 0] > 0),
            "m2g": nchw(x2g), "m3": nchw(v["X3"] > 0), "m4": nchw(v["X4"] > 0),
            "m5": (v["X5"] > 0).double().cpu()}


def _check_masks_are_signs(masks, pre):
    """A mask bit may differ from the sign of the oracle's pre-activation only at a tie."""
    pairs = {"m1i": "z1i", "m1g": "z1g", "m2i": "z2i", "m2g": "z2g", "m3": "z3", "m4": "z4", "m5": "z5"}
    flips = {}
    for m, z in pairs.items():
        zz = pre[z].detach()
        bad = (masks[m] > 0) != (zz > 0)
        if bad.any():
            worst = float(zz[bad].abs().max() / zz.abs().max())
            assert worst <= 1e-5, "%s: mask disagrees with the oracle's sign at |z| = %.3g of scale" % (m, worst)
        flips[m] = int(bad.sum())
    return flips


BIGHOUSE_PAIRS = {"m1": "z1", "m2": "z2", "m3": "z3", "m5": "z5"}


def _bighouse_acts_views(net, acts, n):
    """BigHouseModel's activation store [X1 | X2 | X3 | X5] (no conv4, no conv1 bitmask), each
    sample-contiguous NHWC, of a store of capacity n."""
    sz = [20 * 20 * 32, 9 * 9 * 64, 7 * 7 * 32, 512]
    assert net.act_floats == sum(sz)
    shapes = [(n, 20, 20, 32), (n, 9, 9, 64), (n, 7, 7, 32), (n, 512)]
    out, p = {}, 0
    for key, s, sh in zip(("X1", "X2", "X3", "X5"), sz, shapes):
        out[key] = acts[p:p + n * s].view(sh)
        p += n * s
    return out


def _bighouse_masks(net, acts, n):
    """ReLU masks of BigHouseModel's trunk from its activation store [X1 | X2 | X3 | X5]. Read
    them before the backward runs: it overwrites X1."""
    out = {}
    for key, x in zip(("m1", "m2", "m3", "m5"), _bighouse_acts_views(net, acts, n).values()):
        x = x > 0
        out[key] = (x.permute(0, 3, 1, 2) if x.dim() == 4 else x).double().cpu()
    return out


def _bighouse_forward_masked(ref, image, masks):
    """BigHouseOracle.features with every ReLU replaced by its given mask -> (x3, f, pre)."""
    pre = {}
    pre["z1"] = z1 = ref.conv1(image)
    pre["z2"] = z2 = ref.conv2(z1 * masks["m1"])
    pre["z3"] = z3 = ref.conv3(z2 * masks["m2"])
    x3 = z3 * masks["m3"]
    pre["z5"] = z5 = ref.fc(x3.flatten(1))
    return x3, z5 * masks["m5"], pre


def _ties_only(masks, pre, pairs):
    """_check_masks_are_signs over the given {mask: pre-activation} pairs -> flips per mask."""
    flips = {}
    for m, z in pairs.items():
        zz = pre[z].detach()
        bad = (masks[m] > 0) != (zz > 0)
        if bad.any():
            worst = float(zz[bad].abs().max() / zz.abs().max())
            assert worst <= 1e-5, "%s: mask disagrees with the oracle's sign at |z| = %.3g of scale" % (m, worst)
        flips[m] = int(bad.sum())
    return flips


def _bighouse_grads_vs_oracle(net, grads, ref, tol=1e-4):
    """The 12 trunk + head gradient tensors by reference name -> {name: error of its scale}."""
    mine = net.to_reference(grads)
    errs = {}
    for k, attr in BIGHOUSE_NAMES.items():
        mod = getattr(ref, attr)
        for kind in ("weight", "bias"):
            errs[k + "." + kind] = _err(mine[k + "." + kind].numpy(), getattr(mod, kind).grad.numpy())
    bad = {k: "%.3g" % e for k, e in errs.items() if not e <= tol}
    assert not bad, bad
    return errs


def _grads_vs_oracle(net, grads, ref, heads=None, tol=1e-4):
    mine = net.to_reference(grads)
    errs = {}
    for k, attr in NAMES.items():
        mod = getattr(ref, attr)
        for kind in ("weight", "bias"):
            errs[k + "." + kind] = _err(mine[k + "." + kind].numpy(), getattr(mod, kind).grad.numpy())
    if heads is not None:
        for h, name in zip(heads.heads, AUX_NAMES):
            for i, layer in ((1, h[0]), (3, h[2])):
                for kind in ("weight", "bias"):
                    key = "%s.0.%d.%s" % (name, i, kind)
                    errs[key] = _err(mine[key].numpy(), getattr(layer, kind).grad.numpy())
    bad = {k: "%.3g" % e for k, e in errs.items() if e > tol}
    assert not bad, bad
    return max(errs.values())


NAN_BITS = 0x7FC5A5A5  # a quiet NaN with a payload (as int32): few_env_cases.GUARD_BITS


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def trunk_heads_u8_vs_oracle(tag, pol, frames, img, gl, n, A, actions, rets, nan_fill=False):
    """Forward + backward of n samples of u8 frames through pol.net (the goal trunk and its heads)
    against GoalNetOracle in float64 under the GPU's own ReLU masks: logits, value, X1..X5 and all
    14 parameter gradients of the A2C loss, at the project's bars (module text); every mask bit that
    disagrees with the oracle's sign is asserted to be a tie. The body of tests/test_few_env_gpu.py
    test_trunk_and_heads_u8_vs_fp64_oracle, shared with tests/test_goal_trunk_regimes_gpu.py.

    frames: the vn_frames handed to the kernels (dense or row-gathered); img, gl: the same frames
    per sample, uint8 [n, H, W, 3] on the CPU; actions int32 [n], rets float32 [n] on the CPU.
    The activation store is prefilled with NaN. nan_fill: so are the workspace and grads, with a
    NaN bit pattern: vn_policy_backward overwrites grads (include/vnav.h) and the workspace is
    scratch it owns, so a block of either that a launch regime leaves unwritten shows as NaN in a
    gradient. Returns the errors by name (outputs, activations, the 14 gradient tensors)."""
    hw = tuple(pol.net.frame_hw)
    net, params = pol.net, pol.params.data
    acts = net.new_acts(n)
    acts.fill_(float("nan"))
    out = torch.zeros((n, 8), device="cuda")
    net.forward(params, frames, n, acts, n, 0, out)
    masks = _gpu_masks(net, acts, n)  # before the backward: it overwrites X1
    v = _acts_views(net, acts, n)
    x1, x2, x3, x4, x5 = (v["X%d" % i].cpu().numpy() for i in range(1, 6))
    dout = a2c_loss_grad(out, actions.cuda(), rets.cuda(), A)
    grads = torch.zeros_like(params)
    ws = torch.empty(net.workspace_floats(n), device="cuda")
    if nan_fill:
        grads.view(torch.int32).fill_(NAN_BITS)
        ws.view(torch.int32).fill_(NAN_BITS)
    net.backward(params, frames, n, acts, n, dout, grads, ws)
    torch.cuda.synchronize()

    ref = GoalNetOracle(hw, 3, A).load_reference(pol.reference_state_dict()).double()
    logits, value, rx4, pre = ref.forward_masked(frames_to_float(img).double(), frames_to_float(gl).double(), masks)
    flips = _check_masks_are_signs(masks, pre)
    o = out.cpu().numpy()
    elem = _check_outputs(o[:, :A], o[:, A], logits.detach().numpy(), value.detach().numpy().ravel())
    e = {"logits": _err(o[:, :A], logits.detach().numpy()), "value": _err(o[:, A], value.detach().numpy().ravel()),
         "X1": max(_err(x1[:, 0], _nhwc(pre["z1i"] * masks["m1i"])), _err(x1[:, 1], _nhwc(pre["z1g"] * masks["m1g"]))),
         "X2": max(_err(x2[:, 0], _nhwc(pre["z2i"] * masks["m2i"])), _err(x2[:, 1], _nhwc(pre["z2g"] * masks["m2g"]))),
         "X3": _err(x3, _nhwc(pre["z3"] * masks["m3"])), "X4": _err(x4, _nhwc(rx4)),
         "X5": _err(x5, (pre["z5"] * masks["m5"]).detach().numpy())}
    print("%s %s n=%d A=%d: %s; elementwise %.3g / %.3g of the bound; tie flips %s"
          % (tag, "%dx%d" % hw, n, A, " ".join("%s %.3g" % kv for kv in e.items()), elem[0], elem[1], flips))
    bad = {k: "%.3g" % x for k, x in e.items() if not x <= 1e-5}
    assert not bad, bad
    loss, _ = oa2c.loss(logits, value.view(-1), actions.long(), rets.double())
    loss.backward()
    g = _grad_errs(net, grads, ref)
    print("%s %s n=%d A=%d: worst gradient error %.3g of scale (%s)"
          % (tag, "%dx%d" % hw, n, A, max(g.values()), max(g, key=g.get)))
    assert len(g) == 14
    bad = {k: "%.3g" % x for k, x in g.items() if not x <= 1e-4}
    assert not bad, bad
    e.update(g)
    return e


def _grad_errs(net, grads, ref):
    """The 14 trunk + head gradient tensors by reference name -> {name: error of its scale}."""
    mine = net.to_reference(grads)
    errs = {}
    for k, attr in NAMES.items():
        mod = getattr(ref, attr)
        for kind in ("weight", "bias"):
            errs[k + "." + kind] = _err(mine[k + "." + kind].numpy(), getattr(mod, kind).grad.numpy())
    return errs


def a2c_loss_grad(out, actions, rets, num_actions=4):
    """dL/d(out) [n][8] of the A2C loss (value 0.5, entropy 0.01) by vn_a2c_loss_grad."""
    from vnav import _lib
    lib = _lib.load()
    n = out.shape[0]
    dout = torch.zeros_like(out)
    stats = torch.zeros(4, dtype=torch.float32, device=out.device)
    _lib.check(lib.vn_a2c_loss_grad(_lib.ptr(out), _lib.ptr(actions), _lib.ptr(rets), n, int(num_actions),
                                    ctypes.c_float(0.5), ctypes.c_float(0.01), _lib.ptr(dout), _lib.ptr(stats),
                                    _lib.stream_ptr(out.device)), "vn_a2c_loss_grad")
    return dout


def roundup4(x):
    return (x + 3) // 4 * 4


def lstm_core_check(E, T=3, A=4, masks=None, null_args=False, dh_extra=0, strict=False, inputs=None, nan_fill=False):
    """The recurrent core of E envs x T steps through vn_lstm_forward_step, vn_policy_heads and
    vn_lstm_backward against torch's float64 nn.LSTM with the restated MaskedRNN convention:
    (h, c) of all steps, the heads on h and the gradients of W_ih, W_hh, both biases and both
    heads at 1e-4, dL/dZ5 (masked by the features' ReLU).

    masks: float [T, E] array of 0/1 (None: drawn, 5 % resets). null_args: NULL wherever
    include/vnav.h allows it (lra and mask at every step, h_prev and c_prev at t = 0); the
    reference takes zeros / ones. dh_extra = S > 0: vn_lstm_backward_ex with a gradient w.r.t. h
    of the first S envs; the reference loss gains sum(h[:, :S] * dh_extra). strict adds the
    checks of tests/test_few_env_gpu.py: the layout numbers of vn_policy_lstm_info, the stored
    xcat rows bitwise against [x5 | lra | 0 | m h_prev] built on the host side, (h, c) of every
    step against that step's own scale. Returns the errors by name.

    inputs: a dict of numpy arrays made on the CPU (oracle/lstm_regime_cases.py inputs(): x5 [T E, 512],
    lra [T, E, A + 1], masks [T, E], h0, c0 [E, 512], actions int32 [T E], rets [T E], dh_extra
    [T, S, 512] or None) in place of the tensors drawn here; masks must then be None. nan_fill: every
    buffer the calls write (xcat, gates, acts, c_all, h_all, out, dz5, the workspace and grads) is
    prefilled with NAN_BITS; after the backward no NaN may remain in dz5 or in the heads' and the LSTM's
    gradients, W_cat's pad columns must be exactly zero, and the trunk's part of grads must still hold
    the fill (include/vnav.h: the call writes the head and LSTM gradients)."""
    from vnav.policy import PolicyNet
    net = PolicyNet((84, 84), A, recurrent=True)
    params = net.init_params(3)
    with torch.no_grad():
        params.add_(torch.randn(params.shape, generator=torch.Generator().manual_seed(2)).cuda() * 0.01)
    N = T * E
    L = net.lstm
    if strict:
        assert L["lin"] == 512 + A + 1 and L["xoff"] == roundup4(512 + A + 1) and L["xcat"] == L["xoff"] + 512, L
    g = torch.Generator(device="cuda").manual_seed(4)
    if inputs is not None:
        assert masks is None and (inputs["dh_extra"] is not None) == bool(dh_extra)

        def given(name, shape, dtype=torch.float32):
            t = torch.as_tensor(np.ascontiguousarray(inputs[name]))
            assert t.dtype == dtype and tuple(t.shape) == shape, (name, t.dtype, tuple(t.shape))
            return t.cuda()
        x5, lra, masks = given("x5", (N, 512)), given("lra", (T, E, A + 1)), given("masks", (T, E))
        h0, c0 = given("h0", (E, 512)), given("c0", (E, 512))
        assert torch.equal(lra, lra * masks[..., None])  # a reset env's last action / reward is zero, as below
    else:
        x5 = torch.relu(torch.randn((N, 512), device="cuda", generator=g))
        lra = torch.zeros((T, E, A + 1), device="cuda")
        lra[..., :A].scatter_(2, torch.randint(0, A, (T, E, 1), device="cuda", generator=g), 1.0)
        lra[..., A] = (torch.rand((T, E), device="cuda", generator=g) < 0.1).float()
        if masks is None:
            masks = (torch.rand((T, E), device="cuda", generator=g) > 0.05).float()
        else:
            masks = torch.as_tensor(np.asarray(masks), dtype=torch.float32).cuda().reshape(T, E).contiguous()
        lra *= masks[..., None]
        h0 = torch.randn((E, 512), device="cuda", generator=g) * 0.5
        c0 = torch.randn((E, 512), device="cuda", generator=g) * 0.5
    if null_args:
        lra.zero_()
        masks.fill_(1.0)
        h0.zero_()
        c0.zero_()
    xcat = torch.zeros((N, L["xcat"]), device="cuda")
    la = torch.zeros((N, 2048), device="cuda")
    c_all = torch.zeros((N, 512), device="cuda")
    h_all = torch.zeros((N, 512), device="cuda")
    gates = torch.zeros((E, 2048), device="cuda")
    out = torch.zeros((N, 8), device="cuda")
    if nan_fill:
        for buf in (xcat, la, c_all, h_all, gates, out):
            buf.view(torch.int32).fill_(NAN_BITS)
    for t in range(T):
        sl = slice(t * E, (t + 1) * E)
        hp = h0 if t == 0 else h_all[(t - 1) * E:t * E]
        cp = c0 if t == 0 else c_all[(t - 1) * E:t * E]
        if null_args:
            net.lstm_step(params, E, x5[sl], None, None, None if t == 0 else hp, None if t == 0 else cp, xcat[sl],
                          gates, la[sl], c_all[sl], h_all[sl])
        else:
            net.lstm_step(params, E, x5[sl], lra[t], masks[t], hp, cp, xcat[sl], gates, la[sl], c_all[sl], h_all[sl])
    net.heads(params, h_all, N, out)
    if strict:  # every term is a copy, a zero or a product with 0 / 1: exact in fp32
        for t in range(T):
            sl = slice(t * E, (t + 1) * E)
            hp = h0 if t == 0 else h_all[(t - 1) * E:t * E]
            want = torch.cat((x5[sl], lra[t], torch.zeros((E, L["xoff"] - L["lin"]), device="cuda"),
                              hp * masks[t][:, None]), 1)
            assert torch.equal(xcat[sl].view(torch.int32), want.view(torch.int32)), "xcat rows of step %d" % t
    if inputs is not None:
        actions, rets = given("actions", (N,), torch.int32), given("rets", (N,))
    else:
        actions = torch.randint(0, A, (N,), dtype=torch.int32, device="cuda", generator=g)
        rets = torch.randn(N, device="cuda", generator=g)
    dout = a2c_loss_grad(out, actions, rets, A)
    grads = torch.zeros_like(params)
    dz5 = torch.zeros((N, 512), device="cuda")
    ws = torch.empty(net.lstm_workspace_floats(T, E), device="cuda")
    if nan_fill:
        for buf in (grads, dz5, ws):
            buf.view(torch.int32).fill_(NAN_BITS)
    dhx = None
    if dh_extra and inputs is not None:
        dhx = given("dh_extra", (T, dh_extra, 512))
    elif dh_extra:
        gx = torch.Generator(device="cuda").manual_seed(6)
        dhx = torch.randn((T, dh_extra, 512), device="cuda", generator=gx) * 0.1
    net.lstm_backward(params, T, E, dout, h_all, xcat, la, c_all, c0, masks, x5, dz5, grads, ws, dh_extra=dhx,
                      extra_envs=dh_extra)
    torch.cuda.synchronize()
    if nan_fill:
        gv = net.views(grads)
        assert not bool(torch.isnan(dz5).any()), "dz5: rows left unwritten"
        wcat_g, bih_g, bhh_g = gv["lstm"]
        for name, t in (("W_cat", wcat_g), ("b_ih", bih_g), ("b_hh", bhh_g), ("head weight", gv["head"][0]),
                        ("head bias", gv["head"][1])):
            assert not bool(torch.isnan(t).any()), "%s gradient: values left unwritten" % name
        pad = wcat_g[:, L["lin"]:L["xoff"]]
        assert not bool(pad.any()), "W_cat gradient: pad columns %d..%d not zero" % (L["lin"], L["xoff"] - 1)
        for name in net.offsets:
            if name == "head":
                continue
            for t in gv[name]:
                assert bool((t.contiguous().view(torch.int32) == NAN_BITS).all()), "%s gradient written by vn_lstm_backward" % name

    sd = net.to_reference(params)
    lstm = torch.nn.LSTM(512 + A + 1, 512, batch_first=True).double()
    for name in LSTM_NAMES:
        getattr(lstm, name).data.copy_(sd["rnn.inner." + name].double())
    pl = torch.nn.Linear(512, A).double()
    cr = torch.nn.Linear(512, 1).double()
    for mod, k in ((pl, "policy_logits.0"), (cr, "critic.0")):
        mod.weight.data.copy_(sd[k + ".weight"].double())
        mod.bias.data.copy_(sd[k + ".bias"].double())
    xf = x5.cpu().double().view(T, E, 512).requires_grad_()
    x = torch.cat((xf, lra.cpu().double()), 2)
    h, c = h0.cpu().double()[None], c0.cpu().double()[None]
    m = masks.cpu().double()
    ys, cs = [], []
    for t in range(T):
        y, (h, c) = lstm(x[t][:, None], (h * m[t][None, :, None], c * m[t][None, :, None]))
        ys.append(y[:, 0])
        cs.append(c[0])
    y = torch.cat(ys)
    errs = {"h": _err(h_all.cpu().numpy(), y.detach().numpy()),
            "c": _err(c_all.cpu().numpy(), torch.cat(cs).detach().numpy())}
    assert errs["h"] <= 1e-5
    assert errs["c"] <= 1e-5
    if strict:
        hh, cc = h_all.cpu().numpy(), c_all.cpu().numpy()
        for t in range(T):
            sl = slice(t * E, (t + 1) * E)
            e = (_err(hh[sl], ys[t].detach().numpy()), _err(cc[sl], cs[t].detach().numpy()))
            assert max(e) <= 1e-5, "step %d: h / c %.3g / %.3g of the step's scale" % ((t,) + e)
            errs["h"], errs["c"] = max(errs["h"], e[0]), max(errs["c"], e[1])
    logits, value = pl(y), cr(y)
    o = out.cpu().numpy()
    _check_outputs(o[:, :A], o[:, A], logits.detach().numpy(), value.detach().numpy().ravel())
    errs["logits"] = _err(o[:, :A], logits.detach().numpy())
    errs["value"] = _err(o[:, A], value.detach().numpy().ravel())
    loss, _ = oa2c.loss(logits, value.view(-1), actions.cpu().long(), rets.cpu().double())
    if dh_extra:
        loss = loss + (y.view(T, E, 512)[:, :dh_extra] * dhx.cpu().double()).sum()
    loss.backward()
    mine = net.to_reference(grads)
    gerrs = {"dz5": _err(dz5.cpu().numpy(), (xf.grad * (xf > 0)).reshape(N, 512).detach().numpy())}
    for name in LSTM_NAMES:
        gerrs[name] = _err(mine["rnn.inner." + name].numpy(), getattr(lstm, name).grad.numpy())
    for mod, k in ((pl, "policy_logits.0"), (cr, "critic.0")):
        gerrs[k + ".weight"] = _err(mine[k + ".weight"].numpy(), mod.weight.grad.numpy())
        gerrs[k + ".bias"] = _err(mine[k + ".bias"].numpy(), mod.bias.grad.numpy())
    bad = {k: "%.3g" % e for k, e in gerrs.items() if not e <= 1e-4}  # a NaN error fails too
    assert not bad, bad
    print("LSTM E=%d T=%d A=%d: worst gradient error %.3g of scale" % (E, T, A, max(gerrs.values())))
    errs.update(gerrs)
    return errs
