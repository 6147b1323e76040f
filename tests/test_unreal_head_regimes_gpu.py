"""The UNREAL heads (vn_pc_forward / vn_pc_backward / vn_rp_forward / vn_rp_backward) against the
float64 restatement (oracle/policy.py) on both sides of every launch switch: the cases and the
rules that place them are oracle/unreal_head_cases.py (checked on the CPU by
tests/test_unreal_head_cases.py). Besides the values every case checks that
  * the padding positions of the raw flat gradient stay exactly 0 (W2 off its two blocks,
    b2[A+1:], BigHouseModel's w1[..., A+1:] and b1[A+1:], rp_b[3]): RMSprop steps the whole flat
    buffer, and to_reference reads the live blocks only;
  * two guard rows past every output / scratch row buffer and 64 floats past the workspace keep
    their bits;
  * (n = 4, 336, R = 288) a second run from the same inputs is bitwise the first.
Both sides of a split-K switch compute the same values, so test_split_products_switch_where_the_
restated_rules_say tells them apart by their bits: the library's switches are where the restated
rules put them.
Tolerances: q and the rp logits / input gradient 1e-5, dh and parameter gradients 1e-4 of each
tensor's scale (tests/test_unreal_gpu.py); pc_action's gradients exactly 0. The oracle runs with
the GPU's ReLU masks (no tie can flip between them)."""
import numpy as np
import pytest
import torch

from oracle import unreal_head_cases as uc
from oracle.few_env_cases import GUARD_BITS
from oracle.policy import (BIGHOUSE_UNREAL_PARAM_ORDER, UNREAL_PARAM_ORDER, bighouse_pixel_control,
                           bighouse_reward_prediction, pixel_control, reward_prediction, seeded_bighouse_state,
                           seeded_bighouse_unreal_state, seeded_reference_state, seeded_unreal_state)

pytestmark = pytest.mark.gpu

_NETS = {}


def _net(arch, hw, A):
    from vnav.policy import PolicyNet
    key = (arch, hw, A)
    if key not in _NETS:
        _NETS[key] = PolicyNet(hw, A, device="cuda:0", arch=arch, unreal=True)
    return _NETS[key]


def _err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(n, *rest):
    """[n + 2, *rest] float32 filled with the guard pattern; the calls see rows 0..n-1."""
    t = torch.empty((n + 2,) + rest, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(GUARD_BITS)
    return t


def _guards_kept(bufs, n, ws, wsf):
    for name, t in bufs.items():
        if t is not None:
            assert bool((_bits(t[n:]) == GUARD_BITS).all()), "%s: guard rows written" % name
    assert bool((_bits(ws[wsf:]) == GUARD_BITS).all()), "workspace: written past its size"


def _workspace(net):
    wsf = net.pc_workspace_floats()
    ws = torch.empty(wsf + 64, dtype=torch.float32, device="cuda")
    ws.view(torch.int32).fill_(GUARD_BITS)
    return ws, wsf


def _param_names(arch):
    return BIGHOUSE_UNREAL_PARAM_ORDER if arch == "bighouse" else UNREAL_PARAM_ORDER


def _params(net, arch, hw, A):
    """A = 4: init_weights with the biases moved off zero (the padding entries stay 0). Other
    action counts: the reference's seeded state through from_reference, which must round-trip."""
    if A == 4:
        params = net.init_params(seed=3)
        u = net.views(params)["unreal"]
        g = torch.Generator(device="cpu").manual_seed(4)
        with torch.no_grad():
            for k in ("pc_b", "b1", "b2", "rp_b"):
                if k in u:
                    u[k].copy_((torch.rand(u[k].shape, generator=g) * 0.1 - 0.05).to(u[k].device))
            (u["b1"] if arch == "bighouse" else u["b2"])[A + 1:] = 0.0
            u["rp_b"][3] = 0.0
        return params
    rng = np.random.default_rng(A)
    if arch == "bighouse":
        sd = {**seeded_bighouse_state(0), **seeded_bighouse_unreal_state(7, num_outputs=A)}
    else:
        sd = {**seeded_reference_state(hw, 0), **seeded_unreal_state(hw, 7, num_outputs=A)}
    sd["policy_logits.0.weight"] = rng.uniform(-0.04, 0.04, size=(A, 512)).astype(np.float32)
    sd["policy_logits.0.bias"] = rng.uniform(-0.05, 0.05, size=(A,)).astype(np.float32)
    params = net.from_reference(sd)
    back = net.to_reference(params)
    for k in _param_names(arch):
        np.testing.assert_array_equal(back[k].numpy(), sd[k], err_msg=k)
    return params


def _padding_is_zero(net, grads):
    u, A = net.views(grads)["unreal"], net.num_actions
    assert not u["rp_b"][3].any(), "rp_b[3]"
    if net.arch == "bighouse":
        assert not u["w1"][..., A + 1:].any(), "w1 padding channels"
        assert not u["b1"][A + 1:].any(), "b1 padding channels"
        return
    off = torch.ones((64, 8), dtype=torch.bool, device=grads.device)
    off[:32, :A] = False
    off[32:, A] = False
    assert not (u["w2"] * off[:, None, None, :]).any(), "W2 off its two blocks"
    assert not torch.isnan(u["w2"]).any()
    assert not u["b2"][A + 1:].any(), "b2 padding channels"


def _pc_run(net, params, h, dq, dh0, acc, form="dq", keep=False):
    """forward + backward on guarded buffers. form "dq": q and dq given; "trainer": q = NULL,
    then dL/dp2 = dq under the value ReLU written into p2 by the caller, dq = NULL. keep: also
    return pc_base's output and what the backward leaves in pcb (dpcb) and a1 (dA1)."""
    n, A, s = h.shape[0], net.num_actions, net.pc_side
    ws, wsf = _workspace(net)
    pcb = _guarded(n, 9, 9, 32)
    a1 = None if net.arch == "bighouse" else _guarded(n, 20, 20, 64)
    p2, q, dh = _guarded(n, s, s, 8), _guarded(n, s, s, A), _guarded(n, 512)
    if acc:
        dh[:n] = dh0
    net.pc_forward(params, h, n, pcb, a1, p2, q if form == "dq" else None, ws)
    live = p2[:n]
    first = (a1[:n, ..., :32] > 0, a1[:n, ..., 32:] > 0) if a1 is not None else None
    masks = {"pc_base": pcb[:n] > 0}
    if a1 is not None:
        masks.update({"pc_value.0": first[0], "pc_action.0": first[1], "pc_value.2": live[..., :A] > 0,
                      "pc_action.2": live[..., A:A + 1] > 0})
    else:
        masks.update({"pc_value": live[..., :A] > 0, "pc_action": live[..., A:A + 1] > 0})
    masks = {k: m.permute(0, 3, 1, 2).cpu() for k, m in masks.items()}
    pcb_fwd = pcb[:n].clone() if keep else None
    q_out = q[:n].clone() if form == "dq" else None
    if form == "trainer":
        assert bool((_bits(q) == GUARD_BITS).all()), "q = NULL: q written"
        dp2 = torch.zeros_like(live)
        dp2[..., :A] = torch.where(live[..., :A] > 0, dq, torch.zeros_like(dq))
        live.copy_(dp2)
    grads = torch.zeros_like(params)
    net.pc_backward(params, h, n, pcb, a1, p2, dq if form == "dq" else None, grads, dh, ws, accumulate=bool(acc))
    torch.cuda.synchronize()
    _guards_kept(dict(pcb=pcb, a1=a1, p2=p2, q=q, dh=dh), n, ws, wsf)
    extra = dict(pcb=pcb_fwd, dpcb=pcb[:n].clone(), da1=a1[:n].clone() if a1 is not None else None) if keep else {}
    return dict(q=q_out, dh=dh[:n].clone(), grads=grads, masks=masks, **extra)


def _pc_check(net, params, h, dq, dh0, acc, got, what):
    """q, dh and every pixel-control parameter gradient vs float64; returns the worst errors."""
    arch, names = net.arch, _param_names(net.arch)
    ref = {k: t.double().requires_grad_() for k, t in net.to_reference(params).items() if k in names}
    h64 = h.cpu().double().requires_grad_()
    fn = bighouse_pixel_control if arch == "bighouse" else pixel_control
    q_ref = fn(ref, h64, got["masks"])
    (q_ref * dq.cpu().double().permute(0, 3, 1, 2)).sum().backward()
    errs = {"q": _err(got["q"].permute(0, 3, 1, 2).cpu().numpy(), q_ref.detach().numpy())}
    dh = got["dh"].cpu().double() - (dh0.cpu().double() if acc else 0.0)
    errs["dh"] = _err(dh.numpy(), h64.grad.numpy())
    g = net.to_reference(got["grads"])
    for name in names:
        if name.startswith("rp"):
            continue
        if name.startswith("pc_action"):
            np.testing.assert_array_equal(g[name].numpy(), 0.0, err_msg=name)
        else:
            errs[name] = _err(g[name].numpy(), ref[name].grad.numpy())
    print("%s: q %.2g dh %.2g worst parameter gradient %.2g" % (
        what, errs["q"], errs["dh"], max(v for k, v in errs.items() if k not in ("q", "dh"))))
    assert errs["q"] <= 1e-5, (what, errs)
    bad = {k: "%.3g" % v for k, v in errs.items() if k != "q" and v > 1e-4}
    assert not bad, (what, bad)
    _padding_is_zero(net, got["grads"])
    return errs


def _pc_inputs(net, n):
    h, dq, dh0 = uc.pc_inputs(n, net.num_actions, net.pc_side)
    return torch.as_tensor(h).cuda(), torch.as_tensor(dq).cuda(), torch.as_tensor(dh0).cuda()


def _same_bits(a, b, what):
    for k in ("q", "dh", "grads"):
        if a[k] is not None and b[k] is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("case", uc.PC_CASES + uc.PC_A_CASES + uc.BH_CASES,
                         ids=[uc.pc_id(c) for c in uc.PC_CASES + uc.PC_A_CASES + uc.BH_CASES])
def test_pixel_control_vs_fp64_oracle(case):
    arch, n, A, acc = case
    hw = (84, 84) if arch == "bighouse" else (174, 174)
    net = _net(arch, hw, A)
    params = _params(net, arch, hw, A)
    h, dq, dh0 = _pc_inputs(net, n)
    got = _pc_run(net, params, h, dq, dh0, acc)
    _pc_check(net, params, h, dq, dh0, acc, got, uc.pc_id(case))
    if arch == "goal" and A == 4 and n in uc.PC_DETERMINISM_N and case in uc.PC_CASES[:len(uc.PC_N)]:
        _same_bits(got, _pc_run(net, params, h, dq, dh0, acc), "second run")  # fixed-order reductions


@pytest.mark.parametrize("lo,hi,product,control", [(192, 193, "fwd", None), (200, 201, "dpcb", "da1"),
                                                   (960, 961, "dh", "dpcb")])
def test_split_products_switch_where_the_restated_rules_say(lo, hi, product, control):
    """Both sides of a split-K switch are correct, so the fp64 comparison cannot tell whether a
    case still sits on the side the table claims. The bits can: a product's rows do not depend
    on the other rows of the batch, but the split form sums its K chunks in another order than the
    unsplit kernel. The same lo rows run alone (split, by the restated rules) and as the first
    rows of hi = lo + 1 (unsplit): the product's input (control) is bitwise the same in both
    runs, its output is not. pc_base's forward reads the test's own h (no control needed)."""
    net = _net("goal", (174, 174), 4)
    params = _params(net, "goal", (174, 174), 4)
    key = product + "_splits"
    r_lo, r_hi = uc.pc_regime("goal", lo), uc.pc_regime("goal", hi)
    assert r_lo[key] > 1 and r_hi[key] == 1
    for up in {"fwd": (), "dpcb": ("fwd",), "dh": ("fwd", "dpcb")}[product]:  # nothing upstream switches here
        assert r_lo[up + "_splits"] == r_hi[up + "_splits"] == 1
    h, dq, dh0 = _pc_inputs(net, hi)
    a = _pc_run(net, params, h[:lo].contiguous(), dq[:lo].contiguous(), dh0[:lo].contiguous(), 0, keep=True)
    b = _pc_run(net, params, h, dq, dh0, 0, keep=True)
    out = {"fwd": "pcb", "dpcb": "dpcb", "dh": "dh"}[product]
    if control is not None:
        assert torch.equal(_bits(a[control]), _bits(b[control][:lo])), "%s: differs between the runs" % control
    assert not torch.equal(_bits(a[out]), _bits(b[out][:lo])), \
        "%s at n = %d and %d: the same bits, so the same kernel form ran on both sides" % (product, lo, hi)
    # and only by rounding: the bars of an activation / a gradient against float64
    assert _err(a[out].cpu().numpy(), b[out][:lo].cpu().numpy()) <= (1e-5 if product == "fwd" else 1e-4)


@pytest.mark.parametrize("n", uc.PC_TRAINER_N)
def test_pixel_control_trainer_calling_form(n):
    """The form A2CTrainer calls: q = NULL forward (the loss kernel forms q from p2), then
    dq = NULL backward over the dL/dp2 the loss wrote into p2 — here dq under the value
    channels' ReLU, zeros from channel A on, which is what pc_dq_kernel writes: the same kernels
    run on the same bits afterwards, so dh and the gradients are bitwise those of the q / dq form."""
    net = _net("goal", (174, 174), 4)
    params = _params(net, "goal", (174, 174), 4)
    h, dq, dh0 = _pc_inputs(net, n)
    a = _pc_run(net, params, h, dq, dh0, 1)
    _pc_check(net, params, h, dq, dh0, 1, a, "trainer form n=%d (q / dq side)" % n)
    b = _pc_run(net, params, h, dq, dh0, 1, form="trainer")
    _same_bits(a, b, "q = NULL / dq = NULL form")
    _padding_is_zero(net, b["grads"])


def _rp_run(net, params, x, dout, with_dx=True):
    R, K = x.shape
    ws, wsf = _workspace(net)
    out = _guarded(R, 4)
    dx = _guarded(R, K) if with_dx else None
    net.rp_forward(params, x, R, out)
    grads = torch.zeros_like(params)
    net.rp_backward(params, x, R, dout, grads, dx, ws)
    torch.cuda.synchronize()
    _guards_kept(dict(out=out, dx=dx), R, ws, wsf)
    return dict(q=out[:R].clone(), dh=dx[:R].clone() if with_dx else None, grads=grads)


@pytest.mark.parametrize("case", uc.RP_CASES, ids=[uc.rp_id(c) for c in uc.RP_CASES])
def test_reward_prediction_vs_fp64_oracle(case):
    arch, hw, R = case
    net = _net(arch, hw, 4)
    params = _params(net, arch, hw, 4)
    K = uc.rp_k(arch, hw)
    assert K == 3 * net.fc_in
    x_np, dout_np = uc.rp_inputs(R, K)
    x, dout = torch.as_tensor(x_np).cuda(), torch.as_tensor(dout_np).cuda()
    got = _rp_run(net, params, x, dout)
    wname, bname = ("rp.weight", "rp.bias") if arch == "bighouse" else ("rp.1.weight", "rp.1.bias")
    ref = {k: t.double().requires_grad_() for k, t in net.to_reference(params).items() if k in (wname, bname)}
    h3, w3 = net.o3
    f64 = torch.as_tensor(x_np).double().view(R, 3, h3, w3, 32).permute(0, 1, 4, 2, 3).contiguous().requires_grad_()
    l_ref = (bighouse_reward_prediction if arch == "bighouse" else reward_prediction)(ref, f64)
    (l_ref * torch.as_tensor(dout_np[:, :3]).double()).sum().backward()  # column 3 is padding: no logit reads it
    g = net.to_reference(got["grads"])
    errs = {"logits": _err(got["q"][:, :3].cpu().numpy(), l_ref.detach().numpy()),
            "dx": _err(got["dh"].cpu().numpy(), f64.grad.permute(0, 1, 3, 4, 2).reshape(R, K).numpy()),
            wname: _err(g[wname].numpy(), ref[wname].grad.numpy()),
            bname: _err(g[bname].numpy(), ref[bname].grad.numpy())}
    print("%s: logits %.2g dx %.2g dW %.2g db %.2g" % (uc.rp_id(case), errs["logits"], errs["dx"], errs[wname],
                                                       errs[bname]))
    assert errs["logits"] <= 1e-5 and errs["dx"] <= 1e-5, errs
    assert errs[wname] <= 1e-4 and errs[bname] <= 1e-4, errs
    _padding_is_zero(net, got["grads"])
    # nothing but rp's own entries of the flat gradient is written
    U = net.unreal_layout
    assert not got["grads"][:U["rp_w"]].any()
    if R == uc.RP_NULL_DX_R:  # dx = NULL: the same parameter gradients, bit for bit
        again = _rp_run(net, params, x, dout, with_dx=False)
        assert torch.equal(_bits(again["grads"]), _bits(got["grads"]))
    if R == uc.RP_DETERMINISM_R:
        _same_bits(got, _rp_run(net, params, x, dout), "second run")


def test_head_entry_points_refuse_bad_arguments():
    """VN_EINVAL with a message, nothing launched: the head entry points on a policy created
    without VN_POLICY_UNREAL, n = 0, and a1 = NULL on BigGoalHouseModel's heads (BigHouseModel's
    take it: one deconv layer)."""
    from vnav import _lib
    from vnav.policy import PolicyNet
    lib = _lib.load()
    plain = PolicyNet((84, 84), 4, device="cuda:0")
    goal = _net("goal", (174, 174), 4)
    buf = torch.empty(4096, device="cuda")
    buf.view(torch.int32).fill_(GUARD_BITS)
    B = _lib.ptr(buf)
    f = __import__("ctypes").c_int64(-7)

    def calls(net, n=5, a1=B):
        h = net._h
        return {"pc_forward": lambda: lib.vn_pc_forward(h, B, B, n, B, a1, B, B, B, None),
                "pc_backward": lambda: lib.vn_pc_backward(h, B, B, n, B, a1, B, B, B, B, 0, B, None),
                "rp_forward": lambda: lib.vn_rp_forward(h, B, B, n, B, None),
                "rp_backward": lambda: lib.vn_rp_backward(h, B, B, n, B, B, B, B, None)}

    tried = [("no UNREAL heads", k, fn) for k, fn in calls(plain).items()]
    tried += [("n = 0", k, fn) for k, fn in calls(goal, n=0).items()]
    tried += [("a1 = NULL", k, fn) for k, fn in calls(goal, a1=None).items() if k.startswith("pc")]
    tried.append(("no UNREAL heads", "pc_workspace_floats",
                  lambda: lib.vn_pc_workspace_floats(plain._h, __import__("ctypes").byref(f))))
    for why, name, fn in tried:
        rc = fn()
        assert rc == -1, "%s, %s: returned %d" % (name, why, rc)  # VN_EINVAL
        assert ("vn_" + name) in _lib.last_error(), (name, why, _lib.last_error())
    torch.cuda.synchronize()
    assert f.value == -7 and bool((buf.view(torch.int32) == GUARD_BITS).all())
