"""The BigHouse trunk (forward_bignet / backward_bignet of csrc/vn_policy.hip) against the fp64
oracle at every launch regime.

The launch helpers choose other kernels as the row count n grows: conv_merge's forward splits
K = 1568 into 17, 13, 10, 7, 6 or 5 slabs (two of the chunk lengths leave a 32-long last slab)
and runs unsplit with a 64-wide K tile from n = 961, its epilogue takes 4 lanes per output below
n = 128; every weight gradient goes from the direct EpiWgrad epilogue to slabs and a reduce
whose lanes per output grow from 1 to 64; conv1 (400 n rows), conv2 (81 n) and conv3 (49 n) end
in ragged tiles at every n but 128. Nothing else launches the k8 s4 im2col over one frame (u8,
float and row-gather forms), the stride-1 single-class input gradient with its 3x3 border taps,
or the 64 -> 32 channel parity-class input gradient. oracle/bighouse_cases.py holds the regimes
and the cases, tests/test_bighouse_cases.py checks on the CPU that the cases stand on each side
of every switch and that the seeded inputs expose a dropped last slab, a lost border tap and a
reduce that stops short.

A raw PolicyNet(arch="bighouse", recurrent=False) runs net.forward / net.backward, so that the
heads block of backward_bignet runs (the recurrent update hands it dz5). The oracle is
BigHouseOracle in float64 run with the GPU forward's own ReLU masks, read from the activation
store before the backward overwrites X1; every mask bit that disagrees with the sign of the
oracle's pre-activation is asserted to be a tie (|z| <= 1e-5 of the layer's scale). Bars
(oracle/trunk_checks.py): activations and outputs 1e-5 of scale, logits and values also element
by element, each of the 12 gradient tensors 1e-4 of its scale.
"""
import numpy as np
import pytest
import torch

from oracle import a2c as oa2c
from oracle import bighouse_cases as bc
from oracle import few_env_cases as fc
from oracle.policy import BigHouseOracle, frames_to_float
from oracle.trunk_checks import (BIGHOUSE_NAMES, BIGHOUSE_PAIRS, _bighouse_acts_views, _bighouse_forward_masked,
                                 _bighouse_grads_vs_oracle, _bighouse_masks, _check_outputs, _err, _ties_only,
                                 a2c_loss_grad)

pytestmark = pytest.mark.gpu

FRAME_BYTES = 84 * 84 * 3


def _net_params(n, A, key=0):
    """PolicyNet + a case's parameters: init_params(seed) + N(0, 0.01) on every parameter, built by
    oracle/bighouse_cases.py on the host side (its init_state is asserted to be init_params)."""
    from vnav.policy import PolicyNet
    net = PolicyNet((84, 84), A, recurrent=False, arch="bighouse")
    seed = bc.weight_seed(n, A, key)
    assert torch.equal(net.init_params(seed), net.from_reference(bc.init_state(seed, A))), "init_state != init_params"
    return net, net.from_reference(bc.seeded_state(n, A, key))


def _dense(img):
    """vn_frames of dense frames (raw pointers: the caller keeps img alive); BigHouseModel reads the
    image slot only, the goal slot must be set."""
    from vnav.policy import frames_from_batch
    return frames_from_batch(img, img)


def _forward(net, params, frames, n):
    acts = net.new_acts(n)
    acts.fill_(float("nan"))
    out = torch.zeros((n, 8), device="cuda")
    net.forward(params, frames, n, acts, n, 0, out)
    return acts, out


def _backward(net, params, frames, n, acts, dout):
    grads = torch.zeros_like(params)
    ws = torch.empty(net.workspace_floats(n), device="cuda")
    net.backward(params, frames, n, acts, n, dout, grads, ws)
    return grads


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def _vs_oracle(tag, net, params, frames, image64, n, A):
    """Forward + backward of the A2C loss on the GPU and in float64 with the GPU's masks; asserts
    the bars and returns the errors by name."""
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A))
    acts, out = _forward(net, params, frames, n)
    masks = _bighouse_masks(net, acts, n)  # before the backward: it overwrites X1
    v = {k: x.cpu().numpy() for k, x in _bighouse_acts_views(net, acts, n).items()}
    dout = a2c_loss_grad(out, actions.cuda(), rets.cuda(), A)
    grads = _backward(net, params, frames, n, acts, dout)
    torch.cuda.synchronize()

    ref = BigHouseOracle(A).load_reference(net.to_reference(params)).double()
    x3, f, pre = _bighouse_forward_masked(ref, image64, masks)
    flips = _ties_only(masks, pre, BIGHOUSE_PAIRS)
    logits, value = ref.policy_logits(f), ref.critic(f).view(-1)
    o = out.cpu().numpy()
    e = {"logits": _err(o[:, :A], logits.detach().numpy()), "value": _err(o[:, A], value.detach().numpy()),
         "X1": _err(v["X1"], _nhwc(pre["z1"] * masks["m1"])), "X2": _err(v["X2"], _nhwc(pre["z2"] * masks["m2"])),
         "X3": _err(v["X3"], _nhwc(x3)), "X5": _err(v["X5"], f.detach().numpy())}
    print("bighouse %s n=%d A=%d: %s; tie flips %s" % (tag, n, A, " ".join("%s %.3g" % kv for kv in e.items()), flips))
    elem = _check_outputs(o[:, :A], o[:, A], logits.detach().numpy(), value.detach().numpy())
    bad = {k: "%.3g" % x for k, x in e.items() if not x <= 1e-5}
    assert not bad, bad
    loss, _ = oa2c.loss(logits, value, actions.long(), rets.double())
    loss.backward()
    g = _bighouse_grads_vs_oracle(net, grads, ref)
    assert len(g) == 12
    print("bighouse %s n=%d A=%d: elementwise %.3g / %.3g of the bound; gradients %s"
          % (tag, n, A, elem[0], elem[1], " ".join("%s %.3g" % (k.replace(".weight", ".w").replace(".bias", ".b"), x)
                                                   for k, x in g.items())))
    e.update(g)
    return e


@pytest.mark.parametrize("n", bc.CASE_N)
def test_trunk_heads_backward_u8_vs_fp64_oracle(n):
    """u8 frames, A = 4, every n of the case list: logits, value, X1..X3, X5 and the 12 gradient
    tensors of the A2C loss through the heads block of backward_bignet."""
    A = 4
    net, params = _net_params(n, A)
    u8 = torch.as_tensor(bc.u8_frames(n))
    img = u8.cuda()
    _vs_oracle("u8", net, params, _dense(img), frames_to_float(u8).double(), n, A)


@pytest.mark.parametrize("n,A", bc.ACTION_CASES, ids=["n%d-A%d" % c for c in bc.ACTION_CASES])
def test_other_action_counts_vs_fp64_oracle(n, A):
    """A = 1, 3, 7: N = A + 1 against the heads' 16-wide tile, M = A + 1 of their weight gradient,
    K = A + 1 of dz5 = dout x W."""
    net, params = _net_params(n, A)
    u8 = torch.as_tensor(bc.u8_frames(n))
    img = u8.cuda()
    _vs_oracle("actions", net, params, _dense(img), frames_to_float(u8).double(), n, A)


@pytest.mark.parametrize("n", bc.ROWS_N)
def test_frames_gathered_by_row_vs_fp64_oracle(n):
    """Frames read from an arena by row index (the trainer's zero-copy form): rows repeat, the last
    arena row is used. Against the oracle on the gathered frames, not against the dense run."""
    from vnav.policy import frames_from_rows
    A = 4
    net, params = _net_params(n, A, key=1)
    arena, rows = bc.arena_rows(n)
    arena_d, rows_d = torch.as_tensor(arena).cuda(), torch.as_tensor(rows).cuda()
    frames = frames_from_rows(arena_d.data_ptr(), FRAME_BYTES, rows_d, rows_d)
    image64 = frames_to_float(torch.as_tensor(arena[rows])).double()
    _vs_oracle("rows", net, params, frames, image64, n, A)


@pytest.mark.parametrize("n", bc.FLOAT_N)
def test_float_frames_off_the_u8_grid_vs_fp64_oracle(n):
    """Dense float frames [n, 3, 84, 84] uniform in [0, 1): a float path that quantised its input to
    k/255 misses the oracle on the same floats by ~1e-3."""
    A = 4
    net, params = _net_params(n, A, key=2)
    img = torch.as_tensor(bc.float_frames(n))
    img_d = img.cuda()
    _vs_oracle("float", net, params, _dense(img_d), img.double(), n, A)


def test_float_frames_of_u8_match_u8_run():
    """Float frames that are exactly frames_to_float(u8) against the u8 run: outputs and every
    gradient within 1e-5 of scale (the bar tests/test_few_env_gpu.py holds the two forms to)."""
    n, A = bc.FLOAT_U8_N, 4
    net, params = _net_params(n, A, key=3)
    u8 = torch.as_tensor(bc.u8_frames(n, key=3))
    dout = torch.zeros((n, 8), device="cuda")
    dout[:, :A + 1] = torch.as_tensor(fc.out_cotangent(n, A)).cuda()
    res = []
    for img in (u8.cuda(), frames_to_float(u8).contiguous().cuda()):
        frames = _dense(img)
        acts, out = _forward(net, params, frames, n)
        grads = _backward(net, params, frames, n, acts, dout)
        torch.cuda.synchronize()
        res.append((out.cpu().numpy(), net.to_reference(grads)))
    (uo, ug), (fo, fg) = res
    e = {"out": _err(fo[:, :A + 1], uo[:, :A + 1])}
    for k in ug:
        e[k] = _err(fg[k].numpy(), ug[k].numpy())
    print("bighouse float(u8) vs u8 n=%d: worst %.3g" % (n, max(e.values())))
    bad = {k: "%.3g" % x for k, x in e.items() if not x <= 1e-5}
    assert not bad, bad


@pytest.mark.parametrize("n", bc.GUARD_N)
def test_forward_keeps_guard_rows(n):
    """The forward of n samples into slots 1..n of a store of capacity n + 2 and rows 1..n of an
    (n + 2) x 8 output, all prefilled with a NaN bit pattern: slots 0 and n + 1 of every region
    (X1, X2, X3, X5) and both guard rows of the output keep their bits, and slots 1..n equal the
    forward at offset 0 bit for bit."""
    A = 4
    net, params = _net_params(n, A, key=4)
    img = torch.as_tensor(bc.u8_frames(n, key=4)).cuda()
    frames = _dense(img)

    def run(cap, off):
        acts = net.new_acts(cap)
        acts.view(torch.int32).fill_(fc.GUARD_BITS)
        out = torch.empty((cap, 8), device="cuda")
        out.view(torch.int32).fill_(fc.GUARD_BITS)
        net.forward(params, frames, n, acts, cap, off, out[off:])
        torch.cuda.synchronize()
        return _bighouse_acts_views(net, acts, cap), out

    def bits(t):
        return t.contiguous().view(torch.int32)
    base, base_out = run(n, 0)
    v, out = run(n + 2, 1)
    for k in ("X1", "X2", "X3", "X5"):
        for slot in (0, n + 1):
            assert bool((bits(v[k][slot]) == fc.GUARD_BITS).all()), "%s: guard slot %d written" % (k, slot)
        assert bool(torch.isfinite(base[k]).all()), "%s at offset 0: unwritten or non-finite values" % k
        assert torch.equal(bits(v[k][1:n + 1]), bits(base[k])), "%s differs from the forward at offset 0" % k
    for row in (0, n + 1):
        assert bool((bits(out[row]) == fc.GUARD_BITS).all()), "out: guard row %d written" % row
    assert bool(torch.isfinite(base_out[:, :A + 1]).all())
    assert torch.equal(bits(out[1:n + 1, :A + 1]), bits(base_out[:, :A + 1]))


@pytest.mark.parametrize("n", bc.COTANGENT_N)
def test_dz5_in_and_dx3_extra_vs_fp64_oracle(n):
    """backward_ex with dout = None: the caller's dL/dZ5 (as vn_lstm_backward hands it: masked by
    the features' ReLU, so the drawn cotangent is multiplied by the GPU's mask) and a gradient to
    add at conv_base's output (reward prediction's dX3: EpiMaskAdd on the ragged N = 1568 product).
    The 8 trunk tensors against the oracle's gradient of <dz5, z5 m5> + <dx3, x3>; the head tensors
    of grads stay exactly zero."""
    A = 4
    net, params = _net_params(n, A, key=5)
    u8 = torch.as_tensor(bc.u8_frames(n, key=5))
    img = u8.cuda()
    frames = _dense(img)
    acts, _ = _forward(net, params, frames, n)
    masks = _bighouse_masks(net, acts, n)
    c5, c3 = (torch.as_tensor(c) for c in bc.trunk_cotangents(n))
    dz5 = (c5.cuda() * (_bighouse_acts_views(net, acts, n)["X5"] > 0)).contiguous()
    dx3 = c3.cuda().reshape(n, bc.FCIN).contiguous()
    grads = torch.zeros_like(params)
    ws = torch.empty(net.workspace_floats(n), device="cuda")
    net.backward_ex(params, frames, n, acts, n, None, dz5, dx3, grads, ws)
    torch.cuda.synchronize()

    ref = BigHouseOracle(A).load_reference(net.to_reference(params)).double()
    x3, f, pre = _bighouse_forward_masked(ref, frames_to_float(u8).double(), masks)
    flips = _ties_only(masks, pre, BIGHOUSE_PAIRS)
    assert torch.equal(dz5.cpu().double(), c5.double() * masks["m5"])
    loss = (c5.double() * f).sum() + (c3.double().permute(0, 3, 1, 2) * x3).sum()
    loss.backward()
    mine = net.to_reference(grads)
    e = {}
    for k, attr in BIGHOUSE_NAMES.items():
        for kind in ("weight", "bias"):
            name = k + "." + kind
            if attr in ("policy_logits", "critic"):
                assert getattr(getattr(ref, attr), kind).grad is None
                assert not mine[name].any(), "%s: written without dout" % name
            else:
                e[name] = _err(mine[name].numpy(), getattr(getattr(ref, attr), kind).grad.numpy())
    print("bighouse dz5_in + dx3_extra n=%d: %s; tie flips %s" % (n, " ".join("%s %.3g" % kv for kv in e.items()), flips))
    assert len(e) == 8
    bad = {k: "%.3g" % x for k, x in e.items() if not x <= 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("n", bc.DETERMINISM_N)
def test_backward_is_deterministic(n):
    """Two runs of forward + backward from the same inputs give bitwise-equal outputs and
    gradients (what the trainer's graph-replay tests assume)."""
    A = 4
    net, params = _net_params(n, A, key=6)
    img = torch.as_tensor(bc.u8_frames(n, key=6)).cuda()
    frames = _dense(img)
    actions, rets = (torch.as_tensor(v).cuda() for v in fc.loss_inputs(n, A))
    runs = []
    for _ in range(2):
        acts, out = _forward(net, params, frames, n)
        grads = _backward(net, params, frames, n, acts, a2c_loss_grad(out, actions, rets, A))
        torch.cuda.synchronize()
        runs.append((out.view(torch.int32).clone(), grads.view(torch.int32).clone()))
    assert bool(torch.isfinite(runs[0][1].view(torch.float32)).all()) and bool(runs[0][1].any())
    assert torch.equal(runs[0][0], runs[1][0]), "outputs differ between two runs"
    assert torch.equal(runs[0][1], runs[1][1]), "gradients differ between two runs"
