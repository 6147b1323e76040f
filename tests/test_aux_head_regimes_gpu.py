"""The aux deconv heads (vn_aux_forward / vn_aux_loss_grad / vn_aux_forward_loss_grad /
vn_aux_backward) against the float64 restatement of oracle/aux_head_cases.py on both sides of every
launch switch in n: the cases and the rules that place them are oracle/aux_head_cases.py (checked
on the CPU by tests/test_aux_head_cases.py, which also shows that these checks see a wrong tail,
seam or partial sum). X4 is written straight into the activation store: the trunk does not run.
Every case checks
  * pred and both forms of dpred element by element at 1e-5 of the tensor's scale, channel 7 of
    dpred exactly 0, stats[0..2] at 1e-5 relative in both forms;
  * dX4 and the gradients of W1, b1, W2, b2 (per head, by reference name) at 1e-4 of each tensor's
    scale; W2's gradient off the three diagonal blocks and b2[7] exactly 0 (RMSprop steps the
    whole flat buffer);
  * the flat gradient outside the heads' block, two guard rows past a1 / pred / dpred / dx4, 64
    floats past the workspace and the activation store outside X4's n rows keep their bits.
The oracle runs with the GPU's ReLU masks (a1 > 0 before the backward consumes a1); a mask bit
that disagrees with the oracle's sign must be a tie. Tolerances: the project's bars
(tests/test_prod_oracle_gpu.py, tests/test_unreal_head_regimes_gpu.py); float32 arithmetic alone
stays under 2e-6 of pred, dpred, stats, dX4 and the weight gradients and 1.5e-5 of db1 on these
inputs ("Aux heads at every launch regime")."""
import numpy as np
import pytest
import torch

from oracle import aux_head_cases as ac
from oracle.few_env_cases import GEO_IDS, GUARD_BITS

pytestmark = pytest.mark.gpu

_NETS, _ORACLE = {}, {}


def _net(hw):
    from vnav.policy import PolicyNet
    if hw not in _NETS:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        # the case tables are computed for at most ac.CUS CUs (a larger part would run the
        # "second pass" cases in one pass) and at least ac.MIN_CUS (65 partials, 64 slabs)
        assert ac.MIN_CUS <= cus <= ac.CUS, "%d CUs: recompute oracle/aux_head_cases.py's tables" % cus
        net = PolicyNet(hw, 4, device="cuda:0", aux=True)
        (ih, iw), a_hw, p_hw = ac.maps(hw)
        assert net.aux_layout["a_hw"] == a_hw and net.aux_layout["p_hw"] == p_hw and net.fc_in == 32 * ih * iw
        params = net.init_params(seed=3)
        _, b1, _, b2 = net.views(params)["aux"]
        g = torch.Generator(device="cpu").manual_seed(4)
        with torch.no_grad():   # the biases off zero, the padding entry left at 0
            b1.copy_((torch.rand(48, generator=g) * 0.1 - 0.05).to(b1.device))
            b2[:7] = (torch.rand(7, generator=g) * 0.1 - 0.05).to(b2.device)
        assert float(b2[7]) == 0.0
        sd = {k: v.cpu().numpy() for k, v in net.to_reference(params).items() if k in ac.PARAM_NAMES}
        assert set(sd) == set(ac.PARAM_NAMES)
        _NETS[hw] = (net, params, sd)
    return _NETS[hw]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(n, *rest):
    """[n + 2, *rest] float32 filled with the guard pattern; the calls see rows 0..n-1."""
    t = torch.empty((n + 2,) + rest, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(GUARD_BITS)
    return t


def _guard_flat(floats):
    t = torch.empty(floats, dtype=torch.float32, device="cuda")
    t.view(torch.int32).fill_(GUARD_BITS)
    return t


def _all_guard(t):
    return bool((_bits(t) == GUARD_BITS).all())


def _aux_block(net, flat):
    """0/1 mask over the flat parameter buffer: the heads' W1, b1, W2, b2."""
    X = net.aux_layout
    inside = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    for off, size in ((X["w1"], 32 * 16 * 48), (X["b1"], 48), (X["w2"], 48 * 16 * 8), (X["b2"], 8)):
        inside[off:off + size] = True
    return inside


class _Setup:
    """A case's device buffers: X4 in a guarded activation store of the given capacity, the target
    table and rows, the guarded workspace."""

    def __init__(self, net, inp, n, capacity):
        from vnav.policy import AuxTargets
        self.net, self.n, self.capacity = net, n, capacity
        self.acts = _guard_flat(capacity * net.act_floats)
        self.x4_rows = torch.as_tensor(inp["x4"]).reshape(n, net.fc_in).cuda()
        net.x4(self.acts, capacity)[:n] = self.x4_rows
        self.acts_before = self.acts.clone()
        self.table = torch.as_tensor(inp["table"]).cuda()
        self.rows_i, self.rows_g = torch.as_tensor(inp["image_rows"]).cuda(), torch.as_tensor(inp["goal_rows"]).cuda()
        self.tg = AuxTargets(self.table.data_ptr(), self.rows_i.data_ptr(), self.rows_g.data_ptr())
        self.wsf = net.aux_workspace_floats()
        self.ws = _guard_flat(self.wsf + 64)

    def kept(self, bufs):
        n = self.n
        for name, t in bufs.items():
            assert _all_guard(t[n:]), "%s: guard rows written" % name
        assert _all_guard(self.ws[self.wsf:]), "workspace: written past its size"
        # the activation store: X4's n rows as written, every other float the guard pattern
        assert torch.equal(_bits(self.acts), _bits(self.acts_before)), "activation store written"


def _run(net, params, inp, n, capacity):
    """forward, loss, fused forward + loss, backward on guarded buffers; everything as numpy."""
    (ih, iw), (ah, aw), (ph, pw) = ac.maps(net.frame_hw)
    s = _Setup(net, inp, n, capacity)
    a1, pred, dpred = _guarded(n, ah, aw, 48), _guarded(n, ph, pw, 8), _guarded(n, ph, pw, 8)
    a1f, predf, dpredf = _guarded(n, ah, aw, 48), _guarded(n, ph, pw, 8), _guarded(n, ph, pw, 8)
    dx4 = _guarded(n, net.fc_in)
    stats, statsf = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    net.aux_forward(params, s.acts, capacity, n, a1, pred, s.ws)
    net.aux_loss_grad(pred, n, s.tg, ac.WEIGHT, dpred, stats)
    net.aux_forward_loss_grad(params, s.acts, capacity, n, a1f, predf, s.tg, ac.WEIGHT, dpredf, statsf, s.ws)
    assert torch.equal(_bits(a1[:n]), _bits(a1f[:n])), "a1 of the fused form differs from aux_forward's"
    masks = [(a1[:n, ..., 16 * h:16 * h + 16] > 0).permute(0, 3, 1, 2).cpu().numpy() for h in range(3)]
    a1_fwd = a1[:n].clone()
    grads = _guard_flat(params.numel())
    net.aux_backward(params, s.acts, capacity, n, a1, dpred, grads, dx4, s.ws)
    torch.cuda.synchronize()
    s.kept(dict(a1=a1, pred=pred, dpred=dpred, a1f=a1f, predf=predf, dpredf=dpredf, dx4=dx4))
    inside = _aux_block(net, grads)
    assert _all_guard(grads[~inside]), "gradients outside the heads' block written"
    assert not torch.isnan(grads[inside]).any(), "an entry of the heads' block not written (or NaN)"
    # padding: W2 off the three diagonal blocks and b2[7] exactly 0
    _, _, w2, b2 = net.views(grads)["aux"]
    off = torch.ones((48, 8), dtype=torch.bool, device="cuda")
    for h, (_, c, o) in enumerate(ac.HEADS):
        off[16 * h:16 * h + 16, o:o + c] = False
    assert not (w2 * off[:, None, None, :]).any(), "W2's gradient off its three blocks"
    assert float(b2[7]) == 0.0, "b2[7]"
    assert float(stats[3]) == 0.0 and float(statsf[3]) == 0.0
    got = {k: v.cpu().numpy() for k, v in net.to_reference(grads).items() if k in ac.PARAM_NAMES}
    got.update(pred=pred[:n].cpu().numpy(), dpred=dpred[:n].cpu().numpy(), dpred_fused=dpredf[:n].cpu().numpy(),
               stats=stats.cpu().numpy(), stats_fused=statsf.cpu().numpy(),
               dx4=dx4[:n].view(n, ih, iw, 32).cpu().numpy(), da1=a1[:n].cpu().numpy(), a1=a1_fwd.cpu().numpy(),
               masks=masks, flat=grads[inside].clone())
    return got


def _oracle(hw, n, sd, inp, masks):
    """The float64 reference under the GPU's masks, computed once per (case, masks)."""
    key = np.packbits(np.concatenate([m.ravel() for m in masks])).tobytes()
    if _ORACLE.get("case") != (hw, n, key):
        ref = ac.reference(sd, inp, masks=masks)
        for m, z in zip(masks, ref["pre"]):   # a mask bit against the oracle's sign: a tie
            bad = m != (z > 0)
            if bad.any():
                worst = float(np.abs(z[bad]).max() / np.abs(z).max())
                assert worst <= 1e-5, "a1's mask disagrees with the oracle's sign at |z| = %.3g of scale" % worst
        _ORACLE.update(case=(hw, n, key), ref=ref)
    return _ORACLE["ref"]


def _check(hw, n, got, ref, what):
    errs = ac.errors(got, ref)
    assert set(errs) == set(ac.TOL)
    worst = {"pred": errs["pred"], "dpred": max(errs["dpred"], errs["dpred_fused"]),
             "stats": max(errs["stats"], errs["stats_fused"]), "dx4": errs["dx4"]}
    for part, tag in ((".0.1.weight", "dW1"), (".0.1.bias", "db1"), (".0.3.weight", "dW2"), (".0.3.bias", "db2")):
        worst[tag] = max(e for k, e in errs.items() if k.endswith(part))
    # what aux_backward leaves in a1 (the header says "consumed"): the masked dA1, not asserted
    print("%s: %s | a1 after the backward vs dA1: %.2g, a1 forward %.2g" % (
        what, " ".join("%s %.2g" % kv for kv in worst.items()), ac.err(got["da1"], ref["da1"]), ac.err(got["a1"], ref["a1"])))
    assert not ac.misses(errs), (what, ac.misses(errs))
    for k in ("dpred", "dpred_fused"):
        assert not got[k][..., 7].any(), "%s: channel 7" % k
    assert not got["pred"][..., 7].any(), "pred: channel 7"
    return worst


def _same_bits(a, b, what):
    for k in ("pred", "dpred", "dpred_fused", "dx4", "da1"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), "%s: %s differs" % (what, k)
    assert torch.equal(_bits(a["flat"]), _bits(b["flat"])), "%s: gradients differ" % what


@pytest.mark.parametrize("case", ac.CASES, ids=[ac.case_id(c) for c in ac.CASES])
def test_aux_heads_vs_fp64_oracle(case):
    hw, n = case
    net, params, sd = _net(hw)
    inp = ac.inputs(hw, n)
    got = _run(net, params, inp, n, n)
    ref = _oracle(hw, n, sd, inp, got["masks"])
    _check(hw, n, got, ref, ac.case_id(case))
    if n in ac.REPEAT_N[hw]:   # fixed-order reductions: a second run is bitwise the first
        _same_bits(got, _run(net, params, inp, n, n), "second run")
        # stats are sums of atomics over workgroups: compared with float64 above, not bitwise


@pytest.mark.parametrize("hw", ac.GEOMETRIES, ids=[GEO_IDS[hw] for hw in ac.GEOMETRIES])
def test_activation_store_with_spare_capacity(hw):
    """act_capacity = n + 3 moves X4 inside the store; the same values, bit for bit, as at
    capacity n, and the float64 bars."""
    n = ac.CAPACITY_N[hw]
    net, params, sd = _net(hw)
    inp = ac.inputs(hw, n)
    got = _run(net, params, inp, n, n + 3)
    _check(hw, n, got, _oracle(hw, n, sd, inp, got["masks"]), "%s capacity n + 3" % ac.case_id((hw, n)))
    _same_bits(got, _run(net, params, inp, n, n), "capacity n + 3 against capacity n")


@pytest.mark.parametrize("hw", ac.GEOMETRIES, ids=[GEO_IDS[hw] for hw in ac.GEOMETRIES])
def test_generic_forms_meet_the_same_bars(hw, monkeypatch):
    """VN_DGRAD_GENERIC / VN_WGRAD_GENERIC / VN_AUX_DX4_GENERIC (read per call): the generic
    products in place of the first layer's parity-class kernel, its packed weight gradient and the
    dX4 kernel."""
    n = ac.GENERIC_N[hw]
    net, params, sd = _net(hw)
    inp = ac.inputs(hw, n)
    for var in ("VN_DGRAD_GENERIC", "VN_WGRAD_GENERIC", "VN_AUX_DX4_GENERIC"):
        monkeypatch.setenv(var, "1")
    got = _run(net, params, inp, n, n)
    _check(hw, n, got, _oracle(hw, n, sd, inp, got["masks"]), "%s generic forms" % ac.case_id((hw, n)))


# ---- the reduce forms, told apart by their bits -------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def one_stage(parts):
    """wgrad_reduce_kernel: the slabs in order, from 0."""
    s = np.zeros_like(parts[0])
    for p in parts:
        s = s + p
    return s


def two_stage(parts, kparts=ac.WG_PARTS):
    """slab_partial_kernel (slabs z = y mod kParts in order) then wgrad_reduce_kernel over them."""
    return one_stage([one_stage(parts[y::kparts]) for y in range(kparts)])


def finish(parts, lanes=ac.FINISH_LANES):
    """aux_backward2_finish_kernel: lane l sums partials l, l + 64, .. in order, then the xor tree
    (offsets 32 .. 1); lane 0 holds the result."""
    zero = np.zeros_like(parts[0])
    t = np.stack([one_stage(parts[lane::lanes]) if lane < len(parts) else zero for lane in range(lanes)])
    idx = np.arange(lanes)
    o = lanes // 2
    while o:
        t = t + t[idx ^ o]
        o //= 2
    return t[0]


def _same(a, b):
    return np.array_equal(_f32(a).view(np.int32), _f32(b).view(np.int32))


def test_reduce_forms_switch_where_the_restated_rules_say():
    """Both sides of a reduce switch are correct, so float64 cannot tell whether a case sits on
    the side the table claims. The bits can. At 174x174 every kernel of the backward takes one
    sample an item, and a call on one sample alone returns that item's partial exactly (one
    partial, one slab: the sums add zeros to it). From the 65 partials the restated sums predict
    the bits of a call on the first 63, 64 and 65 samples (the same a1, dpred and X4 rows):
      * dW1: 63 slabs summed in order; from 64 slabs on, 32 sums of every 32nd slab, then those
        in order (launch_conv_wgrad_x6's two stages) — and neither form gives the other's bits;
      * dW2, db1, db2: lane l of the finish kernel sums partials l, l + 64 in order before the
        xor tree: at 65 partials lane 0 adds partial 64 to partial 0 first, which is not the tree
        over 64 partials plus partial 64, nor the sum in order."""
    hw = ac.BITS_HW
    net, params, _ = _net(hw)
    g = ac.geometry(hw)
    assert (g["wa_img"], g["wa_bands"], g["bwd2_bands"]) == (1, 1, 1)
    N = max(ac.BITS_N)
    regimes = {m: ac.aux_regime(hw, m) for m in ac.BITS_N}
    assert [regimes[m]["dw1"]["reduce"] for m in ac.BITS_N] == ["one-stage", "two-stage", "two-stage"]
    assert [regimes[m]["bwd2"]["per_lane"] for m in ac.BITS_N] == [1, 1, 2]
    assert all(regimes[m][k]["one_pass"] for m in ac.BITS_N for k in ("bwd2", "dw1"))
    inp = ac.inputs(hw, N)
    (ih, iw), (ah, aw), (ph, pw) = ac.maps(hw)
    s = _Setup(net, inp, N, N)
    a1, pred, dpred = _guarded(N, ah, aw, 48), _guarded(N, ph, pw, 8), _guarded(N, ph, pw, 8)
    stats = torch.zeros(4, device="cuda")
    net.aux_forward(params, s.acts, N, N, a1, pred, s.ws)
    net.aux_loss_grad(pred, N, s.tg, ac.WEIGHT, dpred, stats)
    inside = _aux_block(net, params)
    X = net.aux_layout
    w1_size = 32 * 16 * 48

    def backward(rows, store, capacity):
        m = rows.stop - rows.start
        a = a1[rows].clone()
        grads, dx4 = _guard_flat(params.numel()), _guarded(m, net.fc_in)
        net.aux_backward(params, store, capacity, m, a, dpred[rows].contiguous(), grads, dx4, s.ws)
        return grads[inside].cpu().numpy()

    one = _Setup(net, {**inp, "x4": inp["x4"][:1]}, 1, 1)
    parts = []
    for i in range(N):
        one.net.x4(one.acts, 1)[:1] = s.x4_rows[i:i + 1]
        parts.append(backward(slice(i, i + 1), one.acts, 1))
    whole = {m: backward(slice(0, m), s.acts, N) for m in ac.BITS_N}
    torch.cuda.synchronize()
    assert X["w1"] < X["b1"] < X["w2"] < X["b2"]   # the block's order: W1 first
    for m in ac.BITS_N:
        p = parts[:m]
        w1 = [x[:w1_size] for x in p]
        rest = [x[w1_size:] for x in p]
        want_w1 = (one_stage if regimes[m]["dw1"]["reduce"] == "one-stage" else two_stage)(w1)
        other_w1 = (two_stage if regimes[m]["dw1"]["reduce"] == "one-stage" else one_stage)(w1)
        assert not _same(want_w1, other_w1)
        assert _same(whole[m][:w1_size], want_w1), "dW1 at n = %d: not the %s sum of the per-sample slabs" % (
            m, regimes[m]["dw1"]["reduce"])
        assert not _same(whole[m][:w1_size], other_w1)
        assert _same(whole[m][w1_size:], finish(rest)), "dW2 / db1 / db2 at n = %d: not the finish kernel's sum" % m
        assert not _same(whole[m][w1_size:], one_stage(rest))
    rest = [x[w1_size:] for x in parts]
    assert not _same(finish(rest[:65]), finish(rest[:64]) + rest[64])
