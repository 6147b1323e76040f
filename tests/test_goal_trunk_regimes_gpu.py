"""The goal trunk (forward_impl / backward_impl of csrc/vn_policy.hip, the default network) against
the fp64 oracle at every launch regime above 16 rows.

tests/test_few_env_gpu.py holds it to float64 up to 17 rows, tests/test_prod_oracle_gpu.py at 4096
(84x84) and 512 rows (174x174, 300x400). In between the launch helpers walk conv3's forward through
16, 11, 8, 7, 6, 5 and 4 K slabs to the unsplit kernel, conv_merge's forward and its input gradient
through their own slab counts, the unsplit 64 x 64 and the 128 x 128 tiles (N = FCIN ends in half a
column tile at every geometry), the heads', conv_merge's and conv4's weight gradients from the
direct epilogue to slabs and a reduce of 1..16 lanes, the x6 weight gradients from a one-stage slab
reduce over fewer than kParts slabs to the two-stage one, and the persistent kernels from one item
per workgroup to grids that wrap for certain. oracle/goal_trunk_cases.py holds the regimes, the
switches and a smallest case list with a case on each side of every switch (its "Not covered"
paragraph says what is left out); tests/test_goal_trunk_cases.py checks the list on the CPU and shows
that the seeded inputs expose a dropped K slab, a dropped ragged column tile, a dropped image of a
part-filled item and a reduce that stops short.

Every case runs oracle/trunk_checks.py trunk_heads_u8_vs_oracle (the body tests/test_few_env_gpu.py
runs below 18 rows): logits, value, X1..X5 and the 14 gradient tensors of the A2C loss against
GoalNetOracle in float64 under the GPU's own ReLU masks, every disagreeing mask bit asserted to be a
tie. Bars: activations and outputs 1e-5 of scale, logits and values also element by element, each
gradient tensor 1e-4 of its scale. The activation store is prefilled with NaN, and so are the
workspace and grads (a NaN bit pattern): vn_policy_backward overwrites grads (include/vnav.h) and
owns the workspace as scratch, nothing of either accumulates across calls.
"""
import pytest
import torch

from oracle import few_env_cases as fc
from oracle import goal_trunk_cases as gc
from oracle.trunk_checks import NAN_BITS, _acts_views, a2c_loss_grad, trunk_heads_u8_vs_oracle

pytestmark = pytest.mark.gpu


def _noisy_policy(hw, A, seed):
    """init_params + N(0, 0.01) on every parameter (biases included), as tests/test_few_env_gpu.py."""
    from vnav.policy import GoalNavPolicy
    torch.manual_seed(seed)
    pol = GoalNavPolicy(3, A, hw)
    with torch.no_grad():
        pol.params.add_(torch.randn_like(pol.params) * 0.01)
    return pol


def _assert_wrap_bounds(hw, n):
    """What the table says of the persistent grids at NOMINAL_CUS holds on this device: no wrap where
    every grid fits the CU count, a wrap whatever the occupancy where the items exceed CUs x 2048 /
    threads, and enough resident workgroups for the two-stage reduce to start at 64 items."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for p, r in gc.trunk_regime(hw, n).items():
        if p not in gc.PERSISTENT:
            continue
        G = 2 if p == "conv3_wgrad" else 1
        if not r["may_wrap"]:
            assert r["items"] <= cus // G, "%s: %d items may wrap on %d CUs" % (p, r["items"], cus)
        if r["must_wrap"]:
            assert r["items"] > cus * (2048 // r["threads"]) // G, "%s: %d items need not wrap on %d CUs" % (p, r["items"], cus)
        if "two_stage" in r:
            assert cus // G >= 2 * gc.KPARTS  # one workgroup of 512 threads per CU at the least


def _dense_case(tag, hw, n, A):
    from vnav.policy import frames_from_batch
    _assert_wrap_bounds(hw, n)
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A))
    img, gl = (torch.as_tensor(f) for f in fc.u8_frames(hw, n))
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A))
    img_d, gl_d = img.cuda(), gl.cuda()
    return trunk_heads_u8_vs_oracle(tag, pol, frames_from_batch(img_d, gl_d), img, gl, n, A, actions, rets, nan_fill=True)


@pytest.mark.parametrize("hw,n", gc.TRUNK_CASES, ids=gc.TRUNK_IDS)
def test_regime_cases_u8_vs_fp64_oracle(hw, n):
    """Every case of the three lists, u8 frames, A = 4."""
    _dense_case("goal-trunk", hw, n, 4)


@pytest.mark.parametrize("hw,n", gc.EDGE_CASES, ids=gc.EDGE_IDS)
def test_two_stage_reduce_edges_u8_vs_fp64_oracle(hw, n):
    """The first n of each two-stage slab reduce (exactly 64 slabs, 2 per part) and the n before it
    (the one-stage reduce at its most slabs); 189 | 190 at 84x84 is also conv3's packing tail at
    its edge (63 full items of 3 images, then 63 and one image)."""
    _dense_case("goal-trunk edge", hw, n, 4)


@pytest.mark.parametrize("hw,n,A", gc.ACTION_CASES, ids=gc.ACTION_IDS)
def test_other_action_counts_vs_fp64_oracle(hw, n, A):
    """A = 1, 3, 7 below 65 rows and at n = 257, the heads' weight gradient on 2 slabs: N = A + 1
    against the heads' 16-wide tile, M = A + 1 of their weight gradient, K = A + 1 of dz5 = dout x W."""
    _dense_case("goal-trunk actions", hw, n, A)


@pytest.mark.parametrize("hw,n", gc.ROWS_CASES, ids=gc.ROWS_IDS)
def test_frames_gathered_by_row_vs_fp64_oracle(hw, n):
    """Frames read from an arena by row index (the form the trainer's update uses): rows repeat within
    and between the image and goal lists, the last arena row is used. Against the oracle on the
    gathered frames."""
    from vnav.policy import frames_from_rows
    A = 4
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A) + 1)
    arena, ri, rg = gc.arena_rows(hw, n)
    arena_d, ri_d, rg_d = torch.as_tensor(arena).cuda(), torch.as_tensor(ri).cuda(), torch.as_tensor(rg).cuda()
    frames = frames_from_rows(arena_d.data_ptr(), hw[0] * hw[1] * 3, ri_d, rg_d)
    actions, rets = (torch.as_tensor(v) for v in fc.loss_inputs(n, A, key=1))
    trunk_heads_u8_vs_oracle("goal-trunk rows", pol, frames, torch.as_tensor(arena[ri]), torch.as_tensor(arena[rg]), n, A,
                             actions, rets, nan_fill=True)


@pytest.mark.parametrize("hw,n", gc.GUARD_CASES, ids=gc.GUARD_IDS)
def test_forward_and_backward_keep_guard_slots(hw, n):
    """An activation store of capacity n + 2 prefilled with a NaN bit pattern. Forward at offset 1:
    slots 0 and n + 1 of every section (the conv1 bitmask, X1..X5) and both guard rows of the
    output keep their bits, and slots 1..n equal the forward at offset 0 of a store of n bit for bit.
    vn_policy_backward takes no offset (include/vnav.h: "the n samples stored from offset 0"), so the
    backward's guards are the two trailing slots: forward at offset 0 of the store of n + 2, then the
    backward, which writes dZ1 over X1 — slots n and n + 1 of every section keep their bits after
    both, and the gradients equal those of the capacity-n run bit for bit."""
    from vnav.policy import frames_from_batch
    A = 4
    pol = _noisy_policy(hw, A, fc.weight_seed(hw, n, A) + 2)
    net, params = pol.net, pol.params.data
    img, gl = (torch.as_tensor(f).cuda() for f in fc.u8_frames(hw, n, key=1))
    frames = frames_from_batch(img, gl)
    actions, rets = (torch.as_tensor(v).cuda() for v in fc.loss_inputs(n, A))
    keys = ("M1", "X1", "X2", "X3", "X4", "X5")

    def bits(t):
        return t.contiguous().view(torch.int32)

    def run(cap, off, backward):
        acts = net.new_acts(cap)
        acts.view(torch.int32).fill_(gc.GUARD_BITS)
        out = torch.empty((cap, 8), device="cuda")
        out.view(torch.int32).fill_(gc.GUARD_BITS)
        net.forward(params, frames, n, acts, cap, off, out[off:])
        torch.cuda.synchronize()
        fwd = {k: bits(x).clone() for k, x in _acts_views(net, acts, cap).items()}
        grads = None
        if backward:
            dout = a2c_loss_grad(out[off:off + n].contiguous(), actions, rets, A)
            grads = torch.empty_like(params)
            grads.view(torch.int32).fill_(NAN_BITS)
            ws = torch.empty(net.workspace_floats(n), device="cuda")
            ws.view(torch.int32).fill_(NAN_BITS)
            net.backward(params, frames, n, acts, cap, dout, grads, ws)
            torch.cuda.synchronize()
        return fwd, {k: bits(x) for k, x in _acts_views(net, acts, cap).items()}, bits(out), grads

    base, _, base_out, base_grads = run(n, 0, True)
    assert all(bool(torch.isfinite(g).all()) for g in net.to_reference(base_grads).values())
    for k in keys[1:]:
        assert bool(torch.isfinite(base[k].view(torch.float32)).all()), "%s at offset 0: unwritten or non-finite values" % k

    fwd, _, out, _ = run(n + 2, 1, False)
    for k in keys:
        for slot in (0, n + 1):
            assert bool((fwd[k][slot] == gc.GUARD_BITS).all()), "%s: guard slot %d written by the forward at offset 1" % (k, slot)
        assert torch.equal(fwd[k][1:n + 1], base[k]), "%s differs from the forward at offset 0" % k
    for row in (0, n + 1):
        assert bool((out[row] == gc.GUARD_BITS).all()), "out: guard row %d written" % row
    assert torch.equal(out[1:n + 1, :A + 1], base_out[:, :A + 1])

    fwd, bwd, out, grads = run(n + 2, 0, True)
    for k in keys:
        assert torch.equal(fwd[k][:n], base[k]), "%s differs at capacity n + 2" % k
        for slot in (n, n + 1):
            assert bool((fwd[k][slot] == gc.GUARD_BITS).all()), "%s: guard slot %d written by the forward" % (k, slot)
            assert bool((bwd[k][slot] == gc.GUARD_BITS).all()), "%s: guard slot %d written by the backward" % (k, slot)
    assert torch.equal(out[:n, :A + 1], base_out[:, :A + 1])
    assert torch.equal(bits(grads), bits(base_grads)), "gradients differ between capacity n and n + 2"
