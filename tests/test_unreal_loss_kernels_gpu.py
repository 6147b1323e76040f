"""The UNREAL loss kernels (csrc/vn_unreal_loss.hip) through the C ABI against the fp64 oracle
(oracle/unreal.py) at the chunk, stride and block edges, on the inputs of
oracle/unreal_cases.py (tests/test_unreal_loss_refs.py vouches for them on the CPU):

  * unreal_pc_loss_kernel: rollouts of 1..20 steps (one chunk of 8, exactly one, one and a
    step, two, two and a step, the production 20), 1..7 actions, S == E, the 42-cell map at
    174x174 and at 300x400 with a padded row pitch; dones placed at the chunk boundaries; one
    case with the action channel times 4096, where q = (v + a) - a differs from v by 1e-4 (at
    the usual scale the channel cancels to rounding, and a kernel reading the wrong one passes);
  * unreal_rp_loss_kernel: n = 4, 1024 (one stride exactly) and 1178 samples, a weight, no used
    sample at all, logits times 30, a trained predictor (margin >= 25);
  * unreal_rp_scatter_kernel, unreal_gather_kernel: bitwise, both modes / all three modes;
  * unreal_vr_kernel: two blocks, the second partial, and a single item; 1, 4 and 7 actions;
  * every entry point's refusals (return codes only: nothing invalid is launched).

Tolerances: gradients 1e-5 of the reference's largest magnitude, loss sums rtol 1e-5 (the
bounds of the existing loss tests; an fp32 restatement of the pc recursion and the rp
reduction stays within 3.4e-7 and 2.5e-7). Copies, untouched elements and the scatter's
fixed-order sums of at most four terms are compared bitwise. Each test prints its worst
error over its bound before asserting."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import unreal_cases as cases

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-5
SUM_RTOL = 1e-5
PREFILL = cases.STATS_PREFILL
SENTINEL = 5.0


def _fig(what, err, bound):
    print("FIGURE %s: %.3g / %.3g = %.3g of the bound" % (what, err, bound, err / bound if bound else 0.0))


def _close(a, b, rtol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max() / scale
    _fig(what, err, rtol)
    assert err <= rtol, "%s: max err %.3g of scale %.3g" % (what, err, scale)


def _sum_close(got, want, what, floor=0.0):
    bound = SUM_RTOL * abs(want) + floor
    _fig(what, abs(got - want), bound)
    assert abs(got - want) <= bound, "%s: %.9g vs %.9g" % (what, got, want)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same_bits(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _dev(a):
    return torch.as_tensor(a).cuda()


def _f(x):
    return ctypes.c_float(x)


@pytest.fixture(scope="module")
def lib():
    from vnav import _lib
    return _lib.load()


def _P(t):
    from vnav import _lib
    return _lib.ptr(t)


# ---- pixel control ---------------------------------------------------------------------------

def _pc_call(lib, c, d, p2, stats, **over):
    a = dict(cells=c["cells"], frame_bytes=c["frame_bytes"], H=c["H"], W=c["W"], T=c["T"], E=c["E"], S=c["S"],
             A=c["A"])
    a.update(over)
    return lib.vn_unreal_pc_loss_grad_ex(_P(p2), a["cells"], _P(d["actions"]), _P(d["dones"]), _P(d["arena"]),
                                         a["frame_bytes"], a["H"], a["W"], _P(d["rows_img"]), _P(d["rows_last"]),
                                         a["T"], a["E"], a["S"], a["A"], _f(cases.GAMMA_PC), _f(cases.PC_WEIGHT),
                                         _P(stats), None)


_PC_INPUTS = ("arena", "rows_img", "rows_last", "actions", "dones")


@pytest.mark.parametrize("spec", cases.PC_CASES, ids=cases.PC_IDS)
def test_pc_loss_kernel_vs_oracle_at_chunk_edges(lib, spec):
    c = cases.pc_case(spec)
    T, S, A, C = c["T"], c["S"], c["A"], c["cells"]
    d = {k: _dev(c[k]) for k in _PC_INPUTS}
    p2 = _dev(c["p2"])
    stats = torch.full((2,), PREFILL, device="cuda")
    assert _pc_call(lib, c, d, p2, stats) == 0
    torch.cuda.synchronize()
    loss, want = cases.pc_expected(c)
    got = p2.cpu().view(T + 1, S, C, C, 8).numpy()
    _close(got.astype(np.float64) / float(np.float32(cases.PC_WEIGHT)), want, GRAD_TOL, "pc dp2 %s" % c["name"])
    assert not got[T].any(), "bootstrap rows"
    assert not got[..., A:].any(), "action channel and padding"
    st = stats.cpu().numpy().astype(np.float64)
    _sum_close(st[0] - PREFILL, loss * T * S * C * C, "pc loss sum %s" % c["name"])
    assert st[1] == PREFILL
    for k in _PC_INPUTS:
        _same_bits(d[k], c[k], k)


# ---- reward prediction -----------------------------------------------------------------------

@pytest.mark.parametrize("spec", cases.RP_CASES, ids=cases.RP_IDS)
def test_rp_loss_kernel_vs_oracle(lib, spec):
    """The trained case's loss (1e-11 per sample) gets an absolute floor of 2^-23 per used sample
    on top of the relative bound: one ulp of z next to 1, which logf(z) cannot see."""
    c = cases.rp_case(spec)
    T, E, S, n, w = c["T"], c["E"], c["S"], c["n"], c["weight"]
    lg, rw, dn = _dev(c["logits"]), _dev(c["rewards"]), _dev(c["dones"])
    dl = torch.full((n + 1, 4), SENTINEL, device="cuda")  # one guard row
    st = torch.full((3,), SENTINEL, device="cuda")
    assert lib.vn_unreal_rp_loss_grad(_P(lg), _P(rw), _P(dn), T, E, S, _f(w), _P(dl), _P(st), None) == 0
    torch.cuda.synchronize()
    loss, grad, count = cases.rp_expected(c)
    used, _ = cases.rp_used(c)
    got, s = dl.cpu().numpy(), st.cpu().numpy()
    assert s[1] == count and s[2] == SENTINEL
    assert (got[n] == SENTINEL).all(), "guard row"
    assert not got[:n, 3].any(), "column 3"
    assert not got[:n][~used].any(), "unused samples"
    if c["kind"] == "all_done":
        assert s[0] == 0.0 and s[1] == 0.0 and not got[:n].any()
    else:
        floor = 2.0 ** -23 if c["kind"] == "trained" else 0.0  # per used sample of the sum: as is on the mean
        _sum_close(float(s[0]), loss, "rp loss %s" % c["name"], floor)
        _close(got[:n, :3].astype(np.float64) / float(np.float32(w)), grad, GRAD_TOL, "rp dlogits %s" % c["name"])
    _same_bits(lg, c["logits"], "logits")
    _same_bits(rw, c["rewards"], "rewards")
    _same_bits(dn, c["dones"], "dones")


# ---- scatter and gather: bitwise -------------------------------------------------------------

@pytest.mark.parametrize("T,F,accumulate", cases.SCATTER_CASES)
def test_rp_scatter_kernel_bitwise(lib, T, F, accumulate):
    E, S = cases.SCATTER_E, cases.SCATTER_S
    dx, dx4 = cases.scatter_case(T, F)
    want = cases.scatter_ref(dx, dx4, T, E, S, F, accumulate)
    src = _dev(dx)
    out = torch.full((T * E + 1, F), SENTINEL, device="cuda")
    out[:T * E] = _dev(dx4)
    assert lib.vn_unreal_rp_scatter(_P(src), T, E, S, F, _P(out), accumulate, None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _same_bits(got[:T * E], want, "scatter")
    _same_bits(got[:T * E].reshape(T, E, F)[:, S:], dx4.reshape(T, E, F)[:, S:], "rows e >= S")
    assert (got[T * E] == SENTINEL).all(), "guard row"
    _same_bits(src, dx, "dx")


@pytest.mark.parametrize("mode,T,F", cases.GATHER_CASES)
def test_gather_kernel_bitwise(lib, mode, T, F):
    E, S = cases.GATHER_E, cases.GATHER_S
    assert ((T + 1) * S) % 2 == 1  # the h half ends inside a block of 256 lanes
    h_all, boot_h, x4 = cases.gather_case(T, F)
    want_h, want_x = cases.gather_ref(h_all, boot_h, x4, T, E, S, F)
    dh, db, dx = _dev(h_all), _dev(boot_h), _dev(x4)
    h_pc = torch.full(((T + 1) * S + 1, 512), SENTINEL, device="cuda")
    rp_x = torch.full((max(T - 2, 0) * S * 3 + 1, F), SENTINEL, device="cuda")
    if mode == "both":
        rc = lib.vn_unreal_gather(_P(dh), _P(db), _P(dx), T, E, S, F, _P(h_pc), _P(rp_x), None)
    elif mode == "rp_only":
        rc = lib.vn_unreal_gather(None, None, _P(dx), T, E, S, F, None, _P(rp_x), None)
    else:
        rc = lib.vn_unreal_gather(_P(dh), _P(db), None, T, E, S, F, _P(h_pc), None, None)
    assert rc == 0
    torch.cuda.synchronize()
    gh, gx = h_pc.cpu().numpy(), rp_x.cpu().numpy()
    if mode != "rp_only":
        _same_bits(gh[:-1], want_h, "h_pc")
    else:
        assert (gh == SENTINEL).all()
    if mode != "h_only":
        _same_bits(gx[:-1], want_x.reshape(-1, F), "rp_x")
    else:
        assert (gx == SENTINEL).all()
    assert (gh[-1] == SENTINEL).all() and (gx[-1] == SENTINEL).all(), "guard rows"
    _same_bits(dh, h_all, "h_all")
    _same_bits(db, boot_h, "boot_h")
    _same_bits(dx, x4, "x4")


# ---- value replay ----------------------------------------------------------------------------

@pytest.mark.parametrize("T,E,S,A", cases.VR_CASES)
def test_vr_kernel_vs_oracle(lib, T, E, S, A):
    out, ret, dout = cases.vr_case(T, E, S, A)
    w = 0.7
    do, dr, dd = _dev(out), _dev(ret), _dev(dout)
    st = torch.full((2,), PREFILL, device="cuda")
    assert lib.vn_unreal_vr_grad(_P(do), _P(dr), T, E, S, A, _f(w), _P(dd), _P(st), None) == 0
    torch.cuda.synchronize()
    loss, grad = cases.vr_expected(out, ret, T, E, S, A)
    got = dd.cpu().numpy()
    # the increment is read back from dout + inc: vr_case keeps |dout| near the gradient's size,
    # so the rounding of that sum stays at 1e-7 of the gradient's scale
    inc = (got[:T * E, A].astype(np.float64) - dout[:T * E, A]).reshape(T, E)[:, :S] / float(np.float32(w))
    _close(inc, grad, GRAD_TOL, "vr grad T%d S%d A%d" % (T, S, A))
    touched = np.zeros(got.shape, dtype=bool)
    touched[:T * E].reshape(T, E, 8)[:, :S, A] = True
    assert np.array_equal(_bits(got)[~touched], _bits(dout)[~touched]), "every other element of dout"
    s = st.cpu().numpy().astype(np.float64)
    _sum_close(s[0] - PREFILL, loss * T * S, "vr loss sum T%d S%d A%d" % (T, S, A))
    assert s[1] == PREFILL
    _same_bits(do, out, "out")
    _same_bits(dr, ret, "returns")


# ---- refusals --------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments(lib):
    """Non-zero return codes for the arguments each entry point's own check lists; the outputs
    keep their bits."""
    buf = torch.full((4096,), SENTINEL, device="cuda")  # stands for every pointer: nothing is launched
    out = torch.full((4096,), SENTINEL, device="cuda")
    st = torch.full((4,), SENTINEL, device="cuda")
    B, O, St = _P(buf), _P(out), _P(st)

    def pc(cells=20, fb=84 * 84 * 3, H=84, W=84, T=5, E=5, S=3, A=4):
        return lib.vn_unreal_pc_loss_grad_ex(O, cells, B, B, B, fb, H, W, B, B, T, E, S, A, _f(0.9), _f(0.05), St, None)

    def rp(T=5, E=5, S=3):
        return lib.vn_unreal_rp_loss_grad(B, B, B, T, E, S, _f(1.0), O, St, None)

    def scatter(T=5, E=5, S=3, F=8):
        return lib.vn_unreal_rp_scatter(B, T, E, S, F, O, 0, None)

    def gather(T=5, E=5, S=3, F=8, rp_x=True):
        return lib.vn_unreal_gather(B, B, B, T, E, S, F, O, O if rp_x else None, None)

    def vr(T=5, E=5, S=3, A=4):
        return lib.vn_unreal_vr_grad(B, B, T, E, S, A, _f(1.0), O, St, None)

    bad = {
        "rp T=2": rp(T=2), "scatter T=2": scatter(T=2), "gather T=2 with rp_x": gather(T=2),
        "pc S>E": pc(S=6), "rp S>E": rp(S=6), "scatter S>E": scatter(S=6), "gather S>E": gather(S=6),
        "gather S>E h only": gather(S=6, rp_x=False), "vr S>E": vr(S=6),
        "pc cells=21": pc(cells=21),
        "pc A=0": pc(A=0), "pc A=8": pc(A=8), "vr A=0": vr(A=0), "vr A=8": vr(A=8),
        "scatter F=6": scatter(F=6), "gather F=6": gather(F=6),
        "pc H<crop": pc(H=79, fb=84 * 84 * 3), "pc W<crop": pc(W=79, fb=84 * 84 * 3),
        "pc 42 cells at 84": pc(cells=42),
        "pc frame_bytes": pc(fb=84 * 84 * 3 - 1),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad.values()), {k: rc for k, rc in bad.items() if rc == 0}
    assert (out == SENTINEL).all() and (st == SENTINEL).all() and (buf == SENTINEL).all()
