"""vn_unreal_rp_sample bit for bit against tests/rp_sample_ref.py, and vn_unreal_rp_loss_grad_labels
against the fp64 reference and, bitwise, against vn_unreal_rp_loss_grad, through raw library calls on
synthetic rings (no env).

The sampler is one workgroup of 1024 threads (csrc/vn_rp_sample.hip). Its chunk edges, in
candidates (capacity (T - 2) S of the filled slots): 64 (one count-table entry, one wave-wide
ballot), 1024 (one chunk per wave), 4096 (one unrolled round of the 16 waves), 65536 (one chunk per
thread; beyond it a thread's run holds two chunks and the select walks the run), and 1024 draws
(one per thread). EDGE_S puts a ring on both sides of each; a select thread re-reads a chunk 16
candidates at a time, which any random ring crosses."""
import ctypes

import numpy as np
import pytest
import torch

import rp_sample_ref as rr

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
SEED = 0x5EED0123456789
GRAD_TOL = 1e-5  # tests/test_unreal_loss_kernels_gpu.py's bounds
SUM_RTOL = 1e-5


@pytest.fixture(scope="module")
def L():
    from vnav import _lib
    _lib.load()
    return _lib


def make_ring(R, T, S, seed, p_reward=0.15, p_neg=0.05, p_done=0.2):
    rng = np.random.default_rng(seed)
    rew = np.where(rng.random((R, T, S)) < p_reward, 1.0, -0.0).astype(np.float32)
    rew[rng.random((R, T, S)) < p_neg] = -0.5
    don = rng.random((R, T, S)) < p_done
    rows = rng.integers(0, 1 << 20, size=(R, 2, (T + 1) * S)).astype(np.int32)
    return rew, don, rows


class DevRing:
    def __init__(self, L, rew, don, rows, filled, ctr):
        self.host = (rew, don, rows)
        self.rew, self.don, self.rows = (torch.as_tensor(a).cuda() for a in (rew, don, rows))
        self.meta = torch.tensor([1, filled, ctr, 0], dtype=torch.int64, device="cuda")
        R, T, S = rew.shape
        self.c = L.RpRing(self.rew.data_ptr(), self.don.data_ptr(), self.rows.data_ptr(), self.meta.data_ptr(),
                          R, T, S)

    def unchanged(self, filled, ctr):
        rew, don, rows = self.host
        return (self.rew.cpu().numpy().tobytes() == rew.tobytes() and
                self.don.cpu().numpy().tobytes() == don.tobytes() and
                self.rows.cpu().numpy().tobytes() == rows.tobytes() and
                self.meta.cpu().tolist() == [1, filled, ctr, 0])


def call(L, ring, count, skew, seed=SEED, with_src=True, stream=None):
    """One call into sentinel-filled outputs with a guard row each; returns them as numpy."""
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(ri=torch.full((count + 1, 3), SENT, **i32), rg=torch.full((count + 1, 3), SENT, **i32),
               lab=torch.full((count + 1,), SENT, **i32), src=torch.full((count + 1,), SENT, **i32),
               st=torch.full((5,), SENT, **i32))
    P = L.ptr
    rc = L.load().vn_unreal_rp_sample(ctypes.byref(ring.c), count, ctypes.c_double(skew), seed, P(out["ri"]),
                                      P(out["rg"]), P(out["lab"]), P(out["src"]) if with_src else None, P(out["st"]),
                                      stream)
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(L, rew, don, rows, filled, ctr, count, skew, with_src=True):
    ring = DevRing(L, rew, don, rows, filled, ctr)
    got = call(L, ring, count, skew, with_src=with_src)
    ri, rg, lab, src, st = rr.sample(rew, don, rows, filled, count, skew, SEED, ctr)
    assert got["ri"][:count].tobytes() == ri.tobytes(), "rows_img"
    assert got["rg"][:count].tobytes() == rg.tobytes(), "rows_goal"
    assert got["lab"][:count].tobytes() == lab.tobytes(), "label"
    if with_src:
        assert got["src"][:count].tobytes() == src.tobytes(), "src"
    else:
        assert (got["src"] == SENT).all()
    assert got["st"][:4].tobytes() == st.tobytes(), ("stats4", got["st"], st)
    for k in ("ri", "rg", "lab", "src"):
        assert (got[k][count:] == SENT).all(), "guard row of " + k
    assert got["st"][4] == SENT
    assert ring.unchanged(filled, ctr), "the ring and meta are only read"
    return lab, st


@pytest.mark.parametrize("filled", (0, 1, 2, 3))
@pytest.mark.parametrize("skew", (0.0, 0.5, 1.0))
def test_small_ring_every_fill_level(L, filled, skew):
    rew, don, rows = make_ring(3, 5, 4, 7)
    for count in (1, 65, 300):
        lab, st = check(L, rew, don, rows, filled, 3, count, skew)
    if filled == 0:
        assert (lab == -1).all() and st.tolist() == [0, 0, 0, 0]
    elif skew == 0.5:
        assert st[0] > 0 and (filled == 1 or st[1] > 0)


def test_filled_beyond_capacity_is_clamped(L):
    rew, don, rows = make_ring(3, 5, 4, 7)
    ring = DevRing(L, rew, don, rows, 9, 3)
    got = call(L, ring, 65, 0.5)
    want = rr.sample(rew, don, rows, 3, 65, 0.5, SEED, 3)
    assert got["src"][:65].tobytes() == want[3].tobytes() and got["st"][:4].tobytes() == want[4].tobytes()


def test_shortest_ring(L):
    """T = 3, S = 1: one window per slot."""
    rew, don, rows = make_ring(4, 3, 1, 11, p_reward=0.5, p_done=0.1)
    for filled in (1, 3, 4):
        check(L, rew, don, rows, filled, 0, 65, 0.5)


EDGE_S = (63, 64, 65, 1023, 1025, 4095, 4097, 65535, 65537)


@pytest.mark.parametrize("S", EDGE_S)
def test_chunk_edges(L, S):
    """capacity 1, T = 3: S candidates, on both sides of each chunk edge of the kernel."""
    rew, don, rows = make_ring(1, 3, S, S)
    lab, st = check(L, rew, don, rows, 1, 1, 300, 0.5)
    assert st[0] > 0 and st[1] > 0


@pytest.mark.parametrize("filled", (2, 3))
def test_two_chunks_per_thread(L, filled):
    """(3, 4, 11000): 44000 candidates at two filled slots (one chunk per thread), 66000 at three
    (two per thread); 1100 draws: more than one per thread."""
    rew, don, rows = make_ring(3, 4, 11000, 5, p_reward=0.01, p_neg=0.002)
    check(L, rew, don, rows, filled, 2 ** 32 + 5, 1100, 0.5)


def test_larger_ring(L):
    rew, don, rows = make_ring(2, 4, 3000, 9)
    for count, skew in ((1, 0.5), (65, 0.0), (300, 1.0), (300, 0.5)):
        check(L, rew, don, rows, 2, 17, count, skew)


def test_empty_sets(L):
    rew, don, rows = make_ring(3, 5, 4, 7)
    zero = np.full_like(rew, -0.0)
    lab, st = check(L, zero, don, rows, 3, 1, 300, 0.5)  # Q1 empty: every draw falls back to Q0
    assert st[1] == 0 and st[0] > 0 and (lab == 0).all()
    ones = np.where(rew == 0, np.float32(2.0), rew).astype(np.float32)
    lab, st = check(L, ones, don, rows, 3, 1, 300, 0.5)  # Q0 empty
    assert st[0] == 0 and st[1] > 0 and (lab > 0).all() and set(lab.tolist()) == {1, 2}
    lab, st = check(L, rew, np.ones_like(don), rows, 3, 1, 300, 0.5)  # both empty: every draw void
    assert st.tolist() == [0, 0, 0, 0] and (lab == -1).all()


def test_counter_and_null_src(L):
    rew, don, rows = make_ring(3, 5, 4, 7)
    labs = [check(L, rew, don, rows, 3, ctr, 300, 0.5)[0] for ctr in (0, 1, 2 ** 32 + 5, 5)]
    assert labs[0].tobytes() != labs[1].tobytes()  # the next update draws anew
    assert labs[2].tobytes() != labs[3].tobytes()  # the counter's high word is part of the draw
    check(L, rew, don, rows, 3, 1, 65, 0.5, with_src=False)


def test_captured_graph_follows_the_meta(L):
    rew, don, rows = make_ring(3, 5, 4, 7)
    ring = DevRing(L, rew, don, rows, 2, 4)
    i32 = dict(dtype=torch.int32, device="cuda")
    count = 65
    ri, rg = torch.zeros((count, 3), **i32), torch.zeros((count, 3), **i32)
    lab, src, st = torch.zeros(count, **i32), torch.zeros(count, **i32), torch.zeros(4, **i32)
    lib, P = L.load(), L.ptr

    def launch():
        dev = torch.device("cuda", torch.cuda.current_device())
        assert lib.vn_unreal_rp_sample(ctypes.byref(ring.c), count, ctypes.c_double(0.5), SEED, P(ri), P(rg), P(lab),
                                       P(src), P(st), L.stream_ptr(dev)) == 0

    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for filled, ctr in ((2, 4), (3, 5), (3, 2 ** 32 + 5)):
        ring.meta.copy_(torch.tensor([1, filled, ctr, 0], dtype=torch.int64))
        g.replay()
        torch.cuda.synchronize()
        want = rr.sample(rew, don, rows, filled, count, 0.5, SEED, ctr)
        for got, w in zip((ri, rg, lab, src, st), want):
            assert got.cpu().numpy().tobytes() == w.tobytes(), (filled, ctr)


# ---- the loss on explicit labels ---------------------------------------------------------------------
def _labels_call(L, lg, lab, w):
    n = lg.shape[0]
    dl = torch.full((n + 1, 4), 5.0, device="cuda")
    st = torch.full((3,), 5.0, device="cuda")
    assert L.load().vn_unreal_rp_loss_grad_labels(L.ptr(lg), L.ptr(lab), n, ctypes.c_float(w), L.ptr(dl), L.ptr(st),
                                                  None) == 0
    torch.cuda.synchronize()
    return dl, st


LOSS_CASES = [(n, kind) for n in (1, 5, 1024, 1178) for kind in ("mixed", "all_unused", "x30")]


@pytest.mark.parametrize("n,kind", LOSS_CASES)
def test_loss_labels_vs_fp64_and_vs_the_sequence_kernel(L, n, kind):
    """The fp64 reference at the sibling's bounds (gradients 1e-5 of scale, loss rtol 1e-5, plus
    2^-23 per sample where the predictor is saturated: logits x 30), and vn_unreal_rp_loss_grad on
    the same logits arranged as T = 3, E = S = n — rewards row 2 carries the class, a done at step
    0 stands for label -1 — bitwise."""
    rng = np.random.default_rng(1000 + n)
    lg_h = rng.standard_normal((n, 4)).astype(np.float32) * (30.0 if kind == "x30" else 1.0)
    lab_h = rng.integers(-1, 3, size=n).astype(np.int32)
    if kind == "all_unused":
        lab_h[:] = -1
    elif n > 1:
        lab_h[0], lab_h[1] = -1, 2  # both kinds are present at every size above 1
    else:
        lab_h[0] = 1
    w = 0.75
    lg, lab = torch.as_tensor(lg_h).cuda(), torch.as_tensor(lab_h).cuda()
    dl, st = _labels_call(L, lg, lab, w)
    got, s = dl.cpu().numpy(), st.cpu().numpy()
    ce, used, grad = rr.rp_loss_labels(lg_h, lab_h, weight=float(np.float32(w)))
    assert s[1] == used and s[2] == 5.0 and (got[n] == 5.0).all() and not got[:n, 3].any()
    assert not got[:n][lab_h < 0].any()
    if used == 0:
        assert s[0] == 0.0 and not got[:n].any()
    else:
        floor = 2.0 ** -23 if kind == "x30" else 0.0
        print("FIGURE loss: %.3g of the bound" % (abs(float(s[0]) - ce) / (SUM_RTOL * abs(ce) + floor)))
        assert abs(float(s[0]) - ce) <= SUM_RTOL * abs(ce) + floor, (float(s[0]), ce)
        scale = np.abs(grad).max()
        err = np.abs(got[:n].astype(np.float64) - grad).max() / scale
        print("FIGURE dlogits: %.3g of the bound" % (err / GRAD_TOL))
        assert err <= GRAD_TOL, err
    assert lg.cpu().numpy().tobytes() == lg_h.tobytes() and lab.cpu().numpy().tobytes() == lab_h.tobytes()
    # the sequence entry point on the equivalent rollout
    rew = np.zeros((3, n), dtype=np.float32)
    rew[2] = np.select([lab_h == 1, lab_h == 2], [1.0, -1.0], 0.0)
    don = np.zeros((3, n), dtype=bool)
    don[0] = lab_h < 0
    dl2 = torch.full((n + 1, 4), 5.0, device="cuda")
    st2 = torch.full((3,), 5.0, device="cuda")
    assert L.load().vn_unreal_rp_loss_grad(L.ptr(lg), L.ptr(torch.as_tensor(rew).cuda()),
                                           L.ptr(torch.as_tensor(don).cuda()), 3, n, n, ctypes.c_float(w), L.ptr(dl2),
                                           L.ptr(st2), None) == 0
    torch.cuda.synchronize()
    assert dl2.cpu().numpy().tobytes() == got.tobytes(), "dlogits bits"
    assert st2.cpu().numpy().tobytes() == s.tobytes(), "stats bits"


def test_refusals_write_nothing(L):
    rew, don, rows = make_ring(3, 5, 4, 7)
    ring = DevRing(L, rew, don, rows, 3, 1)
    lib, P = L.load(), L.ptr
    i32 = dict(dtype=torch.int32, device="cuda")
    out = torch.full((4096,), SENT, **i32)
    O = P(out)

    def sample(c=None, count=8, skew=0.5, ri=O, rg=O, lab=O, st=O):
        return lib.vn_unreal_rp_sample(ctypes.byref(c or ring.c) if c is not False else None, count,
                                       ctypes.c_double(skew), SEED, ri, rg, lab, O, st, None)

    def ringc(**over):
        c = L.RpRing(ring.rew.data_ptr(), ring.don.data_ptr(), ring.rows.data_ptr(), ring.meta.data_ptr(), 3, 5, 4)
        for k, v in over.items():
            setattr(c, k, v)
        return c

    bad = [sample(c=False), sample(ri=None), sample(rg=None), sample(lab=None), sample(st=None), sample(count=0),
           sample(count=-3), sample(skew=-0.01), sample(skew=1.01), sample(skew=float("nan")),
           sample(c=ringc(T=2)), sample(c=ringc(S=0)), sample(c=ringc(capacity=0)), sample(c=ringc(rewards=None)),
           sample(c=ringc(dones=None)), sample(c=ringc(rows=None)), sample(c=ringc(meta4=None)),
           sample(c=ringc(capacity=1024, T=3, S=1025)),  # one window over the limit (nothing of it is read)
           sample(c=ringc(capacity=1 << 30, T=1 << 30, S=1 << 30))]
    assert all(rc != 0 for rc in bad), bad
    assert "vn_unreal_rp_sample" in L.last_error()
    f = torch.full((64,), 5.0, device="cuda")
    F = P(f)

    def loss(lg=F, lab=O, n=4, dl=F, st=F):
        return lib.vn_unreal_rp_loss_grad_labels(lg, lab, n, ctypes.c_float(1.0), dl, st, None)

    bad = [loss(lg=None), loss(lab=None), loss(dl=None), loss(st=None), loss(n=0), loss(n=-1)]
    assert all(rc != 0 for rc in bad), bad
    assert "vn_unreal_rp_loss_grad_labels" in L.last_error()
    torch.cuda.synchronize()
    assert (out == SENT).all() and (f == 5.0).all() and ring.unchanged(3, 1)
