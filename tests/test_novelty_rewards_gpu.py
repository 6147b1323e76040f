"""vn_a2c_novelty_rewards on the GPU: bitwise the numpy float32 restatement of tests/visit_ref.py
at one element, a ragged wave, a second pass of the workgroup's loop and 5 x 1025 elements; counts
of 1, 2, 2^24 + 1 and 2^32 - 1, empty cells and cells of -1 and C; -0.0 rewards; the anneal read
from the device inside a captured graph; stats4 with equal bits over two runs and within 1e-6
relative of an fp64 sum; `rewards` untouched; the refusals."""
import numpy as np
import pytest
import torch

import visit_ref as vr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 63), (20, 65), (5, 1025)]
EDGE_COUNTS = np.array([1, 2, 2**24 + 1, 2**32 - 1, 0, 3, 7, 1000], dtype=np.uint32)
VN_EINVAL = -1


def case(T, E, seed=0):
    """Rewards with -0.0, +0.0 and the env's values; cells over the edge counts, random counts,
    -1 and C; about a third first visits."""
    rng = np.random.RandomState([seed, T, E])
    C = 64
    count = rng.randint(0, 50, C).astype(np.uint32)
    count[:len(EDGE_COUNTS)] = EDGE_COUNTS
    cell = rng.randint(-1, C + 1, (T, E)).astype(np.int32)
    n = min(cell.size, len(EDGE_COUNTS) + 2)
    cell.reshape(-1)[:n] = (list(range(len(EDGE_COUNTS))) + [-1, C])[:n]
    first = (rng.rand(T, E) < 0.35).astype(np.uint8)
    rewards = rng.choice(np.array([-0.0, 0.0, 1.0, -0.01, 0.3], dtype=np.float32), (T, E)).astype(np.float32)
    return rewards, cell, first, count


def launch(lib, r, cell, first, count, wc, wf, steps=None, anneal=0, out=None, stats=None):
    from vnav import _lib
    T, E = r.shape
    out = torch.full((T, E), 7.0, dtype=torch.float32, device="cuda") if out is None else out
    stats = torch.full((4,), 7.0, dtype=torch.float32, device="cuda") if stats is None else stats
    rc = lib.vn_a2c_novelty_rewards(_lib.ptr(r), _lib.ptr(cell), _lib.ptr(first), _lib.ptr(count), count.numel(), T, E,
                                    wc, wf, _lib.ptr(steps), anneal, _lib.ptr(out), _lib.ptr(stats),
                                    _lib.stream_ptr(r.device))
    return rc, out, stats


def dev(x):
    if x.dtype == np.uint32:
        return torch.as_tensor(x.view(np.int32), device="cuda")
    return torch.as_tensor(x, device="cuda")


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def check_stats(stats, want):
    s = stats.cpu().numpy().astype(np.float64)
    for got, ref in zip(s[:3], (want["added"], want["firsts"], want["inv"])):
        assert abs(got - ref) <= 1e-6 * abs(ref) + 1e-30, (got, ref)
    assert bits(stats.cpu().numpy()[3]) == bits(want["wc"])


@pytest.mark.parametrize("T,E", SHAPES)
def test_bitwise_restatement(T, E):
    from vnav import _lib
    lib = _lib.load()
    r, cell, first, count = case(T, E)
    d = [dev(x) for x in (r, cell, first, count)]
    keep = d[0].clone()
    for wc, wf in ((0.1, 0.05), (0.0, 0.3), (1.7, 0.0), (0.0, 0.0)):
        rc, out, stats = launch(lib, *d, wc, wf)
        assert rc == 0
        want, st = vr.novelty_rewards32(r, cell, first, count, wc, wf)
        got = out.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (wc, wf, np.flatnonzero(bits(got) != bits(want))[:8])
        check_stats(stats, st)
        _, out2, stats2 = launch(lib, *d, wc, wf)
        assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32)) and torch.equal(out, out2)
    assert torch.equal(d[0].view(torch.int32), keep.view(torch.int32))  # rewards is never written
    if T * E >= 10:
        # the edge counts, the empty cell and the two cells outside the table were all met
        flat = vr.novelty_rewards32(np.zeros_like(r), cell, first, count, 1.0, 0.0)[0].reshape(-1)[:10]
        assert np.array_equal(bits(flat[:4]), bits([1.0, np.float32(1.0) / np.sqrt(np.float32(2.0)), 1.0 / 4096, 1.0 / 65536]))
        assert flat[4] == 0 and flat[8] == 0 and flat[9] == 0
        # a -0.0 reward with both terms 0 gives IEEE's +0.0, as the restatement pins it
        zero = (bits(r) == 0x80000000) & (bits(vr.novelty_rewards32(r, cell, first, count, 0.0, 0.0)[0]) == 0)
        assert zero.any()


def test_anneal_from_the_device_in_a_captured_graph():
    from vnav import _lib
    lib = _lib.load()
    T, E = 20, 65
    r, cell, first, count = case(T, E, seed=1)
    d = [dev(x) for x in (r, cell, first, count)]
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros((T, E), dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.float32, device="cuda")
    anneal = 1000
    assert launch(lib, *d, 0.3, 0.2, steps, anneal, out, stats)[0] == 0  # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert launch(lib, *d, 0.3, 0.2, steps, anneal, out, stats)[0] == 0
    for n in (0, 1, 333, 999, 1000, 5000):
        steps.fill_(n)
        out.fill_(7.0)
        g.replay()
        want, st = vr.novelty_rewards32(r, cell, first, count, 0.3, 0.2, steps=n, anneal_steps=anneal)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), n
        check_stats(stats, st)
    assert st["wc"] == 0 and st["added"] == 0.0


def test_refusals_write_nothing():
    from vnav import _lib
    lib = _lib.load()
    r, cell, first, count = case(3, 63)
    d = [dev(x) for x in (r, cell, first, count)]
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.full((3, 63), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    st = _lib.stream_ptr(out.device)
    P = [_lib.ptr(x) for x in d]
    C = count.size

    def call(p=P, T=3, E=63, steps_p=_lib.ptr(steps), anneal=0, o=_lib.ptr(out), s=_lib.ptr(stats)):
        return lib.vn_a2c_novelty_rewards(p[0], p[1], p[2], p[3], C, T, E, 0.1, 0.1, steps_p, anneal, o, s, st)

    for k in range(4):
        assert call(p=[None if i == k else x for i, x in enumerate(P)]) == VN_EINVAL, k
    assert call(o=None) == VN_EINVAL and call(s=None) == VN_EINVAL
    assert call(T=0) == VN_EINVAL and call(E=0) == VN_EINVAL and call(T=-1) == VN_EINVAL
    assert call(steps_p=None, anneal=10) == VN_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (stats == 7.0).all()
    assert call(steps_p=None, anneal=0) == 0  # steps_dev is not needed without an anneal
    assert not (out == 7.0).all()
