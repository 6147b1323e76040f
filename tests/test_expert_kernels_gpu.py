"""vn_a2c_loss_grad_expert (csrc/vn_a2c.hip) and vn_set_nav_mask_output against
tests/expert_ref.py (fp64) and, where the header promises it, against vn_a2c_loss_grad by bits.

n = 1, 63, 64, 65, 256, 257, 513 are the wave, workgroup and multi-workgroup edges of a
256-thread kernel with one sample per thread. Bounds are test_loss_grad_vs_fp64's: dout within
1e-5 of its scale with the unused columns exactly 0, each statistic within 1e-5 of the sum of
its terms' magnitudes; the counts and the weight are exact. Outputs are pre-filled with NaN, so
an element the kernel should have written and did not fails. Every comparison prints its worst
element next to its bound ("EXPERTERR ..." lines, shown with pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import expert_ref as er

pytestmark = pytest.mark.gpu

NAN = float("nan")
VN_EINVAL, VN_ESTATE = -1, -4
CF, I64 = ctypes.c_float, ctypes.c_int64
NS = [1, 63, 64, 65, 256, 257, 513]
AS = [1, 3, 4, 7]
VC, EC, W0 = 0.5, 0.01, 0.75
# all 16 values of the four edge bits, then values with bits 4-7 set
MASKS = list(range(16)) + [0x10, 0x80, 0xF0, 0x35, 0xFF, 0x4A, 0x60]


def _l():
    from vnav import _lib
    return _lib, _lib.load(), _lib.stream_ptr(torch.device("cuda", 0))


def dev(a):
    return torch.as_tensor(np.array(a)).cuda()  # a copy: the cached inputs are read-only


def host(t):
    return t.cpu().numpy()


def full(shape, value, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def within(what, got, ref, bound):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err = np.abs(got - ref).reshape(-1)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / b, 0.0)
    k = int(np.argmax(ratio))
    print("EXPERTERR %-44s worst %.3e  bound %.3e" % (what, err[k], b[k]))
    assert (err <= b).all(), "%s: err %.3g > bound %.3g at %d" % (what, err[k], b[k], k)


@functools.lru_cache(maxsize=None)
def inputs(n, A, scale):
    rng = np.random.RandomState([21, n, A, int(scale)])
    out = np.full((n, 8), np.nan, dtype=np.float32)
    out[:, :A] = (rng.randn(n, A) * scale).astype(np.float32)
    out[:, A] = rng.randn(n).astype(np.float32)
    actions = rng.randint(0, A, size=n).astype(np.int32)
    rets = rng.randn(n).astype(np.float32)
    mask = np.array([MASKS[(i + 5 * A + int(scale)) % len(MASKS)] for i in range(n)], dtype=np.uint8)
    for a in (out, actions, rets, mask):
        a.setflags(write=False)
    return out, actions, rets, mask


class Call:
    """Device copies of one input set and NaN-filled outputs of vn_a2c_loss_grad_expert."""

    def __init__(self, out, actions, rets, mask, A):
        self.n, self.A = len(actions), A
        self.out, self.actions, self.rets, self.mask = dev(out), dev(actions), dev(rets), dev(mask)
        self.steps = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.poison()

    def poison(self):
        self.dout, self.stats, self.estats = full((self.n, 8), NAN), full(4, NAN), full(4, NAN)

    def run(self, pg=1.0, w0=W0, anneal=0, n=None, A=None, mask=True, steps=True):
        _lib, lib, st = _l()
        P = _lib.ptr
        return lib.vn_a2c_loss_grad_expert(P(self.out), P(self.actions), P(self.rets), P(self.mask) if mask else None,
                                           self.n if n is None else n, self.A if A is None else A, CF(VC), CF(EC),
                                           CF(pg), CF(w0), P(self.steps) if steps else None, I64(anneal),
                                           P(self.dout), P(self.stats), P(self.estats), st)

    def plain(self):
        """vn_a2c_loss_grad on the same inputs -> (dout, stats4)."""
        _lib, lib, st = _l()
        P = _lib.ptr
        dout, stats = full((self.n, 8), NAN), full(4, NAN)
        _lib.check(lib.vn_a2c_loss_grad(P(self.out), P(self.actions), P(self.rets), self.n, self.A, CF(VC), CF(EC),
                                        P(dout), P(stats), st), "vn_a2c_loss_grad")
        return host(dout), host(stats)


def check_against_ref(tag, c, out, actions, rets, mask, A, pg, w):
    ref = er.expert_loss_grad64(out, actions, rets, mask, A, VC, EC, pg, w)
    d, s, e = host(c.dout), host(c.stats), host(c.estats)
    within(tag + " dout", d[:, :A + 1], ref["dout"][:, :A + 1], 1e-5 * np.abs(ref["dout"][:, :A + 1]).max())
    assert same_bits(d[:, A + 1:], np.zeros((len(actions), 7 - A), dtype=np.float32)), tag
    within(tag + " stats4", s, ref["stats4"], 1e-5 * ref["mags4"])
    within(tag + " -log q sum", e[:1], ref["expert3"][:1], 1e-5 * ref["expert_mag"])
    assert e[1] == ref["expert3"][1] and e[2] == ref["expert3"][2], (tag, e, ref["expert3"])
    assert same_bits(e[3:], np.array([w], dtype=np.float32)), (tag, e[3], w)


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("n", NS)
def test_expert_loss_grad_vs_fp64(n, A, scale):
    out, actions, rets, mask = inputs(n, A, scale)
    c = Call(out, actions, rets, mask, A)
    _lib = _l()[0]
    for pg in (1.0, 0.0, 0.25):
        c.poison()
        _lib.check(c.run(pg=pg), "vn_a2c_loss_grad_expert")
        check_against_ref("n=%d A=%d x%d pg=%g" % (n, A, int(scale), pg), c, out, actions, rets, mask, A, pg,
                          np.float32(W0))
    first = host(c.stats).copy(), host(c.estats).copy()
    _lib.check(c.run(pg=0.25), "vn_a2c_loss_grad_expert")  # the call zeroes both statistics itself
    if n <= 256:
        assert same_bits(host(c.stats), first[0]) and same_bits(host(c.estats), first[1])
    else:
        assert same_bits(host(c.estats)[1:], first[1][1:])


@pytest.mark.parametrize("pg", [1.0, 0.0, 0.25])
def test_mask_mass_extremes(pg):
    """Masks whose actions hold 1.8e-35 of the mass, none that fp32 can represent (e^-120), and
    all but 2.6e-35 of it, beside ordinary samples: finite, and within the same bounds."""
    out, actions, rets, mask = (np.array(a) for a in inputs(65, 4, 1.0))
    out[0, :4] = (80.0, 0.0, -1.0, 0.0)
    out[1, :4] = (120.0, 0.0, -1.0, 0.0)
    out[2, :4] = (80.0, 79.0, 0.0, 0.0)
    out[64, :4] = (0.0, -1.0, 0.0, 120.0)
    mask[[0, 1, 2, 64]] = (0b0110, 0b0110, 0b0011, 0b0011)
    c = Call(out, actions, rets, mask, 4)
    _l()[0].check(c.run(pg=pg, w0=1.0), "vn_a2c_loss_grad_expert")
    check_against_ref("extremes pg=%g" % pg, c, out, actions, rets, mask, 4, pg, np.float32(1.0))
    # the starved masks' gradient is p - (their softmax among themselves), to fp32 rounding
    d = host(c.dout).astype(np.float64) * 65.0  # w / n = 1 / 65
    ref = er.expert_loss_grad64(out, actions, rets, mask, 4, VC, EC, pg, 1.0)["dout"] * 65.0
    for i in (0, 1, 64):
        assert np.abs(d[i, :4] - ref[i, :4]).max() <= 1e-5 * np.abs(ref[i, :4]).max(), (i, d[i], ref[i])


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("n", NS)
def test_bitwise_equal_to_plain_loss_grad(n, A):
    """pg = 1 with w0 = 0, and separately with every mask 0: dout is vn_a2c_loss_grad's by bits
    (all eight columns); stats4 too within one workgroup."""
    for scale in (1.0, 30.0):
        out, actions, rets, mask = inputs(n, A, scale)
        for what, m, w0 in (("w0=0", mask, 0.0), ("masks=0", np.zeros_like(mask), W0)):
            c = Call(out, actions, rets, m, A)
            _l()[0].check(c.run(pg=1.0, w0=w0), "vn_a2c_loss_grad_expert")
            dout, stats = c.plain()
            tag = "%s n=%d A=%d x%d" % (what, n, A, int(scale))
            assert same_bits(host(c.dout), dout), tag
            if n <= 256:
                assert same_bits(host(c.stats), stats), tag
            e = host(c.estats)
            assert same_bits(e[3:], np.array([w0], dtype=np.float32)), tag
            if what == "masks=0":
                assert same_bits(e[:3], np.zeros(3, dtype=np.float32)), tag
            else:
                assert e[2] == (er.mask_bits(mask, A).any(1)).sum(), tag


def test_annealing_reads_the_device_word():
    """expert_stats4[3] = the fp64 rule rounded once to fp32, by bits, at s = 0, anneal / 2,
    anneal, 2 anneal and with anneal_steps = 0; changing only *steps_dev changes dout."""
    out, actions, rets, mask = inputs(65, 4, 1.0)
    c = Call(out, actions, rets, mask, 4)
    _lib = _l()[0]
    anneal, w0 = 1000, 0.7
    douts = {}
    for s in (0, anneal // 2, anneal, 2 * anneal):
        c.steps.fill_(s)
        c.poison()
        _lib.check(c.run(w0=w0, anneal=anneal), "vn_a2c_loss_grad_expert")
        want = er.anneal_weight(w0, s, anneal)
        assert same_bits(host(c.estats)[3:], np.array([want], dtype=np.float32)), (s, host(c.estats)[3], want)
        check_against_ref("anneal s=%d" % s, c, out, actions, rets, mask, 4, 1.0, want)
        douts[s] = host(c.dout).copy()
    assert not same_bits(douts[0], douts[anneal // 2]) and not same_bits(douts[anneal // 2], douts[anneal])
    assert same_bits(douts[anneal], douts[2 * anneal]) and same_bits(douts[anneal], c.plain()[0])
    c.steps.fill_(123456)
    _lib.check(c.run(w0=w0, anneal=0), "vn_a2c_loss_grad_expert")
    assert same_bits(host(c.estats)[3:], np.array([w0], dtype=np.float32))
    _lib.check(c.run(w0=w0, anneal=0, steps=False), "vn_a2c_loss_grad_expert")  # not read when constant
    assert same_bits(host(c.estats)[3:], np.array([w0], dtype=np.float32))
    # a step count past 2^24 (fp32's integers) still moves the weight: the rule runs in fp64
    ws = []
    for s in (2 ** 30 + 1, 2 ** 30 + 129):
        c.steps.fill_(s)
        _lib.check(c.run(w0=1.0, anneal=2 ** 31), "vn_a2c_loss_grad_expert")
        ws.append(host(c.estats)[3])
        assert same_bits(ws[-1:], np.array([er.anneal_weight(1.0, s, 2 ** 31)], dtype=np.float32))
    assert ws[0] != ws[1]


def test_bad_arguments_write_nothing():
    out, actions, rets, mask = inputs(65, 4, 1.0)
    c = Call(out, actions, rets, mask, 4)
    bad = [dict(mask=False), dict(A=0), dict(A=8), dict(A=-1), dict(n=0), dict(n=-3), dict(anneal=10, steps=False)]
    for kw in bad:
        assert c.run(**kw) == VN_EINVAL, kw
    torch.cuda.synchronize()
    for t in (c.dout, c.stats, c.estats):
        assert np.isnan(host(t)).all()


def test_set_nav_mask_output():
    """The setter redirects the mask alone, NULL restores the env's own buffer, and it is
    refused while navigation info is off. E = 257 crosses nav_step_kernel's workgroup."""
    import vnav
    _lib, lib, _ = _l()
    E = 257
    sc = [vnav.synthetic_scene(k, grid=5, frame_shape=(16, 16, 3)) for k in range(2)]
    env = vnav.VectorEnv(sc, E, seed=4, max_episode_steps=5)
    assert lib.vn_set_nav_mask_output(env._ctx, None) == VN_ESTATE
    with pytest.raises(_lib.VnavError):
        env.set_nav_mask_output(None)
    env.set_nav_info(True)
    own = env.nav_outputs()
    guard = torch.full((3, E), 0xEE, dtype=torch.uint8, device="cuda")
    for bad in (guard, guard[0].to(torch.int32), guard[0, :E - 1], guard[:, 0], guard[0].cpu()):
        with pytest.raises(ValueError):
            env.set_nav_mask_output(bad)
    rng = np.random.RandomState(0)
    act = lambda: dev(rng.randint(0, 4, size=E).astype(np.int32))  # noqa: E731
    env.step(act())
    before = {k: v.clone() for k, v in own.items()}
    env.set_nav_mask_output(guard[1])
    _, _, _, info = env.step(act())
    torch.cuda.synchronize()
    assert torch.equal(own["optimal_mask"], before["optimal_mask"])  # not written
    assert (guard[0] == 0xEE).all() and (guard[2] == 0xEE).all()
    # the redirected mask belongs to the step's other outputs: action = its lowest set bit
    m = host(guard[1]).astype(np.int64)
    a = host(info["optimal_action"])
    assert (m < 16).all() and np.array_equal(a, np.where(m == 0, -1, np.log2(np.maximum(m & -m, 1)).astype(np.int64)))
    assert (m != 0).any()
    env.set_nav_mask_output(None)
    _, _, _, info = env.step(act())
    torch.cuda.synchronize()
    assert torch.equal(guard[1], torch.as_tensor(m.astype(np.uint8)).cuda())  # no longer written
    m2 = host(own["optimal_mask"]).astype(np.int64)
    a2 = host(info["optimal_action"])
    assert np.array_equal(a2, np.where(m2 == 0, -1, np.log2(np.maximum(m2 & -m2, 1)).astype(np.int64)))
    env.close()
