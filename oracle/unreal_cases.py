"""Deterministic inputs of the UNREAL loss kernel tests (TEST INFRASTRUCTURE ONLY — see
oracle/__init__.py).

tests/test_unreal_loss_kernels_gpu.py feeds these to csrc/vn_unreal_loss.hip through the C
ABI; tests/test_unreal_loss_refs.py checks on the CPU that every case holds what it claims to
test (the placed dones, every action, both sides of the ReLU mask, every cause of an unused
reward-prediction sample) and that oracle/unreal.py agrees with a restatement in plain loops
on exactly these inputs. Nothing here needs the GPU.

Dones are placed, not drawn: unreal_pc_loss_kernel walks the rollout backwards in chunks of
PC_CHUNK steps and carries the next frame's row across chunks, so a pixel-control case of T
steps has a done at T-1, at T-8 (the last step of the first chunk), at T-9 (the first step of
the second), at T-16 and at 0, wherever those steps exist, spread over the envs; the last
used env never ends an episode; the rest is sparse (p = 0.1).
"""
import numpy as np
import torch

from oracle import unreal

PC_CHUNK = 8      # kPcChunk of csrc/vn_unreal_loss.hip
ARENA_ROWS = 12
GAMMA_PC = 0.9
PC_WEIGHT = 0.05
STATS_PREFILL = 0.25  # exactly representable; small next to every sum the cases produce


def _rng(*key):
    return np.random.RandomState([20161116] + [int(k) for k in key])


def forced_done_steps(T):
    """The steps of a T-step rollout that must hold a done (see the module docstring)."""
    out = []
    for t in (T - 1, T - PC_CHUNK, T - PC_CHUNK - 1, T - 2 * PC_CHUNK, 0):
        if t >= 0 and t not in out:
            out.append(t)
    return out


def placed_dones(T, E, S, rng):
    """dones bool [T, E] and the forced (step, env) pairs. Env S - 1 (the last one the
    kernels read) has no done when S >= 2; the forced ones go round the other used envs."""
    d = rng.rand(T, E) < 0.1
    clean = S - 1 if S >= 2 else None
    if clean is not None:
        d[:, clean] = False
    forced = []
    for k, t in enumerate(forced_done_steps(T)):
        e = k % max(S - 1, 1)
        d[t, e] = True
        forced.append((t, e))
    return d, forced, clean


# ---- pixel control ---------------------------------------------------------------------------

def _pc(name, T, E=5, S=3, A=4, H=84, W=84, cells=20, pad=0, ascale=1.0):
    return dict(name=name, T=T, E=E, S=S, A=A, H=H, W=W, cells=cells, pad=pad, ascale=ascale)


PC_CASES = ([_pc("T%d" % T, T) for T in (1, 7, 8, 9, 16, 17, 20)]
            + [_pc("A%d" % A, 9, A=A) for A in (1, 2, 3, 4, 5, 6, 7)]
            # the action channel times 4096: q = (v + a) - a is then v rounded to the ulp of a
            # (1e-4 and more), so a kernel that formed q from another channel, or took q = v, is
            # 1e-4 off the heads' own q; at the usual scale the channel cancels to rounding
            + [_pc("big_action_channel", 9, ascale=4096.0),
               _pc("S_eq_E", 9, E=3, S=3),
               _pc("174_c42_T17", 17, H=174, W=174, cells=42),
               _pc("300x400_c42_pitch", 9, H=300, W=400, cells=42, pad=64)])
PC_IDS = [c["name"] for c in PC_CASES]


def pc_case(spec):
    """The kernel's inputs (numpy) of one PC_CASES entry: arena u8 [ARENA_ROWS, frame_bytes]
    (frame_bytes = H W 3 + pad: the padding bytes are random too), rows_img i32 [T E],
    rows_last i32 [E], actions i32 [T E] (every action among the used envs when T S >= A,
    else all different), dones u8 [T, E], p2 f32 [(T+1) S, cells, cells, 8] = relu(N(0, 0.3))
    with the channels above A zeroed and the action channel A times ascale."""
    T, E, S, A, H, W, cells, pad = (spec[k] for k in ("T", "E", "S", "A", "H", "W", "cells", "pad"))
    rng = _rng(1, T, E, S, A, H, W, cells, pad)
    frame_bytes = H * W * 3 + pad
    arena = rng.randint(0, 256, size=(ARENA_ROWS, frame_bytes)).astype(np.uint8)
    rows_img = rng.randint(0, ARENA_ROWS, size=T * E).astype(np.int32)
    rows_last = rng.randint(0, ARENA_ROWS, size=E).astype(np.int32)
    actions = rng.randint(0, A, size=(T, E)).astype(np.int32)
    actions[:, :S] = rng.permutation(np.arange(T * S) % A).reshape(T, S)
    dones, forced, clean = placed_dones(T, E, S, rng)
    p2 = np.maximum(rng.randn((T + 1) * S, cells, cells, 8) * 0.3, 0.0).astype(np.float32)
    p2[..., A + 1:] = 0.0
    p2[..., A] *= np.float32(spec["ascale"])
    return dict(spec, frame_bytes=frame_bytes, arena=arena, rows_img=rows_img, rows_last=rows_last,
                actions=actions.reshape(-1), dones=dones.astype(np.uint8), p2=p2, forced=forced, clean=clean)


def pc_oracle_inputs(c):
    """What unreal.pc_loss takes for case c: q f32 [T+1, S, C, C, A] = (v + a) - a as the heads
    emit it, frames u8 [T+1, S, H, W, 3] (steps 0..T-1 from rows_img, T from rows_last; the row
    padding dropped), actions and dones [T, S] of the first S envs."""
    T, E, S, A, H, W, C = (c[k] for k in ("T", "E", "S", "A", "H", "W", "cells"))
    p2 = torch.as_tensor(c["p2"]).view(T + 1, S, C, C, 8)
    q = (p2[..., :A] + p2[..., A:A + 1]) - p2[..., A:A + 1]
    rows = np.concatenate((c["rows_img"].reshape(T, E)[:, :S], c["rows_last"][None, :S])).astype(np.int64)
    frames = torch.as_tensor(c["arena"][:, :H * W * 3].reshape(ARENA_ROWS, H, W, 3)[rows])
    actions = torch.as_tensor(c["actions"].reshape(T, E)[:, :S].astype(np.int64))
    dones = torch.as_tensor(c["dones"].reshape(T, E)[:, :S].astype(bool))
    return q, frames, actions, dones


def pc_expected(c):
    """(loss, d loss / d p2 f64 [T+1, S, C, C, 8]) of the fp64 oracle: the q gradient under the
    value channels' ReLU mask, 0 on the action channel, the padding and the bootstrap row."""
    T, S, A, C = c["T"], c["S"], c["A"], c["cells"]
    q, frames, actions, dones = pc_oracle_inputs(c)
    loss, grad = unreal.pc_loss(q, frames, actions, dones, gamma=float(np.float32(GAMMA_PC)))
    want = torch.zeros((T + 1, S, C, C, 8), dtype=torch.float64)
    want[..., :A] = grad * (torch.as_tensor(c["p2"]).view(T + 1, S, C, C, 8)[..., :A] > 0)
    return loss.item(), want.numpy()


# ---- reward prediction -----------------------------------------------------------------------

RP_REWARDS = (0.0, 1.0, -0.01)  # class 0, 1, 2
RP_TRAINED_MARGIN = 25.0


def _rp(name, T, E, S, kind="plain", weight=1.0):
    return dict(name=name, T=T, E=E, S=S, kind=kind, weight=weight)


RP_CASES = [_rp("n4_T3", 3, 4, 4), _rp("n1024", 34, 32, 32), _rp("n1178", 40, 33, 31),
            _rp("weight", 34, 32, 32, weight=0.37), _rp("all_done", 40, 33, 31, kind="all_done"),
            _rp("x30", 40, 33, 31, kind="x30"), _rp("trained", 40, 33, 31, kind="trained")]
RP_IDS = [c["name"] for c in RP_CASES]


def rp_classes(rewards):
    r = np.asarray(rewards)
    return np.where(r == 0, 0, np.where(r > 0, 1, 2))


def rp_case(spec):
    """logits f32 [(T-2) S, 4] (column 3, the product's padding, is NaN: never read), rewards
    f32 [T, E], dones u8 [T, E]. Steps 0..2 (3 with T >= 4) of envs 0..3 are placed: env 0 ends
    an episode at step 0 only, env 1 at step 1 only (the two causes of an unused sample
    ts = 2), env 2 at step 2 only (sample ts = 2 is used: the done at ts itself is not the
    kernel's business), env 3 at none; the rewards of those used samples are +, - and (T >= 4,
    sample ts = 3 of env 3) 0, so every class is used. kind: "plain", "x30" (logits times 30),
    "trained" (the sample's class leads by RP_TRAINED_MARGIN or more), "all_done"."""
    T, E, S, kind = spec["T"], spec["E"], spec["S"], spec["kind"]
    assert S >= 4 and T >= 3
    rng = _rng(2, T, E, S)
    n = (T - 2) * S
    dones = rng.rand(T, E) < 0.1
    rewards = np.asarray(RP_REWARDS, dtype=np.float32)[rng.choice(3, size=(T, E), p=(0.5, 0.25, 0.25))]
    dones[:min(T, 4), :4] = False
    dones[0, 0] = dones[1, 1] = dones[2, 2] = True
    rewards[2, 2], rewards[2, 3] = RP_REWARDS[1], RP_REWARDS[2]
    if T >= 4:
        rewards[3, 3] = RP_REWARDS[0]
    if kind == "all_done":
        dones[:] = True
    logits = np.full((n, 4), np.nan, dtype=np.float32)
    logits[:, :3] = rng.randn(n, 3).astype(np.float32)
    if kind == "x30":
        logits[:, :3] *= np.float32(30.0)
    if kind == "trained":
        cls = rp_classes(rewards[2:, :S]).reshape(-1)
        lead = logits[:, :3].max(1) + np.float32(RP_TRAINED_MARGIN + 0.5) + (rng.rand(n) * 5.0).astype(np.float32)
        logits[np.arange(n), cls] = lead
    return dict(spec, n=n, logits=logits, rewards=rewards, dones=dones.astype(np.uint8))


def rp_expected(c):
    """(loss, d loss / d logits f64 [n, 3], count) of the fp64 oracle on the first S envs."""
    S = c["S"]
    loss, grad, count = unreal.rp_loss(torch.as_tensor(c["logits"][:, :3]), torch.as_tensor(c["rewards"][:, :S]),
                                       torch.as_tensor(c["dones"][:, :S].astype(bool)))
    return loss.item(), grad.numpy(), count


def rp_used(c):
    """used bool [n], and per sample the dones at (ts-2, ts-1, ts)."""
    T, S = c["T"], c["S"]
    d = c["dones"][:, :S].astype(bool)
    d2, d1, d0 = d[:T - 2].reshape(-1), d[1:T - 1].reshape(-1), d[2:].reshape(-1)
    return ~(d2 | d1), (d2, d1, d0)


# ---- scatter, gather, value replay -----------------------------------------------------------

SCATTER_CASES = [(T, F, acc) for T in (3, 4, 9) for F in (4, 1568) for acc in (0, 1)]
SCATTER_E, SCATTER_S = 5, 3


def scatter_case(T, F, E=SCATTER_E, S=SCATTER_S):
    rng = _rng(3, T, F, E, S)
    return rng.randn((T - 2) * S, 3, F).astype(np.float32), rng.randn(T * E, F).astype(np.float32)


def scatter_ref(dx, dx4, T, E, S, F, accumulate):
    """fp32 sums in the kernel's stated order: slot 2 of sample t, slot 1 of t + 1, slot 0 of
    t + 2 (ts = t + k, 2 <= ts < T), then the old value when accumulating; rows e >= S keep
    their bits."""
    out = dx4.copy().reshape(T, E, F)
    dxv = dx.reshape(T - 2, S, 3, F)
    for t in range(T):
        for e in range(S):
            v = np.zeros(F, dtype=np.float32)
            for k in range(3):
                ts = t + k
                if 2 <= ts < T:
                    v = v + dxv[ts - 2, e, 2 - k]
            out[t, e] = out[t, e] + v if accumulate else v
    return out.reshape(T * E, F)


GATHER_E, GATHER_S = 5, 3
GATHER_CASES = [("both", 4, 4), ("both", 4, 1568), ("rp_only", 4, 4), ("rp_only", 4, 1568), ("h_only", 2, 4)]


def gather_case(T, F, E=GATHER_E, S=GATHER_S):
    rng = _rng(4, T, F, E, S)
    return (rng.randn(T * E, 512).astype(np.float32), rng.randn(E, 512).astype(np.float32),
            rng.randn(T * E, F).astype(np.float32))


def gather_ref(h_all, boot_h, x4, T, E, S, F):
    """h_pc [(T+1) S, 512]: rows t S + e = h_all row t E + e, rows T S + e = boot_h row e;
    rp_x [(T-2) S, 3, F]: slot k of sample (t, e) = x4 row (t + k) E + e (None when T < 3)."""
    h_pc = np.concatenate((h_all.reshape(T, E, 512)[:, :S].reshape(T * S, 512), boot_h[:S]))
    rp_x = None
    if T >= 3:
        xv = x4.reshape(T, E, F)
        rp_x = np.stack([xv[k:k + T - 2, :S] for k in range(3)], axis=2).reshape((T - 2) * S, 3, F)
    return h_pc, rp_x


VR_CASES = [(T, E, S, A) for (T, E, S) in ((20, 16, 13), (1, 1, 1)) for A in (1, 4, 7)]


def vr_case(T, E, S, A):
    """out f32 [T E + 1, 8], returns f32 [T E + 1], dout f32 [T E + 1, 8]: one guard row more
    than the kernel may touch. dout (the gradient the kernel adds to) is N(0, 0.01), the size
    of the increment 2 (V - R) / (T S) at 260 items, so that reading the increment back from the
    fp32 sum costs 1e-7 of its scale, not 1e-5."""
    rng = _rng(5, T, E, S, A)
    n = T * E + 1
    return (rng.randn(n, 8).astype(np.float32), rng.randn(n).astype(np.float32),
            (rng.randn(n, 8) * 0.01).astype(np.float32))


def vr_expected(out, ret, T, E, S, A):
    v = torch.as_tensor(out[:T * E, A].reshape(T, E)[:, :S])
    r = torch.as_tensor(ret[:T * E].reshape(T, E)[:, :S])
    loss, grad = unreal.vr_loss(v, r)
    return loss.item(), grad.numpy()


# ---- aux deconv targets ----------------------------------------------------------------------

def aux_table_ref(depth, seg, ph, pw, cell=4):
    """float64 [rows, ph, pw, 4]: (depth, seg0, seg1, seg2) = the mean over each cell x cell
    block of the centre crop of u8 / 255 (depth u8 [rows, H, W, 1], seg u8 [rows, H, W, 3])."""
    x = np.concatenate((depth, seg), axis=-1).astype(np.float64) / 255.0
    H, W = x.shape[1:3]
    top, left = (H - ph * cell) // 2, (W - pw * cell) // 2
    x = x[:, top:top + ph * cell, left:left + pw * cell]
    return x.reshape(x.shape[0], ph, cell, pw, cell, 4).mean(axis=(2, 4))
