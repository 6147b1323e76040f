"""The recurrent core (lstm_forward_step / heads_forward / lstm_backward of csrc/vn_policy.hip, kernels
in csrc/vn_lstm.h) against float64 at every launch regime from 18 to 1030 envs, and the trainer above
the few-env path.

tests/test_few_env_gpu.py holds the core to float64 at 1..17 envs, tests/test_prod_oracle_gpu.py at
5, 16, 1024 and 2048 envs x 3 steps. In between the launch helpers walk its products through
(oracle/lstm_regime_cases.py, A = 4: xcat = 1032, xoff = 520):

  gates = xcat x W_cat^T (128 x 128 tiles, K = 1032, EpiBias2 through pre_col in the split form)
      slabs 11 (kchunk 96) -> 9 (128, the last slab 8 k-columns, less than one K tile) at E = 187 -> 7 at
      228 -> 6 at 293 -> 5 at 342 -> 4 at 410 -> 3 at 513 -> 2 at 683 -> unsplit at 897; from 187 on the
      count is set by sk_cap. Epilogue lanes 2 below E = 32, 1 from there. Row tiles 1, 2 (from 129), 3+.
  dh = m (dgates x W_hh) (64 x 64 tiles, K = 2048, EpiLstmDh's mask through pre_row in the split form)
      slabs 32 (to E = 128) -> 22 -> 16 -> 13 -> 11 -> 10 -> 8 -> 7 -> 6 -> 5 -> unsplit on the 64-wide K
      tile at 961. Lanes 4 below E = 128, 1 from there. Row tiles 1, 2 (from 65), 3+ (from 129).
  dz5 = relu' (dgates x W_ih[:, :512]) over T E rows (128 x 128 tiles)
      slabs 32, 22, 16, 13, 11, 10, 8, 7, 6, 5, 4, 3, 2 (unsplit only from 3969 rows). Lanes 4 or 1.
  dW_cat | db (launch_wgrad_x6t over T E rows, b_ih and b_hh sharing the bias column through db2)
      the direct EpiWgrad epilogue to 256 rows, then 2..11 slabs; from 2817 rows the slab bound halves 12
      slabs to 6. The last slab full, part filled, part filled with a length that is no multiple of 32.
  the heads' weight gradient (launch_wgrad<32, 64>, M = A + 1)
      1..13 slabs, reduce lanes 1 (to 8 slabs) or 2.
  the heads' forward: 8 slabs of 64, 1 lane throughout.

CASES covers every value of every one of these keys; dh's count only in cases with T = 3, since at T = 1
no step reads dh (tests/test_lstm_regime_cases.py checks that on the CPU, and that the seeded inputs expose a dropped gates slab, a dropped dh slab, a dh mask taken as 1, a
dropped dW_cat slab, an unwritten b_hh gradient and dh_extra on the wrong rows). VARIANT_CASES are the
calling forms only the few-env tests had run against float64: A = 1, 3, 7 at E = 40 and A = 1 at E = 192 (9
gates slabs, the last of 4 k-columns), NULL arguments at E = 18 and 300, vn_lstm_backward_ex with S < E
at (40, 5) and (300, 16), and T = 2 at E = 130.

Every case runs oracle/trunk_checks.py lstm_core_check on inputs made on the CPU, strict, with every
buffer the calls write prefilled with a NaN bit pattern. Bars, the project's own: h and c of every
step 1e-5 of that step's scale; logits and values 1e-5 of scale and element by element; dz5 and every
gradient tensor 1e-4 of its scale; the xcat rows bitwise. After the backward no NaN remains in dz5 or
the head and LSTM gradients, W_cat's pad columns are exactly zero and the trunk's part of grads still
holds the fill.

The trainer: oracle/update_checks.py second_update_vs_fp64 (a whole second rollout + update restated
in float64: carried state, masks from dones, the last-action / reward input, sampling, the bootstrap
step) had only run at 4 and 5 envs. Here the plain recurrent goal net runs at E = 20 and 136, T = 4
(at 136: gates on two row tiles with 8 rows in the second, dh on 22 slabs, dW_cat on 3 slabs over 544
rows) with an episode limit of 3, and BigHouse with UNREAL at E = 20, unreal_envs = 6, T = 6: the first
whole update through vn_lstm_backward_ex with S < E above 16 envs. Every tensor of the total gradient
within 1e-4 of its scale.

Measured errors: profiles/lstm_regimes/README.md.
"""
import numpy as np
import pytest

from oracle import lstm_regime_cases as lc
from oracle.trunk_checks import BIGHOUSE_NAMES, LSTM_NAMES, NAMES, lstm_core_check
from oracle.update_checks import UNREAL_REWARDS, VISIBLE_IN, maze_scene, second_update_vs_fp64

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _run(tag, E, T, A=4, null_args=False, extra=0):
    e = lstm_core_check(E, T, A, null_args=null_args, dh_extra=extra, strict=True, inputs=lc.inputs(E, T, A, extra),
                        nan_fill=True)
    print("lstm-regime %s: %s" % (tag, " ".join("%s %.3g" % kv for kv in e.items())))
    assert set(e) == {"h", "c", "logits", "value", "dz5", "policy_logits.0.weight", "policy_logits.0.bias",
                      "critic.0.weight", "critic.0.bias"} | set(LSTM_NAMES)
    return e


@pytest.mark.parametrize("E,T", lc.CASES, ids=lc.CASE_IDS)
def test_regime_cases_vs_fp64_torch_lstm(E, T):
    """Every case of the cover, A = 4, placed and drawn resets."""
    _run("E%d-T%d" % (E, T), E, T)


@pytest.mark.parametrize("E,T,A,null_args,extra", lc.VARIANT_CASES, ids=lc.VARIANT_IDS)
def test_calling_forms_vs_fp64_torch_lstm(E, T, A, null_args, extra):
    """Other action counts, NULL arguments, vn_lstm_backward_ex below full width and T = 2, above 16 envs."""
    _run(lc.VARIANT_IDS[lc.VARIANT_CASES.index((E, T, A, null_args, extra))], E, T, A, null_args, extra)


def _lstm_keys(names):
    return {k + "." + kind for k in names for kind in ("weight", "bias")} | {"rnn.inner." + n for n in LSTM_NAMES}


@pytest.mark.parametrize("E", (20, 136))
def test_recurrent_trainer_update_above_the_few_env_path_vs_fp64_oracle(E):
    """The plain recurrent goal net, E envs x 4 steps, an episode limit of 3: the second rollout + update
    restated in float64 (the helper asserts the env transitions, the sampled actions, the rollout's
    logits / values and the bootstrap values)."""
    T = 4
    scene, graph, spd, frames = maze_scene((84, 84), aux=False)
    res = second_update_vs_fp64(scene, graph, spd, frames, E=E, T=T, seed=3, env_seed=11, max_steps=3)
    errs, dones = res["errs"], res["tr"].dones.cpu().numpy().reshape(T, E).astype(bool)
    # the trainer's default above 16 envs: shared_base on a goal frame once per goal run (vn_goal_runs); the
    # helper reads a sample's goal masks at the start of its run
    assert res["tr"].dedup_goals
    per_step = dones.sum(1)
    print("recurrent trainer E=%d T=%d: dones per step %s; worst gradient error %.3g (%s)"
          % (E, T, per_step.tolist(), max(errs.values()), max(errs, key=errs.get)))
    assert dones.any(), "no done inside the second rollout"
    assert any(0 < n < E for n in per_step), "every env reset at the same step: %s" % per_step.tolist()
    assert set(errs) == _lstm_keys(NAMES)  # every tensor of the trunk, the heads and the LSTM
    bad = {k: "%.3g" % e for k, e in errs.items() if not e <= TOL}
    assert not bad, bad


# pc_weight as tests/test_unreal_update_gpu.py sets it (the default 0.05 leaves pixel control's share of the LSTM
# gradient under 10 x TOL on these random-frame scenes); rp / vr at the trainer's defaults
WEIGHTS = dict(pc_weight=10.0, rp_weight=1.0, vr_weight=1.0)
# (trainer seed, env seed): chosen so that all three reward classes occur among the 12 used samples
BIGHOUSE = dict(E=20, S=6, T=6, max_steps=4, seed=3, env_seed=14)


def test_bighouse_unreal_update_below_full_width_vs_fp64_oracle():
    """BigHouse with UNREAL at 20 envs, unreal_envs = 6, T = 6, set up as tests/test_unreal_update_gpu.py's
    bighouse-84 case: the first whole update through vn_lstm_backward_ex with S < E above 16 envs."""
    c = BIGHOUSE
    E, S, T = c["E"], c["S"], c["T"]
    scene, graph, spd, frames = maze_scene((84, 84), aux=False, rewards=UNREAL_REWARDS)
    res = second_update_vs_fp64(scene, graph, spd, frames, E=E, T=T, seed=c["seed"], env_seed=c["env_seed"],
                                max_steps=c["max_steps"], aux_weight=0.0, unreal=True, unreal_envs=S,
                                unreal_source="rollout", arch="bighouse", **WEIGHTS)
    tr, errs, info, vis = res["tr"], res["errs"], res["info"], res["visible"]
    assert tr.unreal_S == S and not tr.rp_into_aux
    got, want = res["stats"]
    shares = {t: vis[t][VISIBLE_IN["bighouse"][t]] for t in ("pc", "rp", "vr")}
    print("bighouse unreal E=%d S=%d T=%d: %s\n  losses gpu %s\n  losses f64 %s\n  shares (of scale) %s\n  worst gradient "
          "error %.3g (%s)" % (E, S, T, info, got, want, {t: "%.3g" % v for t, v in shares.items()},
                               max(errs.values()), max(errs, key=errs.get)))
    # the case is not vacuous
    assert info["dones"] >= 1 and info["rp_used"] >= 1 and info["rp_skipped"] >= 1, info
    assert info["classes"] == [0, 1, 2], info   # all three reward-prediction classes among the used samples
    assert got["rp_count"] == want["rp_count"] == info["rp_used"]
    low = {t: "%.3g" % v for t, v in shares.items() if v < 10 * TOL}
    assert not low, "terms under 10 x the tolerance of the total gradient: %s" % low
    for t in ("pc", "rp", "vr"):
        np.testing.assert_allclose(got[t], want[t], rtol=1e-5, err_msg=t)
    want_keys = _lstm_keys(BIGHOUSE_NAMES) | {"%s.0.0.%s" % (n, k) for n in ("pc_base", "pc_value", "pc_action")
                                              for k in ("weight", "bias")} | {"rp.weight", "rp.bias"}
    assert set(errs) == want_keys
    for k in errs:
        if k.startswith("pc_action"):
            np.testing.assert_array_equal(res["mine"][k].numpy(), 0.0, err_msg=k)
            assert not res["want"][k].any()
    bad = {k: "%.3g" % e for k, e in errs.items() if not e <= TOL and not k.startswith("pc_action")}
    assert not bad, bad
    dx4 = tr.unreal_dx4.view(T, E, -1)   # rp's own dX4 buffer: the rows of the envs it never samples stay zero
    assert not dx4[:, S:].any() and dx4[:, :S].any()
