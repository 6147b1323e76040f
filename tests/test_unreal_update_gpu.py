"""The composed UNREAL update (A2CTrainer(unreal=True, unreal_source="rollout"): LSTM + deconv
heads + pixel control / reward prediction / value replay, the pass bench.py times and
thor-cached-auxiliary trains with) against its float64 restatement, oracle/update_checks.py:
the second rollout + update on a small random maze, as the logged-run test of
tests/test_prod_oracle_gpu.py does for the A2C + aux update.

Per case: the env transitions, sampled actions and rollout outputs (asserted inside the
helper); the pc / rp / vr loss means within 1e-5 of the oracle's and the rp sample count
exactly; every tensor of the total gradient within 1e-4 of its scale (pc_action exactly 0);
the rows of envs >= S of rp's own dX4 buffer exactly 0 where that buffer is used.

So that no case passes vacuously it also asserts: a done inside the rollout on an env < S; a
reward-prediction sample skipped and one used; at least two reward classes among the used
samples; and that each UNREAL term is visible at the tolerance — its own gradient is >= 10 x
1e-4 of the total's scale in a tensor it shares with the A2C loss (an LSTM weight for pc, a
conv_base weight for rp, the critic row for vr), so dropping the term (a missing dh_extra, an
unscattered rp gradient) cannot hide under the bound. The loss weights are WEIGHTS below.
"""
import numpy as np
import pytest

from oracle.update_checks import UNREAL_REWARDS, UPDATE_CASES, VISIBLE_IN, maze_scene, second_update_vs_fp64

pytestmark = pytest.mark.gpu

TOL = 1e-4
# pc_weight: the trainer's default 0.05 leaves pixel control's share of the LSTM gradient under
# 10 x TOL on these random-frame scenes; rp / vr at the trainer's defaults
WEIGHTS = dict(pc_weight=10.0, rp_weight=1.0, vr_weight=1.0)
# (trainer seed, env seed): chosen for the reward classes among the used samples (the six used
# samples of a small case reach two classes at best; the logged case all three)
SEEDS = {"goal-174-aux": (3, 12), "goal-174-noaux": (3, 12), "goal-174-logged": (3, 11), "bighouse-84": (3, 12)}


@pytest.mark.parametrize("name", list(UPDATE_CASES))
def test_unreal_update_vs_fp64_oracle(name):
    c = UPDATE_CASES[name]
    arch, S = c["arch"], c["S"]
    scene, graph, spd, frames = maze_scene(c["hw"], aux=c["aux_weight"] > 0, rewards=UNREAL_REWARDS)
    seed, env_seed = SEEDS[name]
    kw = dict(aux_weight=c["aux_weight"], unreal=True, unreal_envs=S, unreal_source="rollout", **WEIGHTS)
    if arch != "goal":
        kw["arch"] = arch
    res = second_update_vs_fp64(scene, graph, spd, frames, E=c["E"], T=c["T"], seed=seed, env_seed=env_seed,
                                max_steps=c["max_steps"], **kw)
    tr, errs, info, vis = res["tr"], res["errs"], res["info"], res["visible"]
    assert tr.unreal_S == S and tr.rp_into_aux == (c["aux_weight"] > 0)
    got, want = res["stats"]
    shares = {t: vis[t][VISIBLE_IN[arch][t]] for t in ("pc", "rp", "vr")}
    groups = {}
    for k, e in errs.items():
        g = k.split(".")[0]
        groups[g] = max(groups.get(g, 0.0), e)
    print("%s: %s\n  losses gpu %s\n  losses f64 %s\n  shares (of scale) %s\n  worst error per group %s" % (
        name, info, got, want, {t: "%.3g" % v for t, v in shares.items()},
        {g: "%.2g" % e for g, e in groups.items()}))
    # the case is not vacuous
    assert info["dones"] >= 1 and info["rp_used"] >= 1 and info["rp_skipped"] >= 1, info
    assert len(info["classes"]) >= 2, info
    assert got["rp_count"] == want["rp_count"] == info["rp_used"]
    low = {t: "%.3g" % v for t, v in shares.items() if v < 10 * TOL}
    assert not low, "terms under 10 x the tolerance of the total gradient: %s" % low
    # the losses
    for t in ("pc", "rp", "vr"):
        np.testing.assert_allclose(got[t], want[t], rtol=1e-5, err_msg=t)
    # every tensor of the total gradient
    names = set(errs)
    assert {"rnn.inner.weight_ih_l0", "critic.0.weight", "pc_base.0.0.weight", "pc_value.0.0.weight"} <= names
    assert ("rp.weight" if arch == "bighouse" else "rp.1.weight") in names
    assert ("deconv_depth.0.1.weight" in names) == (c["aux_weight"] > 0)
    for k in names:
        if k.startswith("pc_action"):
            np.testing.assert_array_equal(res["mine"][k].numpy(), 0.0, err_msg=k)
            assert not res["want"][k].any()
    bad = {k: "%.3g" % e for k, e in errs.items() if e > TOL and not k.startswith("pc_action")}
    assert not bad, bad
    if not tr.rp_into_aux:  # rp's own dX4 buffer: the rows of the envs it never samples stay zero
        dx4 = tr.unreal_dx4.view(c["T"], c["E"], -1)
        assert not dx4[:, S:].any() and dx4[:, :S].any()
