"""PPO and Adam leave the env kernels alone: vn_env.hip's -Rpass-analysis=kernel-resource-usage
listing for gfx950 is still the committed one of the parent (profiles/eval/
resource_usage_env_change.txt). The kernels of csrc/vn_ppo.hip (the advantage statistics, the PPO
loss gradient, the Adam step and its step-count launch) use no scratch, spill nothing and have no
dynamic stack, and their listing is the one committed under profiles/ppo/. CPU only: hipcc
cross-compiles."""
from test_eval_resources import kernels, listing
from test_visit_resources import committed

NEW = ("adv_stats_kernel", "ppo_loss_grad_kernel", "adam_kernel", "adam_advance_kernel")


def test_env_listing_is_the_parents():
    lines = listing("vn_env.hip")
    assert lines == committed("eval", "resource_usage_env_change.txt")
    assert sum(1 for x in lines if x.startswith("Function Name")) >= 20


def test_ppo_kernels_use_no_scratch():
    lines = listing("vn_ppo.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["SGPRs Spill"] == "0" and k[0]["VGPRs Spill"] == "0", name
    assert lines == committed("ppo", "resource_usage_ppo.txt")
