"""The four kernels of csrc/vn_ppo_kl.hip (the KL gate, the gated Adam step and its advance, the
gated RMSprop step) use no scratch, spill nothing and have no dynamic stack; the gate keeps one
double per wave in LDS; their -Rpass-analysis=kernel-resource-usage listing for gfx950 is the one
committed under profiles/ppo_kl/. The feature added no kernel elsewhere: the listings of
csrc/vn_ppo.hip, csrc/vn_ppo_minibatch.hip and csrc/vn_env.hip are still the committed ones. CPU
only: hipcc cross-compiles."""
from test_eval_resources import kernels, listing
from test_visit_resources import committed

NEW = ("kl_gate_kernel", "adam_gated_kernel", "adam_advance_gated_kernel", "rmsprop_gated_kernel")


def test_kl_kernels_use_no_scratch():
    lines = listing("vn_ppo_kl.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["SGPRs Spill"] == "0" and k[0]["VGPRs Spill"] == "0", name
    gate = [v for f, v in ks.items() if NEW[0] in f][0]
    assert gate["LDS Size [bytes/block]"] == str(8 * 1024 // 64)
    assert lines == committed("ppo_kl", "resource_usage_ppo_kl.txt")


def test_the_other_listings_are_the_committed_ones():
    assert listing("vn_ppo.hip") == committed("ppo", "resource_usage_ppo.txt")
    assert listing("vn_ppo_minibatch.hip") == committed("ppo_minibatch", "resource_usage_ppo_minibatch.txt")
    assert listing("vn_env.hip") == committed("eval", "resource_usage_env_change.txt")
