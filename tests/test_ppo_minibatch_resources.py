"""The two kernels of csrc/vn_ppo_minibatch.hip (the env permutation and the minibatch gather) use
no scratch, spill no vector register and have no dynamic stack; the permutation stages exactly one
tile of keys in LDS; their -Rpass-analysis=kernel-resource-usage listing for gfx950 is the one
committed under profiles/ppo_minibatch/. The accumulating loss-gradient entry added no kernel:
csrc/vn_ppo.hip's listing is still the one committed under profiles/ppo/. CPU only: hipcc
cross-compiles."""
from test_eval_resources import kernels, listing
from test_visit_resources import committed

NEW = ("env_permutation_kernel", "minibatch_gather_kernel")


def test_minibatch_kernels_use_no_scratch():
    from vnav import _lib
    lines = listing("vn_ppo_minibatch.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["VGPRs Spill"] == "0", name
    perm = [v for f, v in ks.items() if NEW[0] in f][0]
    assert perm["LDS Size [bytes/block]"] == str(4 * _lib.PPO_PERM_TILE) and perm["SGPRs Spill"] == "0"
    assert lines == committed("ppo_minibatch", "resource_usage_ppo_minibatch.txt")


def test_ppo_listing_is_the_parents():
    assert listing("vn_ppo.hip") == committed("ppo", "resource_usage_ppo.txt")
