"""The visit counts leave the env kernels alone: vn_env.hip gained host code only, so its
-Rpass-analysis=kernel-resource-usage listing for gfx950 is still the committed one of the parent
(profiles/eval/resource_usage_env_change.txt). The kernels of csrc/vn_visit.hip (the visit kernel
with 8, 64 and 1 lanes per env, the table statistics and the novelty bonus) use no
scratch, spill nothing and have no dynamic stack, and their listing is the one committed under
profiles/visits/. CPU only: hipcc cross-compiles."""
import os

from conftest import REPO
from test_eval_resources import kernels, listing

NEW = ("visit_kernelILi64E", "visit_kernelILi8E", "visit_kernelILi1E", "visit_stats_kernel", "novelty_rewards_kernel")


def committed(*path):
    return [x for x in open(os.path.join(REPO, "profiles", *path)).read().split("\n") if x]


def test_env_listing_is_the_parents():
    lines = listing("vn_env.hip")
    assert lines == committed("eval", "resource_usage_env_change.txt")
    assert sum(1 for x in lines if x.startswith("Function Name")) >= 20


def test_visit_kernels_use_no_scratch():
    lines = listing("vn_visit.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["SGPRs Spill"] == "0" and k[0]["VGPRs Spill"] == "0", name
    assert lines == committed("visits", "resource_usage_visits.txt")
