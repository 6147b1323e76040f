"""The geodesic curriculum leaves the env kernels alone: vn_env.hip gained host code only, so its
-Rpass-analysis=kernel-resource-usage listing for gfx950 is still the committed one of the parent
(profiles/eval/resource_usage_env_change.txt, every env_kernel instantiation). The new kernels
of csrc/vn_curriculum.hip use no scratch, and their listing is the one committed under
profiles/curriculum/. CPU only: hipcc cross-compiles."""
import os

from conftest import REPO
from test_eval_resources import kernels, listing

NEW = ("cur_maxd_kernel", "cur_sort_kernel", "cur_count_kernel", "cur_advance_kernel", "cur_set_state_kernel")


def committed(*path):
    return [x for x in open(os.path.join(REPO, "profiles", *path)).read().split("\n") if x]


def test_env_listing_is_the_parents():
    lines = listing("vn_env.hip")
    assert lines == committed("eval", "resource_usage_env_change.txt")
    assert sum(1 for x in lines if x.startswith("Function Name")) >= 20


def test_new_kernels_use_no_scratch():
    lines = listing("vn_curriculum.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["SGPRs Spill"] == "0" and k[0]["VGPRs Spill"] == "0", name
    assert lines == committed("curriculum", "resource_usage_curriculum.txt")
