"""The kernels of csrc/vn_shaping.hip (the progress kernel behind vn_nav_progress and
vn_a2c_returns_ex's scan) use no scratch, spill nothing and have no dynamic stack, and their
-Rpass-analysis=kernel-resource-usage listing for gfx950 is the one committed under
profiles/shaping/. CPU only: hipcc cross-compiles."""
import os

from conftest import REPO
from test_eval_resources import kernels, listing

NEW = ("shape_progress_kernel", "returns_ex_kernel")


def test_shaping_kernels_use_no_scratch():
    lines = listing("vn_shaping.hip")
    ks = kernels(lines)
    assert len(ks) == len(NEW)
    for name in NEW:
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1, name
        assert k[0]["ScratchSize [bytes/lane]"] == "0" and k[0]["Dynamic Stack"] == "False", name
        assert k[0]["SGPRs Spill"] == "0" and k[0]["VGPRs Spill"] == "0", name
    committed = open(os.path.join(REPO, "profiles", "shaping", "resource_usage_shaping.txt")).read().split("\n")
    assert lines == [x for x in committed if x]
