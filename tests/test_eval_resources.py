"""The episode log costs nothing when it is off: the log-off nav_step_kernel keeps the resource
usage it had before the log existed (22 VGPRs, 42 SGPRs, no scratch, occupancy 8), checked by
compiling csrc/vn_nav.hip for gfx950 with -Rpass-analysis=kernel-resource-usage, and the listing
committed under profiles/eval/ is that compile's. CPU only: hipcc cross-compiles."""
import os
import re
import subprocess

from conftest import PKG, REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-result",
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c"]


def listing(src):
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join("csrc", src), "-o", os.devnull], cwd=PKG, check=True,
                       stderr=subprocess.PIPE, text=True)
    out = []
    for line in p.stderr.split("\n"):
        m = re.search(r"remark: *(.*?) *\[-Rpass-analysis=kernel-resource-usage\]$", line)
        if m:
            out.append(m.group(1))
    return out


def kernels(lines):
    """{function name: {field: value}} of a listing."""
    out, cur = {}, None
    for line in lines:
        k, _, v = line.partition(": ")
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None:
            cur[k.strip()] = v.strip()
    return out


def test_log_off_kernel_keeps_its_resources():
    lines = listing("vn_nav.hip")
    ks = kernels(lines)
    off = ks["_ZN2vn15nav_step_kernelENS_7NavArgsE"]
    assert (off["VGPRs"], off["TotalSGPRs"], off["ScratchSize [bytes/lane]"], off["Occupancy [waves/SIMD]"]) == \
        ("22", "42", "0", "8")
    on = [v for k, v in ks.items() if "nav_step_log_kernel" in k]
    assert len(on) == 1 and on[0]["ScratchSize [bytes/lane]"] == "0" and on[0]["Occupancy [waves/SIMD]"] == "8"
    for name in ("nav_count_kernel", "nav_scan_kernel", "nav_draw_kernel"):
        k = [v for f, v in ks.items() if name in f]
        assert len(k) == 1 and k[0]["ScratchSize [bytes/lane]"] == "0", name
    committed = open(os.path.join(REPO, "profiles", "eval", "resource_usage_nav_change.txt")).read().split("\n")
    assert [x for x in committed if x] == lines
    # the parent's listing of the same kernel, committed beside it, says the same
    parent = kernels(open(os.path.join(REPO, "profiles", "eval", "resource_usage_nav_parent.txt")).read().split("\n"))
    assert parent["_ZN2vn15nav_step_kernelENS_7NavArgsE"] == off


def test_env_listing_is_the_parents():
    """vn_env.hip gained host glue only: the committed listings of the parent's and the change's
    compile are equal line for line (every env_kernel instantiation)."""
    a = open(os.path.join(REPO, "profiles", "eval", "resource_usage_env_parent.txt")).read()
    b = open(os.path.join(REPO, "profiles", "eval", "resource_usage_env_change.txt")).read()
    assert a == b and a.count("Function Name") >= 20
