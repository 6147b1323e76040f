"""The conditions the cases of tests/test_unreal_head_regimes_gpu.py rest on, checked on the CPU
from the launch rules restated in oracle/unreal_head_cases.py (splitk_count and the two lines
after it, the slab counts of launch_wgrad / launch_wgrad6, the G of the reduces, colsum's block
count): every switch has a case on each side. A changed threshold fails here and names the
case to move."""
from oracle import unreal_head_cases as uc


def _goal(n):
    return uc.pc_regime("goal", n)


def _ns(cases, arch="goal", A=4):
    return sorted({n for a, n, A_, acc in cases if a == arch and A_ == A})


def test_tables_hold_what_the_issue_sets():
    assert _ns(uc.PC_CASES) == [1, 3, 4, 84, 192, 193, 200, 201, 256, 257, 336, 960, 961]
    first = {}
    for i, (arch, n, A, acc) in enumerate(uc.PC_CASES[:len(uc.PC_N)]):
        assert (arch, A, acc) == ("goal", 4, i % 2)
        first[n] = acc
    for n in (960, 961):  # both values of accumulate on each side of the dh switch
        assert {acc for a, m, A, acc in uc.PC_CASES if m == n} == {0, 1}
    assert {(n, A) for a, n, A, acc in uc.PC_A_CASES} == {(n, A) for n in (5, 201) for A in (1, 2, 7)}
    assert _ns(uc.BH_CASES, "bighouse") == [1, 3, 4, 200, 201, 257]
    assert {(n, A) for a, n, A, acc in uc.BH_CASES if A != 4} == {(5, 1), (5, 7)}
    assert uc.PC_TRAINER_N == (5, 336) and uc.PC_DETERMINISM_N == (4, 336) and uc.RP_DETERMINISM_R == 288
    for hw in ((174, 174), (300, 400)):
        assert [R for a, g, R in uc.RP_CASES if (a, g) == ("goal", hw)] == [1, 64, 65, 72, 256, 257, 288]
    for arch in ("goal", "bighouse"):
        assert [R for a, g, R in uc.RP_CASES if (a, g) == (arch, (84, 84))] == [1, 65, 257]
    ids = [uc.pc_id(c) for c in uc.PC_CASES + uc.PC_A_CASES + uc.BH_CASES] + [uc.rp_id(c) for c in uc.RP_CASES]
    assert len(ids) == len(set(ids))
    assert {acc for a, n, A, acc in uc.PC_A_CASES} == {0, 1} == {acc for a, n, A, acc in uc.BH_CASES}


def test_restated_rules_on_known_launches():
    """Launches whose split counts the source's comments state (the logged run's 4 envs: dpcb is
    54 tiles... at n = 84; every training batch of the bench >= 128 tiles: no split)."""
    assert uc.splitk(4096, 512, 2592, 64, 64) == 1
    assert uc.splitk(84 * 81, 32, 1024, 128, 32) > 1 and -(-84 * 81 // 128) == 54
    assert uc.splitk(4, 5, 512, 32, 16) == 8      # K / (2 BK) bounds a 4-env head product
    assert uc.splitk(4, 512, 96, 64, 64) == 1     # K < 4 BK
    assert uc.reduce_lanes(4, 5, 8) == 1 and uc.reduce_lanes(4, 5, 9) == 2 and uc.reduce_lanes(300, 300, 64) == 1
    assert uc.colsum_blocks(1, 8) == 1 and uc.colsum_blocks(10 ** 6, 8) == 512


def test_pixel_control_switches_have_both_sides():
    ns = _ns(uc.PC_CASES)
    r = {n: _goal(n) for n in ns}
    # W1 weight gradient: the direct EpiWgrad epilogue up to n = 3, slabs from 4
    assert [r[n]["w1_slabs"] for n in (1, 3, 4)] == [1, 1, 2]
    assert _goal(2)["w1_slabs"] == 1
    # half a work item of the parity-class kernel (IMG = 2) at n = 1, 3
    assert r[1]["half_item"] and r[3]["half_item"] and not r[4]["half_item"]
    assert (r[1]["items"], r[3]["items"], r[961]["items"]) == (1, 2, 481)
    # colsum below its 512-block cap on the small cases, at it on the others
    for n in (1, 3, 4):
        assert max(r[n]["b2_blocks"], r[n]["b1_blocks"]) < uc.COLSUM_BLOCKS
    assert r[84]["b2_blocks"] == r[84]["b1_blocks"] == uc.COLSUM_BLOCKS
    assert r[1]["dpcb_G"] == 2 and r[1]["dpcb_splits"] == 16
    # pc_base forward: 4 splits -> unsplit
    assert (r[192]["fwd_splits"], r[193]["fwd_splits"]) == (4, 1)
    # dpcb: 5 splits -> unsplit
    assert (r[200]["dpcb_splits"], r[201]["dpcb_splits"]) == (5, 1)
    # pc_base weight gradient: 1 -> 2 slabs, the bias column through wgrad_reduce
    assert (r[256]["pcw_slabs"], r[257]["pcw_slabs"]) == (1, 2) and r[257]["pcw_G"] == 1
    assert r[336]["pcw_slabs"] == 2
    # dh: 5 splits -> unsplit with EpiAcc
    assert (r[960]["dh_splits"], r[961]["dh_splits"]) == (5, 1)
    # the logged run and the trainer's default sit in regimes of their own (dh at 84: 32 splits
    # asked, the 96-wide chunks of K = 2592 give 27)
    assert (r[84]["fwd_splits"], r[84]["dpcb_splits"], r[84]["dh_splits"], r[84]["pcw_slabs"]) == (6, 8, 27, 1)
    assert (r[336]["fwd_splits"], r[336]["dpcb_splits"], r[336]["dh_splits"]) == (1, 1, 11)
    # the W2 weight gradient always reduces slabs (one tile, n * 400 rows)
    assert all(r[n]["w2_slabs"] >= 2 for n in ns)
    # other action counts: one case below and one past the dpcb switch
    for n in (5, 201):
        assert {A for a, m, A, acc in uc.PC_A_CASES if m == n} == {1, 2, 7}
    assert _goal(5)["dpcb_splits"] > 1 and _goal(5)["w1_slabs"] == 2
    for n in uc.PC_TRAINER_N + uc.PC_DETERMINISM_N:
        assert _goal(n)


def test_bighouse_switches_have_both_sides():
    r = {n: uc.pc_regime("bighouse", n) for n in _ns(uc.BH_CASES, "bighouse") + [5]}
    assert [r[n]["w1_slabs"] for n in (1, 3, 4)] == [1, 1, 2]
    assert not any(v["items"] for v in r.values())  # 32 -> 8 channels: not on the parity-class kernel
    assert (r[200]["dpcb_splits"], r[201]["dpcb_splits"]) == (2, 1)  # K = 128: two chunks of two K tiles
    assert (r[200]["fwd_splits"], r[201]["fwd_splits"]) == (1, 1) and r[4]["fwd_splits"] > 1
    assert (r[201]["pcw_slabs"], r[257]["pcw_slabs"]) == (1, 2)
    assert r[1]["b1_blocks"] < uc.COLSUM_BLOCKS == r[200]["b1_blocks"]
    assert "w2_slabs" not in r[1]


def test_reward_prediction_switches_have_both_sides():
    for hw in ((174, 174), (300, 400)):
        r = {R: uc.rp_regime("goal", hw, R) for R in uc.RP_R}
        assert (r[64]["row_tiles"], r[65]["row_tiles"]) == (1, 2)
        assert (r[256]["w_slabs"], r[257]["w_slabs"], r[288]["w_slabs"]) == (1, 2, 2)
        assert all(v["fwd_splits"] > 1 for v in r.values())
    r = {R: uc.rp_regime("goal", (300, 400), R) for R in uc.RP_R}
    assert r[1]["K"] == 37536 and (r[64]["fwd_G"], r[65]["fwd_G"]) == (64, 32)
    assert uc.rp_regime("goal", (174, 174), 1)["K"] == 7776
    assert uc.rp_regime("goal", (84, 84), 1)["K"] == 864 and uc.rp_regime("bighouse", (84, 84), 1)["K"] == 4704
    for arch in ("goal", "bighouse"):
        r = {R: uc.rp_regime(arch, (84, 84), R) for R in (1, 65, 257)}
        assert (r[1]["row_tiles"], r[65]["row_tiles"]) == (1, 2) and (r[65]["w_slabs"], r[257]["w_slabs"]) == (1, 2)


def test_update_cases_hold_what_the_issue_sets():
    """tests/test_unreal_update_gpu.py: S < E in the small cases (rows t*E + e differ from
    t*S + e), >= 2 reward-prediction samples per env, an episode limit inside the rollout, frames
    the pixel-control crop fits in, and the bench leg's batch as the one larger case."""
    from oracle.update_checks import UNREAL_REWARDS, UPDATE_CASES, VISIBLE_IN
    assert list(UPDATE_CASES) == ["goal-174-aux", "goal-174-noaux", "goal-174-logged", "bighouse-84"]
    for name, c in UPDATE_CASES.items():
        assert c["T"] - 2 >= 2 and 1 <= c["max_steps"] < c["T"], name
        side = 20 if c["arch"] == "bighouse" else 42
        assert min(c["hw"]) >= 4 * side and min(c["hw"]) - 4 * side < 8, name  # the smallest instantiated frame
        assert set(VISIBLE_IN[c["arch"]]) == {"pc", "rp", "vr"}
        if name != "goal-174-logged":
            assert (c["E"], c["S"], c["T"]) == (5, 3, 6) and c["S"] < c["E"]
    lg = UPDATE_CASES["goal-174-logged"]
    assert (lg["E"], lg["S"], lg["T"], lg["aux_weight"]) == (4, 4, 20, 0.1)
    assert UPDATE_CASES["goal-174-aux"]["aux_weight"] == 0.1 and UPDATE_CASES["goal-174-noaux"]["aux_weight"] == 0
    assert UPDATE_CASES["bighouse-84"]["hw"] == (84, 84)
    goal, step, collision = UNREAL_REWARDS
    assert goal > 0 and step == 0 and collision < 0  # the three reward-prediction classes


def test_inputs_are_reproducible_and_mark_the_padding_logit():
    x, dout = uc.rp_inputs(5, 864)
    x2, dout2 = uc.rp_inputs(5, 864)
    assert (x == x2).all() and (dout == dout2).all() and (dout[:, 3] == 3.0).all()
    h, dq, dh0 = uc.pc_inputs(3, 7, 42)
    assert h.shape == (3, 512) and dq.shape == (3, 42, 42, 7) and dh0.shape == (3, 512)
    assert len(uc.regime_table()) == len(uc.PC_CASES + uc.PC_A_CASES + uc.BH_CASES) + len(uc.RP_CASES)
