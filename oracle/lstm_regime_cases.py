"""Case tables of the recurrent core's regime tests and the launch rules they rest on (TEST
INFRASTRUCTURE ONLY — see oracle/__init__.py).

lstm_forward_step / heads_forward / lstm_backward of csrc/vn_policy.hip choose the form of their
products from the env count E, the row count T E and the action count A alone. Above kSkinnyRows =
16 envs every product runs on the generic helpers, whose rules oracle/unreal_head_cases.py restates
(splitk_count and the two lines after it, the slab count of launch_wgrad / launch_wgrad_x6t, the
lanes per output of launch_splitk_epilogue / launch_wgrad_reduce). lstm_regime(E, T, A) feeds them
the core's shapes (xcat = roundup4(512 + A + 1) + 512, xoff = xcat - 512):

  gates  xcat x W_cat^T + b_ih + b_hh   launch_gemm_x6_sk<128, 128>   M = E      N = 2048  K = xcat
         (EpiBias2; the last k-columns are W_hh's: at 9 slabs of 128 the last slab holds xcat - 1024)
  dh     m (dgates x W_hh)              launch_gemm_x6_sk<64, 64, BKN 64>  M = E  N = 512   K = 2048
         (EpiLstmDh: the mask enters through pre_row in the split epilogue)
  dz5    relu' (dgates x W_ih[:, :512]) launch_gemm_x6_sk<128, 128>   M = T E    N = 512   K = 2048
  wcat   dgates^T x [xcat | 1]          launch_wgrad_x6t<128, 128>    M = 2048   N = xcat + 1, P = T E rows
         (b_ih and b_hh share the bias column: db2 of EpiWgrad / launch_wgrad_reduce)
  headw  dout^T x [h | 1]               launch_wgrad<32, 64>          M = A + 1  N = 513,      P = T E rows
  headf  h x W_head^T + b               launch_gemm_sk<64, 16>        M = T E    N = A + 1 K = 512

SWITCHES[T] names every E in 19..1030 at which a product changes form at T steps, found from the
inequalities of the launch code (switch_candidates: a new row tile, splits M N passing sk_cap,
M N reaching the flat reduce, and for the weight gradients the row counts 32 j + 1 at which one of
their ceiling divisions can move) — tests/test_lstm_regime_cases.py asserts that a scan of every E
finds the same list. CASES is a cover: every value of every key of cover_keys that occurs for E in
18..1030 and T in {1, 3} occurs in some case; the dh keys count at T = 3 only, since at T = 1 nothing
reads dh. VARIANT_CASES are the calling forms that only the
few-env tests ran against float64 (other action counts, NULL arguments, vn_lstm_backward_ex below
full width, T = 2), each placed above 16 envs. inputs() draws a case's tensors on the CPU, so
tests/test_lstm_regime_cases.py can show in float64 that they expose the faults these regimes can
hide; tests/test_lstm_regimes_gpu.py runs the cases through oracle/trunk_checks.py
lstm_core_check. numpy only: nothing here needs the GPU.

Not covered (the test named stands on the far side where there is one):
- E above 1030: tests/test_prod_oracle_gpu.py runs E = 2048, T = 3 (6144 rows: dz5 unsplit, dW_cat
  on 7 slabs, the heads' weight gradient on 24 slabs and 4 reduce lanes); nothing runs between.
- T above 3 at the core's own level: rows above 3090, so dW_cat's 7-slab form and dz5's unsplit form
  (from 3969 rows) run at E = 2048 only; the trainer cases of tests/test_lstm_regimes_gpu.py run
  T = 4 and 6 at E = 20 and 136.
- The VN_LSTM_WG_TRANSPOSED form of dW_cat (an A/B switch read from the environment):
  tests/test_lstm_gpu.py compares it with the default form, not with a reference.
- 174x174 and 300x400 policies: the core does not depend on the frame size (the table has no
  geometry argument); tests/test_prod_oracle_gpu.py's logged-run update runs it behind a 174x174 trunk
  at 4 envs.
- headf is one form (8 slabs of 64, 1 lane) below 4673 rows; it is in the table to say so.
"""
import functools

import numpy as np

from . import few_env_cases as fc
from .unreal_head_cases import BK, REDUCE_FLAT, SK_CAP, reduce_lanes, splitk_chunk, wgrad_chunk

FIRST_E = fc.SKINNY_ROWS + 2     # 18: the first E the few-env tests leave (they end at 17)
LAST_E = 1030
STEPS = (1, 3)                   # T of CASES and SWITCHES
HID, GATES = 512, 2048
TILE = {"gates": (128, 128), "dh": (64, 64), "dz5": (128, 128), "wcat": (128, 128), "headw": (32, 64), "headf": (64, 16)}


def _cdiv(a, b):
    return (a + b - 1) // b


def layout(A):
    """(lin, xoff, xcat) of vn_policy_lstm_info at A actions."""
    lin = HID + A + 1
    xoff = (lin + 3) // 4 * 4
    return lin, xoff, xoff + HID


def _split(M, N, K, tile):
    slabs, kchunk = splitk_chunk(M, N, K, *tile)
    return {"slabs": slabs, "kchunk": kchunk, "last": K - (slabs - 1) * kchunk,
            "lanes": reduce_lanes(M, N, slabs) if slabs > 1 else 0, "row_tiles": _cdiv(M, tile[0]), "rem": M % tile[0]}


def _wgrad(M, KP, P, tile):
    slabs, kchunk = wgrad_chunk(M, KP, P, tile[0], tile[1], True)
    return {"slabs": slabs, "kchunk": kchunk, "last": P - (slabs - 1) * kchunk,
            "lanes": reduce_lanes(M, KP + 1, slabs) if slabs > 1 else 0}


def lstm_regime(E, T, A=4):
    """The regime of every product of the core at E > 16 envs, T steps, A actions: {product: {...}}.

    gates, dh, dz5, headf (split-K): slabs (1: the unsplit kernel with its own epilogue), kchunk and
    last (the slab length along K and that of the last slab), lanes (epilogue lanes per output, 0
    unsplit), row_tiles and rem (rows left over against the row tile).
    wcat, headw (weight gradients over P = T E rows): slabs (1: the direct EpiWgrad epilogue), kchunk
    and last along the rows, lanes of launch_wgrad_reduce (0 direct)."""
    _, _, xcat = layout(A)
    N = T * E
    return {"gates": _split(E, GATES, xcat, TILE["gates"]),
            "dh": _split(E, HID, GATES, TILE["dh"]),
            "dz5": _split(N, HID, GATES, TILE["dz5"]),
            "wcat": _wgrad(GATES, xcat, N, TILE["wcat"]),
            "headw": _wgrad(A + 1, HID, N, TILE["headw"]),
            "headf": _split(N, A + 1, HID, TILE["headf"])}


@functools.lru_cache(maxsize=None)
def _regime4(E, T):
    return lstm_regime(E, T, 4)


# ---- the switches ---------------------------------------------------------------------------
def form(E, T, A=4):
    """{product: the part of its regime that is a change of form}: slab count and slab length, lanes,
    and for the per-step products the row tiles up to 3 (one tile, two, a tile with tiles on both
    sides). Remainders and the last slab's length move with every E and are keys of the cover."""
    r = _regime4(E, T) if A == 4 else lstm_regime(E, T, A)
    return {"gates": (r["gates"]["slabs"], r["gates"]["kchunk"], r["gates"]["lanes"], min(r["gates"]["row_tiles"], 3)),
            "dh": (r["dh"]["slabs"], r["dh"]["kchunk"], r["dh"]["lanes"], min(r["dh"]["row_tiles"], 3)),
            "dz5": (r["dz5"]["slabs"], r["dz5"]["kchunk"], r["dz5"]["lanes"]),
            "wcat": (r["wcat"]["slabs"],),
            "headw": (r["headw"]["slabs"], r["headw"]["lanes"]),
            "headf": (r["headf"]["slabs"], r["headf"]["lanes"])}


def _split_candidates(N, K, BM, hi):
    """The row counts M in 2..hi at which a launch_gemm_x6_sk / launch_gemm_sk product of N columns
    and K can change form, from splitk_count and launch_splitk_epilogue:
      tiles = cdiv(M, BM) cdiv(N, BN) moves at M = BM k + 1, and with it the 512-workgroup target
        cdiv(512, tiles) and the cut tiles >= 128;
      `while (splits > 1 && splits * M * N > sk_cap) --splits` first bites for a count s at
        M = sk_cap / (N s) + 1 (s up to K / (2 BK), the most splits a product can start from);
      the epilogue's lanes drop to 1 at M N >= 65536: M = cdiv(65536, N)."""
    c = {BM * k + 1 for k in range(1, hi // BM + 1)}
    c |= {SK_CAP // (N * s) + 1 for s in range(2, K // (2 * BK) + 1)}
    c.add(_cdiv(REDUCE_FLAT, N))
    return {m for m in c if 2 <= m <= hi}


def _wgrad_candidates(hi):
    """The row counts P in 2..hi at which launch_wgrad / launch_wgrad_x6t can change form: every
    quantity there is a ceiling division of P — (P + 255) / 256, (P + splits - 1) / splits rounded up
    to BK = 32 (it passes 32 j at P = 32 j splits + 1) and the recount (P + kchunk - 1) / kchunk with
    kchunk a multiple of 32 — so a change needs P = 32 j + 1. The halving `while (splits * M * N >
    slab_cap) splits /= 2` depends on P through splits = min(.., cdiv(P, 256)) alone: for dW_cat
    splits * 2048 * (xcat + 1) > 24 << 20 holds from 12 splits on, first at P = 11 * 256 + 1."""
    return {p for p in range(33, hi + 1, 32)}


def switch_candidates(T, A=4):
    """The E in FIRST_E + 1 .. LAST_E at which some product may change form at T steps."""
    _, _, xcat = layout(A)
    rows = LAST_E * T
    per_step = _split_candidates(GATES, xcat, TILE["gates"][0], LAST_E) | _split_candidates(HID, GATES, TILE["dh"][0], LAST_E)
    per_rows = (_split_candidates(HID, GATES, TILE["dz5"][0], rows) | _split_candidates(A + 1, HID, TILE["headf"][0], rows)
                | _wgrad_candidates(rows))
    c = per_step | {_cdiv(p, T) for p in per_rows}    # rows T (E - 1) < p <= T E
    return sorted(e for e in c if FIRST_E < e <= LAST_E)


@functools.lru_cache(maxsize=None)
def switches(T):
    """((E, (products that change form between E - 1 and E)), ...) at T steps, from the candidates."""
    out = []
    for e in switch_candidates(T):
        a, b = form(e - 1, T), form(e, T)
        changed = tuple(p for p in a if a[p] != b[p])
        if changed:
            out.append((e, changed))
    return tuple(out)


def scan_switches(T):
    """The same list from a scan of every E (the CPU test compares the two)."""
    out = []
    for e in range(FIRST_E + 1, LAST_E + 1):
        a, b = form(e - 1, T), form(e, T)
        changed = tuple(p for p in a if a[p] != b[p])
        if changed:
            out.append((e, changed))
    return tuple(out)


SWITCHES = {T: switches(T) for T in STEPS}


# ---- the cover ------------------------------------------------------------------------------
def cover_keys(E, T, A=4):
    """The set of (key, value) pairs a case (E, T) holds. The dh keys count for T >= 2 only: dh_{t-1} = m_t
    (dgates_t x W_hh) is launched at every step, but its only reader is the cell backward of step t - 1, so
    at T = 1 no output depends on it and a case there cannot see it wrong."""
    r = _regime4(E, T) if A == 4 else lstm_regime(E, T, A)
    g, d, z, w, hw = r["gates"], r["dh"], r["dz5"], r["wcat"], r["headw"]
    keys = {("gates slabs", g["slabs"]), ("gates lanes", g["lanes"]), ("gates last slab < BK", g["last"] < BK),
            ("gates split, row tiles, remainder", (g["slabs"] > 1, min(g["row_tiles"], 3), g["rem"] != 0)),
            ("dz5 slabs", z["slabs"]), ("dz5 lanes", z["lanes"]), ("dz5 split, remainder", (z["slabs"] > 1, z["rem"] != 0)),
            ("wcat slabs", w["slabs"]),
            ("wcat split, last slab part filled, its length no multiple of 32",
             (w["slabs"] > 1, w["last"] < w["kchunk"], w["last"] % BK != 0)),
            ("headw slabs", hw["slabs"]), ("headw lanes", hw["lanes"])}
    if T >= 2:
        keys |= {("dh slabs", d["slabs"]), ("dh lanes", d["lanes"]),
                 ("dh split, row tiles, remainder", (d["slabs"] > 1, min(d["row_tiles"], 3), d["rem"] != 0))}
    return keys


@functools.lru_cache(maxsize=None)
def all_keys():
    """Every (key, value) that occurs for E in FIRST_E..LAST_E and T in STEPS."""
    out = set()
    for T in STEPS:
        for E in range(FIRST_E, LAST_E + 1):
            out |= cover_keys(E, T)
    return frozenset(out)


def uncovered(cases):
    """The (key, value) pairs of all_keys() that no case of the list holds."""
    have = set()
    for E, T in cases:
        have |= cover_keys(E, T)
    return sorted(all_keys() - have, key=repr)


def greedy_cover(first=((192, 1),)):
    """A cover by the greedy rule (most new pairs first, the smaller rows T E then the smaller E on a
    tie) after the cases of `first` (192 envs x 1 step: the short last gates slab at the E the CPU fault
    check names), then every case dropped that the others make redundant."""
    want, chosen = set(all_keys()), list(first)
    cand = [(E, T) for T in STEPS for E in range(FIRST_E, LAST_E + 1)]
    keys = {c: cover_keys(*c) for c in cand}
    for c in chosen:
        want -= keys[c]
    while want:
        best = max(cand, key=lambda c: (len(keys[c] & want), -c[0] * c[1], -c[0]))
        chosen.append(best)
        want -= keys[best]
    for c in sorted(chosen, key=lambda c: -c[0] * c[1]):
        rest = [x for x in chosen if x != c]
        if not uncovered(rest):
            chosen = rest
    return sorted(chosen)


# greedy_cover() (tests/test_lstm_regime_cases.py asserts that it is a cover, that every case is needed and
# that there are at most MAX_CASES)
CASES = [(18, 3), (64, 3), (86, 3), (128, 3), (171, 3), (192, 1), (256, 3), (288, 3), (293, 1), (384, 3), (427, 3),
         (513, 3), (598, 3), (631, 1), (683, 3), (769, 3), (897, 3), (1024, 3), (1025, 3)]
MAX_CASES = 26
CASE_IDS = ["E%d-T%d" % c for c in CASES]

# ---- the calling forms: (E, T, A, null_args, extra_envs) -------------------------------------
ACTION_COUNTS = fc.ACTION_COUNTS      # 1, 3, 7 besides 4
ACTION_E = 40                          # one row tile everywhere, gates on 11 slabs
SHORT_SLAB_E, SHORT_SLAB_A = 192, 1    # gates on 9 slabs of 128: A = 4 leaves 8 k-columns, A = 1 (xcat 1028) 4
VARIANT_CASES = ([(ACTION_E, 3, A, False, 0) for A in ACTION_COUNTS]
                 + [(SHORT_SLAB_E, 3, SHORT_SLAB_A, False, 0)]
                 + [(18, 3, 4, True, 0), (300, 3, 4, True, 0)]
                 + [(40, 3, 4, False, 5), (300, 3, 4, False, 16)]      # 16: the 174 bench leg's unreal_envs
                 + [(130, 2, 4, False, 0)])                           # one BPTT hop; dh on 22 slabs, 3 row tiles, 2 rows in the last
VARIANT_IDS = ["E%d-T%d-A%d%s%s" % (E, T, A, "-null" if nul else "", "-extra%d" % x if x else "")
               for E, T, A, nul, x in VARIANT_CASES]

# the cases at which tests/test_lstm_regime_cases.py restates each fault in float64
FAULT_GATES_SLAB = (192, 1)      # 1. the last gates slab (8 k-columns) dropped
FAULT_DH_SLAB = (769, 3)         # 2. the last dh slab dropped (5 slabs of 416, the last 384: the widest margin of the T = 3 cases)
FAULT_DH_MASK = (384, 3)         # 3. the mask taken as 1 in the dh epilogue (the widest margin likewise)
TRAINER_CASES = [(20, 4), (136, 4), (20, 6)]   # (E, T) of the whole-update cases of tests/test_lstm_regimes_gpu.py
FAULT_WCAT_SLAB = (1025, 3)      # 4. the last, part-filled dW_cat slab dropped (its length no multiple of 32)
FAULT_DB2 = (293, 1)             # 5. b_hh's gradient left unwritten: a split dW_cat, the db2 path of the reduce
FAULT_EXTRA = (40, 3, 4, False, 5)   # 6. the rows e >= S also given dh_extra


def regime_table(cases=None):
    """The regimes of the cases as text rows (DESIGN.md holds a copy)."""
    rows = []
    for c in (cases if cases is not None else [(E, T, 4) for E, T in CASES] + [(E, T, A) for E, T, A, _, _ in VARIANT_CASES]):
        E, T, A = c
        r = lstm_regime(E, T, A)
        g, d, z, w, hw = r["gates"], r["dh"], r["dz5"], r["wcat"], r["headw"]
        rows.append("E=%-4d T=%d A=%d  gates %2dx%-4d (last %4d, lanes %d, tiles %d rem %3d)  dh %2dx%-4d (last %4d, lanes %d, "
                    "tiles %2d rem %2d)  dz5 %2dx%-4d (lanes %d, rem %3d)  wcat %2dx%-4d (last %3d)  headw %2d (lanes %d)"
                    % (E, T, A, g["slabs"], g["kchunk"], g["last"], g["lanes"], g["row_tiles"], g["rem"], d["slabs"],
                       d["kchunk"], d["last"], d["lanes"], d["row_tiles"], d["rem"], z["slabs"], z["kchunk"], z["lanes"],
                       z["rem"], w["slabs"], w["kchunk"], w["last"], hw["slabs"], hw["lanes"]))
    return rows


# ---- seeded inputs --------------------------------------------------------------------------
RESET_RATE = 0.05
# Seeds of the CPU fault checks' parameter draws. They follow the law of lstm_core_check's parameters (init_params
# + N(0, 0.01)), not its values: the GPU test's come from PolicyNet.init_params(3) over the flat buffer, which
# needs the library. The fault checks hold for each of these draws.
WEIGHT_SEEDS = (2, 3)


def _rng(*key):
    return np.random.RandomState([20251021] + [int(k) for k in key])


def resets(E, T):
    """The placed resets [(t, e)]: few_env_cases.lstm_resets (env 0 at t = 0, env E - 1 at t = T - 1, env
    E // 2 at t = 1 where T >= 3) and, for T >= 2, env 1 at t = 1. dh_{t-1} = m_t (dgates_t x W_hh) is
    used for t >= 1 only, so these put a zero of EpiLstmDh's mask into the first 64-row tile of dh (env 1)
    and into the last (env E - 1 at t = T - 1 >= 1)."""
    out = list(fc.lstm_resets(E, T))
    if T >= 2:
        out.append((1, 1))
    return out


def masks(E, T):
    """float32 [T, E] of 0 / 1: the placed resets and RESET_RATE drawn ones."""
    m = fc.lstm_masks(E, T)
    m[_rng(2, E, T).random_sample((T, E)) < RESET_RATE] = 0.0
    for t, e in resets(E, T):
        m[t, e] = 0.0
    return m


def inputs(E, T, A=4, S=0):
    """The tensors of one case, as lstm_core_check(inputs=...) takes them: x5 [T E, 512] = relu(N(0, 1)),
    lra [T, E, A + 1] (one-hot last action, a reward flag in a tenth of the rows; zero where the env is
    reset), masks [T, E], h0 and c0 [E, 512] = N(0, 0.25), actions int32 [T E], rets [T E] = N(0, 1),
    dh_extra [T, S, 512] = N(0, 0.01) (None for S = 0). float32 unless stated."""
    N = T * E
    rng = _rng(1, E, T, A)
    x5 = np.maximum(rng.standard_normal((N, HID)), 0.0).astype(np.float32)
    lra = np.zeros((T, E, A + 1), dtype=np.float32)
    a_last = rng.randint(0, A, size=(T, E))
    np.put_along_axis(lra, a_last[..., None], 1.0, axis=2)
    lra[..., A] = (rng.random_sample((T, E)) < 0.1).astype(np.float32)
    m = masks(E, T)
    lra *= m[..., None]
    h0 = (rng.standard_normal((E, HID)) * 0.5).astype(np.float32)
    c0 = (rng.standard_normal((E, HID)) * 0.5).astype(np.float32)
    actions = rng.randint(0, A, size=N).astype(np.int32)
    rets = rng.standard_normal(N).astype(np.float32)
    dhx = (_rng(3, E, T, S).standard_normal((T, S, HID)) * 0.1).astype(np.float32) if S else None
    return {"x5": x5, "lra": lra, "masks": m, "h0": h0, "c0": c0, "actions": actions, "rets": rets, "dh_extra": dhx}
