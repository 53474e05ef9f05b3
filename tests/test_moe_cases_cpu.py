"""The pair sets of tests/moe_cases.py, pinned on the host (no GPU): what tests/test_gpu_moe_experts.py relies on -- which
experts, lanes and slots of linear_packed_experts_kernel's wave-wide search every set reaches, how many tiles it has, which tile
width the library takes for it -- so that a later edit of a set cannot empty a GPU test silently.  Also the search itself, lane
by lane as the kernel words it, against the plain loop over experts, and which sets tell a search that only works in lane 0."""
import pytest

import moe_cases as M
from test_moe_prefill_cpu import route_by_sort

torch = pytest.importorskip("torch")

_sets = {}


def pair_set(name):
    """(x_rows, ppr, ids, expert_start, order) of a set: drawn and routed once."""
    if name not in _sets:
        x_rows, ppr, ids = M.PAIR_SETS[name]()
        start, order = route_by_sort(torch.tensor(ids, dtype=torch.int32), M.EXPECT[name]["E"])
        _sets[name] = (x_rows, ppr, ids, start.tolist(), order.tolist())
    return _sets[name]


def widths(name):
    """The tile widths the set runs with: its own, and 128 as well for a wide set (Q4_K, Q5_K and IQ4_XS have no wide tile)."""
    return (256, 128) if M.EXPECT[name]["wide"] else (128,)


def wave_lookup(b, start, E, TT, offset=True, source=None):
    """The kernel's search, lane by lane: lane l reads the starts of experts 4 l .. 4 l + 4 at min(e, E), the lanes' tile counts
    are prefix-summed, the lowest lane whose range holds b walks its four experts.  -> (e, pos0, cnt) or None (no lane holds b).
    offset=False drops the `- (inc - s)` of the hit lane's walk and source=0 broadcasts lane 0's answer: two ways of a search
    that is right only while every tile is lane 0's."""
    st = [[start[min(M.PER * lane + k, E)] for k in range(M.PER + 1)] for lane in range(64)]
    nt = [[-(-(st[lane][k + 1] - st[lane][k]) // TT) for k in range(M.PER)] for lane in range(64)]
    inc, run = [], 0
    for lane in range(64):
        run += sum(nt[lane])
        inc.append(run)
    hit = [lane for lane in range(64) if inc[lane] - sum(nt[lane]) <= b < inc[lane]]
    if not hit:
        return None
    lane = hit[0] if source is None else source
    bb = b - (inc[lane] - sum(nt[lane])) if offset else b
    e = pos0 = cnt = 0
    found = False
    for k in range(M.PER):
        if not found and bb < nt[lane][k]:
            found, e, pos0 = True, M.PER * lane + k, st[lane][k] + bb * TT
            cnt = min(TT, st[lane][k + 1] - pos0)
        bb -= nt[lane][k]
    return e, pos0, cnt


def test_the_tables_name_every_set_and_every_type_meets_both_dtypes():
    assert set(M.PAIR_SETS) == set(M.EXPECT) and set(M.NARROW) | {"wide8", "wide9", "switch1023", "switch1024"} == set(M.PAIR_SETS)
    assert M.SMALL == ["mixtral", "skewed8", "tiny5", "qwen64", "masked8"] and M.MANY == ["each256", "last256", "last255"]
    seen = {(t, dt) for _, t, dt in M.GEMM_NARROW + M.GEMM_WIDE}
    assert seen == {(t, dt) for t in M.ALL8 for dt in (M.F16, M.BF16)}
    assert {n for n, _, _ in M.GEMM_NARROW} == set(M.NARROW) and {n for n, _, _ in M.GEMM_WIDE} == {"wide8", "wide9"}
    for n in M.MANY:  # two types: a 16-byte aligned K-quant, and Q8_0 or IQ4_NL
        assert sorted(t for s, t, _ in M.GEMM_NARROW if s == n) == [M.Q4, M.NL]
    for n in ("wide8", "wide9"):
        assert {t for s, t, _ in M.GEMM_WIDE if s == n} == set(M.WIDE_OK) | {M.Q4, M.XS}
    assert [M.lane_k(e) for e in (0, 3, 4, 8, 254, 255)] == [(0, 0), (0, 3), (1, 0), (2, 0), (63, 2), (63, 3)]


@pytest.mark.parametrize("name", list(M.PAIR_SETS))
def test_the_set_is_what_the_issue_states(name):
    x_rows, ppr, ids, start, order = pair_set(name)
    exp = M.EXPECT[name]
    E, P = exp["E"], len(ids)
    assert P == x_rows * ppr and M.PAIR_SETS[name]() == (x_rows, ppr, ids), "seeded: two draws are one"
    counts = {e: ids.count(e) for e in set(ids) if 0 <= e < E}
    stated = {"mixtral": (300, None), "skewed8": (700, M.SKEWED8), "tiny5": (80, None), "qwen64": (264, None),
              "each256": (256, {e: 1 for e in range(256)}), "last256": (130, {255: 130}), "last255": (130, {254: 130}),
              "masked8": (700, None), "wide8": (1280, M.WIDE8), "wide9": (1152, M.WIDE9), "switch1023": (1023, None),
              "switch1024": (1024, None)}[name]
    assert P == stated[0] and (stated[1] is None or counts == stated[1])
    assert (P >= 128 * E) == exp["wide"], "the library's choice of the tile width: P >= 128 E"
    if ppr > 1 and name != "wide8":  # a router's index: distinct experts per token
        assert all(len(set(ids[i:i + ppr])) == ppr for i in range(0, P, ppr))
    if name in ("mixtral", "tiny5"):
        assert set(counts) == set(range(E)), "every expert is named"
    if name == "wide8":
        assert ids.count(-1) == 134
    if name == "masked8":
        base = M.PAIR_SETS["skewed8"]()[2]
        changed = [p for p in range(P) if ids[p] != base[p]]
        assert len(changed) == 60 and {ids[p] for p in changed} == {-1, 8, 2 ** 30} and set(counts) == set(M.SKEWED8)
    if name.startswith("switch"):
        assert set(ids) == set(M.WIDE8) | {-1} and max(counts.values()) > 256


@pytest.mark.parametrize("name", list(M.PAIR_SETS))
def test_tile_of_yields_every_tile_once_in_expert_order(name):
    x_rows, ppr, ids, start, order = pair_set(name)
    exp = M.EXPECT[name]
    E, P = exp["E"], len(ids)
    for TT in widths(name):
        grid = M.grid_tiles(P, E, TT)
        tiles = [M.tile_of(b, start, TT) for b in range(grid)]
        real = [t for t in tiles if t is not None]
        assert tiles == real + [None] * (grid - len(real)), "every tile, then None"
        want = [(e, p0, min(TT, start[e + 1] - p0)) for e in range(E) for p0 in range(start[e], start[e + 1], TT)]
        assert real == want and len(set(real)) == len(real) and M.tile_of(grid, start, TT) is None
        assert len(real) <= grid, "the host's grid holds every tile"
        assert sum(cnt for _, _, cnt in real) == start[E] == sum(0 <= e < E for e in ids)
        if TT == widths(name)[0]:
            assert exp["tiles"] in (None, len(real)), len(real)
            assert len(real) < grid, "some workgroups find no tile: the early return"
            slots = {M.lane_k(e) for e, _, _ in real}
            if "slots" in exp:
                assert slots == exp["slots"], sorted(slots)
            else:
                assert {lane for lane, _ in slots} == exp["lanes"] and len({k for _, k in slots}) == M.PER
        # masked ids appear in no run, and every pair of a tile names the tile's expert
        for e, p0, cnt in real:
            assert all(ids[p] == e for p in order[p0:p0 + cnt])
        assert all(p == -1 for p in order[start[E]:]) and sorted(order[:start[E]]) == [p for p, e in enumerate(ids) if 0 <= e < E]


def test_the_sets_reach_what_e_le_4_cannot():
    lanes = {n: {M.lane_k(e)[0] for e in set(pair_set(n)[2]) if 0 <= e < M.EXPECT[n]["E"]} for n in M.PAIR_SETS}
    assert lanes["mixtral"] == {0, 1} and lanes["tiny5"] == {0, 1} and lanes["skewed8"] == {0, 1} and lanes["wide9"] == {0, 1, 2}
    assert lanes["qwen64"] == set(range(16)) and lanes["each256"] == set(range(64)) and lanes["last256"] == lanes["last255"] == {63}
    # skewed8: the empty experts sit inside the hit lane (2, 3 after 0, 1) and at the head of lane 1 (4 before 5)
    assert all(e not in M.SKEWED8 for e in (2, 3, 4))
    # tiny5, last255: E is no multiple of 4, so a lane other than lane 0 reads past E and is clamped
    assert M.EXPECT["tiny5"]["E"] % M.PER and M.EXPECT["last255"]["E"] % M.PER
    # each256 has fewer pairs than 128 E: the narrow tile, and the grid's bound is far above its 256 tiles
    assert len(pair_set("each256")[2]) == 256 < 128 * 256 and M.grid_tiles(256, 256, 128) == 258


@pytest.mark.parametrize("name", list(M.PAIR_SETS))
def test_the_lane_wise_search_is_tile_of_and_a_lane_0_search_is_not(name):
    """The kernel's search restated lane by lane gives tile_of's answer for every workgroup of the grid.  The same search
    without the hit lane's offset differs on every set with tiles in two lanes; with lane 0's answer broadcast it differs on
    every set with a tile outside lane 0 -- all of them: a grouped GEMM whose search is right for E <= 4 only passes none of
    the GPU cases."""
    x_rows, ppr, ids, start, order = pair_set(name)
    E, P = M.EXPECT[name]["E"], len(ids)
    for TT in widths(name):
        grid = range(M.grid_tiles(P, E, TT))
        want = [M.tile_of(b, start, TT) for b in grid]
        assert [wave_lookup(b, start, E, TT) for b in grid] == want
        no_offset = [wave_lookup(b, start, E, TT, offset=False) for b in grid] != want
        lane0 = [wave_lookup(b, start, E, TT, source=0) for b in grid] != want
        assert lane0
        assert no_offset == (name not in ("last256", "last255")), "one populated lane: nothing precedes it"
