"""The SYRK launch plan (csrc/gq_syrk_plan.hpp): the workspace sizes the library reports, the schedule the plan
lays out (through tests/syrk_plan_dump.cpp, plain host C++), and the uploaded words against digests recorded from the
launch function as it was before the plan existed."""
import os
import struct
import subprocess
import zlib
from collections import Counter
from types import SimpleNamespace

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc")
NONE = 0xFFFFFFFF
SLOT_BYTES = 256 * 256 * 4
DEFAULTS = dict(image=0, nosplit=0, gw=4, ck=256, wgs=0)

# gq_workspace_bytes(GQ_WS_H_ACCUMULATE, 0, C, T, 0), recorded from the library at f4766b2, before the bound became
# syrk_workspace_bytes: (T, C) -> bytes under the defaults, under syrk_image = 1 and under syrk_nosplit = 1
_RECORDED_H_WS = {
    (128, 256): (11360, 76896, 11360), (100, 256): (76888, 76888, 76888), (37, 384): (109656, 109656, 109656),
    (256, 384): (207976, 207976, 207976), (2048, 1024): (11552, 4205856, 11552), (8192, 2048): (37760880, 33566576, 12144),
    (8576, 2048): (37760904, 35139464, 12168), (8192, 4096): (134230672, 67121808, 12944),
    (262144, 4096): (134246544, 2147512464, 28816), (262144, 14336): (134258224, 7516233264, 40496),
    (200, 5888): (3028216, 3028216, 3028216),
}
# the options that must NOT change the value, each away from its default
_H_WS_NEUTRAL = [dict(syrk_gw=1), dict(syrk_gw=32), dict(syrk_ck=0), dict(syrk_ck=16), dict(syrk_wgs=64),
                 dict(syrk_gw=8, syrk_ck=1024, syrk_wgs=8)]


def test_h_accumulate_workspace_is_the_recorded_table_under_every_option():
    from gptq_gguf_toolkit_amd import _cabi

    def column():
        return {k: int(_cabi.lib().gq_workspace_bytes(_cabi.WS_H_ACCUMULATE, 0, k[1], k[0], 0)) for k in _RECORDED_H_WS}
    for col, setting in enumerate((dict(), dict(syrk_image=1), dict(syrk_nosplit=1))):
        want = {k: v[col] for k, v in _RECORDED_H_WS.items()}
        with _cabi.options(**setting):
            assert column() == want, setting
            for kv in _H_WS_NEUTRAL:
                with _cabi.options(**kv):
                    assert column() == want, (setting, kv)
    assert column() == {k: v[0] for k, v in _RECORDED_H_WS.items()}  # the options are back


# --------------------------------------------------------------------------- the plan, through the dump program
@pytest.fixture(scope="session")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("syrk_plan") / "syrk_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "syrk_plan_dump.cpp"), "-o", exe])
    return exe


def _run(exe, mode, kind, shapes, **opts):
    o = dict(DEFAULTS, **opts)
    args = [exe, mode, str(kind)] + [str(o[k]) for k in ("image", "nosplit", "gw", "ck", "wgs")] + ["%d,%d,%d" % s for s in shapes]
    plans = []
    for line in subprocess.check_output(args, text=True).splitlines():
        f = line.split()
        if f[0] == "plan":
            plans.append(SimpleNamespace(problems=[], words=[], opts=o, **{k: int(v) for k, v in zip(f[1::2], f[2::2])}))
        elif f[0] == "problem":
            plans[-1].problems.append(SimpleNamespace(**{k: int(v) for k, v in zip(f[2::2], f[3::2])}))
        elif f[0] == "words":
            plans[-1].words = [int(v) for v in f[1:]]
    return plans


_C3 = [(8576, 4096, 1)] * 3
_C1 = [(8576, 14336, 1)]
_C4 = _C3 + _C1
# name -> (kind, shapes (T, C, nseg), options away from the defaults)
GROUPS = {
    "a": (2, [(128, 256, 1)], {}),
    "b": (2, [(8576, 2048, 1)], {}),
    "c": (2, _C3, {}),
    "c1": (2, _C1, {}),
    "c4": (2, _C4, {}),
    "d": (2, [(8576, 4096, 1), (8576, 2304, 1), (8576, 2048, 1)], {}),
    "e": (2, [(16384, 4096, 8), (16384, 1024, 1)], {}),
    "f": (1, [(200, 5888, 1)], {}),
    "g": (0, [(37, 384, 1), (100, 128, 1)], {}),
    "h_gw1": (2, _C3, dict(gw=1)), "h_gw2": (2, _C3, dict(gw=2)), "h_gw8": (2, _C3, dict(gw=8)), "h_gw32": (2, _C3, dict(gw=32)),
    "h_nosplit": (2, _C3, dict(nosplit=1)),
    "h4_gw1": (2, _C4, dict(gw=1)), "h4_gw2": (2, _C4, dict(gw=2)), "h4_gw8": (2, _C4, dict(gw=8)), "h4_gw32": (2, _C4, dict(gw=32)),
    "h4_nosplit": (2, _C4, dict(nosplit=1)),
    "h1_gw1": (2, _C1, dict(gw=1)), "h1_gw2": (2, _C1, dict(gw=2)), "h1_gw8": (2, _C1, dict(gw=8)), "h1_gw32": (2, _C1, dict(gw=32)),
    "h1_nosplit": (2, _C1, dict(nosplit=1)),
}
# (sp, per_xcd, ck) by hand.  N tiles, R = N mod 256, s in 2 .. 8 with R s <= 512 minimising ceil(R s / 256) / s below 1:
# b: N = R = 36, s = 4 (0.25); c: N = 408, R = 152, s = 3 (0.67; 2: 1.0); c1: N = 1596, R = 60, s = 4 (0.25); c4: N = 2004,
# R = 212, s = 2 gives 1.0: none; d: N = R = 217, the same: none; e: N = R = 146, s = 3 (0.67).  per_xcd = 32 ceil(units / 256).
_EXPECT = {"a": (1, 32, 0), "b": (4, 32, 0), "c": (3, 96, 256), "c1": (4, 224, 256), "c4": (1, 256, 256), "d": (1, 32, 0),
           "e": (3, 64, 256), "f": (1, 64, 0), "h_nosplit": (1, 64, 256), "h1_nosplit": (1, 224, 256), "h4_nosplit": (1, 256, 256)}
for _g in (1, 2, 8, 32):
    _EXPECT.update({"h_gw%d" % _g: _EXPECT["c"], "h1_gw%d" % _g: _EXPECT["c1"], "h4_gw%d" % _g: _EXPECT["c4"]})
# CRC32 of the uploaded words (little-endian), recorded from the body of syrk16_launch at f4766b2 with its HIP calls stubbed
# and the table vector captured (block addresses null)
_RECORDED_CRC = {
    "a": 0x3142941e, "b": 0xd7fb72b8, "c": 0xc20f6eeb, "c1": 0x2f19628c, "c4": 0xc223d201, "d": 0xa4204d20, "e":
    0x3b357b31, "f": 0x40ccbc89, "g": 0x00000000, "h_gw1": 0x6a7087db, "h_gw2": 0x50c94a6a, "h_gw8": 0x9ad2ee10,
    "h_gw32": 0x0a2e6f27, "h_nosplit": 0xfdfdd912, "h4_gw1": 0x554a5935, "h4_gw2": 0xb7d548be, "h4_gw8": 0xf7367290,
    "h4_gw32": 0xb31996b5, "h4_nosplit": 0xc223d201, "h1_gw1": 0xc59aa689, "h1_gw2": 0x62cd99bf, "h1_gw8": 0xcec6f7de,
    "h1_gw32": 0x49744c2d, "h1_nosplit": 0xc3cf9715,
}


@pytest.fixture(scope="session")
def plans(dump_exe):
    return {name: _run(dump_exe, "plan", kind, shapes, **opts)[0] for name, (kind, shapes, opts) in GROUPS.items()}


def _crc(words):
    return zlib.crc32(struct.pack("<%dI" % len(words), *words))


@pytest.mark.parametrize("name", list(GROUPS))
def test_uploaded_words_are_the_recorded_ones(plans, name):
    assert _crc(plans[name].words) == _RECORDED_CRC[name]


@pytest.mark.parametrize("name", list(GROUPS))
def test_plan_properties(plans, name):
    kind, shapes, _ = GROUPS[name]
    pl = plans[name]
    P = pl.problems
    assert pl.kind == kind and pl.m == len(shapes) and [p.syrk_kind for p in P] == [kind] * len(shapes)
    tile = 256 if kind else 128
    for p, (T, C, nseg) in zip(P, shapes):
        assert p.Tp == -(-T // 128) * 128 and p.nt == C // tile
    # ---- the workspace: aligned where the launch function aligned it, areas in order and apart, below the bound
    at = 0
    for p, (T, C, nseg) in zip(P, shapes):
        assert p.img_off == at and p.img_off % 256 == 0
        assert p.img_bytes == (0 if kind == 2 else C * p.Tp * 2)
        at += -(-p.img_bytes // 256) * 256
    assert pl.img_end == at == pl.table_off and pl.table_off % 256 == 0
    end = pl.table_off + 4 * pl.n_words
    if pl.sp > 1:
        assert pl.partial_off % 256 == 0 and end <= pl.partial_off < end + 256
        assert pl.partial_bytes == pl.n_reduce * pl.sp * SLOT_BYTES
        end = pl.partial_off + pl.partial_bytes
    else:
        assert pl.partial_bytes == 0 and pl.n_reduce == 0 and pl.aux_word == pl.reduce_word == -1
    assert pl.total == end
    assert 256 + pl.total <= pl.bound  # the bound dominates
    if kind == 0:
        ns = [-(-p.nt // 8) for p in P]
        assert [p.tile_begin for p in P] == [sum(n * (n + 1) // 2 for n in ns[:k]) for k in range(len(P))]
        assert pl.total_tiles == sum(n * (n + 1) // 2 for n in ns) and pl.grid == -(-pl.total_tiles // 8) * 8 * 64 and pl.block == 256
        assert pl.n_words == 0 and pl.words == [] and pl.sp == 1 and pl.bar_word == -1 and pl.ck == 0
        return
    # ---- the upload: [table | aux | reduce list | rendezvous | pad | block addresses], in this order and apart
    tl, w = pl.tl, pl.words
    assert len(w) == pl.n_words and tl == 8 * pl.per_xcd and pl.per_xcd % 32 == 0
    at = 2 * tl
    if pl.sp > 1:
        assert (pl.aux_word, pl.reduce_word) == (tl, 2 * tl)
        at += 2 * pl.n_reduce
    persistent = kind == 2 and pl.per_xcd > 32
    assert (pl.bar_word != -1) == persistent
    if persistent:
        assert pl.bar_word == at and w[at:at + 16] == [0] * 16
        at += 16
    if at & 1:  # the pad word: block addresses are 8 bytes
        assert w[at] == NONE
        at += 1
    for p, (T, C, nseg) in zip(P, shapes):
        if nseg > 1:
            assert p.seg_word == at and at % 2 == 0 and w[at:at + 2 * nseg] == [0] * (2 * nseg) and p.hs_per_seg == T // nseg // 32
            at += 2 * nseg
        else:
            assert p.seg_word == -1 and p.hs_per_seg == 0
    assert at == len(w)
    assert pl.block == (512 if kind == 1 else 256) and pl.grid == (256 if persistent else 8 * pl.per_xcd)
    # ---- the schedule
    table, aux = w[:tl], w[tl:2 * tl]
    valid = {k << 24 | ti << 12 | tj for k, p in enumerate(P) for ti in range(p.nt) for tj in range(ti, p.nt)}
    assert all((t == NONE and a == NONE) or t in valid for t, a in zip(table, aux))  # empty entries are 0xffffffff
    units = [(t, a) for t, a in zip(table, aux) if t != NONE]
    count = Counter(t for t, _ in units)
    assert set(count) == valid
    reduce_list = {}
    if pl.sp > 1:
        rl = w[pl.reduce_word:pl.reduce_word + 2 * pl.n_reduce]
        reduce_list = dict(zip(rl[0::2], rl[1::2]))
        assert len(reduce_list) == pl.n_reduce
    slots = []
    for t in valid:
        auxes = sorted(a for u, a in units if u == t)
        if t not in reduce_list:
            assert auxes == [NONE], hex(t)  # exactly once, the whole token range
            continue
        first, sp = reduce_list[t] >> 8, reduce_list[t] & 255
        assert sp == pl.sp and auxes == [(first + k) << 12 | k << 6 | sp for k in range(sp)], hex(t)
        slots += range(first, first + sp)
    assert len(slots) == len(set(slots)) == pl.n_reduce * (pl.sp if pl.sp > 1 else 0)
    assert all(s < pl.partial_bytes // SLOT_BYTES for s in slots)
    assert pl.n_reduce * pl.sp <= 512
    rows = [sum(t != NONE for t in table[x * pl.per_xcd:(x + 1) * pl.per_xcd]) for x in range(8)]
    assert max(rows) - min(rows) <= 32
    for x in range(8):  # a row is filled from its start: no workgroup meets a hole before its last unit
        row = table[x * pl.per_xcd:(x + 1) * pl.per_xcd]
        assert all(t != NONE for t in row[:rows[x]]) and all(t == NONE for t in row[rows[x]:])
    # ---- when a split, and when checkpoints
    if pl.sp > 1:
        assert kind == 2 and not pl.opts["nosplit"] and all(T >= 8192 for T, _, _ in shapes)
        assert 2 <= pl.sp <= 8 and pl.n_reduce == len(valid) % 256
    if pl.ck:
        ck = pl.ck
        assert persistent and len({p.Tp for p in P}) == 1 and ck >= 16 and ck & (ck - 1) == 0 and P[0].Tp // 32 > ck
        assert pl.nck == (P[0].Tp // 32 - 1) // ck
    else:
        assert pl.nck == 0
    assert (pl.sp, pl.per_xcd, pl.ck) == _EXPECT[name]


def test_checkpoints_need_equal_token_counts_and_a_valid_option(dump_exe):
    two = [(8576, 4096, 1), (8576, 4096, 1), (8704, 4096, 1)]
    assert _run(dump_exe, "plan", 2, two)[0].ck == 0
    same = [(8576, 4096, 1)] * 3
    assert [_run(dump_exe, "plan", 2, same, ck=ck)[0].ck for ck in (0, 16, 128, 256, 512)] == [0, 16, 128, 256, 0]  # 8576 / 32 = 268
    assert [_run(dump_exe, "plan", 2, same, wgs=e)[0].grid for e in (0, 64, 100, 4, 4096)] == [256, 64, 96, 256, 256]


def test_the_bound_dominates_every_single_problem(dump_exe):
    shapes = [(T, C, 1) for C in range(256, 16384 + 1, 256) for T in (128, 8192, 8320, 262144)]
    split = 0
    for opts in (dict(), dict(gw=1), dict(gw=32)):
        got = _run(dump_exe, "sweep", 0, shapes, **opts)
        assert len(got) == len(shapes)
        for pl in got:
            assert pl.kind == 2 and 256 + pl.total <= pl.bound, (opts, pl.problems[0].T, pl.problems[0].C, pl.total, pl.bound)
            assert pl.n_reduce * pl.sp <= 512
            split += pl.sp > 1
    assert split > 100  # the sweep does reach the K-split


def test_the_bound_dominates_a_group_sorted_into_three_launches(dump_exe):
    # the group of test_h_accumulate_grouped_mixed_kinds_equal_single_calls: every launch starts at the next multiple of 256
    group = [(256, 512, 1), (200, 512, 1), (200, 384, 1), (256, 5888, 1)]
    single = _run(dump_exe, "sweep", 0, group)
    assert [pl.kind for pl in single] == [2, 1, 0, 2]
    launches = [_run(dump_exe, "plan", k, [s for s, pl in zip(group, single) if pl.kind == k])[0] for k in (2, 1, 0)]
    assert launches[0].bar_word != -1  # 276 + 3 tiles: the persistent form
    assert sum(255 + pl.total for pl in launches) <= sum(pl.bound for pl in single)
