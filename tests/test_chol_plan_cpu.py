"""The plan of the Cholesky chain (csrc/gq_chol_plan.hpp, DESIGN.md K2+K3), through tests/chol_plan_dump.cpp (plain host
C++): the steps and regimes against a recursion stated here, the uploaded words and the workspace sizes the library reports
against tables recorded from gq_cholesky.hip as it was before the plan existed (cc07dad), and the layout of the workspace."""
import os
import struct
import subprocess
import zlib
from types import SimpleNamespace

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc")
NB = 128
PARTIAL_BYTES = 1024 * 256 * 256 * 4
# 1152 (blocks 4 | 5: the top node cannot take images, its left child 256 | 256 could) is the one width where the rule "no
# images anywhere unless the top node takes them" decides a regime
WIDTHS = [128, 256, 384, 512, 640, 1024, 1152, 1280, 1536, 2048, 3584, 4096, 4992, 7168, 14336, 28672]
DEFAULTS = dict(p3_min=1792, b3_min=1024, planes=2, fp32=0, no_pair=0, max64=256)
# name -> (the plan's options away from the defaults, the same as library options)
SETS = {
    "default": ({}, {}),
    "3p_min0": (dict(p3_min=0), dict(chol_3p_min=0)),
    "3p_min128": (dict(p3_min=128), dict(chol_3p_min=128)),
    "planes3": (dict(planes=3), dict(chol_planes=3)),
    "fp32": (dict(fp32=1, p3_min=0), dict(chol_fp32=1, chol_3p_min=0)),
    "no_pair": (dict(no_pair=1), dict(chol_no_pair=1)),
    "g64max0": (dict(max64=0), dict(gemm32_64_max=0)),
}
LEAF, FRONT, BACK = 0, 1, 2
IMAGE, SPLIT_BF16, FP32, FP32_PAIR = 0, 1, 2, 3

# gq_workspace_bytes(GQ_WS_H_PREPARE, 64, C, 0, 0) for C in WIDTHS, recorded from the library at cc07dad
_RECORDED_H_WS = {
    "default": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 396981856, 436317696,
                199391488, 782453848, 2324135240, 8490443792],
    "3p_min0": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 102782976, 134243328,
                199391488, 411085824, 1644254208, 6576841728],
    "3p_min128": [132864, 526848, 1182976, 271074928, 3281664, 278957280, 10624768, 13115904, 292070256, 310453024, 396994592,
                  436369472, 199391488, 782479320, 2324186184, 8490545680],
    "planes3": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 409826736, 453095024,
                199391488, 833833904, 2529655984, 9312527088],
    "fp32": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 102782976, 134243328,
             199391488, 411085824, 1644254208, 6576841728],
    "no_pair": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 396981856, 436317696,
                199391488, 782453848, 2324135240, 8490443792],
    "g64max0": [132864, 526848, 1182976, 2101248, 3281664, 8395776, 10624768, 13115904, 18884608, 33567744, 396981856, 436317696,
                199391488, 782453848, 2324135240, 8490443792],
}
# gq_workspace_bytes(GQ_WS_CHOL_GEMM, M, N, K, 0) at the shapes of test_chol_gemm_against_fp64, recorded at cc07dad
_RECORDED_GEMM_WS = {(512, 512, 512): 271594592, (1024, 1024, 1024): 281041504, (512, 768, 640): 273366400,
                     (1024, 768, 640): 275337344}
# (C, chol_3p_min, chol_planes) -> (words, CRC32 of the words, little-endian) of P3Plans::words at cc07dad, written out by
# p3_plans_for under gq_workspace_bytes: every combination of the grid that has image nodes
_RECORDED_WORDS = {
    (512, 128, 2): (796, 0x53de2c11), (1024, 128, 2): (2488, 0x9def2d52), (1536, 128, 2): (1116, 0x1eae6749),
    (2048, 128, 2): (6472, 0x4853ceda), (3584, 128, 2): (6536, 0xd43737a9), (3584, 1792, 2): (3352, 0xedfac907),
    (3584, 1792, 3): (3308, 0x88788e4c), (4096, 128, 2): (17040, 0x48203752), (4096, 1792, 2): (4096, 0xb7087376),
    (4096, 1792, 3): (4124, 0x7f21340d), (7168, 128, 2): (20086, 0xedd6630e), (7168, 1792, 2): (13718, 0xedcfe584),
    (7168, 1792, 3): (13676, 0xcfe98c83), (14336, 128, 2): (55698, 0x68f069db), (14336, 1792, 2): (42962, 0xd5b2d7ed),
    (14336, 1792, 3): (42924, 0x1cb2cd89), (28672, 128, 2): (160004, 0xf4f3dac7), (28672, 1792, 2): (134532, 0x95edc033),
    (28672, 1792, 3): (134460, 0x91ef25e9),
}


@pytest.fixture(scope="session")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chol_plan") / "chol_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "chol_plan_dump.cpp"), "-o", exe])
    return exe


def _fields(f):
    return {k: int(v) for k, v in zip(f[0::2], f[1::2])}


@pytest.fixture(scope="session")
def plans(dump_exe):
    """(option set, C) -> the plan"""
    out = {}
    for name, (kv, _) in SETS.items():
        o = SimpleNamespace(**dict(DEFAULTS, **kv))
        args = [dump_exe, "plan"] + [str(getattr(o, k)) for k in ("p3_min", "b3_min", "planes", "fp32", "no_pair", "max64")]
        pl = None
        for line in subprocess.check_output(args + [str(C) for C in WIDTHS], text=True).splitlines():
            f = line.split()
            if f[0] == "plan":
                pl = SimpleNamespace(opts=o, steps=[], nodes=[], gemms=[], words=[], **_fields(f[1:]))
                out[name, pl.C] = pl
            elif f[0] == "steps":
                pl.steps = [tuple(int(x) for x in s.split(":")) for s in f[1:]]
            elif f[0] == "node":
                pl.nodes.append(SimpleNamespace(**_fields(f[1:])))
            elif f[0] == "gemm":
                pl.gemms.append(SimpleNamespace(shapes=[tuple(int(x) for x in s.split(",")) for s in f[8:]], **_fields(f[1:7])))
            elif f[0] == "words":
                pl.words = [int(v) for v in f[1:]]
    assert len(out) == len(SETS) * len(WIDTHS)
    return out


GRID = [(name, C) for name in SETS for C in WIDTHS]


# --------------------------------------------------------------------------- 1. steps
def _expected_steps(C, o):
    """The rules of the recursion as gq_cholesky.hip stated them at cc07dad (p3_used, p3_node, min3b under chol_fp32, the
    pair expression with gemm32_uses_64_full), independently of the header.  -> (steps, nodes)"""
    def p3(n1, n2):
        return o.p3_min > 0 and n1 >= o.p3_min and n2 >= o.p3_min and n1 % 256 == 0 and n2 % 256 == 0

    def full64(M, N, K, lower):
        return -(-M // 128) * -(-N // 128) // (2 if lower else 1) < o.max64 and M % 64 == 0 and N % 64 == 0 and K % 32 == 0
    nblk = C // NB
    images = nblk >= 2 and p3(nblk // 2 * NB, (nblk - nblk // 2) * NB)
    steps, nodes = [], []

    def rec(lo, hi):
        if hi - lo == 1:
            return steps.append((LEAF, lo))
        mid = (lo + hi) // 2
        n1, n2 = (mid - lo) * NB, (hi - mid) * NB
        rec(lo, mid)
        if images and p3(n1, n2):
            regime = IMAGE
        elif min(n1, n2) >= (1 << 40 if o.fp32 else o.b3_min):
            regime = SPLIT_BF16
        elif not o.no_pair and C % 4 == 0 and full64(n2, n2, n1, True) and full64(n2, n1, n1, False):
            regime = FP32_PAIR
        else:
            regime = FP32
        nodes.append((lo, mid, hi, regime))
        i = len(nodes) - 1
        steps.append((FRONT, i))
        rec(mid, hi)
        steps.append((BACK, i))
    rec(0, nblk)
    return steps, nodes


def _regimes_by_half(pl):
    """{(n1, n2): {regimes}} over the plan's nodes"""
    out = {}
    for n in pl.nodes:
        out.setdefault(((n.mid - n.lo) * NB, (n.hi - n.mid) * NB), set()).add(n.regime)
    return out


@pytest.mark.parametrize("name,C", GRID)
def test_steps_are_the_recursions(plans, name, C):
    pl = plans[name, C]
    steps, nodes = _expected_steps(C, pl.opts)
    assert pl.steps == steps and pl.n_steps == len(steps)
    assert [(n.lo, n.mid, n.hi, n.regime) for n in pl.nodes] == nodes and pl.n_nodes == len(nodes)
    assert pl.planes == pl.opts.planes and pl.too_many_slots == 0
    # ---- an image node's three schedules: made for the shape lists p3_collect stated, in the order of the launches
    used, gran = [], 2 if pl.planes == 3 else 4
    for i, n in enumerate(pl.nodes):
        g = [n.g0, n.g1, n.g2]
        if n.regime != IMAGE:
            assert g == [-1, -1, -1]
            continue
        t1, t2, k1, k2 = (n.mid - n.lo) // 2, (n.hi - n.mid) // 2, (n.mid - n.lo) * 4, (n.hi - n.mid) * 4
        assert pl.gemms[g[0]].shapes == [(t2, t1, k1, 1, 0)]                       # L21 = A21 X11^T
        assert pl.gemms[g[1]].shapes == [(t2, t2, k1, 0, 1), (t2, t1, k1, 2, 0)]   # A22 -= L21 L21^T  and  L21 X11
        assert pl.gemms[g[2]].shapes == [(t2, t1, k2, 3, 0)]                       # X21 = -X22 (L21 X11)
        # the words are appended in issue order: front schedules where the FRONT step stands, the third at the BACK step
        front, back = pl.steps.index((FRONT, i)), pl.steps.index((BACK, i))
        used += [(front, 0, g[0]), (front, 1, g[1]), (back, 0, g[2])]
    assert [g for _, _, g in sorted(used)] == list(range(pl.n_gemms)) and pl.n_gemms == len(pl.gemms)
    assert pl.images == (1 if pl.gemms else 0)
    # ---- the schedules tile the words: each starts on a multiple of 4 words behind at most 3 zero words of padding
    at = 0
    for g in pl.gemms:
        assert g.table_at % 4 == 0 and 0 <= g.table_at - at < 4 and pl.words[at:g.table_at] == [0] * (g.table_at - at)
        table = pl.words[g.table_at:g.rlist_at]
        assert len(table) >= 260 and (len(table) - 260) % 4 == 0 and table[256] == (len(table) - 260) // 4  # 4 words per unit
        assert table[:257] == sorted(table[:257]) and table[0] == 0
        for cb, ce in zip(table[261::4], table[262::4]):
            assert cb < ce and cb % gran == 0 and ce % gran == 0
        at = g.rlist_at + 2 * g.n_reduce
    assert at == len(pl.words) == pl.n_words


def test_the_default_regimes_at_4096_and_1280(plans):
    # 4096: image on top, split-bf16 at halves of 1024, paired fp32 below
    r = _regimes_by_half(plans["default", 4096])
    assert r == {(2048, 2048): {IMAGE}, (1024, 1024): {SPLIT_BF16}, (512, 512): {FP32_PAIR}, (256, 256): {FP32_PAIR},
                 (128, 128): {FP32_PAIR}}
    assert {x for s in _regimes_by_half(plans["g64max0", 4096]).values() for x in s} == {IMAGE, SPLIT_BF16, FP32}
    # 1280: no image node, and no words
    pl = plans["default", 1280]
    assert all(IMAGE not in s for s in _regimes_by_half(pl).values()) and pl.images == 0 and pl.words == [] and pl.gemms == []
    assert _regimes_by_half(pl)[(640, 640)] == {FP32_PAIR}
    # a top node that cannot take images keeps its children off them too
    pl = plans["3p_min128", 1152]
    assert pl.images == 0 and _regimes_by_half(pl)[(256, 256)] == {FP32_PAIR}
    assert _regimes_by_half(plans["3p_min128", 1024])[(256, 256)] == {IMAGE}


# --------------------------------------------------------------------------- 2. words
def test_every_combination_with_image_nodes_is_recorded(plans):
    have = {(C, pl.opts.p3_min, pl.planes) for (name, C), pl in plans.items() if pl.images}
    assert have == set(_RECORDED_WORDS)


@pytest.mark.parametrize("name,C", GRID)
def test_uploaded_words_are_the_recorded_ones(plans, name, C):
    pl = plans[name, C]
    if not pl.images:
        assert pl.words == []
        return
    assert (len(pl.words), zlib.crc32(struct.pack("<%dI" % len(pl.words), *pl.words))) == _RECORDED_WORDS[C, pl.opts.p3_min, pl.planes]


# --------------------------------------------------------------------------- 3. the bound the library reports
def test_h_prepare_workspace_is_the_recorded_table_under_every_option(plans):
    from gptq_gguf_toolkit_amd import _cabi

    def column():
        return [int(_cabi.lib().gq_workspace_bytes(_cabi.WS_H_PREPARE, 64, C, 0, 0)) for C in WIDTHS]
    for name, (_, setting) in SETS.items():
        with _cabi.options(**setting):
            assert column() == _RECORDED_H_WS[name], name
        assert [plans[name, C].bound for C in WIDTHS] == _RECORDED_H_WS[name], name  # the header the library reads
    assert column() == _RECORDED_H_WS["default"]  # the options are back


def test_chol_gemm_workspace_is_the_recorded_table():
    from gptq_gguf_toolkit_amd import _cabi
    got = {s: int(_cabi.lib().gq_workspace_bytes(_cabi.WS_CHOL_GEMM, s[0], s[1], s[2], 0)) for s in _RECORDED_GEMM_WS}
    assert got == _RECORDED_GEMM_WS


# --------------------------------------------------------------------------- 4. layout
def _up256(v):
    return -(-v // 256) * 256


@pytest.mark.parametrize("name,C", GRID)
def test_layout_is_the_one_h_prepare_carved(plans, name, C):
    pl = plans[name, C]
    # A | X | dead | zc | scales (256-aligned), as h_prepare bumped its pointer at cc07dad
    assert (pl.A, pl.X, pl.dead, pl.zc) == (0, 4 * C * C, 8 * C * C, 8 * C * C + C)
    assert pl.scales == _up256(pl.zc + C) and pl.scales % 256 == 0
    regions = [(pl.A, 4 * C * C), (pl.X, 4 * C * C), (pl.dead, C), (pl.zc, C), (pl.scales, 4 * C)]
    if pl.images:
        image = (C // 2) * (C // 2) * 2 * pl.planes
        assert pl.img0 == pl.scales + _up256(4 * C) and pl.img1 == pl.img0 + _up256(image) and pl.partial == pl.img1 + _up256(image)
        assert pl.img0 % 256 == 0 and pl.img1 % 256 == 0 and pl.partial % 256 == 0
        regions += [(pl.img0, image), (pl.img1, image), (pl.partial, PARTIAL_BYTES)]
        after = pl.partial + PARTIAL_BYTES
        if pl.planes == 2:
            assert (pl.rmax, pl.inv_scale) == (after, after + 4 * C)
            regions += [(pl.rmax, 4 * C), (pl.inv_scale, 4 * C)]
        else:
            assert (pl.rmax, pl.inv_scale) == (-1, -1)
        assert pl.words_at == _up256(after + 8 * C) and pl.words_at % 256 == 0
        regions.append((pl.words_at, 4 * pl.n_words))
    else:
        assert (pl.img0, pl.img1, pl.partial, pl.rmax, pl.inv_scale, pl.words_at) == (-1,) * 6 and pl.n_words == 0
    # in this order, apart, and the plan's total is the end of the last
    for (a, na), (b, _) in zip(regions, regions[1:]):
        assert a + na <= b
    assert pl.total == regions[-1][0] + regions[-1][1]
    assert pl.total + 255 <= pl.bound  # 255: rounding the caller's pointer up to 256
    assert pl.too_many_slots == 0


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("kr,lower", [(1, 0), (0, 1), (2, 0), (3, 0), (0, 0)])
def test_chol_gemm_layout(dump_exe, planes, kr, lower):
    shapes = ["%d,%d,%d" % s for s in _RECORDED_GEMM_WS]
    lines = subprocess.check_output([dump_exe, "gemm", str(planes), str(kr), str(lower)] + shapes, text=True).splitlines()
    assert len(lines) == len(shapes)
    for line in lines:
        p = SimpleNamespace(**_fields(line.split()[1:]))
        M, N, K = p.M, p.N, p.K
        sizes = [planes * 2 * M * K, planes * 2 * N * K, PARTIAL_BYTES, 4 * M, 4 * N, 4 * M, 4 * N, 4 * p.n_words]
        at = 0
        for off, size in zip([p.ia, p.ib, p.partial, p.rma, p.rmb, p.isa, p.isb, p.words_at], sizes):  # chol_gemm_np's take chain
            assert off == at and off % 256 == 0
            at += _up256(size)
        assert p.total == at and p.total + 255 <= p.bound == _RECORDED_GEMM_WS[M, N, K]
        assert p.too_many_slots == 0 and p.n_words == p.rlist_at + 2 * p.n_reduce and p.rlist_at >= 260
