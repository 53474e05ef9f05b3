"""The shapes of tests/test_gpu_second_turn.py as data, and the two things that file relies on without a GPU: the arithmetic (the
turns of every shape exceed the kernel's grid cap, the last turn is partial, every "part" of a whole-equals-parts comparison stays
at or below the cap) and the cap literals of the sources, read by regular expression.  A cap that changes in csrc/ fails here:
without this file the GPU tests would silently become one-turn tests again."""
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc")
REDERIVE = ("the grid cap or the units per turn of this kernel changed: re-derive the shapes of tests/test_second_turn_shapes_cpu.py "
            "(SHAPES / LITERALS) so that tests/test_gpu_second_turn.py still sends workgroups through a second turn")

# ---------------------------------------------------------------------------------------------------------------- the table
# name -> units (blocks, 16-value groups, ...) per workgroup turn, grid cap, the [R, C] of the whole call, values per unit, and
# the row counts of the parts (None: the test has another anchor than whole == parts)
SHAPES = {
    # 32-value blocks, 128 per turn: q8_0_encode_kernel, dequantize_b32_kernel (Q8_0, IQ4_NL)
    "b32": dict(per_turn=128, cap=16384, R=16260, C=4128, unit=32, parts=(8130, 8130)),
    # 256-value blocks, 16 per turn: dequantize_blocks_kernel, unpack_kernel
    "b256": dict(per_turn=16, cap=16384, R=29134, C=2304, unit=256, parts=(14567, 14567)),
    # pack_kernel at the b256 shape: 32 blocks per turn (the random bytes are the reference: a half crosses this cap itself)
    "pack": dict(per_turn=32, cap=4096, R=29134, C=2304, unit=256, parts=None),
    # dequantize_kernel at the b256 shape: 256 threads x 16 values per turn
    "dequantize": dict(per_turn=256, cap=8192, R=29134, C=2304, unit=16, parts=None),
    # iq4_pack_kernel / iq4_encode_kernel: 256 blocks of 32 values per turn
    "iq4_xs": dict(per_turn=256, cap=4096, R=14569, C=2304, unit=32, parts=(7285, 7284)),
    "iq4_nl": dict(per_turn=256, cap=4096, R=8132, C=4128, unit=32, parts=(4066, 4066)),
    # fwd_silu_mul_kernel: 256 threads x 8 values per turn, a 1-D input
    "silu": dict(per_turn=256, cap=16384, R=1, C=33554432 + 8 * 777, unit=8, parts=None),
}
PROBE_ROWS = 10  # the last rows of a whole call, checked against the CPU spec: they hold every block of the turns past the cap

# fwd_moe_combine_kernel: one token per turn, COMBINE_GRID_CAP workgroups; (T, K, E, H)
COMBINE_CAP = 2048
COMBINE_CASES = [(4101, 2, 8, 264), (7, 2, 8, 520), (7, 2, 8, 1032), (7, 2, 8, 4104), (4101, 2, 8, 4096), (2053, 8, 128, 520)]
COMBINE_EDGE = dict(T=4101, K=2, E=8, H=264, unused=4, masked=[(3, 1), (2500, 0)], all_masked=3000, neg_zero_token=2051)

# the staging copies: 256 threads x 4 x 16 bytes (16 KiB) or 256 x 1 byte per turn
STAGE_HOST = dict(wgs=1, byte_case=12345, row_case=(4096, 33))             # stage_to_host under stage_host_wgs = 1
STAGE = dict(cap=4096, rows_case=(8201, 4104), bytes_case=(1100, 1001), fill=3)   # h_stage, fp16
STAGE_MANY = dict(cap=2048, blocks=48, C=4096, rows=(1, 400), total=(4100, 4200), seed=0)   # h_stage_many, fp16


def turns(name):
    s = SHAPES[name]
    units = s["R"] * s["C"] // s["unit"]
    return units, -(-units // s["per_turn"]), units % s["per_turn"]


def stage_many_rows():
    """The seeded ragged row counts of the h_stage_many case (few long blocks, many short ones, as an expert's share of the
    calibration samples is): the first seed from STAGE_MANY['seed'] on whose total lies in range and is odd -- a row is 8 KiB,
    half a trip of a workgroup, so an odd total ends on a partial trip."""
    import random
    m = STAGE_MANY
    lo, hi = m["rows"]
    for seed in range(m["seed"], m["seed"] + 10000):
        rng = random.Random(seed)
        rows = [lo + int((hi - lo) * rng.random() ** 3) for _ in range(m["blocks"])]
        if m["total"][0] <= sum(rows) <= m["total"][1] and sum(rows) % 2:
            return rows
    raise AssertionError("no seed gives a total in range")


# ---------------------------------------------------------------------------------------------------------------- arithmetic
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_crosses_its_cap_and_ends_on_a_partial_turn(name):
    s = SHAPES[name]
    assert s["C"] % s["unit"] == 0
    units, n_turns, rest = turns(name)
    assert n_turns > s["cap"], REDERIVE
    assert 0 < rest < s["per_turn"], REDERIVE
    if s["parts"] is not None:
        assert sum(s["parts"]) == s["R"]
        for rows in s["parts"]:
            assert -(-(rows * s["C"] // s["unit"]) // s["per_turn"]) <= s["cap"], REDERIVE
        assert s["parts"][0] < s["R"] - PROBE_ROWS  # the probe rows lie in the last part
        # the probe rows hold every unit past the first pass of the grid
        assert (s["R"] - PROBE_ROWS) * (s["C"] // s["unit"]) <= s["cap"] * s["per_turn"], REDERIVE


def test_the_figures_the_gpu_file_quotes():
    assert turns("b32") == (2097540, 16388, 4) and SHAPES["b32"]["C"] // 32 == 129
    assert 4 * 34 == 136 == 8 * 16 + 8                       # Q8_0's last turn: eight 16-byte chunks and a tail of 2-byte stores
    assert 16384 * 128 == 16256 * 129 + 128                  # turn 2 begins at the last block of row 16256
    assert turns("b256") == (262206, 16388, 14) and SHAPES["b256"]["C"] // 256 == 9
    assert turns("pack") == (262206, 8194, 30)               # workgroups 0 and 1 take a third turn
    assert 2 * SHAPES["pack"]["cap"] < 8194 <= 3 * SHAPES["pack"]["cap"]
    assert SHAPES["pack"]["parts"] is None and -(-131103 // 32) > SHAPES["pack"]["cap"]   # a half crosses the pack cap itself
    units, n_turns, rest = turns("dequantize")
    assert units * 16 == 67124736 and 2 * 8192 < n_turns < 3 * 8192 and rest
    assert turns("iq4_xs") == (1048968, 4098, 136) and 136 * 17 == 2312 and 2312 % 16 == 8
    assert turns("iq4_nl") == (1049028, 4098, 196) and 196 * 18 == 3528 and 3528 % 16 == 8
    assert turns("silu") == (4194304 + 777, 16388, 9) and 777 == 3 * 256 + 9


def test_combine_cases_cross_the_grid_cap_and_every_block_size():
    assert [c for c in COMBINE_CASES if c[0] > 2 * COMBINE_CAP] and 4101 - 2 * COMBINE_CAP == 5  # five workgroups take three tokens
    blocks = {(64 if H // 8 <= 64 else 128 if H // 8 <= 128 else 256) for _, _, _, H in COMBINE_CASES}
    assert blocks == {64, 128, 256}
    assert 520 // 8 == 65 and 1032 // 8 == 129 and 4104 // 8 == 513 == 2 * 256 + 1   # one live lane in the last wave / trip
    assert all(H % 8 == 0 and K <= 8 and K <= E for _, K, E, H in COMBINE_CASES)
    e = COMBINE_EDGE
    assert e["all_masked"] > COMBINE_CAP and e["neg_zero_token"] > COMBINE_CAP and e["T"] > 2 * COMBINE_CAP
    assert any(t > COMBINE_CAP for t, _ in e["masked"])


def test_staging_cases_cross_their_caps():
    s = STAGE_HOST
    assert -(-s["byte_case"] // 256) == 49 and s["byte_case"] % 16                      # the byte kernel, 49 trips of one workgroup
    n16 = s["row_case"][0] * s["row_case"][1] * 2 // 16
    assert s["row_case"][0] * s["row_case"][1] * 2 % 16 == 0 and n16 / 1024 == 16.5     # the 16-byte kernel, a half last trip
    s = STAGE
    nbytes = s["rows_case"][0] * s["rows_case"][1] * 2
    assert nbytes % 16 == 0 and (s["fill"] * s["rows_case"][1] * 2) % 16 == 0
    # 64 MiB and 12.5 trips: workgroups 0 .. 12 take a second one, the last of them two full 4 KiB steps and 9 lanes of a third
    assert -(-nbytes // 16384) == s["cap"] + 13 and nbytes // 16 % 1024 == 2 * 256 + 9, REDERIVE
    nbytes = s["bytes_case"][0] * s["bytes_case"][1] * 2
    assert nbytes == 2202200 and nbytes % 16 and -(-nbytes // 256) > s["cap"], REDERIVE  # the byte kernel past 4096 workgroups
    m = STAGE_MANY
    rows = stage_many_rows()
    assert len(rows) == m["blocks"] and min(rows) >= 1 and max(rows) <= 400 and len(set(rows)) > 24
    total = sum(rows) * m["C"] * 2
    assert m["total"][0] <= sum(rows) <= m["total"][1] and total > (32 << 20) + (16 << 10), REDERIVE
    assert -(-total // 16384) > m["cap"] and (total // 16) % 1024, REDERIVE               # a second trip, and a partial last one


# ---------------------------------------------------------------------------------------------------------------- the sources
LITERALS = [
    ("q8/gq_q8_0.hip", r"constexpr int SPAN = 128;", 1),
    ("q8/gq_q8_0.hip", r"spans < 16384 \? spans : 16384", 1),
    ("search/gq_block_decode.hpp", r"constexpr int DB = 16;", 1),
    ("search/gq_block_decode.hpp", r"constexpr int B32_DB = 128,", 1),
    ("decode/gq_decode.hip", r"unsigned turns_grid\(int64_t nblocks, int per_turn = DB\) \{\s*const int64_t g = \(nblocks \+ per_turn - 1\) / "
                             r"per_turn;\s*return \(unsigned\)\(g < 16384 \? g : 16384\);", 1),
    ("decode/gq_decode.hip", r"turns_grid\(", 3),   # its definition, gq_dequantize_blocks and gq_unpack
    ("gq_pack_layout.hpp", r"constexpr int PB = 32;", 1),
    ("gq_codec.hip", r"dim3 grid\(\(unsigned\)\(g < 4096 \? g : 4096\)\)", 1),                                    # pack_kernel
    ("gq_codec.hip", r"\(n16 \+ 255\) / 256 < 8192 \? \(n16 \+ 255\) / 256 : 8192", 2),                          # dequantize, rtn
    ("iq4/gq_iq4_gptq.hip", r"constexpr int PK_TILE = 256, PK_MAX_GRID = 4096;", 1),
    ("iq4/gq_iq4_encode.hip", r"constexpr int TILE = 256;", 1),
    ("iq4/gq_iq4_encode.hip", r"constexpr int MAX_GRID = 4096;", 1),
    ("gq_forward.hip", r"\(n8 \+ 255\) / 256 < 16384 \? \(n8 \+ 255\) / 256 : 16384", 1),
    ("calib/gq_moe_combine.hip", r"constexpr int COMBINE_GRID_CAP = 2048;", 1),
    ("calib/gq_moe_combine.hip", r"block\(H8 <= 64 \? 64 : H8 <= 128 \? 128 : 256\)", 1),
    ("gq_hessian.hip", r"const int64_t cap = max_wgs > 0 \? max_wgs : 4096;", 1),                                 # h_stage
    ("gq_hessian.hip", r"int64_t blocks = \(n16 \+ 1023\) / 1024;\s*if \(blocks > 2048\) blocks = 2048;", 1),      # h_stage_many
    ("gq_hessian.hip", r"const int64_t wgs = \(n16 \+ 1023\) / 1024;", 1),
    ("gq_hessian.hip", r"const int64_t wgs = \(nbytes \+ 255\) / 256;", 1),
]


@pytest.mark.parametrize("path,pattern,count", LITERALS, ids=[f"{p}:{i}" for i, (p, _, _) in enumerate(LITERALS)])
def test_the_cap_literals_still_read_as_the_table_says(path, pattern, count):
    text = open(os.path.join(CSRC, path)).read()
    assert len(re.findall(pattern, text)) == count, f"{path}: /{pattern}/ -- {REDERIVE}"


def test_the_table_and_the_literals_name_the_same_numbers():
    caps = {n: s["cap"] for n, s in SHAPES.items()}
    per = {n: s["per_turn"] for n, s in SHAPES.items()}
    assert caps == {"b32": 16384, "b256": 16384, "pack": 4096, "dequantize": 8192, "iq4_xs": 4096, "iq4_nl": 4096, "silu": 16384}
    assert per == {"b32": 128, "b256": 16, "pack": 32, "dequantize": 256, "iq4_xs": 256, "iq4_nl": 256, "silu": 256}
    assert COMBINE_CAP == 2048 and STAGE["cap"] == 4096 and STAGE_MANY["cap"] == 2048
