"""The segment kernel of the column walk on the IQ4 grid (gq_gptq.hip, gptq_segment_iq4_kernel) keeps everything in registers:
no VGPR spill, no SGPR spill, no private segment -- read from the code object's metadata the way
tests/test_segment_codeobj_cpu.py reads the four gptq_segment_kernel symbols (its fixture compiles gq_gptq.hip device-only to
assembly with the Makefile's flags).  Wave 0's best() must not go through scratch any more than through LDS."""
from test_segment_codeobj_cpu import FIELDS, metadata  # noqa: F401  (the fixture)


def test_iq4_segment_kernel_spills_nothing(metadata):  # noqa: F811
    syms = [n for n in metadata if "gptq_segment_iq4_kernel" in n]
    assert len(syms) == 1, syms
    got = metadata[syms[0]]
    assert set(got) == set(FIELDS), got
    assert got == dict.fromkeys(FIELDS, 0), got
    # the four existing instantiations are still there, under their names
    assert len([n for n in metadata if "gptq_segment_kernelILb" in n]) == 4
