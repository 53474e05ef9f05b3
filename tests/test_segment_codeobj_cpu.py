"""The column-loop segment kernel keeps everything in registers: no VGPR spill, no SGPR spill, no private segment, in all
four instantiations (K-quant, act_order, uniform grid, bands).

gq_gptq.hip is compiled device-only to assembly with the Makefile's flags and only the code object's METADATA is read:
the three fields below for the four gptq_segment_kernel symbols.  Wave 0 of that kernel walks a chain of dependent
columns out of LDS; a spill puts scratch round trips -- and, on gfx9, a wait for the previous tile's global stores -- into
every 16 columns of it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gptq-gguf-toolkit_amd", "csrc")
FIELDS = ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
# template arguments <PERM, UNI, BANDS> as the mangled names spell them
KERNELS = {"kquant": "ILb0ELb0ELb0EE", "act_order": "ILb1ELb0ELb0EE", "uniform": "ILb0ELb1ELb0EE", "bands": "ILb0ELb0ELb1EE"}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile with its defaults filled in (the test follows the build)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{symbol: {field: int}} for every kernel of gq_gptq.hip"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("segasm") / "gq_gptq.s"
    subprocess.check_call([hipcc, *_makefile_flags(), "--cuda-device-only", "-S", "gq_gptq.hip", "-o", str(out)], cwd=CSRC,
                          stderr=subprocess.DEVNULL)
    table, name = {}, None
    for line in open(out):
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name" and val.startswith("_Z"):
            name = val
            table.setdefault(name, {})
        elif key in FIELDS and name is not None:
            table[name][key] = int(val)
    return table


@pytest.mark.parametrize("kind", list(KERNELS))
def test_segment_kernel_spills_nothing(metadata, kind):
    syms = [n for n in metadata if "gptq_segment_kernel" + KERNELS[kind] in n]
    assert len(syms) == 1, f"{kind}: {syms}"
    got = metadata[syms[0]]
    assert set(got) == set(FIELDS), got
    assert got == dict.fromkeys(FIELDS, 0), f"{kind}: {got}"
