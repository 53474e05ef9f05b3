"""bench.py's plain run: one headline line, --steps honoured, --dump-outputs writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_run_prints_one_line_and_dumps_the_same_outputs_twice(tmp_path, oracle):
    """Two plain runs with the same arguments: exactly one JSON line each (the headline, none of the --full figures), the
    requested step counts, and the same dumped arrays -- float32, < 64 MB, one file per Linear and field, every field of a
    Linear cut to the same rows (the dumped GGUF bytes are the oracle's packing of the dumped codes and scales)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--workload", "tinyllama-block-q4k", "--calib-seqs", "8"]
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        p = subprocess.run(cmd + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        line = json.loads(lines[0])
        assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
        assert line["metric"] == "Mparams/s GPTQ-quantized" and line["unit"] == "Mparams/s" and line["value"] > 0
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["ms_per_step"] > 0
        assert not {"roofline", "step_latency_ms", "cpu_baseline", "trailing_update", "whole_model"} & set(line)
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert len(arrays) == 7 * 7  # 7 Linears x (weight, qweight, d, s, dmin, m, packed)
        assert all(a.dtype == np.float32 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) < 64e6
        for name in ("q_proj", "down_proj"):
            f = {k: arrays[f"{name}.{k}"] for k in ("qweight", "d", "s", "dmin", "m", "packed")}
            u8 = lambda a: a.astype(np.uint8)  # noqa: E731
            packed = oracle.pack(oracle.Q4_K, u8(f["qweight"]), f["d"].astype(np.float16), u8(f["s"]),
                                 f["dmin"].astype(np.float16), u8(f["m"]))
            assert np.array_equal(packed, u8(f["packed"])), name
            assert arrays[f"{name}.weight"].shape == f["qweight"].shape
        dumps.append(arrays)
    assert all(np.array_equal(dumps[0][k], dumps[1][k]) for k in dumps[0])
