#!/usr/bin/env python3
"""GGUF splitter -- the EvoPress database producer of the reference (mapper/gguf_splitter.py:33-636).

GGUF side (`split_gguf_model`, the default): one directory per GGUF tensor holding the tensor's raw bytes as
"<bitwidth>[-<quantization>].pth" plus a metadata JSON, a manifest of all tensors with the file's key/value metadata, and the
layer database (name -> type / bit width / shape / offset).  HF side (`split_hf_model`, `--hf-layers`, reference :448-636): one
directory per `model.layers.*.(q|k|v|o|gate|up|down)_proj` holding the DEQUANTIZED weight in HF row layout as a `torch.save`d
tensor, its metadata JSON with the `gguf_info` record, a manifest with `mapping_stats`, and `hf_to_gguf_mapping.json`.
Same file names, JSON keys and CLI as the reference (`model_path output_dir [--exact] [--gguf-layers | --hf-layers | --both]
[--bitwidth B] [--dtype float16|float32]`, plus `--device`); with none of the new flags the command does what it always did.
The reference reads the container with gguf-py and obtains the HF weights through transformers' GGUF loader; neither is
installable here, so the container is read by this package's spec-level reader (F32 / F16 / BF16 / Q8_0 / K-quants) and the
weights are decoded on the GPU by gguf_loader.py (gq_dequantize_blocks).  No tokenizer is loaded.  Like the reference, both
sides write into `output_dir` itself and `--both` leaves the HF manifest as `manifest.json`.
"""
import argparse
import json
import os
import re
import sys
import time
from pathlib import Path
from typing import Dict, Iterable, Optional, Tuple, Union


if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from .gguf_writer import parse_gguf  # noqa: E402
# TYPE_NAMES / EXACT_BITS: level_db's narrow views on the types the reference's splitter names; level_records: the JSON
# records of a level, shared with level_db.LevelDbWriter
from .level_db import EXACT_BITS, TYPE_NAMES, level_records, level_stem, write_manifests, write_sidecar  # noqa: E402


class GGUFSplitter:
    def __init__(self, model_path: str, output_dir: str, use_exact_bitwidth: bool = False):
        self.model_path, self.output_dir = Path(model_path), Path(output_dir)
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self.use_exact_bitwidth = use_exact_bitwidth
        self.gguf_layer_database: Dict[str, dict] = {}

    def get_quantization_info(self, tensor_name: str, tensor_type: int) -> str:
        return TYPE_NAMES.get(tensor_type, f"UNKNOWN_{tensor_type}")

    def get_tensor_bit_width(self, quantization: str) -> float:
        return EXACT_BITS.get(quantization, 32.0)

    def extract_bitwidth_from_quantization(self, quantization: str) -> Union[int, float]:
        """gguf_splitter.py:98-122: the exact fractional width, or the integer class of the type."""
        if self.use_exact_bitwidth:
            return self.get_tensor_bit_width(quantization)
        for digit in "234568":
            if quantization.startswith(("Q" + digit, "IQ" + digit)):
                return int(digit)
        if quantization in ("F16", "F32"):
            return 16 if quantization == "F16" else 32
        return 1 if quantization.startswith("IQ1") else 4

    def _entries(self):
        kv, tensors, buf = parse_gguf(str(self.model_path))
        for name, shape, gt, off, nbytes in tensors:
            q = self.get_quantization_info(name, gt)
            yield name, shape, gt, off, nbytes, q, buf
        self._kv = kv

    def build_gguf_layer_database(self) -> Dict[str, dict]:
        db = {}
        for name, shape, gt, off, nbytes, q, _ in self._entries():
            db[name] = level_records(name, shape, gt, q, self.extract_bitwidth_from_quantization(q), self.get_tensor_bit_width(q),
                                     nbytes, "", off)[2]
        self.gguf_layer_database = db
        return db

    def split_gguf_model(self, overwrite_bitwidth=None):
        self.build_gguf_layer_database()
        manifest = {"model_info": {"original_file": self.model_path.name, "total_tensors": len(self.gguf_layer_database),
                                   "split_timestamp": None, "use_exact_bitwidth": self.use_exact_bitwidth},
                    "metadata": {}, "layers": {}}
        n = 0
        for name, shape, gt, off, nbytes, q, buf in self._entries():
            n += 1
            bitwidth = self.extract_bitwidth_from_quantization(q)
            prefix = level_stem(bitwidth, q if self.use_exact_bitwidth else None)
            layer_dir = self.output_dir / name
            layer_dir.mkdir(parents=True, exist_ok=True)
            (layer_dir / f"{prefix}.pth").write_bytes(buf[off:off + nbytes])  # raw bytes, not a torch pickle (:378-380)
            sidecar, level, _ = level_records(name, shape, gt, q, bitwidth, self.get_tensor_bit_width(q), nbytes, prefix, off)
            write_sidecar(layer_dir / f"{prefix}-metadata.json", sidecar)
            layer = manifest["layers"].setdefault(name, {"original_name": name, "dims": list(reversed(shape)), "bitwidths": {}})
            layer["bitwidths"][str(bitwidth)] = level
        for key, (value, types) in self._kv.items():
            manifest["metadata"][key] = {"types": types, "value": value}
        manifest["model_info"]["split_timestamp"] = time.time()
        manifest["model_info"]["processed_tensors"] = n
        write_manifests(self.output_dir, manifest, self.gguf_layer_database)
        return manifest


    # ---- HF side (reference :448-636) ----
    HF_LAYER = re.compile(r"^model\.layers\..*\.(q_proj|k_proj|v_proj|o_proj|gate_proj|up_proj|down_proj)\.weight$")

    def map_hf_to_gguf_name(self, hf_name: str) -> Optional[str]:
        """The GGUF tensor an HF parameter was written as, or None when the file has no such tensor (:148-282)."""
        from .pack_gptq_into_gguf import map_tensor_name
        try:
            name = map_tensor_name(hf_name)
        except ValueError:
            return None
        return name if name in self.gguf_layer_database else None

    def resolve_hf_bitwidth(self, gguf_name: Optional[str], overwrite_bitwidth) -> Tuple[Optional[float], Optional[str], bool]:
        """-> (bitwidth, quantization, skip) of one HF layer, the reference's rule (:527-551): without an overwrite the
        GGUF tensor's own class; an overwrite is a number (quantization None) or a type name such as "Q4_K" (its bit-width
        class), and a layer whose GGUF class differs from a positive overwrite is skipped.  A layer the file does not hold
        needs an overwrite and takes it (the reference goes on to format a bit width of None there and fails)."""
        if overwrite_bitwidth is None:
            if gguf_name is None:
                raise ValueError("No GGUF mapping found for the layer and no overwrite_bitwidth provided")
            rec = self.gguf_layer_database[gguf_name]
            return rec["bitwidth"], rec["quantization"], False
        try:
            bitwidth, quantization = float(overwrite_bitwidth), None
        except ValueError:
            quantization = overwrite_bitwidth
            bitwidth = self.extract_bitwidth_from_quantization(overwrite_bitwidth.upper())
        if gguf_name is None:
            return bitwidth, quantization, False
        return bitwidth, quantization, bool(self.gguf_layer_database[gguf_name]["bitwidth"] != bitwidth and bitwidth > 0)

    def split_hf_model(self, dtype: str = "float16", overwrite_bitwidth=None, device: str = "cuda:0",
                       tensors: Optional[Iterable] = None):
        """Dequantize the file's decoder projections and write them, in HF layout and names, as the reference does.
        `tensors`: an iterable of (HF name, tensor) to use instead of decoding the file (gguf_loader.iter_gguf_tensors)."""
        import torch
        if not self.gguf_layer_database:
            self.build_gguf_layer_database()
        torch_dtype = torch.float16 if dtype == "float16" else torch.float32
        if tensors is None:
            from .gguf_loader import iter_gguf_tensors
            tensors = iter_gguf_tensors(str(self.model_path), device, torch_dtype, hf_layout=True)
        manifest = {"model_info": {"original_file": self.model_path.name, "dtype": dtype, "bitwidth": overwrite_bitwidth,
                                   "use_exact_bitwidth": self.use_exact_bitwidth, "split_timestamp": time.time()},
                    "layers": {}, "mapping_stats": {"total_layers": 0, "mapped_layers": 0, "unmapped_layers": 0}}
        processed = mapped = 0
        mapping = {}
        for name, t in tensors:
            if not self.HF_LAYER.search(name):
                continue
            processed += 1
            gguf_name = self.map_hf_to_gguf_name(name)
            mapping[name] = gguf_name
            mapped += gguf_name is not None
            try:
                bitwidth, quantization, skip = self.resolve_hf_bitwidth(gguf_name, overwrite_bitwidth)
            except ValueError as e:
                raise ValueError(f"{name}: {e}") from None
            if skip:
                print(f"Warning: overwrite bitwidth {overwrite_bitwidth} does not match the GGUF bitwidth "
                      f"{self.gguf_layer_database[gguf_name]['bitwidth']} of {name}, layer not saved")
                continue
            t = t.detach().to(torch_dtype).cpu().contiguous()
            layer_dir_name = name.replace(".weight", "")
            layer_dir = self.output_dir / layer_dir_name
            layer_dir.mkdir(parents=True, exist_ok=True)
            prefix = level_stem(bitwidth, quantization)
            filename, metadata_filename = f"{prefix}.pth", f"{prefix}-metadata.json"
            torch.save(t, layer_dir / filename)
            n_bytes = t.numel() * t.element_size()
            meta = {"tensor_info": {"name": name, "gguf_mapped_name": gguf_name, "bitwidth": bitwidth, "dtype": str(t.dtype),
                                    "shape": list(t.shape), "n_elements": t.numel(), "n_bytes": n_bytes,
                                    "data_filename": filename,
                                    "requires_grad": True}}  # the reference records a loaded model's parameter
            if gguf_name is not None:
                meta["gguf_info"] = self.gguf_layer_database[gguf_name]
            (layer_dir / metadata_filename).write_text(json.dumps(meta, indent=2))
            manifest["layers"][name] = {"original_name": name, "gguf_mapped_name": gguf_name, "layer_directory": layer_dir_name,
                                        "dims": list(t.shape), "bitwidth": bitwidth, "filename": filename,
                                        "metadata_filename": metadata_filename, "dtype": str(t.dtype), "size_bytes": n_bytes,
                                        "shape": list(t.shape), "n_elements": t.numel()}
        manifest["mapping_stats"] = {"total_layers": processed, "mapped_layers": mapped, "unmapped_layers": processed - mapped}
        (self.output_dir / "manifest.json").write_text(json.dumps(manifest, indent=2))
        (self.output_dir / "hf_to_gguf_mapping.json").write_text(json.dumps(mapping, indent=2))
        return manifest


def hf_overwrite_from_cli(bitwidth) -> Optional[int]:
    """The reference's rule for `--bitwidth` on the HF side (:751-757): a number <= 0 stores the layers as "0.pth" whatever
    their GGUF type; anything else (the default 16, a positive number, a type name) keeps each tensor's own class."""
    try:
        return 0 if float(bitwidth) <= 0 else None
    except ValueError:
        return None


def main(argv=None):
    p = argparse.ArgumentParser(description="Split a GGUF model into per-tensor directories (EvoPress database)")
    p.add_argument("model_path", help="Path to input GGUF model")
    p.add_argument("output_dir", help="Directory to store split layers")
    p.add_argument("--exact", action="store_true", help='exact fractional bit widths in the file names ("4.5-Q4_K.pth")')
    p.add_argument("--gguf-layers", action="store_true", help="split the GGUF tensors (raw bytes); the default")
    p.add_argument("--hf-layers", action="store_true",
                   help="dequantize the decoder projections on the GPU and split them under their HF names")
    p.add_argument("--both", action="store_true", help="both of the above")
    p.add_argument("--bitwidth", type=str, default=16,
                   help="HF side: a value <= 0 stores every layer as bit width 0 (default: each tensor's own GGUF class)")
    p.add_argument("--dtype", choices=["float16", "float32"], default="float16", help="dtype of the HF-side tensors")
    p.add_argument("--device", default="cuda:0", help="GPU that decodes the HF-side tensors")
    a = p.parse_args(argv)
    if a.both:
        a.gguf_layers = a.hf_layers = True
    elif not a.hf_layers:
        a.gguf_layers = True
    sp = GGUFSplitter(a.model_path, a.output_dir, use_exact_bitwidth=a.exact)
    if a.gguf_layers:
        m = sp.split_gguf_model()
        print(f"GGUF split complete! {m['model_info']['processed_tensors']} tensors into {len(m['layers'])} layer directories")
    if a.hf_layers:
        m = sp.split_hf_model(a.dtype, hf_overwrite_from_cli(a.bitwidth), device=a.device)
        st = m["mapping_stats"]
        print(f"HuggingFace split complete! {st['total_layers']} layers processed, {st['mapped_layers']} mapped to GGUF names")


if __name__ == "__main__":
    main()
