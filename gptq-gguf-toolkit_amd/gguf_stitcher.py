#!/usr/bin/env python3
"""GGUF stitcher -- the last step of the reference's workflow (mapper/gguf_stitcher.py): a level database written by
gguf_splitter.py plus a per-tensor configuration -> one mixed-precision .gguf.

    python -m gptq_gguf_toolkit_amd.gguf_stitcher SPLIT_DIR OUT.gguf [--config F] [--original-model F]
        [--default-bitwidth B] [--default-quant-type T] [--validate-only] [--list-tensors] [--inspect-metadata]
        [--llama-ftype] [--verify | --verify-only [--device D]]

    stitch_search_result(db, "evo-kl-configuration-4.0.txt", "mixed.gguf", original_model="q4.gguf", verify=True)

No arithmetic happens here: the bytes the configuration chooses are copied into a container.  Kept as the reference has
them (its line numbers): layer discovery (:70-141, manifest order first -- the original file's tensor order), the three
configuration line forms (:316-415), the level choice `_find_best_matching_config` (:143-168), the type of the written
tensor (:504-577), the payload / metadata lookup with its `32-F32` fallback (:579-625), the key/value data (:676-774) and
the reports of validate_config / list_available_tensors / inspect_metadata.

`general.file_type` (:644-674) is reproduced INCLUDING ITS QUIRK: the reference counts tensors per bit width, takes int() of
the dominant width (4.5 -> 4) and, when that width has more than half of the tensors, looks it up in a table of ggml TYPE
ids (12 for Q4_K, 14 for Q6_K), otherwise writes 12; ties go to the width seen first.  llama.cpp reads the key as a
LLAMA_FTYPE id, where 12 means Q3_K_M.  `--llama-ftype` / `llama_ftype=True` writes that enumeration instead (F32 0, F16 1,
Q8_0 7, Q2_K 10, Q3_K_M 12, Q4_K_M 15, Q5_K_M 17, Q6_K 18, IQ4_NL 25, IQ4_XS 30, BF16 32; mixed or no majority 15).

Deliberately different from the reference:
  * streaming: the reference loads every tensor into a list before it writes; here each tensor is a
    GGUFWriter.add_tensor_lazy producer that reads its level file when its turn comes, so the host holds what the writer's
    pipeline holds (LAZY_DEPTH + LAZY_WORKERS payloads), not the model;
  * no broken file: the container is written to `<output>.partial` and renamed on success; on any error the partial file is
    removed and nothing appears at the output path;
  * no silent drops: the reference prints "Error preparing tensor" and goes on (:793-795), ending with exit status 0 and a
    file that lacks the tensor.  Here every tensor of the complete configuration is resolved -- files present, byte counts
    consistent, type writable -- BEFORE the output is opened, and the failures raise together (StitchError);
  * key/value data keeps each key's recorded type and array element type (our splitter's manifest has them; the
    reference's inference :741-760 is used only for a manifest without types), and empty strings / arrays are kept;
  * a source without key/value data (a --both database, whose manifest.json is the HF side's, with no original model to be
    found) and a source whose general.alignment is not the writer's 32 are refused like a tensor that cannot be written: the
    reference would write a file without keys, or one whose alignment key contradicts its layout.
Only F32 / F16 / BF16 / Q8_0 / Q2_K..Q6_K / IQ4_NL / IQ4_XS payloads can be written by gguf_writer.py; a tensor that resolves
to any other type (the other IQ types, Q4_0, Q8_K, ...: known by name for the reports) is refused by name, never written under
another type.

`verify` (a keyword here, `--verify` on the command line) is the guarantee the reference does not give -- the file written is
the model the search scored: the renamed file is read back through gguf_loader (mapped, decoded on the GPU by
gq_dequantize_blocks) and every K-quant or plain tensor must equal, bit for bit, level_db.load_level of the level
file the configuration chose -- the load path the search's LevelStore is tested against.  It adds no kernel.
`--verify-only` checks a file stitched earlier against the same database and configuration and writes nothing.

PARITY: gguf-py cannot be run here, so this module is checked against the reference by reading it (the citations above)
and by an independent spec-level reader (tests/test_stitch_cpu.py), not by golden files."""
import argparse
import os
import re
import sys
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from . import level_db  # noqa: E402
from .config_converter import config_text as render_config, convert_hf_to_gguf_config, detect_moe_model, read_config_file  # noqa: E402
from .gguf_writer import ALIGNMENT, GGML_QUANT_SIZES, GGUFValueType, GGUFWriter, parse_gguf  # noqa: E402

# WRITABLE is what gguf_writer.py can write of the type names the reference knows (level_db.GGML_TYPE_IDS)
WRITABLE = {name: t for name, t in level_db.GGML_TYPE_IDS.items() if t in GGML_QUANT_SIZES}
# the width-class table of :516-577: (low, high, {exact width: type}, (types kept when the level's own quantization names
# them), type of the class); walked in this order, an integer width equal to `low` belongs to the class
WIDTH_CLASSES = ((2.0, 2.7, {2.0625: "IQ2_XXS", 2.3125: "IQ2_XS", 2.5: "IQ2_S", 2.7: "IQ2_M"}, (), "Q2_K"),
                 (3.0, 3.7, {3.0625: "IQ3_XXS", 3.44: "IQ3_S", 3.66: "IQ3_M"}, (), "Q3_K"),
                 (4.0, 4.6, {4.25: "IQ4_XS", 4.56: "IQ4_NL"}, ("Q4_0", "Q4_1"), "Q4_K"),
                 (5.0, 6.0, {}, ("Q5_0", "Q5_1"), "Q5_K"),
                 (6.0, 7.0, {}, (), "Q6_K"),
                 (8.0, 9.0, {}, ("Q8_0", "Q8_1"), "Q8_K"),
                 (1.0, 1.6, {}, (), "IQ1_S"))
FILE_TYPE_BY_WIDTH = {32: 0, 16: 1, 8: 7, 6: 14, 5: 13, 4: 12, 3: 11, 2: 10}  # the reference's table (:660-669): ggml TYPE ids
LLAMA_FTYPE = {"F32": 0, "F16": 1, "Q8_0": 7, "Q2_K": 10, "Q3_K": 12, "Q4_K": 15, "Q5_K": 17, "Q6_K": 18, "IQ4_NL": 25, "IQ4_XS": 30,
               "BF16": 32}
LLAMA_FTYPE_MIXED = 15  # LLAMA_FTYPE_MOSTLY_Q4_K_M
SKIP_KEYS = ("general.file_type", "general.quantization_version")  # re-added last (:679-682, :766-774)
VALUE_TYPE_NAMES = {v: k for k, v in vars(GGUFValueType).items() if k.isupper()}

_EXACT_LINE = re.compile(r"^([0-9.]+)\s*\(([0-9.]+-[^)]+\.pth)\)$")  # "bw (bw-TYPE.pth)" (:337)


class StitchError(Exception):
    """The configuration cannot be stitched, or the stitched file is not what the configuration names."""


class QuantizationConfig:
    """The level chosen for one tensor (:27-41): its bit width, file name and, when the file name carries one, its type."""

    def __init__(self, bitwidth: float, filename: str, quant_type: Optional[str] = None, metadata: Dict[str, Any] = None):
        self.bitwidth = bitwidth
        self.filename = filename
        self.filename_prefix = level_db.level_stem(bitwidth, quant_type or None)
        self.meta_data = metadata or {}
        self.quant_type = quant_type


class _Planned:
    """One tensor as it will be written: resolved before the output is opened."""
    __slots__ = ("name", "shape", "type_name", "ggml_type", "path", "nbytes")


class GGUFStitcher:
    def __init__(self, split_dir: str, config_path: Optional[str], output_path: str,
                 original_model_path: Optional[str] = None, default_bitwidth: float = 4.0,
                 default_quant_type: str = "Q4_K", llama_ftype: bool = False, config_text: Optional[str] = None,
                 quiet: bool = False):
        """config_text: the configuration itself instead of a file (stitch_search_result hands the converted text over).
        quiet: leave out the line per tensor that the reference prints while it completes the configuration."""
        self.split_dir = Path(split_dir)
        self.config_path = Path(config_path) if config_path else None
        self.config_text = config_text
        self.output_path = Path(output_path)
        self.original_model_path = Path(original_model_path) if original_model_path else None
        self.default_bitwidth = default_bitwidth
        self.default_quant_type = default_quant_type
        self.llama_ftype = llama_ftype
        self.quiet = quiet
        self.manifest = self._load_manifest()
        self.available_layers = self._discover_layers()
        self.config = self._build_complete_config()
        self.original_metadata = self._load_original_metadata()
        self.writer = None
        self.planned: Optional[List[_Planned]] = None  # set by the first plan()

    # ---- the database ----
    def _load_manifest(self) -> Dict[str, Any]:
        try:
            manifest = level_db.read_manifest(self.split_dir)
        except Exception as e:
            raise ValueError(f"Error loading manifest: {e}")
        if manifest is None:
            print(f"Warning: Manifest not found at {self.split_dir / 'manifest.json'}, creating minimal manifest from directory scan")
            return {"layers": {d.name: {"bitwidths": {}} for d in sorted(self.split_dir.iterdir()) if d.is_dir()}}
        print(f"Loaded manifest with {len(manifest.get('layers', {}))} layers")
        return manifest

    def _scan_dir(self, layer_dir: Path) -> List[Dict[str, Any]]:
        """The levels one directory offers, ordered by bit width and name (the reference takes glob order)."""
        found = []
        for p in layer_dir.glob("*.pth"):
            parsed = level_db.parse_level_name(p.name)
            if parsed is not None:
                found.append({"bitwidth": parsed[0], "filename": p.name, "quant_type": parsed[1]})
        return sorted(found, key=lambda lv: (lv["bitwidth"], lv["filename"]))

    def _discover_layers(self) -> Dict[str, List[Dict[str, Any]]]:
        """{tensor name: its levels}: the manifest's layers first, in manifest order -- the original file's tensor order,
        which the stitched file keeps -- then the directories the manifest does not name (:70-141).  Two refinements for a
        database split with --both, whose manifest.json is the HF side's: the HF side's directories (torch-saved dense
        tensors, `layer_directory` of that manifest) are not GGUF tensors and are left out, and the remaining directories
        follow gguf_layer_database.json (the file's tensor order again) before any others, by name."""
        discovered: Dict[str, List[Dict[str, Any]]] = {}
        layers = self.manifest.get("layers", {})
        hf_side = {info["layer_directory"] for info in layers.values() if isinstance(info, dict) and "layer_directory" in info}
        for name in layers:
            layer_dir = self.split_dir / name
            if name in hf_side or not layer_dir.is_dir():
                continue
            levels = self._scan_dir(layer_dir)
            if levels:
                discovered[name] = levels
        rest = sorted(d.name for d in self.split_dir.iterdir() if d.is_dir())
        database = level_db.read_manifest(self.split_dir, "gguf_layer_database.json")
        if database is not None:
            order = {name: i for i, name in enumerate(database)}
            rest.sort(key=lambda n: (order.get(n, len(order)), n))
        for name in rest:
            if name in discovered or name in hf_side:
                continue
            levels = self._scan_dir(self.split_dir / name)
            if levels:
                discovered[name] = levels
        print(f"Discovered {len(discovered)} layers in split directory")
        return discovered

    def _find_best_matching_config(self, available_configs: List[Dict[str, Any]], target_bitwidth: float,
                                   target_quant_type: Optional[str]) -> Dict[str, Any]:
        """Exact width and type, then exact width, then the closest width with the preferred type, then the closest width
        (:143-168); among equally close widths the first of `available_configs` wins."""
        same_width = [c for c in available_configs if c["bitwidth"] == target_bitwidth]
        if target_quant_type:
            for c in same_width:
                if c["quant_type"] == target_quant_type:
                    return c
        if same_width:
            return same_width[0]
        by_distance = sorted(available_configs, key=lambda c: abs(c["bitwidth"] - target_bitwidth))
        if target_quant_type:
            for c in by_distance:
                if c["quant_type"] == target_quant_type:
                    return c
        return by_distance[0]

    # ---- the configuration ----
    def _config_lines(self) -> List[str]:
        if self.config_text is not None:
            return self.config_text.split("\n")
        if self.config_path and self.config_path.exists():
            with open(self.config_path, "r") as f:
                return f.read().split("\n")
        return []

    def _load_config(self) -> Dict[str, QuantizationConfig]:
        """`name: bw (bw-TYPE.pth)` (taken as written), `name: bw` and `name: bw TYPE` (the best available match of the
        tensor's directory); '#' lines and lines without ':' are skipped, anything else that does not parse is a warning."""
        config = {}
        for line_num, line in enumerate(self._config_lines(), 1):
            line = line.strip()
            if not line or line.startswith("#") or ":" not in line:
                continue
            tensor_name, rest = (s.strip() for s in line.split(":", 1))
            exact = _EXACT_LINE.match(rest)
            if exact:
                filename = exact.group(2)
                config[tensor_name] = QuantizationConfig(float(exact.group(1)), filename, level_db.level_type(filename))
                continue
            parts = rest.split()
            try:
                if len(parts) not in (1, 2):
                    raise ValueError(rest)
                bitwidth, quant_type = float(parts[0]), (parts[1] if len(parts) == 2 else None)
            except ValueError:
                print(f"Warning: Could not parse line {line_num}: {line}")
                continue
            if tensor_name in self.available_layers:
                best = self._find_best_matching_config(self.available_layers[tensor_name], bitwidth, quant_type)
                config[tensor_name] = QuantizationConfig(best["bitwidth"], best["filename"], best["quant_type"])
            else:  # not a directory of the database: kept, so that validate_config can name it
                filename = f"{bitwidth}-{quant_type}.pth" if quant_type else f"{bitwidth}.pth"
                config[tensor_name] = QuantizationConfig(bitwidth, filename, quant_type)
        print(f"Loaded user configuration for {len(config)} tensors")
        return config

    def _build_complete_config(self) -> Dict[str, QuantizationConfig]:
        """Every discovered tensor, in discovery order: the user's level, or the default through the same rule (:170-227)."""
        user_config = self._load_config()
        complete = {}
        say = (lambda *a: None) if self.quiet else print
        for name, levels in self.available_layers.items():
            if name in user_config:
                c = complete[name] = user_config[name]
                say(f"  {name}: Using user config - {c.bitwidth}-bit ({c.quant_type or 'default'})")
                continue
            best = self._find_best_matching_config(levels, self.default_bitwidth, self.default_quant_type)
            complete[name] = QuantizationConfig(best["bitwidth"], best["filename"], best["quant_type"])
            asked = f"[requested: {self.default_bitwidth}-bit {self.default_quant_type}]"
            if best["bitwidth"] != self.default_bitwidth or best["quant_type"] != self.default_quant_type:
                say(f"  {name}: Using closest available - {best['bitwidth']}-bit ({best['quant_type'] or 'default'}) {asked}")
            else:
                say(f"  {name}: Using default - {best['bitwidth']}-bit ({best['quant_type'] or 'default'})")
        self.unknown_tensors = [n for n in user_config if n not in self.available_layers]
        if self.unknown_tensors:
            print(f"Warning: the configuration names {len(self.unknown_tensors)} tensors the database does not hold (ignored, as "
                  f"the reference does): {self.unknown_tensors}")
        print(f"\nTotal configuration: {len(complete)} tensors")
        print(f"  User-specified: {len(user_config)} tensors")
        print(f"  Using defaults: {len(complete) - sum(n in user_config for n in complete)} tensors")
        return complete

    def get_tensor_bit_width(self, quantization: str) -> float:
        return level_db.BIT_WIDTHS.get(quantization, 32.0)

    # ---- key/value data ----
    def _find_original_model(self) -> Optional[Path]:
        if self.original_model_path and self.original_model_path.exists():
            return self.original_model_path
        name = self.manifest.get("model_info", {}).get("original_file")
        if name:
            for candidate in (self.split_dir.parent / name, self.split_dir / name, Path(name)):
                if candidate.exists():
                    return candidate
        return None

    def _load_original_metadata(self) -> Optional[Dict[str, Any]]:
        """{key: {"value", "types"}} of the original file through parse_gguf, or None (the manifest is used then)."""
        path = self._find_original_model()
        if not path:
            print("Warning: Original model not found. Will use metadata from manifest.")
            return None
        try:
            print(f"Loading metadata from original model: {path}")
            kv, _, _ = parse_gguf(str(path), mmap=True)
        except Exception as e:
            print(f"Error loading original model metadata: {e}")
            return None
        print(f"Loaded {len(kv)} metadata fields from original model")
        return {key: {"value": value, "types": list(types)} for key, (value, types) in kv.items()}

    def _metadata_source(self) -> Dict[str, Any]:
        return self.original_metadata if self.original_metadata else self.manifest.get("metadata", {})

    def _get_architecture_from_metadata(self) -> str:
        for key, field in self._metadata_source().items():
            if "architecture" in key.lower() and isinstance(field, dict) and "value" in field:
                return field["value"]
        return "llama"

    def _calculate_file_type(self) -> int:
        """The reference's value, quirk included (module docstring); with llama_ftype the LLAMA_FTYPE id of the type that
        more than half of the tensors are written as, LLAMA_FTYPE_MIXED otherwise."""
        if self.llama_ftype:
            counts: Dict[str, int] = {}
            for p in self.plan():
                counts[p.type_name] = counts.get(p.type_name, 0) + 1
            top = max(counts, key=counts.get)
            return LLAMA_FTYPE.get(top, LLAMA_FTYPE_MIXED) if counts[top] / sum(counts.values()) > 0.5 else LLAMA_FTYPE_MIXED
        counts = {}
        for c in self.config.values():
            counts[c.bitwidth] = counts.get(c.bitwidth, 0) + 1
        dominant = max(counts, key=counts.get)  # the first-seen width among equals
        if counts[dominant] / len(self.config) > 0.5:
            return FILE_TYPE_BY_WIDTH.get(int(dominant), 12)
        return 12

    def _add_metadata_to_writer(self):
        """Every key of the source in its order with its recorded type; `general.architecture` is the writer's first key
        already; file_type and quantization_version come last."""
        w = self.writer
        for key, field in self._metadata_source().items():
            if key in SKIP_KEYS or key == "general.architecture":
                continue
            if not isinstance(field, dict) or "value" not in field:
                continue
            value, types = field["value"], field.get("types")
            if types:
                w.add(key, int(types[0]), value, int(types[1]) if len(types) > 1 else None)
            elif isinstance(value, str):  # a manifest without types: the reference's inference (:741-760)
                if value:
                    w.add_string(key, value)
            elif isinstance(value, bool):
                w.add_bool(key, value)
            elif isinstance(value, int):
                if 0 <= value < 2 ** 32:
                    w.add_uint32(key, value)
                elif -2 ** 31 <= value < 2 ** 31:
                    w.add(key, GGUFValueType.INT32, value)
                elif 0 <= value < 2 ** 64:
                    w.add(key, GGUFValueType.UINT64, value)
                else:
                    w.add(key, GGUFValueType.INT64, value)
            elif isinstance(value, float):
                w.add_float32(key, value)
            elif isinstance(value, list) and value:
                w.add_array(key, value)
        w.add_uint32("general.file_type", self._calculate_file_type())
        w.add_uint32("general.quantization_version", 2)

    # ---- resolving a tensor ----
    def _get_quantization_type_from_config(self, config: QuantizationConfig, original_quantization: str = "") -> str:
        """The NAME of the type a tensor is written as (:504-577): the explicit type of the level's file name, else the
        class of its width, where the level's own quantization decides between the members of a class."""
        if config.quant_type and config.quant_type in level_db.GGML_TYPE_IDS:
            return config.quant_type
        bw = config.bitwidth
        if bw == 32:
            return "F32"
        if bw == 16:
            return "F16"
        for low, high, exact, kept, fallback in WIDTH_CLASSES:
            if low <= bw <= high:
                if bw in exact:
                    return exact[bw]
                return next((t for t in kept if t in original_quantization), fallback)
        return "Q4_K"

    def _level_files(self, tensor_name: str, config: QuantizationConfig) -> Tuple[Path, Path, bool]:
        """(payload file, its metadata file, whether the `32-F32` fallback was taken) (:579-608)."""
        layer_dir = self.split_dir / tensor_name
        if not layer_dir.exists():
            raise FileNotFoundError(f"Layer directory not found: {layer_dir}")
        tensor_file = layer_dir / (config.filename or f"{config.bitwidth}.pth")
        candidates = [layer_dir / f"{tensor_file.name[:-4]}-metadata.json", layer_dir / f"{config.filename_prefix}-metadata.json"]
        metadata_file = next((m for m in candidates if m.exists()), candidates[0])
        fallback = False
        if not tensor_file.exists():
            if not (layer_dir / "32-F32.pth").exists():
                raise FileNotFoundError(f"Tensor file not found: {tensor_file}")
            print(f"Warning: Using fallback tensor file {layer_dir / '32-F32.pth'} for {tensor_name}")
            tensor_file, metadata_file, fallback = layer_dir / "32-F32.pth", layer_dir / "32-F32-metadata.json", True
        if not metadata_file.exists():
            if fallback or not (layer_dir / "32-F32-metadata.json").exists():
                raise FileNotFoundError(f"Metadata file not found: {metadata_file}")
            print(f"Warning: Using fallback metadata file {layer_dir / '32-F32-metadata.json'} for {tensor_name}")
            metadata_file = layer_dir / "32-F32-metadata.json"
        return tensor_file, metadata_file, fallback

    def _resolve(self, tensor_name: str, config: QuantizationConfig) -> _Planned:
        """Files, type and byte counts of one tensor, all checked; raises with the file's name on any inconsistency."""
        tensor_file, metadata_file, fallback = self._level_files(tensor_name, config)
        info = level_db.read_sidecar(tensor_file, metadata_file)
        if info.ggml_type is None:
            raise StitchError(f"{metadata_file}: no np_dtype / np_shape -- not a level of the GGUF side of the splitter")
        if fallback:  # the payload is the F32 one, whatever the configuration asked for
            config = QuantizationConfig(32.0, "32-F32.pth", "F32")
        type_name = self._get_quantization_type_from_config(config, info.quantization)
        if type_name not in WRITABLE:
            raise StitchError(f"tensor {tensor_name!r}: type {type_name} (level {tensor_file.name}) cannot be written; "
                              f"writable types are {sorted(WRITABLE)}")
        p = _Planned()
        p.name, p.type_name, p.ggml_type, p.path = tensor_name, type_name, WRITABLE[type_name], tensor_file
        p.shape = info.shape
        if info.nbytes is None:
            raise StitchError(f"{metadata_file}: np_dtype {info.np_dtype!r} is not one of {sorted(level_db.NP_ITEMSIZE)}")
        block, type_size = GGML_QUANT_SIZES[p.ggml_type]
        n_elements = int(np.prod(p.shape, dtype=np.int64))
        if not p.shape or p.shape[-1] % block:
            raise StitchError(f"{tensor_file}: rows of {p.shape[-1] if p.shape else 0} values are no multiple of {type_name}'s "
                              f"block of {block}")
        p.nbytes = n_elements // block * type_size
        on_disk = level_db.check_level_size(info, StitchError)
        if on_disk != p.nbytes:
            raise StitchError(f"{tensor_file}: {on_disk} bytes on disk, a {type_name} tensor of shape {p.shape} takes {p.nbytes}")
        return p

    def _check_metadata_source(self) -> None:
        """The key/value data must exist and must agree with the layout GGUFWriter gives the file."""
        source = self._metadata_source()
        if not source:
            raise StitchError(f"{self.split_dir}: no key/value data to write -- the original model was not found and "
                              f"manifest.json records none (a --both database keeps the HF side's manifest); pass --original-model")
        field = source.get("general.alignment")
        if isinstance(field, dict) and "value" in field and int(field["value"]) != ALIGNMENT:
            raise StitchError(f"general.alignment is {field['value']} in the source's key/value data; the writer lays tensors out "
                              f"at {ALIGNMENT} only")

    def plan(self) -> List[_Planned]:
        """Every tensor of the complete configuration, resolved, and the key/value source checked; raises StitchError listing
        ALL that failed.  The work is done once: later calls (stitch_model, file_type, verify) get the same list."""
        if self.planned is not None:
            return self.planned
        planned, failed = [], []
        try:
            self._check_metadata_source()
        except StitchError as e:
            failed.append(f"key/value data: {e}")
        n_other = len(failed)
        for name, config in self.config.items():
            try:
                planned.append(self._resolve(name, config))
            except (OSError, KeyError, ValueError, StitchError) as e:
                failed.append(f"{name}: {e}")
        if failed:
            raise StitchError(f"{len(failed) - n_other} tensors cannot be stitched:\n  " + "\n  ".join(failed))
        if not planned:
            raise StitchError(f"{self.split_dir}: no tensors could be prepared")
        self.planned = planned
        return planned

    # ---- writing ----
    def _read_payload(self, planned: _Planned) -> np.ndarray:
        """A tensor's bytes, read when the writer's pipeline reaches it."""
        return level_db.read_level_raw(planned)

    def stitch_model(self) -> Path:
        print(f"\n{'=' * 60}\nStarting model reconstruction...\n{'=' * 60}")
        print(f"Input directory: {self.split_dir}")
        print(f"Output file: {self.output_path}")
        print(f"Config file: {self.config_path if self.config_path else 'None (using defaults)'}")
        print(f"Default bitwidth: {self.default_bitwidth}")
        print(f"Default quant type: {self.default_quant_type}")
        planned = self.plan()  # every refusal comes before the output is opened
        arch = self._get_architecture_from_metadata()
        print(f"Architecture: {arch}")
        partial = self.output_path.with_name(self.output_path.name + ".partial")
        try:
            self.writer = GGUFWriter(str(partial), arch)
            self._add_metadata_to_writer()
            print(f"\nAdding {len(planned)} tensors to writer...")
            for p in planned:
                self.writer.add_tensor_lazy(p.name, p.shape, p.ggml_type, lambda p=p: self._read_payload(p))
            print("\nWriting GGUF file...")
            self.writer.write()
            os.replace(partial, self.output_path)
        except BaseException:
            if partial.exists():
                partial.unlink()
            raise
        finally:
            self.writer = None
        print(f"\n{'=' * 60}\nModel reconstruction complete!\n{'=' * 60}")
        print(f"Processed {len(planned)} tensors")
        print(f"Output saved to: {self.output_path}")
        widths, types = {}, {}
        for c in self.config.values():
            widths[c.bitwidth] = widths.get(c.bitwidth, 0) + 1
            if c.quant_type:
                types[c.quant_type] = types.get(c.quant_type, 0) + 1
        print("\nBitwidth distribution:")
        for bw, count in sorted(widths.items()):
            print(f"  {bw}-bit: {count} tensors")
        if types:
            print("\nQuantization type distribution:")
            for t, count in sorted(types.items()):
                print(f"  {t}: {count} tensors")
        return self.output_path

    def verify(self, device="cuda") -> int:
        """The file at output_path against the level files the configuration chose: read back through gguf_loader (mapped,
        decoded on the GPU) and compared bit for bit with level_db.load_level, tensor by tensor in file order.
        Raises StitchError naming the first tensor that differs; returns the number of tensors compared (Q8_0, IQ4_NL and
        IQ4_XS tensors are compared as stored bytes: the loader decodes them to fp32 and load_level to fp16, and equal bytes are the stricter
        check of the two)."""
        import torch
        from .gguf_loader import iter_gguf_tensors
        planned = {p.name: p for p in self.plan()}
        _, tensors, buf = parse_gguf(str(self.output_path), mmap=True)
        names = [t[0] for t in tensors]
        if names != list(planned):
            raise StitchError(f"{self.output_path}: tensors {sorted(set(planned) ^ set(names)) or 'in another order'} differ "
                              f"from the configuration's")
        compared = 0
        as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
        where = dict((t[0], t) for t in tensors)
        for name, got in iter_gguf_tensors(str(self.output_path), device, None, hf_layout=False, quant_dtype=torch.float16):
            p = planned[name]
            _, shape, ggml_type, off, nbytes = where[name]
            if ggml_type != p.ggml_type or tuple(shape) != p.shape:
                raise StitchError(f"verify: tensor {name!r} is type {ggml_type} of shape {tuple(shape)} in {self.output_path}, "
                                  f"level {p.path.name} is {p.type_name} of shape {p.shape}")
            if p.type_name in ("Q8_0", "IQ4_NL", "IQ4_XS"):
                same = bool(np.array_equal(np.asarray(buf[off:off + nbytes]), level_db.read_level_raw(p)))
            else:
                want = level_db.load_level(str(p.path), got.device).reshape(got.shape)
                same = want.dtype == got.dtype and torch.equal(got.view(as_int[got.element_size()]),
                                                               want.view(as_int[want.element_size()]))
            if not same:
                raise StitchError(f"verify: tensor {name!r} of {self.output_path} differs from level {p.path}")
            compared += 1
        print(f"Verified {compared} tensors of {self.output_path} against their level files: identical")
        return compared

    # ---- reports ----
    def validate_config(self) -> bool:
        """The reference's report (missing directories, levels without files and without the 32-F32 fallback) and then
        everything else plan() would refuse (byte counts, unwritable types): nothing is written."""
        print("Validating configuration...")
        missing, invalid = [], []
        for name, c in self.config.items():
            layer_dir = self.split_dir / name
            if not layer_dir.exists():
                missing.append(name)
                continue
            try:
                self._level_files(name, c)
            except FileNotFoundError:
                invalid.append((name, c))
        if missing:
            print(f"Error: Missing tensor directories: {missing}")
        if invalid:
            print("Error: Invalid configurations specified:")
            for name, c in invalid:
                available = sorted(f.name for f in (self.split_dir / name).glob("*.pth"))
                print(f"  {name}: requested {c.filename or f'{c.bitwidth}.pth'}, available: {available}")
        problems = ""
        try:
            self.plan()
        except StitchError as e:
            problems = str(e)
            print(f"Error: {problems}")
        ok = not missing and not invalid and not problems
        if ok:
            print("Configuration validation passed!")
        return ok

    def list_available_tensors(self):
        print("\n" + "=" * 60 + "\nAvailable tensors and configurations:\n" + "=" * 60)
        for name, levels in sorted(self.available_layers.items()):
            print(f"\n{name}:")
            for lv in sorted(levels, key=lambda c: c["bitwidth"]):
                quant = f" ({lv['quant_type']})" if lv["quant_type"] else ""
                print(f"  - {lv['bitwidth']}-bit{quant} [{lv['filename']}]")

    def inspect_metadata(self):
        def short(v):
            return v[:50] + "..." if isinstance(v, str) and len(v) > 50 else v

        def type_of(field):
            return "/".join(VALUE_TYPE_NAMES.get(t, str(t)) for t in field.get("types") or []) or None

        print("Metadata comparison:")
        om = self.original_metadata
        if om:
            print(f"\nOriginal model metadata: {len(om)} keys")
            print("Important model parameters:")
            for key in sorted(k for k in om if any(x in k.lower() for x in ("context_length", "vocab_size", "embedding_length",
                                                                            "block_count"))):
                print(f"  {key}: {om[key]['value']} (type: {type_of(om[key])})")
            print("\nFirst 10 metadata keys:")
            for key in sorted(om)[:10]:
                print(f"  {key}: {short(om[key]['value'])} (type: {type_of(om[key])})")
            if len(om) > 10:
                print(f"  ... and {len(om) - 10} more")
        if "metadata" in self.manifest:
            mm = self.manifest["metadata"]
            print(f"\nManifest metadata: {len(mm)} keys")
            for key in sorted(mm)[:10]:
                if isinstance(mm[key], dict) and "value" in mm[key]:
                    print(f"  {key}: {short(mm[key]['value'])}")
            if len(mm) > 10:
                print(f"  ... and {len(mm) - 10} more")


def stitch_search_result(db: str, hf_configuration_file: str, output_path: str, *, original_model: Optional[str] = None,
                         is_moe: Optional[bool] = None, verify: bool = False, device: str = "cuda",
                         llama_ftype: bool = False) -> Path:
    """From evo_quant_search's output file to a .gguf in one call: read the HF-named configuration, convert it
    (config_converter.convert_hf_to_gguf_config; is_moe None: detect_moe_model decides; a projection the search did not name
    gets the closest level to 32 bits its directory offers), stitch, and with `verify` read the file back on `device`."""
    text = read_config_file(str(hf_configuration_file))
    gguf_config = convert_hf_to_gguf_config(text, is_moe=detect_moe_model(text) if is_moe is None else is_moe)
    stitcher = GGUFStitcher(db, None, output_path, original_model, llama_ftype=llama_ftype, config_text=render_config(gguf_config),
                            quiet=True)
    out = stitcher.stitch_model()
    if verify:
        stitcher.verify(device)
    return out


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Reconstruct GGUF model from split layers with mixed bitwidths")
    p.add_argument("split_dir", help="Directory containing split model layers")
    p.add_argument("output_path", help="Output path for reconstructed GGUF model")
    p.add_argument("--config", help="Path to bitwidth configuration file (optional)")
    p.add_argument("--original-model", help="Path to original GGUF model (for metadata)")
    p.add_argument("--default-bitwidth", type=float, default=4.0,
                   help="Default bitwidth for tensors not in config (default: 4.0)")
    p.add_argument("--default-quant-type", default="Q4_K",
                   help="Default quantization type for tensors not in config (default: Q4_K)")
    p.add_argument("--validate-only", action="store_true", help="Only validate configuration without reconstructing")
    p.add_argument("--list-tensors", action="store_true", help="List available tensors and their configurations")
    p.add_argument("--inspect-metadata", action="store_true", help="Inspect metadata from different sources")
    p.add_argument("--llama-ftype", action="store_true",
                   help="write general.file_type as llama.cpp's LLAMA_FTYPE id instead of the reference's ggml type id")
    p.add_argument("--verify", action="store_true",
                   help="read the written file back on the GPU and compare every tensor with its level file, bit for bit")
    p.add_argument("--verify-only", action="store_true",
                   help="write nothing: compare the file already at output_path with the level files, as --verify does")
    p.add_argument("--device", default="cuda", help="GPU that decodes the file for --verify / --verify-only")
    a = p.parse_args(argv)
    stitcher = GGUFStitcher(a.split_dir, a.config, a.output_path, a.original_model, a.default_bitwidth, a.default_quant_type,
                            llama_ftype=a.llama_ftype)
    if a.inspect_metadata:
        stitcher.inspect_metadata()
        return 0
    if a.list_tensors:
        stitcher.list_available_tensors()
        return 0
    if a.validate_only:
        ok = stitcher.validate_config()
        print("Configuration is valid!" if ok else "Configuration has issues that need to be resolved.")
        return 0 if ok else 1
    if not stitcher.validate_config():
        print("Configuration validation failed. Please fix the issues and try again.")
        return 1
    if not a.verify_only:
        stitcher.stitch_model()
    if a.verify or a.verify_only:
        try:
            stitcher.verify(a.device)
        except StitchError as e:
            print(f"Error: {e}", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
