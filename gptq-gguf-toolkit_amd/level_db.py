"""The per-layer level database that gguf_splitter.py writes, and the only module that knows how it is laid out and named:

    <db>/<layer>/<bpw>[-<type>].pth      one level: a torch-saved dense tensor (--hf-layers) or raw GGUF bytes (--gguf-layers)
    <db>/<layer>/<stem>-metadata.json    its sidecar; `np_dtype` / `np_shape` in it mean raw GGUF bytes
    <db>/manifest.json                   the layers and the original file's key/value data
    <db>/gguf_layer_database.json        tensor name -> type / bit width / shape / offset, in the file's tensor order

Top to bottom: names -> directories -> sidecar -> manifest -> bytes on a device -> the ggml type tables -> the records and the
writer.  torch, ops and gguf_loader are imported where a tensor is made, so the readers that only look at names and JSON (the
stitcher's) need none.

The database has two producers.  gguf_splitter.py cuts a finished .gguf; LevelDbWriter (the one-pass level build,
quant.py --level_db) writes the same files without a .gguf in between.  Both take every JSON record from level_records, so
a reader cannot tell them apart -- except for what a database that never was a file cannot say:
  * no `original_file` in model_info and no `data_offset` / `data_offset_original` anywhere: there is no source file.  Nothing
    in the package reads the offsets; the stitcher, not finding an original model, takes the manifest's `metadata`;
  * layers[name]["bitwidths"] holds ALL levels of a tensor (splitting one file per level into one directory rewrites the
    manifest each time and leaves the last level only);
  * gguf_layer_database.json carries, per tensor, the record of the level registered LAST (the last level of --levels: what
    splitting the per-level files in that order leaves); its tensor order and manifest.json's are set_order's -- the order the
    converter writes for the model -- whatever order the tensors arrived in;
  * nothing is visible under <db> before close(): files are written under <db>.partial, which close() renames."""
import glob
import json
import os
import re
import shutil
import threading
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .gguf_writer import GGML_QUANT_SIZES, PLAIN_TYPES

# ------------------------------------------------------------------------------------------------ names
# Two rules read a level's file name, kept apart on purpose.  They agree on every name the splitter writes and differ on
# malformed ones only: level_key takes the float prefix of anything ("4-Q4_K.extra.pth" -> 4.0, "4..5.pth" -> 4.0, ".5.pth"
# refused), parse_level_name whole names only ("4-Q4_K.extra.pth" -> None, "4..5.pth" -> float()'s ValueError, ".5.pth" -> 0.5).
_NUM = re.compile(r"^[0-9]+(?:\.[0-9]+)?")
_LEVEL_FILE = re.compile(r"^([0-9.]+)(?:-([^.]+))?\.pth$")  # "<bw>-<type>.pth" / "<bw>.pth" (reference mapper/gguf_stitcher.py:89,99)

Levels = Dict[str, List[Tuple[float, str]]]


def level_stem(bitwidth, quantization: Optional[str] = None) -> str:
    """"4", "4.5", "4-Q4_K": the file-name stem of a level (reference mapper/gguf_splitter.py:560-566)."""
    stem = str(int(bitwidth)) if bitwidth == int(bitwidth) else str(bitwidth)
    return f"{stem}-{quantization}" if quantization is not None else stem


def level_type(filename: str) -> Optional[str]:
    """The type a typed level name carries ("4-Q4_K.pth" -> "Q4_K"), whatever its number is."""
    m = _LEVEL_FILE.match(filename)
    return m.group(2) if m else None


def parse_level_name(filename: str) -> Optional[Tuple[float, Optional[str]]]:
    """The stitcher's rule: (bit width, type or None) of "<bw>-<type>.pth" / "<bw>.pth", None for any other name."""
    m = _LEVEL_FILE.match(filename)
    return (float(m.group(1)), m.group(2)) if m else None


def level_key(filename: str) -> float:
    """The search's rule: the numeric prefix as a float, "4-Q4_K.pth" -> 4.0, "4.5-Q4_K.pth" -> 4.5, "3.pth" -> 3.0."""
    m = _NUM.match(filename[:-4] if filename.endswith(".pth") else filename)
    if not m:
        raise ValueError(f"level file {filename!r} does not start with a number")
    return float(m.group(0))


def level_files(layer_dir: str) -> List[str]:
    """The `.pth` files of one layer directory, ordered by numeric prefix (ties by name)."""
    return sorted((f for f in os.listdir(layer_dir) if f.endswith(".pth")), key=lambda f: (level_key(f), f))


def find_level_file(layer_dir: str, level) -> str:
    """The weight file of `level` in one layer directory: `<level>.pth` as the reference reads it (eval/ppleval.py:138), else
    level_stem's typed names.  `level` is a whole stem ("4-Q4_K") or a number alone ("4", 4, "4.5"), which must pick ONE file."""
    stem = str(level).strip()
    try:
        stem = level_stem(float(stem))
    except ValueError:
        pass
    exact = os.path.join(layer_dir, f"{stem}.pth")
    if os.path.isfile(exact):
        return exact
    typed = sorted(glob.glob(os.path.join(glob.escape(layer_dir), f"{glob.escape(stem)}-*.pth")))
    if len(typed) == 1:
        return typed[0]
    raise FileNotFoundError(f"{layer_dir}: no weight file for level {level!r} (looked for {stem}.pth and {stem}-<type>.pth, "
                            f"found {[os.path.basename(f) for f in typed]})")


def match_level(levels: Iterable[Tuple[float, object]], bitwidth: float):
    """The item of the first (key, item) pair whose key is `bitwidth` (|difference| < 1e-6, the reference's rule), or None."""
    return next((item for key, item in levels if abs(key - bitwidth) < 1e-6), None)


def filename_of(available_bitwidths: Levels, layer_name: str, bitwidth: float) -> Optional[str]:
    return match_level(available_bitwidths[layer_name], bitwidth)


def scan_available_bitwidths(quant_weights_path: str, layer_names: Optional[Sequence[str]] = None) -> Levels:
    """{layer name: [(bitwidth, file name), ...] sorted by bitwidth} (reference evopress/evo_quant_search.py:26-52).  Without
    layer_names every directory of the database is a layer, named as the directory; with them (HF module names) the
    directory is layer_dir's, which also finds the --gguf-layers layout."""
    if layer_names is None:
        layer_names = [n for n in os.listdir(quant_weights_path) if os.path.isdir(os.path.join(quant_weights_path, n))]
    return {n: [(level_key(f), f) for f in level_files(layer_dir(quant_weights_path, n))] for n in layer_names}


# ------------------------------------------------------------------------------------------------ directories
EXPERT_UNIT_ROLES = ("gate_proj", "up_proj", "down_proj")  # the three searchable units of a fused experts module


def expert_unit(layer_name: str) -> Optional[Tuple[str, str]]:
    """("<experts module name>", "gate" | "up" | "down") of an expert unit `<experts module name>.{gate,up,down}_proj` -- the
    names config_converter maps to `ffn_{gate,up,down}_exps.weight` --, None for any other name.  By name alone: the module
    is `...mlp.experts` of a decoder block."""
    mod, _, leaf = layer_name.rpartition(".")
    if leaf in EXPERT_UNIT_ROLES and mod.endswith(".mlp.experts"):
        return mod, leaf[:-len("_proj")]
    return None


def expert_unit_tensor(layer_name: str) -> Optional[str]:
    """`blk.N.ffn_{gate,up,down}_exps.weight` of the expert unit `model.layers.N.mlp.experts.{gate,up,down}_proj`, else None."""
    unit = expert_unit(layer_name)
    parts = layer_name.split(".")
    if parts[0] == "model":
        parts = parts[1:]
    if unit is None or len(parts) != 5 or parts[0] != "layers" or not parts[1].isdecimal():
        return None
    return f"blk.{parts[1]}.ffn_{unit[1]}_exps.weight"


def layer_dir(db: str, layer_name: str) -> str:
    """<db>/<HF module name> (gguf_splitter --hf-layers), else <db>/<GGUF tensor name> (--gguf-layers; an expert unit
    `<experts module>.{gate,up,down}_proj` is the stacked tensor `blk.N.ffn_{gate,up,down}_exps.weight`)."""
    d = os.path.join(db, layer_name)
    if os.path.isdir(d):
        return d
    from .pack_gptq_into_gguf import map_tensor_name
    try:
        g = os.path.join(db, expert_unit_tensor(layer_name) or map_tensor_name(layer_name + ".weight"))
    except ValueError:
        g = d
    if not os.path.isdir(g):
        raise FileNotFoundError(f"{db}: no directory for {layer_name}")
    return g


def has_layer(db: str, layer_name: str) -> bool:
    try:
        layer_dir(db, layer_name)
        return True
    except FileNotFoundError:
        return False


# ------------------------------------------------------------------------------------------------ sidecar
class LevelInfo:
    """What `<stem>-metadata.json` says of a level file.  ggml_type None: a torch-saved tensor (no sidecar, or the HF side's,
    without np_dtype / np_shape); the fields after it are unset then.  np_shape: the stored array, [R, C] values for plain
    types, [R, C / block * type_size] bytes for block types ([E, R, ..] for a stacked expert tensor); nbytes: what np_shape of
    np_dtype describes; shape: logical, outermost first ([R, C] or [E, R, C])."""
    __slots__ = ("path", "name", "quantization", "ggml_type", "np_dtype", "np_shape", "shape", "nbytes")


def read_sidecar(path, meta_path=None) -> LevelInfo:
    """The sidecar of level file `path` (`meta_path`: another file than `<stem>-metadata.json`, the stitcher's fallbacks)."""
    path = str(path)
    meta_path = str(meta_path) if meta_path is not None else path[:-4] + "-metadata.json"
    info = {}
    if os.path.isfile(meta_path):
        with open(meta_path) as f:
            info = json.load(f).get("tensor_info", {})
    rec = LevelInfo()
    rec.path, rec.name, rec.quantization = path, info.get("name", ""), info.get("quantization", "")  # name: the GGUF tensor's
    rec.ggml_type = rec.np_dtype = rec.np_shape = rec.shape = rec.nbytes = None
    if "np_dtype" in info and "np_shape" in info:
        rec.ggml_type, rec.np_dtype = int(info["type"]), info["np_dtype"]
        rec.np_shape = [int(n) for n in info["np_shape"]]
        rec.shape = tuple(int(n) for n in reversed(info["shape"]))  # "shape" is ggml's ne order, innermost first
        if rec.np_dtype in NP_ITEMSIZE:
            rec.nbytes = int(np.prod(rec.np_shape, dtype=np.int64)) * NP_ITEMSIZE[rec.np_dtype]
    return rec


def check_level_size(rec: LevelInfo, error=ValueError) -> int:
    """The size of a raw level file, which must be what its sidecar describes (else `error`)."""
    on_disk = os.path.getsize(rec.path)
    if on_disk != rec.nbytes:
        raise error(f"{rec.path}: {on_disk} bytes on disk, np_shape {rec.np_shape} of {rec.np_dtype} describes {rec.nbytes}")
    return on_disk


# ------------------------------------------------------------------------------------------------ manifest
def read_manifest(db, name: str = "manifest.json"):
    """`manifest.json` (or `gguf_layer_database.json`) of the database, None where it cannot be opened."""
    try:
        with open(os.path.join(str(db), name)) as f:
            return json.load(f)
    except OSError:
        return None


def rotary_rows(db: str, gguf_name: str, R: int, device):
    """gguf_loader.rotary_row_src with the manifest's architecture and head counts (opened for attn_q / attn_k only)."""
    from .gguf_loader import ROTARY_TENSORS, kv_int, rotary_row_src
    if not gguf_name.endswith(ROTARY_TENSORS):
        return None
    md = (read_manifest(db) or {}).get("metadata", {})
    val = lambda k: md[k]["value"] if k in md else None  # noqa: E731
    arch = val("general.architecture")
    n_head, n_kv = (kv_int(val(k), k) for k in (f"{arch}.attention.head_count", f"{arch}.attention.head_count_kv"))
    return rotary_row_src(gguf_name, R, arch, n_head, n_kv, device)


# ------------------------------------------------------------------------------------------------ bytes on a device
def read_level_raw(rec) -> np.ndarray:
    """The bytes of a raw level file (`rec.path`), as they lie on disk."""
    return np.fromfile(rec.path, dtype=np.uint8)


def load_level(path: str, device, db: Optional[str] = None):
    """One level's weight on `device`: a torch-saved tensor (--hf-layers) as it is; raw GGUF bytes (--gguf-layers) as a view
    for plain types, decoded to fp16 by ops.dequantize_blocks for K-quants, Q8_0, IQ4_NL and IQ4_XS, with the manifest's q / k
    row gather if `db`."""
    import torch
    rec = read_sidecar(path)
    if rec.ggml_type is None:
        return torch.load(path, map_location=device)
    from . import ops
    raw = torch.from_numpy(read_level_raw(rec)).to(device)
    lead = rec.np_shape[:-1]  # [R], or [E, R] of a stacked expert tensor (no row gather: not a rotary tensor)
    rows = rotary_rows(db, rec.name, rec.np_shape[0], device) if db and len(lead) == 1 else None
    if rec.ggml_type in PLAIN_TYPES:
        w = raw.view(getattr(torch, PLAIN_TYPES[rec.ggml_type][0])).reshape(rec.np_shape)
        return w[rows.long()] if rows is not None else w
    w = ops.dequantize_blocks(rec.ggml_type, raw.view(int(np.prod(lead, dtype=np.int64)), -1), torch.float16, rows)
    return w if len(lead) == 1 else w.view(*rec.shape)


# ------------------------------------------------------------------------------------------------ ggml type tables
# every type name the reference knows (mapper/gguf_stitcher.py:272-314) -> ggml type id
GGML_TYPE_IDS = {"F32": 0, "F16": 1, "Q4_0": 2, "Q4_1": 3, "Q5_0": 6, "Q5_1": 7, "Q8_0": 8, "Q8_1": 9, "Q2_K": 10, "Q3_K": 11,
                 "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "Q8_K": 15, "IQ2_XXS": 16, "IQ2_XS": 17, "IQ3_XXS": 18, "IQ1_S": 19,
                 "IQ4_NL": 20, "IQ3_S": 21, "IQ2_S": 22, "IQ4_XS": 23, "I8": 24, "I16": 25, "I32": 26, "I64": 27, "IQ1_M": 29,
                 "BF16": 30, "IQ2_M": None, "IQ3_M": None}  # IQ2_M / IQ3_M are file types, not tensor types
BIT_WIDTHS = {"F32": 32.0, "F16": 16.0, "BF16": 16.0, "I8": 8.0, "I16": 16.0, "I32": 32.0, "I64": 64.0, "Q4_0": 4.5, "Q4_1": 5.0,
              "Q5_0": 5.5, "Q5_1": 6.0, "Q8_0": 8.5, "Q8_1": 9.0, "Q2_K": 2.5625, "Q3_K": 3.4375, "Q4_K": 4.5, "Q5_K": 5.5,
              "Q6_K": 6.5625, "Q8_K": 8.5, "IQ2_XXS": 2.0625, "IQ2_XS": 2.3125, "IQ2_S": 2.5, "IQ2_M": 2.7, "IQ3_XXS": 3.0625,
              "IQ3_S": 3.44, "IQ3_M": 3.66, "IQ4_NL": 4.56, "IQ4_XS": 4.25, "IQ1_S": 1.5625, "IQ1_M": 1.75}  # :232-268
# numpy dtype names a sidecar may carry -> item size: bytes of block types, and the plain types' own
NP_ITEMSIZE = {"uint8": 1, "int8": 1, **{np_name: size for _, np_name, size in PLAIN_TYPES.values()}}


# Views of the tables on the types the reference's splitter names (mapper/gguf_splitter.py:42-50, :56-96; + BF16), narrow on
# purpose: any other name ("IQ2_XS") keeps the exact width 32.0 there (resolve_hf_bitwidth with --exact), not the full table's.
# IQ4_NL / IQ4_XS are the two IQ types whose bytes this package reads (include/gptq_gguf_iq4.h): their levels are named and
# sized as the reference's splitter does, "4.56-IQ4_NL.pth" / "4.25-IQ4_XS.pth".
SPLIT_TYPES = ("F32", "F16", "Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0", "Q8_1", "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K", "BF16",
               "IQ4_NL", "IQ4_XS")
TYPE_NAMES = {GGML_TYPE_IDS[name]: name for name in SPLIT_TYPES}
EXACT_BITS = {name: BIT_WIDTHS[name] for name in SPLIT_TYPES}


# ------------------------------------------------------------------------------------------------ records
def level_records(name: str, shape: Sequence[int], ggml_type: int, quantization: str, bitwidth, exact_bitwidth: float,
                  nbytes: int, stem: str, data_offset: Optional[int] = None):
    """The three JSON records of one level of one tensor -- the ONE definition the splitter and the writer share:
    (sidecar `tensor_info`, its entry of manifest layers[name]["bitwidths"], its gguf_layer_database.json record).  `shape` is
    logical, outermost first; `data_offset` (the splitter's: where the bytes lay in the source file) is left out when None."""
    shape = [int(n) for n in shape]
    bs, ts = GGML_QUANT_SIZES[ggml_type]
    if bs > 1:
        np_dtype, np_shape = "uint8", [*shape[:-1], shape[-1] // bs * ts]
    else:
        np_dtype, np_shape = PLAIN_TYPES[ggml_type][1], list(shape)
    off = lambda key: {} if data_offset is None else {key: data_offset}  # noqa: E731
    common = {"type": ggml_type, "quantization": quantization, "bitwidth": bitwidth, "exact_bitwidth": exact_bitwidth,
              "shape": list(reversed(shape)), "n_elements": int(np.prod(shape))}  # "shape": ggml ne order
    sidecar = {"name": name, **common, "n_bytes": nbytes, **off("data_offset_original"), "data_filename": f"{stem}.pth",
               "np_dtype": np_dtype, "np_shape": np_shape}
    level = {"filename": f"{stem}.pth", "metadata_filename": f"{stem}-metadata.json", **common, "size_bytes": nbytes,
             **off("data_offset")}
    record = {"tensor_type": ggml_type, "quantization": quantization, "bitwidth": bitwidth, "exact_bitwidth": exact_bitwidth,
              "shape": list(reversed(shape)), "n_elements": int(np.prod(shape)), "n_bytes": nbytes, **off("data_offset")}
    return sidecar, level, record


def write_sidecar(path, sidecar: dict) -> None:
    with open(path, "w") as f:
        f.write(json.dumps({"tensor_info": sidecar}, indent=2))


def write_manifests(db, manifest: dict, database: dict) -> None:
    with open(os.path.join(str(db), "manifest.json"), "w") as f:
        f.write(json.dumps(manifest, indent=2))
    with open(os.path.join(str(db), "gguf_layer_database.json"), "w") as f:
        f.write(json.dumps(database, indent=2))


# ------------------------------------------------------------------------------------------------ writer
class LevelDbWriter:
    """Writes what `GGUFSplitter(..., use_exact_bitwidth=True).split_gguf_model()` writes, level by level and without a
    .gguf (the differences: module docstring).  register() books one level and returns where its bytes go -- the driver's
    writer process fills the file --, add_level() also writes them; set_metadata / set_order may come at any time before
    close(), which checks every file against its sidecar, writes manifest.json and gguf_layer_database.json in set_order's
    order and renames <db>.partial to <db>.  abort() (and leaving a `with` block by an exception) removes the partial
    directory: a failed run leaves nothing that looks like a database.  Thread-safe."""

    def __init__(self, db):
        self.db = os.path.abspath(str(db))
        self.tmp = self.db + ".partial"
        if os.path.lexists(self.db):
            raise FileExistsError(f"{self.db} exists: a level database is written whole (remove it, or name another directory)")
        if os.path.isdir(self.tmp):
            shutil.rmtree(self.tmp)  # what a failed run left
        os.makedirs(self.tmp)
        self._layers: Dict[str, dict] = {}    # tensor -> manifest layer record, in arrival order
        self._records: Dict[str, dict] = {}   # tensor -> database record of its last level
        self._files: List[str] = []
        self._order: List[str] = []
        self._metadata: Dict[str, dict] = {}
        self._lock = threading.Lock()
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *_):
        if exc_type is not None:
            self.abort()
        elif not self._closed:
            self.close()
        return False

    def set_metadata(self, kv) -> None:
        """The key/value data: {key: (value, [value type ids])} as gguf_writer.parse_gguf / kv_records give it."""
        self._metadata = {key: {"types": list(types), "value": value} for key, (value, types) in kv.items()}

    def set_order(self, names: Iterable[str]) -> None:
        """Tensor names in the file's order; tensors it does not name follow in arrival order."""
        self._order = list(names)

    def register(self, name: str, shape: Sequence[int], ggml_type: int) -> str:
        """Book one level of GGUF tensor `name` (logical `shape`, outermost first) and write its sidecar -> the path its raw
        bytes belong at (under <db>.partial).  A tensor's levels are registered in the order of --levels: the last one is its
        gguf_layer_database.json record."""
        if self._closed:
            raise RuntimeError("LevelDbWriter is closed")
        ggml_type = int(ggml_type)
        if ggml_type not in TYPE_NAMES or ggml_type not in GGML_QUANT_SIZES:
            raise ValueError(f"tensor {name!r}: ggml type {ggml_type} cannot be a level")
        shape = [int(n) for n in shape]
        bs, ts = GGML_QUANT_SIZES[ggml_type]
        if not shape or shape[-1] % bs:
            raise ValueError(f"tensor {name!r}: rows of {shape[-1] if shape else 0} values are no multiple of the block of {bs}")
        q = TYPE_NAMES[ggml_type]
        bitwidth = EXACT_BITS[q]
        stem = level_stem(bitwidth, q)
        nbytes = int(np.prod(shape, dtype=np.int64)) // bs * ts
        sidecar, level, record = level_records(name, shape, ggml_type, q, bitwidth, bitwidth, nbytes, stem)
        d = os.path.join(self.tmp, name)
        with self._lock:
            os.makedirs(d, exist_ok=True)
            layer = self._layers.setdefault(name, {"original_name": name, "dims": list(reversed(shape)), "bitwidths": {}})
            if str(bitwidth) in layer["bitwidths"]:
                raise ValueError(f"tensor {name!r}: level {stem} registered twice")
            layer["bitwidths"][str(bitwidth)] = level
            self._records[name] = record
            path = os.path.join(d, f"{stem}.pth")
            self._files.append(path)
        write_sidecar(os.path.join(d, f"{stem}-metadata.json"), sidecar)
        return path

    def add_level(self, name: str, shape: Sequence[int], ggml_type: int, data) -> str:
        """register() and write the bytes: `data` is bytes-like or a C-contiguous numpy array of the level's byte count."""
        path = self.register(name, shape, ggml_type)
        buf = memoryview(np.ascontiguousarray(data)).cast("B") if isinstance(data, np.ndarray) else memoryview(data)
        with open(path, "wb") as f:
            f.write(buf)
        return path

    def abort(self) -> None:
        self._closed = True
        shutil.rmtree(self.tmp, ignore_errors=True)

    def close(self) -> str:
        """Check, write the two manifests, rename -> <db>.  Any failure aborts: no <db> appears."""
        if self._closed:
            raise RuntimeError("LevelDbWriter is closed")
        try:
            for path in self._files:  # every booked file is there and as long as its sidecar says
                if not os.path.isfile(path):
                    raise FileNotFoundError(f"{path}: registered, never written")
                check_level_size(read_sidecar(path))
            rank = {n: i for i, n in enumerate(self._order)}
            names = sorted(self._layers, key=lambda n: rank.get(n, len(rank)))  # stable: the rest keeps arrival order
            manifest = {"model_info": {"total_tensors": len(names), "split_timestamp": time.time(), "use_exact_bitwidth": True,
                                       "processed_tensors": len(names)},
                        "metadata": self._metadata, "layers": {n: self._layers[n] for n in names}}
            write_manifests(self.tmp, manifest, {n: self._records[n] for n in names})
            os.rename(self.tmp, self.db)
        except BaseException:
            self.abort()
            raise
        self._closed = True
        return self.db
