"""Every level of every Linear of a per-layer level database, resident on the device in the form it is stored in, and the
switch of the model from one level assignment to another in ONE kernel call (ops.level_switch / gq_level_switch).

    store = LevelStore(model, db, device)          # uploads each level once; packed GGUF bytes stay packed
    store.switch({"model.layers.0.mlp.up_proj": 4.0, ...})   # or the search's nested lists; decodes into weight.data

The reference's load_layers (evopress/evo_quant_search.py:110-138) reads a dense [R, C] file per changed Linear and per
candidate.  Here a switch reads the stored level where it lies on the device and writes the Linear's existing weight
storage: no file, no host copy, no [R, C] temporary, no reallocation (weight.data_ptr() does not change).

Both database layouts of gguf_splitter are read, through level_db:
  --hf-layers   <db>/<HF module name>/<bpw>-<Qn_K>.pth   torch-saved dense tensors: kept dense in their own dtype; a switch
                is a cast copy with .to(dtype) rounding, so the weight equals torch.load(file).to(dtype) bit for bit;
  --gguf-layers <db>/<GGUF tensor name>/<bpw>.pth + -metadata.json   raw block bytes (K-quants, Q8_0, IQ4_NL, IQ4_XS): kept packed; a switch decodes them
                (with the q / k rotary row gather of the manifest) straight to the weight dtype.  For fp16 weights that is
                level_db.load_level(file).to(dtype) bit for bit; for bf16 / fp32 weights the value is rounded ONCE
                from the fp32 decode, where load_level's fp16 tensor followed by .to(dtype) rounds twice.

resident="packed" (default "dense") keeps NO dense live copy: every held Linear becomes a packed_linear.PackedLinear whose
forward reads the current level's block bytes (ops.linear_packed), its dense storage is freed, and a switch is a change of
references -- no launch, no device memory moves.  The levels must then be packed (K-quants, Q8_0, IQ4_NL, IQ4_XS) or dense in the model's
dtype; fp16 / bf16 models only.

Besides nn.Linear names the store takes EXPERT UNITS, `<experts module name>.{gate_proj,up_proj,down_proj}` (the names
config_converter maps to `blk.N.ffn_{gate,up,down}_exps.weight`): the three stacked [E, R, C] tensors of a module that keeps its
experts the way transformers' MixtralExperts does (packed_experts.experts_shaped: gate_up_proj [E, 2I, H], down_proj [E, H, I]).
A unit is one searchable layer with all its levels resident.  Dense residency: a switch adds ONE stacked job per changed unit
(ops.level_switch_experts / gq_level_switch_experts) that decodes the E experts into the unit's slice of the fused parameter
-- gate rows [0, I) and up rows [I, 2I) of every expert of gate_up_proj, or down_proj --; the parameters' data_ptr()s do not
change.  Packed residency: the module becomes a packed_experts.PackedExperts (its dense parameters freed and credited) and a
switch is PackedExperts.set_level(role, blocks, kind), no launch; all three units of a module must then be held.
One rank.  nn.Linear and expert units only: per-expert w1 / w2 / w3 layouts are refused."""
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import level_db, ops, packed_experts, packed_linear
from .gguf_writer import PACKED_TYPES, PLAIN_TYPES

_DENSE = (torch.float32, torch.float16, torch.bfloat16)

State = Union[Dict[str, float], Sequence[Sequence[float]]]


class _Level:
    """One stored level: what its sidecar says (`info`) and, after upload, where it is on the device."""
    __slots__ = ("info", "key", "file", "kind", "nbytes", "dtype", "data", "rows")


def packed_peak_bytes(level_bytes: Sequence[int], dense_bytes: Sequence[int]) -> int:
    """The most device memory packed residency takes beyond what is held at its start: Linear i (in upload order) first
    frees dense_bytes[i] -- its dense weight --, then level_bytes[i] -- all its levels -- are uploaded.  Negative when
    the model shrinks from the first Linear on.  Pure arithmetic."""
    held, peak = 0, None
    for lv, dn in zip(level_bytes, dense_bytes):
        held += int(lv) - int(dn)
        peak = held if peak is None else max(peak, held)
    return 0 if peak is None else peak


def packed_fits(level_bytes: Sequence[int], dense_bytes: Sequence[int], capacity_bytes: int) -> bool:
    """Whether the levels fit `capacity_bytes` of free device memory once the bytes that installing PackedLinear frees are
    credited (packed_peak_bytes)."""
    return packed_peak_bytes(level_bytes, dense_bytes) <= int(capacity_bytes)


class LevelStore:

    def __init__(self, model: nn.Module, db: str, device, layer_names: Optional[Sequence[str]] = None,
                 capacity_bytes: Optional[int] = None, resident: str = "dense", moe_prefill: str = "loop"):
        """layer_names: the Linears and expert units to hold (default: every nn.Linear of the model that has a directory in
        `db`, and the units `<module>.{gate,up,down}_proj` of every experts-shaped module that have one).
        capacity_bytes: the device memory the levels may take (default: what torch reports free on `device`).
        resident: "dense" -- the model keeps its nn.Linear weights and a switch decodes into them; "packed" -- the Linears
        become PackedLinear, their dense weights are freed (credited in the capacity check) and a switch swaps references.
        moe_prefill: packed residency's PackedExperts.prefill ("loop" or "grouped")."""
        if resident not in ("dense", "packed"):
            raise ValueError(f"resident must be 'dense' or 'packed', got {resident!r}")
        if moe_prefill not in ("loop", "grouped"):
            raise ValueError(f"moe_prefill must be 'loop' or 'grouped', got {moe_prefill!r}")
        self.resident, self.freed_bytes, self.moe_prefill = resident, 0, moe_prefill
        self.model, self.db, self.device = model, db, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # "cuda" -> the current device, as tensors report it
            self.device = torch.device("cuda", torch.cuda.current_device())
        if layer_names is None:
            layer_names = default_layer_names(model, db)
        self.layers: Dict[str, nn.Module] = {}        # a Linear, or the experts module of a unit
        self.units: Dict[str, Tuple[str, str]] = {}   # expert unit -> (experts module name, "gate" | "up" | "down")
        self.levels: Dict[str, List[_Level]] = {}
        need, per_layer, layer, credited = 0, [], None, set()
        for name in layer_names:  # pass 1: the files only -- every refusal comes before the first upload
            layer, unit = resolve_layer(model, name)
            if unit is not None:
                self.units[name] = unit
            self.layers[name], self.levels[name] = layer, []
            dtype = self._dtype(name)
            if dtype not in _DENSE:
                raise TypeError(f"{name}: weight dtype {dtype} is not fp32 / fp16 / bf16")
            ldir = level_db.layer_dir(db, name)
            if resident == "packed" and dtype not in (torch.float16, torch.bfloat16):
                raise TypeError(f"{name}: packed residency computes in fp16 / bf16, the weight is {dtype}: use "
                                f"dense residency")
            for f in level_db.level_files(ldir):
                lv = self._inspect(os.path.join(ldir, f), name)
                if resident == "packed" and lv.kind is None and lv.dtype != dtype:
                    what = "a torch-saved dense tensor" if lv.info.ggml_type is None else f"a plain {lv.dtype} matrix"
                    raise ValueError(f"{os.path.join(ldir, f)}: {what}, neither packed blocks nor dense in the model's dtype "
                                     f"({dtype}): packed residency cannot hold this level of {name}, use dense "
                                     f"residency")
                self.levels[name].append(lv)
                need += lv.nbytes
            if not self.levels[name]:
                raise FileNotFoundError(f"{ldir}: no level file for {name}")
            if unit is None:
                dense = packed_linear.dense_bytes(layer)
            else:  # the whole module is freed when its first unit is installed: credited there, once
                dense = 0 if unit[0] in credited else _experts_dense_bytes(layer)
                credited.add(unit[0])
            per_layer.append((sum(lv.nbytes for lv in self.levels[name]), dense))
        del layer
        if resident == "packed":  # PackedExperts computes with all three of its levels
            for mod in credited:
                missing = [f"{mod}.{r}" for r in level_db.EXPERT_UNIT_ROLES if f"{mod}.{r}" not in self.units]
                if missing:
                    raise ValueError(f"{mod}: packed residency needs all three expert units of a module, {missing} are not held")
        if capacity_bytes is None:
            capacity_bytes = torch.cuda.mem_get_info(self.device)[0] if self.device.type == "cuda" else None
        if resident == "packed":
            lvb, dnb = [a for a, _ in per_layer], [b for _, b in per_layer]
            if capacity_bytes is not None and not packed_fits(lvb, dnb, capacity_bytes):
                raise MemoryError(f"the levels of {db} need {need} bytes on {self.device}, at most "
                                  f"{packed_peak_bytes(lvb, dnb)} beyond what is held now once the {sum(dnb)} bytes of the "
                                  f"dense weights are freed; {capacity_bytes} are available "
                                  f"({sum(len(v) for v in self.levels.values())} levels of {len(self.levels)} Linears)")
        elif capacity_bytes is not None and need > capacity_bytes:
            raise MemoryError(f"the levels of {db} need {need} bytes on {self.device}, {capacity_bytes} are available "
                              f"({sum(len(v) for v in self.levels.values())} levels of {len(self.levels)} Linears)")
        self._rows: Dict[Tuple[str, int], Optional[torch.Tensor]] = {}
        for name, lvs in self.levels.items():  # pass 2: upload, each level once
            if resident == "packed" and name in self.units:  # the module's first unit frees its dense parameters
                mod = self.units[name][0]
                if not isinstance(self.layers[name], packed_experts.PackedExperts):
                    self.freed_bytes += _experts_dense_bytes(self.layers[name])
                    packed = packed_experts.replace_experts(model, mod, moe_prefill)
                    for other, (m, _) in self.units.items():
                        if m == mod:
                            self.layers[other] = packed
            elif resident == "packed":  # the dense weight goes first, so that the peak is packed_peak_bytes'
                self.freed_bytes += packed_linear.dense_bytes(self.layers[name])
                self.layers[name] = packed_linear.replace_linear(model, name)
            for lv in lvs:
                self._upload(name, lv)
        self.state: Dict[str, Optional[float]] = {name: None for name in self.layers}
        self.jobs_issued = 0  # jobs of all switches so far (the diff is observable)

    # ---- construction ----
    def shape_of(self, name: str) -> Tuple[int, ...]:
        """The logical shape of a held layer: a Linear's [R, C]; a unit's [E, I, H] (gate, up) or [E, H, I] (down)."""
        if name not in self.units:
            return tuple(self.layers[name].weight.shape)
        E, H, I = self.layers[name].down_proj.shape
        return (E, H, I) if self.units[name][1] == "down" else (E, I, H)

    def _dtype(self, name: str) -> torch.dtype:
        return self.layers[name].down_proj.dtype if name in self.units else self.layers[name].weight.dtype

    def _live(self, name: str) -> torch.Tensor:
        """Dense residency: the storage a switch of `name` writes -- a Linear's weight, or a unit's [E, R, C] view of the fused
        parameter (expert stride 2 I H for gate and up)."""
        if name not in self.units:
            w = self.layers[name].weight.data
            if w.device != self.device or not w.is_contiguous():
                raise RuntimeError(f"{name}: the weight must be contiguous and on {self.device} (it is on {w.device})")
            return w
        m, role = self.layers[name], self.units[name][1]
        p = (m.down_proj if role == "down" else m.gate_up_proj).data
        if p.device != self.device or not p.is_contiguous():
            raise RuntimeError(f"{name}: the fused parameter must be contiguous and on {self.device} (it is on {p.device})")
        I = m.down_proj.shape[2]
        return p if role == "down" else p[:, :I] if role == "gate" else p[:, I:]

    def _inspect(self, path: str, name: str) -> _Level:
        lv = _Level()
        lv.info, lv.file, lv.key = level_db.read_sidecar(path), os.path.basename(path), level_db.level_key(os.path.basename(path))
        lv.data = lv.rows = lv.kind = lv.dtype = None
        gt, want = lv.info.ggml_type, self.shape_of(name)
        if gt is None:  # torch-saved: the shape is only known after loading; the file size bounds the bytes
            lv.nbytes = os.path.getsize(path)
            return lv
        if gt in PLAIN_TYPES:
            lv.dtype = getattr(torch, PLAIN_TYPES[gt][0])
        elif gt in PACKED_TYPES:
            lv.kind, lv.dtype = int(gt), torch.uint8
        else:
            raise ValueError(f"{path}: ggml type {gt} is not a K-quant, Q8_0, IQ4_NL, IQ4_XS or a plain fp32 / fp16 / bf16 matrix")
        if lv.info.shape != want:
            raise ValueError(f"{name}: level {lv.file!r} has shape {lv.info.shape}, the {self._what(name)} {want}")
        lv.nbytes = level_db.check_level_size(lv.info)
        return lv

    def _what(self, name: str) -> str:
        return "expert unit" if name in self.units else "Linear"

    def _upload(self, name: str, lv: _Level) -> None:
        want = self.shape_of(name)
        if lv.info.ggml_type is None:  # a torch-saved dense tensor (--hf-layers): kept as saved
            t = torch.load(lv.info.path, map_location="cpu")
            if tuple(t.shape) != want:
                raise ValueError(f"{name}: level {lv.file!r} has shape {tuple(t.shape)}, the {self._what(name)} {want}")
            if t.dtype not in _DENSE:
                t = t.float()
            lv.dtype, lv.data = t.dtype, t.contiguous().to(self.device)
        else:  # raw bytes: packed levels stay packed, dense ones stay in their dtype
            raw = torch.from_numpy(level_db.read_level_raw(lv.info)).to(self.device)
            lv.data = raw if lv.kind is not None else raw.view(lv.dtype).reshape(lv.info.np_shape)
            if name in self.units:  # a stacked expert tensor: rows as stored, no rotary gather
                lv.nbytes = lv.data.numel() * lv.data.element_size()
                return
            key = (lv.info.name.rsplit(".", 2)[-2] if lv.info.name.count(".") >= 2 else "", want[0])
            if key not in self._rows:  # the q / k row gather, built once per (tensor kind, R)
                self._rows[key] = level_db.rotary_rows(self.db, lv.info.name, want[0], self.device)
            lv.rows = self._rows[key]
        if self.resident == "packed" and lv.kind is None and lv.rows is not None:
            lv.data, lv.rows = lv.data[lv.rows.long()].contiguous(), None  # F.linear takes the level as it lies: gather once
        lv.nbytes = lv.data.numel() * lv.data.element_size()

    # ---- use ----
    def bytes(self) -> int:
        """Device memory held: every level as stored, plus the row-gather index vectors."""
        held = sum(lv.nbytes for lvs in self.levels.values() for lv in lvs)
        return held + sum(r.numel() * 4 for r in self._rows.values() if r is not None)

    def level_keys(self, name: str) -> List[float]:
        return [lv.key for lv in self.levels[name]]

    def find(self, name: str, key) -> _Level:
        """The level of `name` whose numeric prefix is `key` (|difference| < 1e-6, as the reference matches bitwidths) or
        whose file name / stem is `key`."""
        lv = (next((lv for lv in self.levels[name] if key in (lv.file, lv.file[:-4])), None) if isinstance(key, str)
              else level_db.match_level(((lv.key, lv) for lv in self.levels[name]), float(key)))
        if lv is not None:
            return lv
        raise KeyError(f"{name}: no level {key!r} (have {[lv.file for lv in self.levels[name]]})")

    def flatten(self, state: State, grouped_layer_names=None) -> Dict[str, float]:
        if isinstance(state, dict):
            return state
        if grouped_layer_names is None:
            grouped_layer_names = self.grouped_layer_names
        return {n: k for names, keys in zip(grouped_layer_names, state) for n, k in zip(names, keys)}

    grouped_layer_names: Optional[Sequence[Sequence[str]]] = None  # set by the search: the meaning of nested-list states

    @torch.no_grad()
    def switch(self, state: State) -> int:
        """Make `state` ({layer_name: level key} or the search's nested lists) current: the Linears whose level differs
        from the recorded one are rewritten, in place, by ONE ops.level_switch call.  Layers the state does not name keep
        their level.  Returns the number of Linears rewritten; no host read."""
        flat = self.flatten(state)
        if self.resident == "packed":
            return self._switch_packed(flat)
        jobs, stacked, new = [], [], {}
        for name, key in flat.items():
            lv = self.find(name, key)
            if self.state[name] is not None and self.state[name] == lv.key:
                continue
            if name in self.units:  # ONE job for the E experts of the unit
                stacked.append((lv.data, self._live(name), lv.kind))
            else:
                jobs.append((lv.data, self._live(name), lv.kind, lv.rows))
            new[name] = lv.key
        ops.level_switch(jobs)
        ops.level_switch_experts(stacked)
        self.state.update(new)
        self.jobs_issued += len(jobs) + len(stacked)
        return len(jobs) + len(stacked)

    def _switch_packed(self, flat: Dict[str, float]) -> int:
        """Packed residency: the Linears whose level differs get references to the stored level (PackedLinear.set_level).
        No launch (jobs_issued does not move), no allocation."""
        n = 0
        for name, key in flat.items():
            lv = self.find(name, key)
            if self.state[name] is not None and self.state[name] == lv.key:
                continue
            if name in self.units:
                self.layers[name].set_level(self.units[name][1], lv.data, lv.kind)
            else:
                self.layers[name].set_level(lv.data, lv.kind, lv.rows)
            self.state[name] = lv.key
            n += 1
        return n

    def weight_of(self, name: str, key, dtype=None) -> torch.Tensor:
        """A fresh tensor holding level `key` of `name` in `dtype` (default: the layer's), decoded by the same call
        as a switch; the model is not touched.  [R, C] for a Linear, [E, R, C] for an expert unit."""
        lv = self.find(name, key)
        out = torch.empty(self.shape_of(name), dtype=dtype or self._dtype(name), device=self.device)
        if name in self.units:
            ops.level_switch_experts([(lv.data, out, lv.kind)])
        else:
            ops.level_switch([(lv.data, out, lv.kind, lv.rows)])
        return out

    def level_tensor(self, name: str, key) -> torch.Tensor:
        """Level `key` of `name` as level_db.load_level returns it: the stored dense tensor itself (no copy), or
        the packed blocks decoded to fp16."""
        lv = self.find(name, key)
        if lv.kind is None and lv.rows is None:
            return lv.data
        return self.weight_of(name, key, dtype=torch.float16 if lv.kind is not None else lv.dtype)


# ---- the layers a store can hold ----
def _experts_dense_bytes(layer: nn.Module) -> int:
    """The device bytes the two fused parameters of an experts module hold (0 for tensors without storage)."""
    return sum(t.numel() * t.element_size() for t in (layer.gate_up_proj, layer.down_proj) if t.device.type != "meta")


def resolve_layer(model: nn.Module, name: str):
    """(module, unit) of a layer name: an nn.Linear and None, or the experts module of the expert unit
    `<experts module name>.{gate_proj,up_proj,down_proj}` and (module name, role).  Anything else is refused by name."""
    try:
        layer = model.get_submodule(name)
    except AttributeError:
        layer = None
    if isinstance(layer, nn.Linear):
        return layer, None
    mod, _, leaf = name.rpartition(".")
    if layer is None and leaf in level_db.EXPERT_UNIT_ROLES and mod:
        try:
            experts = model.get_submodule(mod)
        except AttributeError:
            raise TypeError(f"LevelStore: {name} is neither a module of the model nor an expert unit ({mod} does not "
                            f"exist)") from None
        if packed_experts.experts_shaped(experts):
            return experts, (mod, leaf[:-len("_proj")])
        if any(n.rpartition(".")[2] in ("w1", "w2", "w3") for n, _ in experts.named_modules()):
            raise TypeError(f"LevelStore: {name}: {mod} keeps its experts as per-expert w1 / w2 / w3 Linears (a "
                            f"{type(experts).__name__}); expert units need the fused layout gate_up_proj [E, 2I, H] / down_proj "
                            f"[E, H, I]")
        raise TypeError(f"LevelStore: {name}: {mod} is a {type(experts).__name__} without gate_up_proj [E, 2I, H] and down_proj "
                        f"[E, H, I]: not an experts module an expert unit can name")
    if layer is None:
        raise TypeError(f"LevelStore: {name} is neither a module of the model nor an expert unit "
                        f"(<experts module>.gate_proj / .up_proj / .down_proj)")
    raise TypeError(f"LevelStore supports nn.Linear and expert units only, {name} is a {type(layer).__name__}")


def default_layer_names(model: nn.Module, db: str) -> List[str]:
    """Every nn.Linear of the model that has a directory in `db`, and the expert units of every experts-shaped module that
    have one, in module order."""
    names = []
    for n, m in model.named_modules():
        if isinstance(m, nn.Linear):
            if level_db.has_layer(db, n):
                names.append(n)
        elif packed_experts.experts_shaped(m):
            names += [f"{n}.{r}" for r in level_db.EXPERT_UNIT_ROLES if level_db.has_layer(db, f"{n}.{r}")]
    return names
