#!/usr/bin/env python3
"""Which Linear was hurt, and by how much, at each level of a per-layer level database: the reference's
evopress/src/error_estimator.py on gq_h_accumulate (the Hessian) and gq_quad_form (both sums of its estimate()).

    err(W_c) = sum((W - W_c) @ H * (W - W_c)) / sum(W @ H * W),    H = (2/n) sum x^T x

    python -m gptq_gguf_toolkit_amd.error_estimator --model_name_or_path HF_DIR --calibration_data ids.pt \
        --quant_weights_path DB --output_file errors.json [--calibration_tokens N] [--sequence_length L] [--verbose]

`LayerErrorEstimator` has the reference's methods (update, reset, pre_step, estimate); estimate returns a 0-dim fp64
DEVICE tensor.  Weights are never copied to fp32 (the kernel converts on load), activations are read in their own dtype,
and H is not modified: the dead-channel fix of pre_step (:88-89) happens where the kernel reads the diagonal.
`ErrorEstimator` takes the reference's constructor arguments and returns the same dict from estimate(group_by_numel).

The one deliberate difference: the levels of a Linear are ordered by the file name's numeric prefix parsed as a FLOAT
("4.5-Q4_K.pth" after "4-Q4_K.pth"; the reference's int(name.split(".")[0]) cannot tell them apart), and the file names
are kept next to the values (`ErrorEstimator.levels`).  Left out: convolutions (nn.Linear only), more than one rank.

Fused experts (transformers 5.x's MixtralExperts: two 3-D parameters) are scored as the three units the search and LevelStore
move, `<experts module>.{gate,up,down}_proj`: err(unit) = sum_e num_e / sum_e den_e over the E experts, each with its own
Hessian on ONE common scale (`ExpertUnitsEstimator`), both sums one ops.quad_form_experts call on the fused parameter read in
place.  A unit is scored when target_modules matches its name, the database has its directory and the module is adaptable
(moe_calibration.why_not_adaptable); every nn.Linear, and a model without such modules, is treated as before."""
import argparse
import json
import os
import re
import sys
from collections import defaultdict
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn

if __package__ in (None, ""):  # run as a script: make the package importable under its alias
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gptq_gguf_toolkit_amd  # noqa: F401
    __package__ = "gptq_gguf_toolkit_amd"

from . import dist_utils, level_db, metrics, moe_calibration, packed_experts, ops as _ops  # noqa: E402
from .model_utils import LINEAR_LAYERS, ForwardInterrupt, InputCollector, _to, select_layers  # noqa: E402


def _count_tokens(input_args, input_kwargs) -> int:
    """The calibration tokens of the collected block inputs: rows of the hidden states, summed over the samples."""
    n = 0
    for args, kwargs in zip(input_args, input_kwargs):
        x = args[0] if len(args) > 0 else kwargs.get("hidden_states")
        if isinstance(x, torch.Tensor) and x.dim() >= 2:
            n += x.numel() // x.shape[-1]
    return max(n, 1)


def _single_rank():
    if dist_utils.is_dist_available_and_initialized() and dist_utils.get_world_size() > 1:
        raise NotImplementedError("error_estimator runs on one rank (torch.distributed is initialised with "
                                  f"{dist_utils.get_world_size()} ranks)")


class LayerErrorEstimator:

    def __init__(self, layer: nn.Module):
        self._validate_layer(layer)
        self.layer = layer
        self.W = layer.weight
        self.d_row, self.d_col = layer.weight.shape
        self.W_device, self.W_dtype, self.W_shape = self.W.device, self.W.dtype, self.W.shape
        self.H = None
        self.num_samples = 0
        self.shared_H_with = None  # another handle fed by the SAME input tensor (q/k/v, gate/up): its H is this one's
        self.pre_step_completed = False
        self._norm = None

    @staticmethod
    def _validate_layer(layer):
        if not isinstance(layer, nn.Linear):
            raise TypeError(f"LayerErrorEstimator supports nn.Linear only, got {type(layer).__name__}")

    @torch.no_grad()
    def update(self, input: torch.Tensor) -> None:
        """H <- n/(n+b) H + 2/(n+b) X^T X with b = input.shape[0] samples at once (the telescoped form of b single
        updates, as GPTQ.update); X is read where it lies, in its own dtype."""
        batch_size = input.shape[0]
        if self.shared_H_with is None:
            x = input.reshape(-1, input.shape[-1])
            if x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                x = x.float()
            if not x.is_contiguous():
                x = x.contiguous()
            if self.H is None:
                self.H = torch.zeros((self.d_col, self.d_col), device=x.device, dtype=torch.float32)
            n = self.num_samples
            _ops.h_accumulate(self.H, x, n / (n + batch_size), 2.0 / (n + batch_size))
        self.num_samples += batch_size

    def reset(self) -> None:
        self.W = self.layer.weight
        self.H = None
        self.num_samples = 0
        self.shared_H_with = None
        self.pre_step_completed = False
        self._norm = None

    def hessian(self) -> Optional[torch.Tensor]:
        return self.H if self.shared_H_with is None else self.shared_H_with.hessian()

    @torch.no_grad()
    def pre_step(self) -> None:
        assert self.hessian() is not None, "One has to process at least one sample of calibration data to estimate errors"
        _single_rank()
        self.pre_step_completed = True

    @torch.no_grad()
    def norm(self) -> torch.Tensor:
        """sum(W @ H * W), computed once per Linear."""
        assert self.pre_step_completed
        if self._norm is None:
            self._norm = _ops.quad_form(self.W.detach(), self.hessian())
        return self._norm

    @torch.no_grad()
    def estimate(self, W_c: torch.Tensor) -> torch.Tensor:
        """sum((W - W_c) @ H * (W - W_c)) / sum(W @ H * W) as a 0-dim fp64 tensor on the device (no host read)."""
        assert self.pre_step_completed
        if tuple(W_c.shape) != tuple(self.W_shape):
            raise ValueError(f"the compressed weight has shape {tuple(W_c.shape)}, the layer {tuple(self.W_shape)}")
        return _ops.quad_form(self.W.detach(), self.hessian(), W_c) / self.norm()


class ExpertUnitsEstimator:
    """The three units `<experts module>.{gate,up,down}_proj` of one fused experts module (gate_up_proj [E, 2I, H], down_proj
    [E, H, I]) while a moe_calibration.CalibExperts stands in for it: per expert one Hessian for w1 and w3, which share an
    input, and one for w2, each a view of a stacked [E, C, C] fp32 buffer, all with ONE scale:

        H_e = (2/N) sum_{tokens routed to e} x^T x,    N = the number of calibration tokens, the same for every expert,

    so that err(unit) = sum_e num_e / sum_e den_e is the unit's calibration-weighted output error: an expert that sees more
    tokens weighs more (per-expert normalisation by n_e would weigh all experts alike, which is not what the search's
    fitness sees).  An expert no token reaches keeps H_e = 0, which the kernel reads as the identity."""
    ROLES = {"gate_proj": "in", "up_proj": "in", "down_proj": "mid"}

    def __init__(self, name: str, original: nn.Module, roles: List[str], n_tokens: int, buffers: dict, ordinal: int = 0):
        self.name, self.original, self.roles = name, original, list(roles)
        self.E, self.hidden, self.inter = (int(n) for n in original.down_proj.shape)
        self.alpha = 2.0 / n_tokens
        dev = original.down_proj.device
        self.H = {}
        for kind, C in (("in", self.hidden), ("mid", self.inter)):
            if any(self.ROLES[r] == kind for r in self.roles):
                key = (kind, self.E, C, dev, ordinal)  # ordinal: the module's place in its block -- two experts modules of
                if key not in buffers:                 # one shape under one block never share storage; once per role for the walk
                    buffers[key] = torch.empty((self.E, C, C), device=dev, dtype=torch.float32)
                self.H[kind] = buffers[key].zero_()
        self._norm = {}

    def hooks(self, stand_in) -> list:
        """Forward pre-hooks on the synthesized children (CalibExperts fires pre-hooks only): w1 feeds the shared Hessian
        of w1 / w3, w2 its own."""
        def feed(H):
            def _hook(_, inp):
                x = inp[0].reshape(-1, inp[0].shape[-1])
                if x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                    x = x.float()
                _ops.h_accumulate(H, x if x.is_contiguous() else x.contiguous(), 1.0, self.alpha)
            return _hook

        out = []
        for e in range(self.E):
            ex = stand_in.expert(e)
            if "in" in self.H:
                out.append(ex.w1.register_forward_pre_hook(feed(self.H["in"][e])))
            if "mid" in self.H:
                out.append(ex.w2.register_forward_pre_hook(feed(self.H["mid"][e])))
        return out

    def weight(self, role: str) -> torch.Tensor:
        """The unit's [E, R, C] tensor: a view of the fused parameter, read in place."""
        o, I = self.original, self.inter
        return {"gate_proj": o.gate_up_proj.detach()[:, :I], "up_proj": o.gate_up_proj.detach()[:, I:],
                "down_proj": o.down_proj.detach()}[role]

    def numel(self, role: str) -> int:
        return self.weight(role).numel()

    def _quad(self, role: str, W_c: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sum_e of the E quadratic forms, fp64 on the device."""
        W, H = self.weight(role), self.H[self.ROLES[role]]
        if -(-W.shape[1] // 128) * (W.shape[2] // 128) <= GROUPED_MAX_TILES_PER_EXPERT:
            return _ops.quad_form_experts(W, H, W_c).sum()
        return torch.stack([_ops.quad_form(W[e], H[e], None if W_c is None else W_c[e]) for e in range(self.E)]).sum()

    @torch.no_grad()
    def estimate(self, role: str, W_c: torch.Tensor) -> torch.Tensor:
        """sum_e num_e / sum_e den_e as a 0-dim fp64 tensor on the device (no host read); the denominator once per unit."""
        W = self.weight(role)
        if tuple(W_c.shape) != tuple(W.shape):
            raise ValueError(f"{self.name}.{role}: the compressed unit has shape {tuple(W_c.shape)}, the experts "
                             f"{tuple(W.shape)}")
        if role not in self._norm:
            self._norm[role] = self._quad(role)
        return self._quad(role, W_c) / self._norm[role]


# The grouped call (ops.quad_form_experts: two launches) scores a unit whose experts have at most this many 128 x 128 tiles
# each, the per-expert ops.quad_form loop (2 E launches) a unit of larger experts; the values are the same bit for bit.
# profiles/quad_form_experts_rate.txt: at 96 tiles per expert (E = 128, 768 x 2048 and 2048 x 768) one expert leaves most of
# the device idle and the grouped call takes 0.16 - 0.18x the loop's time; at 3584 tiles per expert (E = 8, 14336 x 4096 and
# 4096 x 14336) every expert fills the device by itself and the grouped call takes 1.12 - 1.14x (presumably because the
# loop's concurrent tiles share ONE panel of H where the grouped launch reads E; not profiled).  Nothing between was measured: the threshold is two rounds of the
# 512 workgroups the device holds at once (256 CUs x 2), below which a single expert's launch ends in a partly filled round.
GROUPED_MAX_TILES_PER_EXPERT = 1024


class ErrorEstimator:

    def __init__(
        self,
        model: nn.Module,
        data_loader: Iterable,
        target_modules: str,
        pre_block_modules: List[str],
        block_modules: str,
        compressed_weights_path: str,
        device: Optional[torch.device] = None,
        cpu_offload_modules: bool = False,
        cpu_offload_activations: bool = False,
        verbose: bool = False,
        level_store=None,
    ) -> None:
        """level_store: an optional level_store.LevelStore holding the database on the device; the levels are then read
        from it instead of from the files (the values are the same)."""
        if getattr(level_store, "resident", "dense") != "dense":
            raise ValueError("ErrorEstimator needs the model's dense Linears: it cannot work on a packed-resident LevelStore "
                             "(resident='packed'); build the store with resident='dense'")
        self.level_store = level_store
        self.model = model
        self.data_loader = data_loader
        self.target_modules = target_modules
        self.pre_block_modules = pre_block_modules
        self.block_modules = block_modules
        self.device = device
        self.cpu_offload_modules = cpu_offload_modules
        self.cpu_offload_activations = cpu_offload_activations
        self.verbose = verbose
        self.compressed_weights_path = compressed_weights_path
        self.levels: Dict[str, List[str]] = {}  # layer name -> level file names, in the order of its error list
        self.hessians_built = 0                 # Hessians accumulated (not shared) over the whole walk

    @torch.no_grad()
    def estimate(self, group_by_numel: bool = False) -> Dict[int, Dict[str, List[float]]]:
        """{-1: {layer: [error per level]}} or, with group_by_numel, {weight.numel(): {layer: [...]}} (reference :133-220)."""
        _single_rank()
        device = self.device or next(self.model.parameters()).device
        blocks = self.model.get_submodule(self.block_modules)
        pre_blocks = [self.model.get_submodule(name) for name in self.pre_block_modules]
        blocks[0] = blocks[0].to(device)
        for module in pre_blocks:
            module.to(device)
        has_cache = hasattr(self.model.config, "use_cache")
        if has_cache:
            use_cache = self.model.config.use_cache
            self.model.config.use_cache = False
        blocks[0] = InputCollector(blocks[0], cpu_offload=self.cpu_offload_activations)
        for inp_args, inp_kwargs in self.data_loader:
            try:
                self.model(*_to(inp_args, device=device), **_to(inp_kwargs, device=device))
            except ForwardInterrupt:
                pass
        input_args, input_kwargs = blocks[0].input_args, blocks[0].input_kwargs
        blocks[0] = blocks[0].module
        if self.cpu_offload_modules:
            for module in pre_blocks:
                module.cpu()

        n_tokens = _count_tokens(input_args, input_kwargs)  # the common scale of every expert Hessian
        moe_calibration.reset_verdicts()  # every walk re-verifies the routed forward on its own first inputs
        unit_buffers = {}
        all_errors = defaultdict(dict)
        for block_id, block in enumerate(blocks):
            if self.verbose:
                dist_utils.print_on_main(f"Processing {self.block_modules} {block_id}/{len(blocks)}.")
            block = block.to(device)
            layer_prefix = f"{self.block_modules}.{block_id}."
            layers = select_layers(self.model, layer_prefix, self.target_modules, LINEAR_LAYERS)  # a conv raises below
            handles, hooks, seen = self._prepare_hooks_and_handles(layers)
            installed, units, unit_hooks = [], [], []
            try:  # the model gets its own experts modules back whatever happens in between
                units, unit_hooks = self._install_expert_units(layer_prefix, device, n_tokens, unit_buffers, installed)
                for i, (inp_args, inp_kwargs) in enumerate(zip(input_args, input_kwargs)):
                    inp_args, inp_kwargs = _to(inp_args, device=device), _to(inp_kwargs, device=device)
                    out = block(*inp_args, **inp_kwargs)
                    seen.clear()
                    out = out[0] if isinstance(out, (list, tuple)) else out
                    if self.cpu_offload_activations:
                        out = out.cpu()
                    # only the first input argument changes from block to block
                    if len(inp_args) > 0:
                        input_args[i] = (out, *inp_args[1:])
                    elif "hidden_states" in inp_kwargs:
                        input_kwargs[i] = {**input_kwargs[i], "hidden_states": out}
                    else:
                        raise ValueError("Unsupported block input format.")
            finally:
                for h in unit_hooks:
                    h.remove()
                moe_calibration.restore(installed)
            for h in hooks.values():
                h.remove()
            self.hessians_built += sum(h.shared_H_with is None for h in handles.values())
            self.hessians_built += sum(u.E * len(u.H) for u in units)
            block_errors = self._estimate_errors_group(handles)
            numel = {k: handles[k].W.numel() for k in block_errors}
            for u in units:
                unit_errors = self._estimate_unit_errors(u)
                block_errors.update(unit_errors)
                numel.update({k: u.numel(k.rpartition(".")[2]) for k in unit_errors})
            if group_by_numel:
                for k, v in block_errors.items():
                    all_errors[numel[k]][k] = v
            else:
                all_errors[-1].update(block_errors)
            for h in handles.values():
                h.reset()
            if self.cpu_offload_modules:
                block = block.cpu()
            del handles, hooks, units
        if has_cache:
            self.model.config.use_cache = use_cache
        return all_errors

    def _prepare_hooks_and_handles(self, layers: Dict[str, nn.Module]):
        handles, hooks = {}, {}
        seen = {}  # inputs of the current forward: key -> (the handle that folds them, the tensor); cleared after every sample

        def update_handle_hook(name):
            def _hook(_, inp, out):
                h, x = handles[name], inp[0]
                # Linears fed the very same tensor (q/k/v, gate/up) share one Hessian, as BlockSchedule.feed
                key = (x.data_ptr(), tuple(x.shape), tuple(x.stride()), x.dtype, x._version)
                leader = seen.get(key, (None, None))[0]
                if leader is not None and leader is not h and leader.d_col == h.d_col:
                    assert h.shared_H_with in (None, leader) and h.H is None, "input sharing pattern changed between samples"
                    h.shared_H_with = leader
                else:
                    assert h.shared_H_with is None, "input sharing pattern changed between samples"
                    seen[key] = (h, x)  # x is kept so that its address is not reused within the sample
                h.update(x)
            return _hook

        for layer_name, layer in layers.items():
            handles[layer_name] = self._create_handle(layer)
            hooks[layer_name] = layer.register_forward_hook(update_handle_hook(layer_name))
        return handles, hooks, seen

    def _create_handle(self, layer):
        return LayerErrorEstimator(layer)

    def _has_unit(self, name: str) -> bool:
        if self.level_store is not None and name not in self.level_store.units:
            return False
        return level_db.has_layer(self.compressed_weights_path, name)

    def _install_expert_units(self, layer_prefix: str, device, n_tokens: int, buffers: dict, installed: list):
        """Put a CalibExperts in place of every adaptable fused experts module under the prefix that has a unit
        `<module>.{gate,up,down}_proj` which target_modules matches and the database holds; -> (their
        ExpertUnitsEstimators, the hooks on the synthesized children).  `installed` collects moe_calibration.restore's
        records as they are made.  "routed" on the GPU in 16-bit, else "loop": the Quantizer's rule, and CalibExperts
        verifies routed against loop on the first input of every class as it does there."""
        units, hooks = [], []
        root = layer_prefix.rstrip(".")
        for name, layer in list(self.model.get_submodule(root).named_modules(prefix=root)):
            if not packed_experts.experts_shaped(layer) or moe_calibration.why_not_adaptable(layer):
                continue
            roles = [r for r in level_db.EXPERT_UNIT_ROLES
                     if re.search(self.target_modules, f"{name}.{r}") and self._has_unit(f"{name}.{r}")]
            if not roles:
                continue
            routed = torch.device(device).type == "cuda" and layer.down_proj.dtype in (torch.float16, torch.bfloat16)
            parent_name, _, leaf = name.rpartition(".")
            parent = self.model.get_submodule(parent_name)
            stand_in = moe_calibration.CalibExperts(layer, "routed" if routed else "loop")
            setattr(parent, leaf, stand_in)
            installed.append((parent, leaf, layer, name))
            unit = ExpertUnitsEstimator(name, layer, roles, n_tokens, buffers, ordinal=len(units))
            hooks += unit.hooks(stand_in)
            units.append(unit)
        return units, hooks

    def _estimate_unit_errors(self, unit: ExpertUnitsEstimator) -> Dict[str, List[float]]:
        errors = {}
        for role in unit.roles:
            name = f"{unit.name}.{role}"
            ldir = level_db.layer_dir(self.compressed_weights_path, name)
            files = level_db.level_files(ldir)
            if self.level_store is not None:
                vals = [unit.estimate(role, self.level_store.level_tensor(name, f)) for f in files]
            else:
                vals = [unit.estimate(role, level_db.load_level(os.path.join(ldir, f), unit.original.down_proj.device,
                                                                self.compressed_weights_path)) for f in files]
            # the E-element sums and the division ran on the device in fp64: ONE host read per unit
            errors[name] = torch.stack(vals).tolist() if vals else []
            self.levels[name] = files
            if self.verbose:
                dist_utils.print_on_main(f"{name}: " + "  ".join(f"{f[:-4]} {e:.4e}" for f, e in zip(files, errors[name])))
        return errors

    def _estimate_errors_group(self, handles: Dict[str, LayerErrorEstimator]) -> Dict[str, List[float]]:
        errors = {}
        for name, handle in handles.items():
            handle.pre_step()
            ldir = level_db.layer_dir(self.compressed_weights_path, name)
            files = level_db.level_files(ldir)
            if self.level_store is not None:
                vals = [handle.estimate(self.level_store.level_tensor(name, f)) for f in files]
            else:
                vals = [handle.estimate(level_db.load_level(os.path.join(ldir, f), handle.W_device,
                                                           self.compressed_weights_path))
                        for f in files]
            # numerators and the denominator were divided on the device in fp64: ONE host read per Linear
            errors[name] = torch.stack(vals).tolist() if vals else []
            self.levels[name] = files
            if self.verbose:
                dist_utils.print_on_main(f"{name}: " + "  ".join(f"{f[:-4]} {e:.4e}" for f, e in zip(files, errors[name])))
        return errors


def report(errors: Dict[int, Dict[str, List[float]]], levels: Dict[str, List[str]]) -> Dict[str, List[dict]]:
    """{layer: [{"level": file stem, "error": value}, ...]} in level order: what the CLI writes."""
    out = {}
    for group in errors.values():
        for name, vals in group.items():
            out[name] = [{"level": f[:-4], "error": float(e)} for f, e in zip(levels[name], vals)]
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model_name_or_path", type=str, required=True, help="The name or path to the model")
    p.add_argument("--calibration_data", type=str, required=True, help=".pt file of [1, L] token-id tensors")
    p.add_argument("--calibration_tokens", default=None, type=int, help="Number of tokens for calibration (default: all).")
    p.add_argument("--sequence_length", default=None, type=int, help="Length of sequences.")
    p.add_argument("--quant_weights_path", type=str, required=True, help="Path to the per-layer level database")
    p.add_argument("--output_file", type=str, required=True, help="Path to output JSON file for storing results")
    p.add_argument("--dtype", type=str, default="float16", choices=["auto", "float16", "float32", "bfloat16"],
                   help="dtype to load the model.")
    p.add_argument("--seed", default=0, type=int, help="Random seed.")
    p.add_argument("--attn_implementation", type=str, default=None, choices=["eager", "sdpa", "flash_attention_2"])
    p.add_argument("--target_modules", type=str, default=r".*layers.*((q|k|v|o|gate|up|down)_proj)$",
                   help="regex of the Linears to score")
    p.add_argument("--pre_block_modules", nargs="+", type=str, default=["model.embed_tokens", "model.rotary_emb"])
    p.add_argument("--block_modules", type=str, default="model.layers")
    p.add_argument("--verbose", action="store_true", help="one line per Linear")
    args = p.parse_args(argv)
    if not os.path.isfile(args.calibration_data):  # refused BEFORE any work
        p.error(f"calibration_data must be a .pt file of token-id tensors (got {args.calibration_data!r}); "
                "dataset downloads are not part of this package")
    if not os.path.isdir(args.quant_weights_path):
        p.error(f"quant_weights_path {args.quant_weights_path!r} is not a directory")
    return args


def main(argv=None):
    args = parse_args(argv)
    assert torch.cuda.is_available(), "error_estimator needs a GPU (there is no CPU path)"
    from .ppleval import load_hf_model
    device = torch.device("cuda")
    metrics.fix_seed(args.seed)
    model = load_hf_model(args, device)
    seq_len = args.sequence_length or model.config.max_position_embeddings
    data = metrics.load_eval_data(args.calibration_data, args.calibration_tokens, seq_len, what="calibration_data")
    pre = [m for m in args.pre_block_modules if _has_submodule(model, m)]
    est = ErrorEstimator(model, [([], {"input_ids": ids}) for ids in data], args.target_modules, pre, args.block_modules,
                         args.quant_weights_path, device=device, verbose=args.verbose)
    out = report(est.estimate(), est.levels)
    with open(args.output_file, "w") as f:
        json.dump(out, f, indent=2)
    print(f"Results saved to {args.output_file}")
    return out


def _has_submodule(model, name) -> bool:
    try:
        model.get_submodule(name)
        return True
    except AttributeError:
        return False


if __name__ == "__main__":
    main()
