"""GGUF -> HF tensors on the GPU: the inverse of pack_gptq_into_gguf.py for the dense Llama family and for Mixtral.

The reference reads a .gguf back through transformers' GGUF loader (mapper/gguf_splitter.py:469-474), which needs gguf-py;
that package is not installable here, so the file is parsed by gguf_writer.parse_gguf (spec level) and the K-quant, Q8_0,
IQ4_NL and IQ4_XS payloads are decoded by this package's own kernel: bytes are uploaded as they lie in the file and `ops.dequantize_blocks` writes the
weights in one pass.  The q_proj / k_proj rotary row permutation the converter applied (reference
pack_gptq_into_gguf.py:2177-2183) is undone inside that pass by a row gather (`row_src`), for architecture "llama" only.
F32 / F16 / BF16 tensors pass through with a cast.  Q8_0 (`--outtype q8_0` writes it for the tensors GPTQ did not quantize, and
it may be a level of the search) takes the same one call as the K-quants: d * q of ggml-quants.c dequantize_row_q8_0, the row
gather folded in, one cast to `dtype`.  IQ4_NL and IQ4_XS (include/gptq_gguf_iq4.h), which llama.cpp writes and this package
does not encode, are read in the same way; a tensor of a 32-value type whose rows are no multiple of 256 loads dense and is
never kept packed.  The file is mapped, never read whole.
Merged 3-D expert tensors (`blk.N.ffn_{gate,up,down}_exps.weight`, [E, R, C]) are decoded in one call over [E * R, C] and
come back under the names the target model has (EXPERT_LAYOUTS): "fused", transformers 5.x, where a layer keeps
`mlp.experts.gate_up_proj` [E, 2I, H] (per expert the gate rows, then the up rows) and `mlp.experts.down_proj` [E, H, I] and the
router is `mlp.gate.weight`; or "per_expert", transformers up to 4.56, E tensors `block_sparse_moe.experts.<e>.w1 / w3 / w2
.weight` (gate / up / down) and the router `block_sparse_moe.gate.weight`.  load_into_model takes the layout from the model;
with packed=True the expert tensors stay block bytes on the device (packed_experts.PackedExperts, or per expert a
PackedLinear on a slice view), uploaded once.
"""
from typing import Dict, Iterator, Optional, Tuple

import numpy as np
import torch

from . import ops
from .gguf_writer import K_QUANTS, PACKED_TYPES, PLAIN_TYPES, parse_gguf
from .pack_gptq_into_gguf import _BLOCK_TABLE

ROTARY_TENSORS = (".attn_q.weight", ".attn_k.weight")  # the tensors whose rows the converter permutes
_TOP = {"token_embd.weight": "model.embed_tokens.weight", "output_norm.weight": "model.norm.weight",
        "output.weight": "lm_head.weight"}
_BLOCK_INV = {v: k for k, v in _BLOCK_TABLE.items() if not v.endswith("_exps.weight")}
EXPERT_LAYOUTS = ("fused", "per_expert")
EXPERT_ROLES = {"ffn_gate_exps.weight": ("gate", "w1"), "ffn_up_exps.weight": ("up", "w3"), "ffn_down_exps.weight": ("down", "w2")}
ROUTER = "ffn_gate_inp.weight"


def unpermute(weights: torch.Tensor, n_head: int, n_head_kv) -> torch.Tensor:
    """Exact inverse of pack_gptq_into_gguf.permute: GGUF's rotary row layout back to HF's; any trailing shape."""
    if n_head_kv is not None and n_head != n_head_kv:
        n_head = n_head_kv
    return (weights.reshape(n_head, weights.shape[0] // n_head // 2, 2, *weights.shape[1:])
            .swapaxes(1, 2).reshape(weights.shape))


def unpermute_rows(R: int, n_head: int, n_head_kv) -> torch.Tensor:
    """int32 [R]: x[unpermute_rows(R, h, kv)] == unpermute(x, h, kv) -- the `row_src` of ops.dequantize_blocks."""
    return unpermute(torch.arange(R, dtype=torch.int32), n_head, n_head_kv).contiguous()


def rotary_row_src(name: str, R: int, arch, n_head, n_head_kv, device) -> Optional[torch.Tensor]:
    """The `row_src` on `device` that undoes the converter's rotary row permutation of GGUF tensor `name` with R rows, or
    None: attn_q / attn_k of architecture "llama" with a head count only.  The one statement of the rule; the values come
    from a parsed file (iter_gguf_tensors) or from a level database's manifest (level_db.rotary_rows)."""
    if arch != "llama" or not n_head or not name.endswith(ROTARY_TENSORS):
        return None
    return unpermute_rows(R, n_head, n_head if name.endswith(".attn_q.weight") else n_head_kv).to(device)


_ROW_DST: Dict[tuple, torch.Tensor] = {}  # (q or k, R, heads, device) -> rotary_row_dst's index


def rotary_row_dst(gguf_name: str, R: int, n_head, n_kv, device) -> Optional[torch.Tensor]:
    """The other direction, HF -> GGUF, as an index: int32 [R] on `device` with x[rotary_row_dst(...)] == permute(x, ...) of
    pack_gptq_into_gguf for attn_q / attn_k (None for any other tensor) -- the `row_src` of ops.pack_bands, which packs an
    HF-ordered band straight into GGUF row order.  rotary_row_src of the same tensor undoes it: either composition is the
    identity.  One tensor per (q or k, R, heads, device), kept for the process."""
    if not n_head or not gguf_name.endswith(ROTARY_TENSORS):
        return None
    from .pack_gptq_into_gguf import permute
    is_q = gguf_name.endswith(".attn_q.weight")
    heads = int(n_head if is_q or n_kv is None else n_kv)
    key = ("q" if is_q else "k", int(R), heads, str(device))
    if key not in _ROW_DST:
        _ROW_DST[key] = permute(torch.arange(R, dtype=torch.int32), heads, heads).contiguous().to(device)
    return _ROW_DST[key]


def expert_tensor(gguf_name: str):
    """(layer, role, per-expert weight name) of a merged expert tensor `blk.<layer>.ffn_{gate,up,down}_exps.weight` --
    ("gate", "w1"), ("up", "w3"), ("down", "w2") -- or None for any other name."""
    parts = gguf_name.split(".")
    if len(parts) == 4 and parts[0] == "blk" and parts[1].isdecimal() and ".".join(parts[2:]) in EXPERT_ROLES:
        return (int(parts[1]),) + EXPERT_ROLES[".".join(parts[2:])]
    return None


def expert_layout_of(model: torch.nn.Module) -> str:
    """The layout `model` keeps its experts in: "per_expert" if it has modules `...block_sparse_moe.experts.<e>.w1`, else
    "fused" (which a model without experts never asks about)."""
    for name, _ in model.named_modules():
        if ".block_sparse_moe.experts." in name:
            return "per_expert"
    return "fused"


def hf_tensor_name(gguf_name: str, expert_layout: str = "per_expert") -> str:
    """Inverse of pack_gptq_into_gguf.map_tensor_name for the dense Llama table and Mixtral's router (`mlp.gate.weight` in
    the fused expert layout, `block_sparse_moe.gate.weight` in the per-expert one)."""
    if gguf_name in _TOP:
        return _TOP[gguf_name]
    parts = gguf_name.split(".")
    if len(parts) >= 4 and parts[0] == "blk" and parts[1].isdecimal():
        rest = ".".join(parts[2:])
        if rest == ROUTER and expert_layout == "fused":
            return f"model.layers.{parts[1]}.mlp.gate.weight"
        if rest in _BLOCK_INV:
            return f"model.layers.{parts[1]}.{_BLOCK_INV[rest]}"
    raise ValueError(f"Can not map GGUF tensor {gguf_name!r} to an HF name")


def kv_int(v, key) -> Optional[int]:
    """A key/value entry (None: not there) that has to be one integer; `key` names it in the refusal."""
    if v is None:
        return None
    if isinstance(v, (list, tuple)):  # per-layer head counts: one value for all layers, or refuse
        if len(set(v)) != 1:
            raise NotImplementedError(f"{key} differs from layer to layer: {sorted(set(v))}")
        v = v[0]
    return int(v)


def _host(buf, off: int, nbytes: int) -> torch.Tensor:
    """One tensor's bytes out of the mapped file (the only copy made on the host)."""
    return torch.from_numpy(np.array(buf[off:off + nbytes], dtype=np.uint8, copy=True))


def iter_gguf_tensors(path: str, device="cuda:0", dtype: Optional[torch.dtype] = None,
                      hf_layout: bool = True, quant_dtype: Optional[torch.dtype] = None,
                      skip=(), expert_layout: str = "fused") -> Iterator[Tuple[str, torch.Tensor]]:
    """Yield (name, tensor on `device`) for every tensor of the file, in file order.  hf_layout: HF names and HF row order
    of attn_q / attn_k (`rope_freqs.weight`, which no HF module owns, is left out); otherwise GGUF names and rows as stored.
    dtype None: fp32 for quantized tensors (`quant_dtype` for the K-quants when given), the stored dtype for F32 / F16 / BF16.
    A merged expert tensor [E, R, C] is decoded in one call; with hf_layout it comes back in `expert_layout`: "fused" --
    `mlp.experts.down_proj`, and `mlp.experts.gate_up_proj` = cat(gate, up) along the rows, yielded where the later of the two
    stands in the file -- or "per_expert", E tensors `block_sparse_moe.experts.<e>.w1 / w3 / w2.weight` (views of the one
    decoded tensor); without hf_layout it is the 3-D tensor under its GGUF name."""
    if expert_layout not in EXPERT_LAYOUTS:
        raise ValueError(f"expert_layout must be one of {EXPERT_LAYOUTS}, got {expert_layout!r}")
    device = torch.device(device)
    kv, tensors, buf = parse_gguf(str(path), mmap=True)
    arch = kv["general.architecture"][0] if "general.architecture" in kv else None
    n_head, n_kv = (kv_int(kv[k][0] if k in kv else None, k)
                    for k in (f"{arch}.attention.head_count", f"{arch}.attention.head_count_kv"))
    halves: Dict[int, Dict[str, torch.Tensor]] = {}  # layer -> the gate / up tensor that waits for the other one
    for name, shape, gt, off, nbytes in tensors:
        exp = expert_tensor(name)
        if (exp is None and len(shape) > 2) or (exp is not None and len(shape) != 3):
            raise NotImplementedError(f"tensor {name!r} (shape {tuple(shape)}): only blk.N.ffn_{{gate,up,down}}_exps.weight "
                                      f"are read as merged [E, R, C] expert tensors")
        if (hf_layout and name == "rope_freqs.weight") or name in skip:  # (skip: GGUF names the caller handles itself)
            continue
        rows = rotary_row_src(name, shape[0], arch, n_head, n_kv, device) if hf_layout and exp is None else None
        raw = _host(buf, off, nbytes).to(device)
        flat = (int(np.prod(shape[:-1])), shape[-1])  # an expert tensor: E * R rows
        if gt in K_QUANTS:
            t = ops.dequantize_blocks(gt, raw.view(flat[0], -1), dtype or quant_dtype or torch.float32, rows)
        elif gt in PACKED_TYPES:  # Q8_0, IQ4_NL, IQ4_XS (quant_dtype is the K-quants' alone)
            t = ops.dequantize_blocks(gt, raw.view(flat[0], -1), dtype or torch.float32, rows)
        else:
            if gt not in PLAIN_TYPES:
                raise ValueError(f"tensor {name!r}: ggml type {gt} is not supported")
            t = raw.view(getattr(torch, PLAIN_TYPES[gt][0])).reshape(flat)
            if dtype is not None:
                t = t.to(dtype)
            if rows is not None:
                t = t[rows.long()]
        t = t.view(*shape)
        if exp is None or not hf_layout:
            yield (hf_tensor_name(name, expert_layout) if hf_layout else name), t
            continue
        layer, role, wname = exp
        if expert_layout == "per_expert":
            for e in range(shape[0]):
                yield f"model.layers.{layer}.block_sparse_moe.experts.{e}.{wname}.weight", t[e]
        elif role == "down":
            yield f"model.layers.{layer}.mlp.experts.down_proj", t
        else:
            pair = halves.setdefault(layer, {})
            pair[role] = t
            if len(pair) == 2:
                del halves[layer]
                if pair["gate"].shape != pair["up"].shape:
                    raise ValueError(f"blk.{layer}: ffn_gate_exps {tuple(pair['gate'].shape)} and ffn_up_exps "
                                     f"{tuple(pair['up'].shape)} differ in shape")
                yield f"model.layers.{layer}.mlp.experts.gate_up_proj", torch.cat([pair["gate"], pair["up"]], dim=1)
    for layer, pair in sorted(halves.items()):  # half of a fused parameter: there is no HF tensor to give it to
        (role,) = pair
        raise NotImplementedError(f"tensor 'blk.{layer}.ffn_{role}_exps.weight': the file has no "
                                  f"ffn_{'up' if role == 'gate' else 'gate'}_exps of that layer to fuse it with into "
                                  f"mlp.experts.gate_up_proj")


def load_state_dict(path: str, device="cuda:0", dtype: Optional[torch.dtype] = None,
                    expert_layout: str = "fused") -> Dict[str, torch.Tensor]:
    """{HF name: tensor} of the whole file (HF row layout; merged expert tensors in `expert_layout`)."""
    return dict(iter_gguf_tensors(path, device, dtype, hf_layout=True, expert_layout=expert_layout))


def packed_linear_tensors(model: torch.nn.Module, path: str) -> Dict[str, tuple]:
    """{HF module name: (GGUF tensor name, ggml type)} of the file's K-quant / Q8_0 / IQ4_NL / IQ4_XS tensors that are the weight of an
    nn.Linear of a block of `model` with in_features % 256 == 0 -- what load_into_model(packed=True) keeps packed.
    lm_head, embeddings and norms are not among them."""
    _, tensors, _ = parse_gguf(str(path), mmap=True)
    out = {}
    for name, shape, gt, _, _ in tensors:
        if not gt in PACKED_TYPES or len(shape) != 2 or not name.startswith("blk."):
            continue
        hf = hf_tensor_name(name)
        mod = hf[:-len(".weight")] if hf.endswith(".weight") else None
        try:
            layer = model.get_submodule(mod) if mod else None
        except AttributeError:
            layer = None
        if isinstance(layer, torch.nn.Linear) and tuple(layer.weight.shape) == tuple(shape) and shape[1] % 256 == 0:
            out[mod] = (name, gt)
    return out


def packed_vocab_tensors(model: torch.nn.Module, path: str) -> Dict[str, tuple]:
    """{HF module name: (GGUF tensor name, ggml type)} of the vocabulary ends that load_into_model(packed="all") keeps packed
    beside packed_linear_tensors: `model.embed_tokens` (token_embd.weight) when it is an nn.Embedding and `lm_head`
    (output.weight) when it is an nn.Linear, each if its tensor is a K-quant / Q8_0 of the module's shape with hidden % 256
    == 0.  A file without output.weight ties the two: lm_head then names token_embd.weight as well, and both are kept or
    neither.  A tensor stored as F16 / F32 is not among them (it loads dense)."""
    _, tensors, _ = parse_gguf(str(path), mmap=True)
    by_name = {name: (shape, gt) for name, shape, gt, _, _ in tensors}

    def fits(gguf_name, mod, kind):
        if gguf_name not in by_name:
            return False
        shape, gt = by_name[gguf_name]
        try:
            layer = model.get_submodule(mod)
        except AttributeError:
            return False
        return (gt in PACKED_TYPES and len(shape) == 2 and isinstance(layer, kind)
                and tuple(layer.weight.shape) == tuple(shape) and shape[1] % 256 == 0)

    out = {}
    emb = fits("token_embd.weight", "model.embed_tokens", torch.nn.Embedding)
    if "output.weight" in by_name:
        if emb:
            out["model.embed_tokens"] = ("token_embd.weight", by_name["token_embd.weight"][1])
        if fits("output.weight", "lm_head", torch.nn.Linear):
            out["lm_head"] = ("output.weight", by_name["output.weight"][1])
    elif emb and fits("token_embd.weight", "lm_head", torch.nn.Linear):
        out["model.embed_tokens"] = out["lm_head"] = ("token_embd.weight", by_name["token_embd.weight"][1])
    return out


def packed_expert_tensors(model: torch.nn.Module, path: str) -> Dict[str, dict]:
    """{HF module name: {role: (GGUF tensor name, ggml type, expert index or None)}} of the merged expert tensors that
    load_into_model(packed=True) keeps packed.  Fused layout: a module with gate_up_proj [E, 2I, H] and down_proj [E, H, I]
    (packed_experts.experts_shaped) is named with the roles "gate", "up", "down" (index None) when all three of its layer's
    tensors are K-quant / Q8_0 of the matching shapes with H % 256 == 0 and I % 256 == 0: it becomes a PackedExperts.
    Per-expert layout: every nn.Linear `...block_sparse_moe.experts.<e>.w1 / w3 / w2` whose layer's tensor is K-quant /
    Q8_0 of shape [E, out_features, in_features] with in_features % 256 == 0 is named with the role "weight" and its
    index e: it becomes a PackedLinear on the e-th slice of the tensor's bytes."""
    from .packed_experts import experts_shaped
    _, tensors, _ = parse_gguf(str(path), mmap=True)
    by_layer: Dict[int, dict] = {}
    for name, shape, gt, _, _ in tensors:
        exp = expert_tensor(name)
        if exp is not None and len(shape) == 3 and gt in PACKED_TYPES and shape[2] % 256 == 0:
            by_layer.setdefault(exp[0], {})[exp[1]] = (name, tuple(shape), gt, exp[2])

    def module(mod):
        try:
            return model.get_submodule(mod)
        except AttributeError:
            return None

    out: Dict[str, dict] = {}
    for layer, roles in sorted(by_layer.items()):
        fused = f"model.layers.{layer}.mlp.experts"
        m = module(fused)
        if m is not None and experts_shaped(m):
            E, H, I = m.down_proj.shape
            if (len(roles) == 3 and roles["gate"][1] == roles["up"][1] == (E, I, H) and roles["down"][1] == (E, H, I)
                    and H % 256 == 0 and I % 256 == 0):
                out[fused] = {r: (n, gt, None) for r, (n, _, gt, _) in roles.items()}
            continue
        for n, shape, gt, wname in roles.values():
            for e in range(shape[0]):
                mod = f"model.layers.{layer}.block_sparse_moe.experts.{e}.{wname}"
                m = module(mod)
                if isinstance(m, torch.nn.Linear) and tuple(m.weight.shape) == shape[1:]:
                    out[mod] = {"weight": (n, gt, e)}
    return out


def _load_packed(model: torch.nn.Module, path: str, ref: torch.Tensor, vocab: bool = False,
                 moe_prefill: str = "loop") -> Dict[str, torch.Tensor]:
    """The packed half of load_into_model: the Linears of packed_linear_tensors become PackedLinear holding the file's
    block bytes (with the rotary row gather of attn_q / attn_k as row_src); the modules of packed_expert_tensors become
    PackedExperts (or, per expert, PackedLinear on a slice view) on ONE device copy of each merged tensor; with `vocab` also
    the modules of packed_vocab_tensors (one device copy per GGUF tensor: a tied pair shares it) -> the state dict of
    everything else."""
    from .packed_embedding import replace_embedding
    from .packed_experts import replace_experts
    from .packed_linear import replace_linear
    if ref.dtype not in (torch.float16, torch.bfloat16):
        raise TypeError(f"load_into_model(packed=True) computes in fp16 / bf16, the model is {ref.dtype}")
    keep = packed_linear_tensors(model, path)
    ends = packed_vocab_tensors(model, path) if vocab else {}
    experts = packed_expert_tensors(model, path)
    users: Dict[str, list] = {}  # GGUF name of a merged tensor -> [(module name, role, expert index)]
    for mod, roles in experts.items():
        for role, (g, _, e) in roles.items():
            users.setdefault(g, []).append((mod, role, e))
    by_gguf = {g: m for m, (g, _) in keep.items()}
    kv, tensors, buf = parse_gguf(str(path), mmap=True)
    arch = kv["general.architecture"][0] if "general.architecture" in kv else None
    n_head, n_kv = (kv_int(kv[k][0] if k in kv else None, k)
                    for k in (f"{arch}.attention.head_count", f"{arch}.attention.head_count_kv"))
    rows: Dict[tuple, Optional[torch.Tensor]] = {}  # one gather per (q or k, R)
    held: Dict[str, torch.Tensor] = {}              # the vocabulary tensors' block bytes on the device, by GGUF name
    for name, shape, gt, off, nbytes in tensors:
        if name in by_gguf:
            key = (name.rsplit(".", 2)[-2], shape[0])
            if key not in rows:
                rows[key] = rotary_row_src(name, shape[0], arch, n_head, n_kv, ref.device)
            packed = replace_linear(model, by_gguf[name])
            packed.set_level(_host(buf, off, nbytes).to(ref.device), int(gt), rows[key])
        elif name in users:
            held[name] = dev = _host(buf, off, nbytes).to(ref.device)  # the merged tensor's bytes: uploaded once
            for mod, role, e in users[name]:
                if e is None:
                    m = model.get_submodule(mod)
                    (m if hasattr(m, "set_level") else replace_experts(model, mod, moe_prefill)).set_level(role, dev, int(gt))
                else:
                    replace_linear(model, mod).set_level(dev.view(shape[0], -1)[e], int(gt))
        elif any(g == name for g, _ in ends.values()):
            held[name] = _host(buf, off, nbytes).to(ref.device)
    for mod, (g, gt) in ends.items():
        if mod == "lm_head":
            replace_linear(model, mod).set_level(held[g], int(gt))
        else:
            replace_embedding(model, mod).set_level(held[g], int(gt))
    skip = {m + ".weight" for m in list(keep) + list(ends) + [m for m, r in experts.items() if "weight" in r]}
    gone = set(by_gguf) | set(held)
    return {k: t for k, t in iter_gguf_tensors(path, ref.device, ref.dtype, hf_layout=True, skip=gone,
                                               expert_layout=expert_layout_of(model)) if k not in skip}


def load_into_model(model: torch.nn.Module, path: str, packed=False, moe_prefill: str = "loop") -> torch.nn.Module:
    """Load the file's weights into `model` (parameters on a GPU), strict on names and shapes.  A tied lm_head (no
    `output.weight` in the file) follows token_embd.
    packed=True: the K-quant, Q8_0, IQ4_NL and IQ4_XS tensors of the blocks' nn.Linear modules stay packed on the device -- each such Linear
    becomes a packed_linear.PackedLinear whose forward reads the block bytes (the q / k rotary permutation undone by its
    row_src), about 4.5 bits per parameter for a Q4_K file instead of 16; embeddings, norms and lm_head load as without it.
    The merged expert tensors of a MoE file stay packed in the same way (packed_expert_tensors): a transformers-5.x expert
    module becomes a packed_experts.PackedExperts on the three stacked tensors, a per-expert w1 / w2 / w3 Linear a
    PackedLinear on its slice; the router loads dense.
    packed="all": that, and the vocabulary ends of packed_vocab_tensors: model.embed_tokens becomes a
    packed_embedding.PackedEmbedding and lm_head a PackedLinear on the file's block bytes (a file without output.weight gives
    both the same tensor: one device copy); an end stored as F16 / F32 loads dense as without it.
    moe_prefill (with packed): "loop" or "grouped", the prefill path of the PackedExperts modules (PackedExperts.prefill)."""
    if packed not in (False, True, "all"):
        raise ValueError(f"load_into_model: packed must be False, True or 'all', got {packed!r}")
    if moe_prefill not in ("loop", "grouped") or (moe_prefill != "loop" and not packed):
        raise ValueError(f"load_into_model: moe_prefill must be 'loop' or 'grouped' (with packed), got {moe_prefill!r} with "
                         f"packed={packed!r}")
    ref = next(model.parameters())
    sd = (_load_packed(model, path, ref, vocab=packed == "all", moe_prefill=moe_prefill) if packed
          else load_state_dict(path, ref.device, ref.dtype, expert_layout_of(model)))
    want = model.state_dict()
    if "lm_head.weight" in want and "lm_head.weight" not in sd and "model.embed_tokens.weight" in sd:
        sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or extra:
        raise KeyError(f"{path}: tensors missing from the file {missing}, tensors the model does not have {extra}")
    for k, t in sd.items():
        if tuple(t.shape) != tuple(want[k].shape):
            raise ValueError(f"{path}: {k} has shape {tuple(t.shape)}, the model expects {tuple(want[k].shape)}")
    model.load_state_dict(sd, strict=True)
    return model
