"""The level database of tests/moe_gguf.py's tiny Mixtral, by the route the reference takes to one: the model's .gguf written
once per level with every searchable tensor (the four attention projections and the three stacked expert tensors of each
block) at ONE type -- RTN through ops.rtn_quantize + ops.pack, ops.quantize_q8_0, ops.quantize_iq4, or plain fp16 --, and each
file cut into the same directory by `gguf_splitter --gguf-layers --exact`.  token_embd / output stay Q6_K and the router and
the norms F32 in every file, so those tensors have one level.  Test scaffolding only."""
import numpy as np

import moe_gguf as M

Q2, Q4, Q6, Q8, IQ4_XS, F16 = 10, 12, 14, 8, 23, 1
# level name -> (ggml type, the exact bit width the splitter names the level file by)
LEVELS = {"Q2_K": (Q2, 2.5625), "Q4_K": (Q4, 4.5), "Q6_K": (Q6, 6.5625), "Q8_0": (Q8, 8.5), "IQ4_XS": (IQ4_XS, 4.25), "F16": (F16, 16.0)}
ROLES = ("gate", "up", "down")
UNITS = [f"model.layers.{n}.mlp.experts.{r}_proj" for n in range(M.LAYERS) for r in ROLES]
ATTENTION = [f"model.layers.{n}.self_attn.{p}_proj" for n in range(M.LAYERS) for p in "qkvo"]


def level_file(name: str) -> str:
    bw = LEVELS[name][1]
    return f"{int(bw) if bw == int(bw) else bw}-{name}.pth"


def encode(ops, w, t):
    """[.., R, C] on the device -> what the file stores, as a numpy array: packed uint8 [.., R, row bytes], or fp16 values."""
    if t == F16:
        return w.half().cpu().numpy()
    flat = w.reshape(-1, w.shape[-1]).float().contiguous()
    if t == Q8:
        packed = ops.quantize_q8_0(flat)
    elif t == IQ4_XS:
        packed = ops.quantize_iq4(flat, IQ4_XS)
    else:
        packed = ops.pack(t, *ops.rtn_quantize(flat, t))
    return packed.view(*w.shape[:-1], -1).cpu().numpy()


def write_uniform_gguf(model, path, t):
    """The .gguf of `model` (on the GPU) with the attention projections and the expert tensors at ggml type `t`, in the tensor
    order and row layout of moe_gguf.write_gguf."""
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.gguf_writer import GGUFWriter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import permute
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    w = GGUFWriter(str(path), "llama")
    w.add_uint32("llama.block_count", M.LAYERS)
    w.add_uint32("llama.attention.head_count", M.HEADS)
    w.add_uint32("llama.attention.head_count_kv", M.KV_HEADS)
    w.add_uint32("llama.expert_count", M.E)
    w.add_uint32("llama.expert_used_count", M.K)

    def level(name, tensor, typ=t):
        w.add_tensor(name, encode(ops, tensor, typ), raw_dtype=typ)

    def plain(name, tensor):
        w.add_tensor(name, tensor.float().cpu().numpy().astype(np.float32))

    level("token_embd.weight", sd["model.embed_tokens.weight"], Q6)
    for n in range(M.LAYERS):
        pre, blk = f"model.layers.{n}.", f"blk.{n}."
        plain(blk + "attn_norm.weight", sd[pre + "input_layernorm.weight"])
        level(blk + "attn_q.weight", permute(sd[pre + "self_attn.q_proj.weight"], M.HEADS, M.HEADS))
        level(blk + "attn_k.weight", permute(sd[pre + "self_attn.k_proj.weight"], M.HEADS, M.KV_HEADS))
        level(blk + "attn_v.weight", sd[pre + "self_attn.v_proj.weight"])
        level(blk + "attn_output.weight", sd[pre + "self_attn.o_proj.weight"])
        plain(blk + "ffn_norm.weight", sd[pre + "post_attention_layernorm.weight"])
        plain(blk + "ffn_gate_inp.weight", sd[pre + "mlp.gate.weight"])
        gate_up = sd[pre + "mlp.experts.gate_up_proj"]  # [E, 2I, H]: per expert the gate rows, then the up rows
        level(blk + "ffn_gate_exps.weight", gate_up[:, :M.I].contiguous())
        level(blk + "ffn_down_exps.weight", sd[pre + "mlp.experts.down_proj"])
        level(blk + "ffn_up_exps.weight", gate_up[:, M.I:].contiguous())
    plain("output_norm.weight", sd["model.norm.weight"])
    level("output.weight", sd["lm_head.weight"], Q6)
    w.write()


def build(model, tmp, levels=tuple(LEVELS)):
    """Write `<tmp>/<level>.gguf` per level and split them all into `<tmp>/db` -> {"db": path, "files": {level: path}}."""
    from gptq_gguf_toolkit_amd import gguf_splitter
    files = {}
    for name in levels:
        files[name] = str(tmp / f"{name}.gguf")
        write_uniform_gguf(model, files[name], LEVELS[name][0])
        gguf_splitter.main([files[name], str(tmp / "db"), "--gguf-layers", "--exact"])
    return {"db": str(tmp / "db"), "files": files}


def uniform_state(name: str, layers=None):
    """{layer or unit: the level's bit width} for `layers` (default: every unit and every attention projection)."""
    return {n: LEVELS[name][1] for n in (UNITS + ATTENTION if layers is None else layers)}
