"""A 2-layer MixtralForCausalLM (hidden 256, intermediate 512, 4 heads, 2 KV heads, 4 experts, top-2, vocab 512, fp16) and
its .gguf, written directly: every tensor quantized with ops.rtn_quantize + ops.pack (Q8_0: ops.quantize_q8_0) and stored by
the package's gguf_writer under the names and in the row order pack_gptq_into_gguf gives them (q / k rows permuted, the
experts stacked [E, R, C]).  Test scaffolding only: the Quantizer does not take transformers 5.x's fused experts yet.

  layer 0: gate Q4_K, up Q5_K, down Q6_K        layer 1: gate Q2_K, up Q3_K, down Q8_0
  attention Q4_K, router and norms F32, token_embd and output Q6_K"""
import numpy as np
import torch

Q2, Q3, Q4, Q5, Q6, Q8 = 10, 11, 12, 13, 14, 8
EXPERT_TYPES = ({"gate": Q4, "up": Q5, "down": Q6}, {"gate": Q2, "up": Q3, "down": Q8})
E, K, H, I, V, HEADS, KV_HEADS, LAYERS = 4, 2, 256, 512, 512, 4, 2, 2


def config():
    from transformers import MixtralConfig
    return MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         num_key_value_heads=KV_HEADS, num_local_experts=E, num_experts_per_tok=K, vocab_size=V,
                         max_position_embeddings=128, tie_word_embeddings=False, router_jitter_noise=0.0)


def build_hf(path, seed=0):
    """Save the randomly initialised fp16 model to `path` (it is then LOADED from there, as ppleval and generate load it)."""
    from transformers import MixtralForCausalLM
    torch.manual_seed(seed)
    MixtralForCausalLM(config()).half().save_pretrained(str(path), safe_serialization=True)


def load_hf(path):
    from transformers import AutoModelForCausalLM
    return AutoModelForCausalLM.from_pretrained(str(path), dtype=torch.float16, attn_implementation="eager",
                                                experts_implementation="eager").cuda().eval()  # MixtralExperts.forward's own loop


def _blocks(ops, w, t):
    """[.., R, C] on the device -> packed uint8 [.., R, row bytes] as a numpy array."""
    flat = w.reshape(-1, w.shape[-1]).float().contiguous()
    packed = ops.quantize_q8_0(flat) if t == Q8 else ops.pack(t, *ops.rtn_quantize(flat, t))
    return packed.view(*w.shape[:-1], -1).cpu().numpy()


def write_gguf(model, path):
    """The .gguf of `model` (on the GPU) -> {GGUF tensor name: ggml type} of what was written."""
    from gptq_gguf_toolkit_amd import ops
    from gptq_gguf_toolkit_amd.gguf_writer import GGMLType, GGUFWriter
    from gptq_gguf_toolkit_amd.pack_gptq_into_gguf import permute
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    w = GGUFWriter(str(path), "llama")
    w.add_uint32("llama.block_count", LAYERS)
    w.add_uint32("llama.attention.head_count", HEADS)
    w.add_uint32("llama.attention.head_count_kv", KV_HEADS)
    w.add_uint32("llama.expert_count", E)
    w.add_uint32("llama.expert_used_count", K)
    types = {}

    def quant(name, t, tensor):
        types[name] = t
        w.add_tensor(name, _blocks(ops, tensor, t), raw_dtype=t)

    def plain(name, tensor):
        types[name] = int(GGMLType.F32)
        w.add_tensor(name, tensor.float().cpu().numpy().astype(np.float32))

    quant("token_embd.weight", Q6, sd["model.embed_tokens.weight"])
    for n in range(LAYERS):
        pre, blk = f"model.layers.{n}.", f"blk.{n}."
        plain(blk + "attn_norm.weight", sd[pre + "input_layernorm.weight"])
        quant(blk + "attn_q.weight", Q4, permute(sd[pre + "self_attn.q_proj.weight"], HEADS, HEADS))
        quant(blk + "attn_k.weight", Q4, permute(sd[pre + "self_attn.k_proj.weight"], HEADS, KV_HEADS))
        quant(blk + "attn_v.weight", Q4, sd[pre + "self_attn.v_proj.weight"])
        quant(blk + "attn_output.weight", Q4, sd[pre + "self_attn.o_proj.weight"])
        plain(blk + "ffn_norm.weight", sd[pre + "post_attention_layernorm.weight"])
        plain(blk + "ffn_gate_inp.weight", sd[pre + "mlp.gate.weight"])
        gate_up = sd[pre + "mlp.experts.gate_up_proj"]  # [E, 2I, H]: per expert the gate rows, then the up rows
        quant(blk + "ffn_gate_exps.weight", EXPERT_TYPES[n]["gate"], gate_up[:, :I].contiguous())
        quant(blk + "ffn_down_exps.weight", EXPERT_TYPES[n]["down"], sd[pre + "mlp.experts.down_proj"])
        quant(blk + "ffn_up_exps.weight", EXPERT_TYPES[n]["up"], gate_up[:, I:].contiguous())
    plain("output_norm.weight", sd["model.norm.weight"])
    quant("output.weight", Q6, sd["lm_head.weight"])
    w.write()
    return types
