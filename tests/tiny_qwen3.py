"""Test scaffolding shared by tests/test_qwen3_cpu.py and tests/test_gpu_qk_norm_rope.py: a 2-layer random Qwen3 (hidden 256,
4 / 2 heads of head_dim 64, vocab 512) whose q_norm / k_norm weights are not the constructor's ones, its calibration ids, and a
synthetic byte-level BPE tokenizer.json of the same vocabulary size.  The product package never imports it."""
import json

import torch

H, FFN, LAYERS, N_HEAD, N_KV, HEAD_DIM, VOCAB = 256, 512, 2, 4, 2, 64, 512
LINEARS = r".*layers.*((q|k|v|o|gate|up|down)_proj)$"


def tiny_qwen3(seed=0, dtype=torch.float32, tie=False):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(hidden_size=H, intermediate_size=FFN, num_hidden_layers=LAYERS, num_attention_heads=N_HEAD,
                      num_key_value_heads=N_KV, head_dim=HEAD_DIM, vocab_size=VOCAB, max_position_embeddings=128,
                      rms_norm_eps=1e-6, tie_word_embeddings=tie, attn_implementation="eager")
    torch.manual_seed(seed)
    model = Qwen3ForCausalLM(cfg)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        for layer in model.model.layers:  # a norm of ones would hide a q / k weight mix-up
            layer.self_attn.q_norm.weight.copy_(0.5 + torch.rand(HEAD_DIM, generator=g))
            layer.self_attn.k_norm.weight.copy_(0.5 + torch.rand(HEAD_DIM, generator=g))
    return model.to(dtype).eval()


def tiny_calib(n=8, L=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (1, L), generator=g) for _ in range(n)]


def bytes_to_unicode():
    """GPT-2's byte-level alphabet: every byte as one printable letter."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


def write_bpe_tokenizer(dir_model, vocab_size=VOCAB):
    """tokenizer.json / tokenizer_config.json of a byte-level BPE vocabulary: the 256 letters, merges of letter pairs up to
    vocab_size - 2, and two special tokens at the end (Qwen's <|endoftext|> and <|im_end|>).  -> (tokens in id order, merges)."""
    letters = [bytes_to_unicode()[b] for b in range(256)]
    vocab = {t: i for i, t in enumerate(letters)}
    merges = []
    a = bytes_to_unicode()
    lower = [a[b] for b in range(ord("a"), ord("z") + 1)]
    for x in [a[ord(" ")]] + lower:
        for y in lower:
            if len(vocab) >= vocab_size - 2:
                break
            merges.append(f"{x} {y}")
            vocab[x + y] = len(vocab)
    assert len(vocab) == vocab_size - 2
    added = [{"id": vocab_size - 2, "content": "<|endoftext|>", "special": True},
             {"id": vocab_size - 1, "content": "<|im_end|>", "special": True}]
    tok = {"version": "1.0", "added_tokens": added,
           "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": False, "use_regex": True},
           "decoder": {"type": "ByteLevel"},
           "model": {"type": "BPE", "vocab": vocab, "merges": merges}}
    (dir_model / "tokenizer.json").write_text(json.dumps(tok), encoding="utf-8")
    (dir_model / "tokenizer_config.json").write_text(json.dumps({"eos_token": "<|endoftext|>", "pad_token": "<|endoftext|>",
                                                                 "add_bos_token": False}))
    return list(vocab) + [t["content"] for t in added], merges
