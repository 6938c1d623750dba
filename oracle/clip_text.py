"""CPU restatement (TEST INFRASTRUCTURE ONLY - see oracle/__init__.py) of the text conditioner on the T23D path.

sgm.modules.encoders.modules.FrozenCLIPEmbedder (/root/reference/sgm/modules/encoders/modules.py:347-405) wraps the
third-party HuggingFace `CLIPTextModel` ("openai/clip-vit-large-patch14", layer="last", always_return_pooled=True,
sgm/configs/txt2img-clipl-compat.yaml).  The arithmetic therefore lives in `transformers` (not vendored in the reference);
it IS installed in the build container, so this restatement is pinned against it by tests/golden/make_golden_clip.py
(fixtures clip_text_*.npz).  Published algorithm: token + learned position embeddings; pre-LN transformer with CAUSAL
self-attention (no padding mask is passed by the reference), quick-GELU MLP; final LayerNorm; pooled = final-LN state at the
EOS position (legacy configs with eos_token_id == 2: position of the largest token id).
State-dict keys follow the hub checkpoint: text_model.{embeddings,encoder.layers.N.*,final_layer_norm}.

Working precision and rounding are oracle.dit's: the state dict's dtype is kept (fp32 stays fp32, float64 runs in float64 end to end)
and every GEMM, norm and attention goes through oracle.dit.linear / layer_norm / sdpa, so operand_rounding(torch.bfloat16,
kernel_arith=True) restates the HIP tower (tests/cond_token_refs.py): bf16 GEMM operands with the bias and the residual on the
fp32 accumulator, q / k / v stored bf16, the single-pass causal softmax of attn_short_kernel.  The quick-GELU stays the exact
x * sigmoid(1.702 x) in every mode (oracle.dit.quick_gelu says why).
"""
import torch

from .dit import _fp, layer_norm, linear, quick_gelu, sdpa


def eos_positions(ids, eos_token_id=2):
    """the pooled position of every prompt: the FIRST eos_token_id; legacy configs (eos_token_id == 2): the first largest id"""
    ids = ids.to(torch.int)
    return ids.argmax(-1) if eos_token_id == 2 else (ids == eos_token_id).int().argmax(-1)


def clip_text_forward(sd, ids, heads, eos_token_id=2, eps=1e-5, prefix='text_model.'):
    g = lambda k: _fp(sd[prefix + k])
    B, T = ids.shape
    h = g('embeddings.token_embedding.weight')[ids] + g('embeddings.position_embedding.weight')[:T][None]
    D = h.shape[-1]
    Dh = D // heads
    n_layers = 1 + max(int(k[len(prefix):].split('.')[2]) for k in sd if k.startswith(prefix + 'encoder.layers.'))
    for i in range(n_layers):
        L = f'encoder.layers.{i}.'
        x = layer_norm(h, eps, g(L + 'layer_norm1.weight'), g(L + 'layer_norm1.bias'))
        q, k, v = (linear(x, g(L + f'self_attn.{n}_proj.weight'), g(L + f'self_attn.{n}_proj.bias')) for n in 'qkv')
        q, k, v = (t.reshape(B, T, heads, Dh).transpose(1, 2) for t in (q, k, v))
        a = sdpa(q, k, v, causal=True).transpose(1, 2).reshape(B, T, D)
        h = h + linear(a, g(L + 'self_attn.out_proj.weight'), g(L + 'self_attn.out_proj.bias'))
        x = layer_norm(h, eps, g(L + 'layer_norm2.weight'), g(L + 'layer_norm2.bias'))
        x = linear(x, g(L + 'mlp.fc1.weight'), g(L + 'mlp.fc1.bias'))
        x = quick_gelu(x)
        h = h + linear(x, g(L + 'mlp.fc2.weight'), g(L + 'mlp.fc2.bias'))
    last = layer_norm(h, eps, g('final_layer_norm.weight'), g('final_layer_norm.bias'))
    return last, last[torch.arange(B), eos_positions(ids, eos_token_id)]
