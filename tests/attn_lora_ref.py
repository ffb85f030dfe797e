"""Float restatement of a vision block whose attention projections carry adapters (LoraCfg.targets with 'attn').

There is no reference behaviour for this placement, so this helper is the yardstick of the attention-site tests.  It is
written with the oracle's own pieces - `layer_norm`, `fairlora_linear`, `quick_gelu` and the body of `mha` - and is itself
checked against the UNCHANGED oracle on merged weights (tests/test_attn_lora_cpu.py).  `adapted_oracle()` substitutes it
for `oracle.fairlora_oracle.vision_block`, so `clip_logits` / `loss_and_grads` / `train_step` are reused as they are.
A site whose keys are absent from the state dict is a plain linear, so one block function serves every `targets`."""
from contextlib import contextmanager

import torch
import torch.nn.functional as F

from oracle import fairlora_oracle as O


def _site(inp, sd, q, W, b, attr, scaling):
    """y = inp W^T + b (+ the adapter under prefix q, if the state dict has one)."""
    if q + "lora_A.weight" not in sd:
        return F.linear(inp, W, b)
    return O.fairlora_linear(inp, W, b, sd[q + "lora_A.weight"], sd.get(q + "lora_S.weight"), sd[q + "lora_B.weight"],
                             attr, scaling, sd.get(q + "lora_S_global.weight"))


def adapted_block(x, sd, p, heads, attr, scaling):
    """ResidualAttentionBlock (clip/model.py:325-357) with adapters on attn.in_proj / attn.out_proj and / or the MLP."""
    h = O.layer_norm(x, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
    # the body of oracle.mha: the adapter acts on the packed projection, before q is scaled
    L, N, E = h.shape
    hd = E // heads
    qkv = _site(h, sd, p + "attn.in_proj_lora.", sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"], attr, scaling)
    q, k, v = qkv.chunk(3, dim=-1)
    q = q.reshape(L, N * heads, hd).transpose(0, 1) * (hd ** -0.5)
    k = k.reshape(L, N * heads, hd).transpose(0, 1)
    v = v.reshape(L, N * heads, hd).transpose(0, 1)
    pr = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    o = (pr @ v).transpose(0, 1).reshape(L, N, E)
    x = x + _site(o, sd, p + "attn.out_proj_lora.", sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"], attr, scaling)
    h = O.layer_norm(x, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])

    def mlp(name, inp):
        q_ = f"{p}mlp.{name}."
        return _site(inp, sd, q_, sd[q_ + "original_linear.weight"], sd[q_ + "original_linear.bias"], attr, scaling)

    return x + mlp("c_proj", O.quick_gelu(mlp("c_fc", h)))


@contextmanager
def adapted_oracle():
    """Inside: the oracle's vision tower runs `adapted_block`.  oracle/ itself is not edited."""
    keep = O.vision_block
    O.vision_block = adapted_block
    try:
        yield O
    finally:
        O.vision_block = keep


def merged_state_dict(sd, cfg):
    """A default-targets state dict computing the same function for attr=None: the dense update of the attention adapters,
    scaling * (A diag(s_bar) B)^T with s_bar the uniform group mix, added to in_proj_weight / out_proj.weight, and the
    attention adapters' keys dropped."""
    lo = cfg.lora
    out = {k: v.clone() for k, v in sd.items() if ".attn.in_proj_lora." not in k and ".attn.out_proj_lora." not in k}
    for i in range(cfg.vision.layers):
        p = f"image_encoder.transformer.resblocks.{i}.attn."
        for site, wkey in (("in_proj_lora.", "in_proj_weight"), ("out_proj_lora.", "out_proj.weight")):
            q = p + site
            A, B = sd[q + "lora_A.weight"].double(), sd[q + "lora_B.weight"].double()
            S = sd.get(q + "lora_S.weight")
            if S is None:
                s = torch.ones(A.shape[1], dtype=torch.float64)
            elif S.dim() == 1:
                s = S.double()
            else:
                s = S.double().mean(0)
            if q + "lora_S_global.weight" in sd:
                s = s + sd[q + "lora_S_global.weight"].double()
            dw = lo.scaling * ((A * s[None]) @ B).t()
            out[p + wkey] = (sd[p + wkey].double() + dw).to(sd[p + wkey].dtype)
        # targets 'attn' has no MLP adapters, the unchanged oracle's block always reads them: give it the no-op (A = B = 0)
        for name in ("c_fc", "c_proj"):
            q = f"image_encoder.transformer.resblocks.{i}.mlp.{name}."
            if q + "lora_A.weight" not in out:
                W = sd[q + "original_linear.weight"]
                out[q + "lora_A.weight"] = torch.zeros(W.shape[1], lo.rank, dtype=W.dtype)
                out[q + "lora_B.weight"] = torch.zeros(lo.rank, W.shape[0], dtype=W.dtype)
    return out
