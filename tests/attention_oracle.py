"""CPU fp32 restatement of UNetModel(bottleneck_attention=True) (TEST INFRASTRUCTURE ONLY).

The concatenating model of oracle.unet with the middle block's AttentionBlock
(the reference's guided_diffusion/unet.py:314-360, its two attention orders
:383-444, placed at :635-642) between the two middle ResBlocks; the ResBlock
after it is then ``middle_block.2``.  Per block, on x (B, C, T):

    n   = GroupNorm(groups, C)(x)                    (no activation)
    qkv = W_qkv n + b_qkv                            (3C rows)
    w   = softmax_s(q_t . k_s / sqrt(ch)),  a_t = sum_s w_ts v_s    per head
    y   = x + W_proj a + b_proj

Legacy order: head i owns the qkv rows [q_i | k_i | v_i] (3 ch each); new
order: the rows are [Q of all heads | K of all | V of all].  oracle.unet's
ResBlock, time embedding and weight-drawing scheme are reused; ``proj_out`` is
drawn non-zero (the reference zero-initialises it, which would make every
comparison of the block vacuous).
"""
import math

import torch
import torch.nn.functional as F

from oracle import unet as ou

ATTN = "middle_block.1"


def topology(**cfg):
    """oracle.unet.topology with the attention block inserted after middle_block.0."""
    out = []
    for b in ou.topology(**cfg):
        b = dict(b)
        if b["prefix"] == "middle_block.1":
            out.append(dict(kind="attn", prefix=ATTN, cin=b["cin"], cout=b["cin"]))
            b["prefix"] = "middle_block.2"
        out.append(b)
    return out


def param_shapes(**cfg):
    """Ordered (name, shape) list of the attention model's state_dict."""
    plain = ou.param_shapes(**cfg)
    C = next(b["cin"] for b in topology(**cfg) if b["kind"] == "attn")
    out = []
    done = False
    for name, shape in plain:
        if name.startswith("middle_block.1."):
            if not done:
                out += [(ATTN + ".norm.weight", (C,)), (ATTN + ".norm.bias", (C,)),
                        (ATTN + ".qkv.weight", (3 * C, C, 1)), (ATTN + ".qkv.bias", (3 * C,)),
                        (ATTN + ".proj_out.weight", (C, C, 1)), (ATTN + ".proj_out.bias", (C,))]
                done = True
            name = "middle_block.2." + name[len("middle_block.1."):]
        out.append((name, shape))
    return out


def random_params(seed=1, std=0.05, **cfg):
    """oracle.unet.random_params' scheme over the attention model's shapes:
    GroupNorm gammas around 1, betas around 0 (the block's norm included),
    everything else -- proj_out too -- N(0, min(std, 1.5 / sqrt(fan_in)))."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, shape in param_shapes(**cfg):
        if len(shape) == 1 and (".in_layers.0." in name or ".out_layers.0." in name or name.startswith("out.0.")
                                or ".norm." in name):
            base = 1.0 if name.endswith("weight") else 0.0
            params[name] = base + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            scale = std if len(shape) == 1 else min(std, 1.0 / math.sqrt(max(fan_in, 1)) * 1.5)
            params[name] = scale * torch.randn(shape, generator=g)
    return params


def num_heads_of(C, num_heads=1, num_head_channels=-1):
    return num_heads if num_head_channels == -1 else C // num_head_channels


def split_heads(qkv, heads, new_order):
    """qkv (B, 3C, T) -> q, k, v each (B, heads, T, ch)."""
    B, C3, T = qkv.shape
    ch = C3 // (3 * heads)
    if new_order:
        q, k, v = (p.reshape(B, heads, ch, T) for p in qkv.chunk(3, dim=1))
    else:
        q, k, v = qkv.reshape(B, heads, 3 * ch, T).split(ch, dim=2)
    return tuple(p.transpose(2, 3) for p in (q, k, v))


def attention_ref(q, k, v):
    """softmax(q k^T / sqrt(ch)) v in float64: q, k, v (..., T, ch) -> (out, logsumexp of the scaled scores)."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)


def attention_block(P, x, groups, heads, new_order, p=ATTN):
    """x (B, C, *spatial) -> same shape, in x's dtype (fp32 in the tests)."""
    B, C = x.shape[:2]
    xt = x.reshape(B, C, -1)
    n = F.group_norm(xt, groups, P[p + ".norm.weight"], P[p + ".norm.bias"], eps=1e-5)
    qkv = F.conv1d(n, P[p + ".qkv.weight"], P[p + ".qkv.bias"])
    q, k, v = split_heads(qkv, heads, new_order)
    w = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), dim=-1)
    a = (w @ v).transpose(2, 3).reshape(B, C, -1)
    y = xt + F.conv1d(a, P[p + ".proj_out.weight"], P[p + ".proj_out.bias"])
    return y.reshape(x.shape)


def unet_forward(P, x, t, model_channels=64, num_groups=32, in_channels=32, out_channels=8, num_res_blocks=2,
                 channel_mult=(1, 2, 2, 4, 4), trace=None, resblock_updown=True, num_heads=1, num_head_channels=-1,
                 new_order=False):
    """UNetModel.forward with the middle attention; ``trace`` collects every block output."""
    emb = ou.timestep_embedding(t, model_channels)
    emb = F.linear(emb, P["time_embed.0.weight"], P["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), P["time_embed.2.weight"], P["time_embed.2.bias"])
    hs = []
    h = x
    for b in topology(in_channels=in_channels, model_channels=model_channels, out_channels=out_channels,
                      num_res_blocks=num_res_blocks, channel_mult=channel_mult, resblock_updown=resblock_updown):
        p = b["prefix"]
        if b["kind"] == "conv_in":
            h = F.conv3d(h, P[p + ".weight"], P[p + ".bias"], padding=1)
            hs.append(h)
        elif b["kind"] == "down":
            h = F.conv3d(h, P[p + ".weight"], P[p + ".bias"], stride=2, padding=1)
            hs.append(h)
        elif b["kind"] == "up":
            h = F.conv3d(F.interpolate(h, scale_factor=2, mode="nearest"), P[p + ".weight"], P[p + ".bias"],
                         padding=1)
        elif b["kind"] == "attn":
            h = attention_block(P, h, num_groups, num_heads_of(b["cin"], num_heads, num_head_channels), new_order)
        elif b["kind"] == "res":
            if "pop" in b:
                h = torch.cat([h, hs.pop()], dim=1)
            h = ou._resblock(P, p, h, emb, num_groups, b["updown"])
            if b.get("push"):
                hs.append(h)
        else:
            h = ou._gn_silu(h, P[p + ".0.weight"], P[p + ".0.bias"], num_groups)
            h = F.conv3d(h, P[p + ".2.weight"], P[p + ".2.bias"], padding=1)
        if trace is not None:
            trace.append(h)
    return h


class AttentionOracleUNet:
    """Callable ``model(x, t)`` seam around unet_forward (for oracle.diffusion)."""

    def __init__(self, params, **cfg):
        self.P = params
        self.cfg = cfg

    def __call__(self, x, t, **kw):
        with torch.no_grad():
            return unet_forward(self.P, x, t, **self.cfg)


def grads(cfg, groups, P, x, t, R, **attn):
    """Output and autograd gradients of sum(out * R) for every parameter."""
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = unet_forward(Pr, x, t, num_groups=groups, **cfg, **attn)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in Pr.items()}
