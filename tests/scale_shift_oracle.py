"""CPU fp32 restatement of UNetModel(use_scale_shift_norm=True) (TEST INFRASTRUCTURE ONLY).

The reference's guided_diffusion/unet.py ResBlock with FiLM conditioning:
``emb_layers.1`` is ``Linear(E, 2 C_out)`` and, with ``scale, shift =
chunk(emb_out, 2, dim=1)``,

    h = out_layers.0(h) * (1 + scale) + shift          (then SiLU, out_layers.3)

replaces ``h = h + emb_out`` before ``out_layers``; nothing else in the block
changes.  Time embedding, topology and the weight-drawing scheme are those of
oracle.unet; the decoder of ``additive_skips=True`` and the bottleneck
AttentionBlock come from tests/additive_oracle.py and tests/attention_oracle.py.
``out_layers.3`` is drawn non-zero, as everywhere in these restatements.
"""
import math

import torch
import torch.nn.functional as F

import additive_oracle as ado
import attention_oracle as ato
from oracle import unet as ou

ATTN = ato.ATTN


def topology(additive_skips=False, bottleneck_attention=False, **cfg):
    """The block list of the plain / additive model, the attention block inserted after middle_block.0."""
    out = []
    for b in (ado.topology(**cfg) if additive_skips else ou.topology(**cfg)):
        b = dict(b)
        if bottleneck_attention and b["prefix"] == "middle_block.1":
            out.append(dict(kind="attn", prefix=ATTN, cin=b["cin"], cout=b["cin"]))
            b["prefix"] = "middle_block.2"
        out.append(b)
    return out


def param_shapes(additive_skips=False, bottleneck_attention=False, **cfg):
    """Ordered (name, shape) list of the FiLM model's state_dict: the plain one's with
    ``emb_layers.1`` of shape (2 C_out, E) / (2 C_out)."""
    ted = 4 * cfg.get("model_channels", 64)
    out = [("time_embed.0.weight", (ted, ted // 4)), ("time_embed.0.bias", (ted,)),
           ("time_embed.2.weight", (ted, ted)), ("time_embed.2.bias", (ted,))]
    for b in topology(additive_skips, bottleneck_attention, **cfg):
        p, ci, co = b["prefix"], b["cin"], b["cout"]
        if b["kind"] in ("conv_in", "down", "up"):
            out += [(p + ".weight", (co, ci, 3, 3, 3)), (p + ".bias", (co,))]
        elif b["kind"] == "attn":
            out += [(p + ".norm.weight", (ci,)), (p + ".norm.bias", (ci,)),
                    (p + ".qkv.weight", (3 * ci, ci, 1)), (p + ".qkv.bias", (3 * ci,)),
                    (p + ".proj_out.weight", (ci, ci, 1)), (p + ".proj_out.bias", (ci,))]
        elif b["kind"] == "res":
            out += [(p + ".in_layers.0.weight", (ci,)), (p + ".in_layers.0.bias", (ci,)),
                    (p + ".in_layers.2.weight", (co, ci, 3, 3, 3)), (p + ".in_layers.2.bias", (co,)),
                    (p + ".emb_layers.1.weight", (2 * co, ted)), (p + ".emb_layers.1.bias", (2 * co,)),
                    (p + ".out_layers.0.weight", (co,)), (p + ".out_layers.0.bias", (co,)),
                    (p + ".out_layers.3.weight", (co, co, 3, 3, 3)), (p + ".out_layers.3.bias", (co,))]
            if ci != co:
                out += [(p + ".skip_connection.weight", (co, ci, 1, 1, 1)), (p + ".skip_connection.bias", (co,))]
        else:
            out += [(p + ".0.weight", (ci,)), (p + ".0.bias", (ci,)),
                    (p + ".2.weight", (co, ci, 3, 3, 3)), (p + ".2.bias", (co,))]
    return out


def random_params(seed=1, std=0.05, **cfg):
    """oracle.unet.random_params' scheme over the FiLM shapes: GroupNorm gammas around 1, betas
    around 0, everything else N(0, min(std, 1.5 / sqrt(fan_in)))."""
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


def film_rows(P, p, emb):
    """(scale, shift) of block ``p``: the two halves of emb_layers(emb), each (B, C_out)."""
    e = F.linear(F.silu(emb), P[p + ".emb_layers.1.weight"], P[p + ".emb_layers.1.bias"])
    return torch.chunk(e, 2, dim=1)


def resblock(P, p, x, emb, groups, updown):
    """ResBlock._forward with use_scale_shift_norm=True."""
    h = ou._gn_silu(x, P[p + ".in_layers.0.weight"], P[p + ".in_layers.0.bias"], groups)
    if updown == "down":
        h = F.avg_pool3d(h, kernel_size=2, stride=2)
        x = F.avg_pool3d(x, kernel_size=2, stride=2)
    elif updown == "up":
        h = F.interpolate(h, scale_factor=2, mode="nearest")
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    h = F.conv3d(h, P[p + ".in_layers.2.weight"], P[p + ".in_layers.2.bias"], padding=1)
    scale, shift = film_rows(P, p, emb)
    h = F.group_norm(h, groups, P[p + ".out_layers.0.weight"], P[p + ".out_layers.0.bias"], eps=1e-5)
    h = h * (1 + scale[:, :, None, None, None]) + shift[:, :, None, None, None]
    h = F.conv3d(F.silu(h), P[p + ".out_layers.3.weight"], P[p + ".out_layers.3.bias"], padding=1)
    if (p + ".skip_connection.weight") in P:
        x = F.conv3d(x, P[p + ".skip_connection.weight"], P[p + ".skip_connection.bias"])
    return x + h


def time_embed(P, t, model_channels):
    emb = ou.timestep_embedding(t, model_channels)
    emb = F.linear(emb, P["time_embed.0.weight"], P["time_embed.0.bias"])
    return F.linear(F.silu(emb), P["time_embed.2.weight"], P["time_embed.2.bias"])


def unet_forward(P, x, t, model_channels=64, num_groups=32, in_channels=32, out_channels=8, num_res_blocks=2,
                 channel_mult=(1, 2, 2, 4, 4), trace=None, resblock_updown=True, additive_skips=False,
                 bottleneck_attention=False, num_heads=1, num_head_channels=-1, new_order=False, scales=None):
    """UNetModel.forward with FiLM ResBlocks; ``trace`` collects every block output,
    ``scales`` every ResBlock's scale half (the tests' non-vacuity check)."""
    emb = time_embed(P, t, model_channels)
    hs = []
    h = x
    for b in topology(additive_skips, bottleneck_attention, in_channels=in_channels, model_channels=model_channels,
                      out_channels=out_channels, num_res_blocks=num_res_blocks, channel_mult=channel_mult,
                      resblock_updown=resblock_updown):
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
            h = ato.attention_block(P, h, num_groups, ato.num_heads_of(b["cin"], num_heads, num_head_channels),
                                    new_order)
        elif b["kind"] == "res":
            if "pop" in b:
                h = (h + hs.pop()) / 2 if additive_skips else torch.cat([h, hs.pop()], dim=1)
            if scales is not None:
                scales.append(film_rows(P, p, emb)[0].detach())
            h = resblock(P, p, h, emb, num_groups, b["updown"])
            if b.get("push"):
                hs.append(h)
        else:
            h = ou._gn_silu(h, P[p + ".0.weight"], P[p + ".0.bias"], num_groups)
            h = F.conv3d(h, P[p + ".2.weight"], P[p + ".2.bias"], padding=1)
        if trace is not None:
            trace.append(h)
    return h


class ScaleShiftOracleUNet:
    """Callable ``model(x, t)`` seam around unet_forward (for oracle.diffusion)."""

    def __init__(self, params, **cfg):
        self.P = params
        self.cfg = cfg

    def __call__(self, x, t, **kw):
        with torch.no_grad():
            return unet_forward(self.P, x, t, **self.cfg)


def grads(cfg, groups, P, x, t, R, **opts):
    """Output and autograd gradients of sum(out * R) for every parameter."""
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = unet_forward(Pr, x, t, num_groups=groups, **cfg, **opts)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in Pr.items()}
