"""CPU fp32 restatement of UNetModel(num_classes=n) (TEST INFRASTRUCTURE ONLY).

The reference's guided_diffusion/unet.py:541-542 registers
``label_emb = nn.Embedding(num_classes, 4 * model_channels)`` between
``time_embed`` and ``input_blocks`` and, in forward (:763-774),

    emb = time_embed(timestep_embedding(t)) + label_emb(y)

with ``y`` an integer tensor of shape (B,); every ResBlock then reads this
``emb``.  Nothing else changes.  Time embedding, ResBlock, topology and the
weight-drawing scheme are those of oracle.unet; the FiLM ResBlock, the decoder
of ``additive_skips=True`` and the bottleneck AttentionBlock come from
tests/scale_shift_oracle.py, tests/additive_oracle.py and
tests/attention_oracle.py, so one forward covers the class-conditional model
with each of those switches.  The table's rows are drawn N(0, ``std``) (the
reference's N(0, 1) would swamp the time embedding in every comparison).
"""
import math

import torch
import torch.nn.functional as F

import attention_oracle as ato
import scale_shift_oracle as sso
from oracle import unet as ou

LABEL = "label_emb.weight"


def param_shapes(num_classes, use_scale_shift_norm=False, additive_skips=False, bottleneck_attention=False, **cfg):
    """Ordered (name, shape) list of the class-conditional state_dict: the model's own list with
    ``label_emb.weight`` right after ``time_embed.2.bias``."""
    base = sso.param_shapes(additive_skips, bottleneck_attention, **cfg)
    ted = 4 * cfg.get("model_channels", 64)
    out = []
    for name, shape in base:
        if not use_scale_shift_norm and ".emb_layers.1." in name:
            shape = (shape[0] // 2,) + tuple(shape[1:])
        out.append((name, tuple(shape)))
        if name == "time_embed.2.bias":
            out.append((LABEL, (num_classes, ted)))
    return out


def random_params(num_classes, seed=1, std=0.05, **opts):
    """oracle.unet.random_params' scheme over the class-conditional shapes: GroupNorm gammas around 1, betas
    around 0, the table's rows N(0, std), everything else N(0, min(std, 1.5 / sqrt(fan_in)))."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, shape in param_shapes(num_classes, **opts):
        if len(shape) == 1 and (".in_layers.0." in name or ".out_layers.0." in name or name.startswith("out.0.")
                                or ".norm." in name):
            base = 1.0 if name.endswith("weight") else 0.0
            params[name] = base + 0.1 * torch.randn(shape, generator=g)
        elif name == LABEL:
            params[name] = std * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            scale = std if len(shape) == 1 else min(std, 1.0 / math.sqrt(max(fan_in, 1)) * 1.5)
            params[name] = scale * torch.randn(shape, generator=g)
    return params


def embedding(P, t, y, model_channels):
    """emb = time_embed(t) + label_emb(y), the reference's order; ``y`` None: the plain model's emb."""
    emb = sso.time_embed(P, t, model_channels)
    if y is not None:
        assert y.shape == (t.shape[0],)
        emb = emb + F.embedding(y, P[LABEL])
    return emb


def unet_forward(P, x, t, y, model_channels=64, num_groups=32, in_channels=32, out_channels=8, num_res_blocks=2,
                 channel_mult=(1, 2, 2, 4, 4), resblock_updown=True, use_scale_shift_norm=False,
                 additive_skips=False, bottleneck_attention=False, num_heads=1, num_head_channels=-1,
                 new_order=False):
    """UNetModel.forward(x, t, y) of the class-conditional model, with the other switches."""
    emb = embedding(P, t, y, model_channels)
    resblock = sso.resblock if use_scale_shift_norm else ou._resblock
    hs = []
    h = x
    for b in sso.topology(additive_skips, bottleneck_attention, in_channels=in_channels,
                          model_channels=model_channels, out_channels=out_channels, num_res_blocks=num_res_blocks,
                          channel_mult=channel_mult, resblock_updown=resblock_updown):
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
            h = resblock(P, p, h, emb, num_groups, b["updown"])
            if b.get("push"):
                hs.append(h)
        else:
            h = ou._gn_silu(h, P[p + ".0.weight"], P[p + ".0.bias"], num_groups)
            h = F.conv3d(h, P[p + ".2.weight"], P[p + ".2.bias"], padding=1)
    return h


class ClassCondOracleUNet:
    """Callable ``model(x, t, y=y)`` seam around unet_forward."""

    def __init__(self, params, **cfg):
        self.P = params
        self.cfg = cfg

    def __call__(self, x, t, y=None, **kw):
        with torch.no_grad():
            return unet_forward(self.P, x, t, y, **self.cfg)


def grads(cfg, groups, P, x, t, y, R, **opts):
    """Output and autograd gradients of sum(out * R) for every parameter (the table's included: rows of classes
    absent from ``y`` come out as zeros)."""
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = unet_forward(Pr, x, t, y, num_groups=groups, **cfg, **opts)
    (out * R).sum().backward()
    return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pr.items()}
