"""CPU fp32 restatement of UNetModel(additive_skips=True) (TEST INFRASTRUCTURE ONLY).

Restated from the reference's guided_diffusion/unet.py:661-719 (construction)
and :785-798 (forward): every output block pops a skip and takes
``h = (h + skip) / 2`` instead of ``cat([h, skip], 1)``; its first ResBlock maps
``ch -> mid_ch`` with ``mid_ch`` = the channels of the next entry left on the
skip stack (``model_channels`` when it is empty), and the level's up block keeps
``mid_ch``.  Encoder, middle block, head and all parameter names are those of
the concatenating model (oracle.unet), whose ResBlock, time embedding and
weight-drawing scheme are reused.
"""
import math

import torch
import torch.nn.functional as F

from oracle import unet as ou


def topology(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4),
             resblock_updown=True):
    """oracle.unet.topology with the decoder of additive_skips=True; a decoder
    block's ``pop`` = the channels of the skip it averages with (== its cin)."""
    cat = ou.topology(in_channels, model_channels, out_channels, num_res_blocks, channel_mult, resblock_updown)
    n_dec = sum(1 for b in cat if "pop" in b)
    first = next(i for i, b in enumerate(cat) if "pop" in b)
    blocks = [dict(b) for b in cat[:first]]          # conv_in, encoder, middle: unchanged
    chans = [model_channels]
    for b in blocks:
        if b.get("push"):
            chans.append(b["cout"])
    assert len(chans) == n_dec
    ch = blocks[-1]["cout"]
    idx = 0
    for level, _ in list(enumerate(channel_mult))[::-1]:
        for i in range(num_res_blocks + 1):
            ich = chans.pop()
            assert ich == ch, (ich, ch)                # h always has the channels of the skip it meets
            mid = chans[-1] if chans else model_channels
            blocks.append(dict(kind="res", prefix=f"output_blocks.{idx}.0", cin=ch, cout=mid, updown=None, pop=ich))
            ch = mid
            if level and i == num_res_blocks:
                if resblock_updown:
                    blocks.append(dict(kind="res", prefix=f"output_blocks.{idx}.1", cin=ch, cout=ch, updown="up"))
                else:
                    blocks.append(dict(kind="up", prefix=f"output_blocks.{idx}.1.conv", cin=ch, cout=ch))
            idx += 1
    blocks.append(dict(kind="out", prefix="out", cin=ch, cout=out_channels))
    return blocks


def param_shapes(in_channels=32, model_channels=64, out_channels=8, num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4),
                 resblock_updown=True):
    """Ordered (name, shape) list of the additive model's state_dict."""
    ted = 4 * model_channels
    out = [("time_embed.0.weight", (ted, model_channels)), ("time_embed.0.bias", (ted,)),
           ("time_embed.2.weight", (ted, ted)), ("time_embed.2.bias", (ted,))]
    for b in topology(in_channels, model_channels, out_channels, num_res_blocks, channel_mult, resblock_updown):
        p, ci, co = b["prefix"], b["cin"], b["cout"]
        if b["kind"] in ("conv_in", "down", "up"):
            out += [(p + ".weight", (co, ci, 3, 3, 3)), (p + ".bias", (co,))]
        elif b["kind"] == "res":
            out += [(p + ".in_layers.0.weight", (ci,)), (p + ".in_layers.0.bias", (ci,)),
                    (p + ".in_layers.2.weight", (co, ci, 3, 3, 3)), (p + ".in_layers.2.bias", (co,)),
                    (p + ".emb_layers.1.weight", (co, ted)), (p + ".emb_layers.1.bias", (co,)),
                    (p + ".out_layers.0.weight", (co,)), (p + ".out_layers.0.bias", (co,)),
                    (p + ".out_layers.3.weight", (co, co, 3, 3, 3)), (p + ".out_layers.3.bias", (co,))]
            if ci != co:
                out += [(p + ".skip_connection.weight", (co, ci, 1, 1, 1)), (p + ".skip_connection.bias", (co,))]
        else:
            out += [(p + ".0.weight", (ci,)), (p + ".0.bias", (ci,)),
                    (p + ".2.weight", (co, ci, 3, 3, 3)), (p + ".2.bias", (co,))]
    return out


def random_params(seed=1, std=0.05, **cfg):
    """oracle.unet.random_params' scheme over the additive shapes: GroupNorm
    gammas around 1, betas around 0, everything else N(0, min(std, 1.5 / sqrt(fan_in)))."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, shape in param_shapes(**cfg):
        if len(shape) == 1 and (".in_layers.0." in name or ".out_layers.0." in name or name.startswith("out.0.")):
            base = 1.0 if name.endswith("weight") else 0.0
            params[name] = base + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            scale = std if len(shape) == 1 else min(std, 1.0 / math.sqrt(max(fan_in, 1)) * 1.5)
            params[name] = scale * torch.randn(shape, generator=g)
    return params


def unet_forward(P, x, t, model_channels=64, num_groups=32, in_channels=32, out_channels=8, num_res_blocks=2,
                 channel_mult=(1, 2, 2, 4, 4), trace=None, resblock_updown=True):
    """UNetModel.forward with additive skips; ``trace`` collects every block output."""
    emb = ou.timestep_embedding(t, model_channels)
    emb = F.linear(emb, P["time_embed.0.weight"], P["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), P["time_embed.2.weight"], P["time_embed.2.bias"])
    hs = []
    h = x
    for b in topology(in_channels, model_channels, out_channels, num_res_blocks, channel_mult, resblock_updown):
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
        elif b["kind"] == "res":
            if "pop" in b:
                h = (h + hs.pop()) / 2
            h = ou._resblock(P, p, h, emb, num_groups, b["updown"])
            if b.get("push"):
                hs.append(h)
        else:
            h = ou._gn_silu(h, P[p + ".0.weight"], P[p + ".0.bias"], num_groups)
            h = F.conv3d(h, P[p + ".2.weight"], P[p + ".2.bias"], padding=1)
        if trace is not None:
            trace.append(h)
    return h


class AdditiveOracleUNet:
    """Callable ``model(x, t)`` seam around unet_forward (for oracle.diffusion)."""

    def __init__(self, params, **cfg):
        self.P = params
        self.cfg = cfg

    def __call__(self, x, t, **kw):
        with torch.no_grad():
            return unet_forward(self.P, x, t, **self.cfg)


def grads(cfg, groups, P, x, t, R):
    """Output and autograd gradients of sum(out * R) for every parameter."""
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = unet_forward(Pr, x, t, num_groups=groups, **cfg)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in Pr.items()}
