"""CPU fp32 restatement of UNetModel(dropout=p) in training mode (TEST INFRASTRUCTURE ONLY).

The reference's ResBlock puts ``nn.Dropout(p)`` between out_layers' SiLU and its conv
(guided_diffusion/unet.py:255-262).  torch's own dropout stream is not reproducible on the device, so the
native model specifies its mask (include/cwdm.h, cwdm_gn_silu_dropout) and this module restates it with
oracle.philox:

    blk  = philox4x32_10(ctr = (v & 0xffffffff, v >> 32, site, (b << 16) | (c >> 2)),
                         key = (seed & 0xffffffff, seed >> 32))
    keep = (blk[c & 3] >> 8) >= floor(p * 2^24)
    u    = keep ? SiLU(...) * inv : 0,   inv = 1.0f / (1.0f - (float)p)

v = voxel index of conv2's grid inside batch entry b (NDHWC order), c = channel, site = ordinal of the ResBlock
among the model's ResBlocks in forward order.  Topology, time embedding and weights are oracle.unet's; the FiLM
variant (use_scale_shift_norm) takes its rows from tests/scale_shift_oracle.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

import scale_shift_oracle as sso
from oracle import philox
from oracle import unet as ou


def threshold(p):
    return int(np.floor(float(p) * 2.0 ** 24))


def inv_keep(p):
    """1.0f / (1.0f - (float)p) as the kernels' host side computes it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed, site, B, V, C, p):
    """The keep mask of one dropout site, bool numpy (B, V, C)."""
    assert C % 4 == 0 and B < 65536
    v = np.arange(V, dtype=np.int64)
    ctr = np.empty((B, V, C // 4, 4), np.uint32)
    ctr[..., 0] = (v & 0xFFFFFFFF).astype(np.uint32)[None, :, None]
    ctr[..., 1] = (v >> 32).astype(np.uint32)[None, :, None]
    ctr[..., 2] = np.uint32(site)
    ctr[..., 3] = (np.arange(B, dtype=np.uint32)[:, None, None] << np.uint32(16)) | \
        np.arange(C // 4, dtype=np.uint32)[None, None, :]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    blk = philox.philox4x32_10(ctr, key)                       # (B, V, C / 4, 4): channel 4 k + j at [k, j]
    return ((blk >> np.uint32(8)) >= np.uint32(threshold(p))).reshape(B, V, C)


def mask_ncdhw(seed, site, shape, p):
    """keep_mask for an NCDHW activation of ``shape``, as a float tensor of 0 / 1."""
    B, C, D, H, W = shape
    m = keep_mask(seed, site, B, D * H * W, C, p)
    return torch.from_numpy(m).view(B, D, H, W, C).permute(0, 4, 1, 2, 3).float()


def resblock(P, p, x, emb, groups, updown, film, mask_of):
    """ResBlock._forward with the dropout between out_layers' SiLU and conv; mask_of(shape) -> 0/1 mask * inv."""
    h = ou._gn_silu(x, P[p + ".in_layers.0.weight"], P[p + ".in_layers.0.bias"], groups)
    if updown == "down":
        h = F.avg_pool3d(h, kernel_size=2, stride=2)
        x = F.avg_pool3d(x, kernel_size=2, stride=2)
    elif updown == "up":
        h = F.interpolate(h, scale_factor=2, mode="nearest")
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    h = F.conv3d(h, P[p + ".in_layers.2.weight"], P[p + ".in_layers.2.bias"], padding=1)
    if film:
        scale, shift = sso.film_rows(P, p, emb)
        h = F.group_norm(h, groups, P[p + ".out_layers.0.weight"], P[p + ".out_layers.0.bias"], eps=1e-5)
        h = F.silu(h * (1 + scale[:, :, None, None, None]) + shift[:, :, None, None, None])
    else:
        e = F.linear(F.silu(emb), P[p + ".emb_layers.1.weight"], P[p + ".emb_layers.1.bias"])
        h = ou._gn_silu(h + e[:, :, None, None, None], P[p + ".out_layers.0.weight"], P[p + ".out_layers.0.bias"],
                        groups)
    h = h * mask_of(h.shape)
    h = F.conv3d(h, P[p + ".out_layers.3.weight"], P[p + ".out_layers.3.bias"], padding=1)
    if (p + ".skip_connection.weight") in P:
        x = F.conv3d(x, P[p + ".skip_connection.weight"], P[p + ".skip_connection.bias"])
    return x + h


def unet_forward(P, x, t, p_drop, seed, film=False, model_channels=64, num_groups=32, in_channels=32, out_channels=8,
                 num_res_blocks=2, channel_mult=(1, 2, 2, 4, 4), resblock_updown=True, kept=None):
    """UNetModel.forward in training mode with dropout p_drop and the masks of ``seed``; ``kept`` (optional list)
    collects every site's kept fraction.  p_drop = 0 is the plain forward."""
    emb = sso.time_embed(P, t, model_channels)
    inv = float(inv_keep(p_drop))
    hs = []
    h = x
    site = 0
    for b in ou.topology(in_channels, model_channels, out_channels, num_res_blocks, channel_mult, resblock_updown):
        pre = b["prefix"]
        if b["kind"] == "conv_in":
            h = F.conv3d(h, P[pre + ".weight"], P[pre + ".bias"], padding=1)
            hs.append(h)
        elif b["kind"] == "down":
            h = F.conv3d(h, P[pre + ".weight"], P[pre + ".bias"], stride=2, padding=1)
            hs.append(h)
        elif b["kind"] == "up":
            h = F.conv3d(F.interpolate(h, scale_factor=2, mode="nearest"), P[pre + ".weight"], P[pre + ".bias"],
                         padding=1)
        elif b["kind"] == "res":
            if "pop" in b:
                h = torch.cat([h, hs.pop()], dim=1)

            def mask_of(shape, site=site):
                m = mask_ncdhw(seed, site, shape, p_drop)
                if kept is not None:
                    kept.append(float(m.mean()))
                return m * inv

            h = resblock(P, pre, h, emb, num_groups, b["updown"], film, mask_of)
            site += 1
            if b.get("push"):
                hs.append(h)
        else:
            h = ou._gn_silu(h, P[pre + ".0.weight"], P[pre + ".0.bias"], num_groups)
            h = F.conv3d(h, P[pre + ".2.weight"], P[pre + ".2.bias"], padding=1)
    return h


def grads(cfg, groups, P, x, t, R, p_drop, seed, film=False, kept=None):
    """Output and autograd gradients of sum(out * R) for every parameter."""
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    out = unet_forward(Pr, x, t, p_drop, seed, film=film, num_groups=groups, kept=kept, **cfg)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in Pr.items()}
