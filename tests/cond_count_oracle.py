"""Test infrastructure: oracle.diffusion.training_losses restated for a list of N condition volumes and for
the unconditional mode (N = 0), on oracle.haar and oracle.diffusion.q_sample.  With the three BraTS conditions
in order it is oracle.diffusion.training_losses line for line; oracle.unet is general in in_channels already.

The reference's own family (run.sh:65, "8 + 8x" input channels): x = 0 is scripts/train.py's default
(in_channels=8, mode='default'), whose training_losses never binds ``target`` (gaussian_diffusion.py:1139), so
the unconditional loss is defined here as the i2i loss with no condition."""
import torch

from oracle import diffusion as od
from oracle import haar


def front_end(tab, target, conds, t, noise_img):
    """(x_in (B, 8 + 8 N, d, h, w), x0 (B, 8, d, h, w)): q_sample of the target's DWT (LLL / 3) with the noise
    image's DWT (no / 3), then the conditions' DWTs (LLL / 3) in the order given."""
    x0 = haar.dwt_cat(target)
    eps = torch.cat(list(haar.dwt3d(noise_img)), dim=1)
    x_t = od.q_sample(tab, x0, t, eps)
    return torch.cat([x_t] + [haar.dwt_cat(c) for c in conds], dim=1), x0


def training_losses(tab, model, target, conds, t, noise_img):
    """(terms{"mse_wav": [8]}, model_output, model_output_idwt) for N = len(conds) conditions."""
    x_in, x0 = front_end(tab, target, conds, t, noise_img)
    model_t = torch.tensor(tab.timestep_map, dtype=t.dtype)[t]
    out = model(x_in, model_t)
    out_idwt = haar.idwt_split(out)
    mse = ((x0 - out) ** 2).mean(dim=list(range(2, out.dim()))).mean(dim=0)
    return {"mse_wav": mse}, out, out_idwt
