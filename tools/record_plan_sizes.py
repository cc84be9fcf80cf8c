"""Print the sizes and FLOPs of a set of U-Net plans as JSON (no GPU needed: plan creation and the size
queries are host code).  tests/golden/cond_count_sizes.json is this script's output from the library of the
commit before unaligned in_channels were supported; tests/test_cond_count_cpu.py holds later trees to it.

    python tools/record_plan_sizes.py > tests/golden/cond_count_sizes.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-cwdm_amd"))

MODELS = {   # name: (model_channels, num_res_blocks, channel_mult, num_groups)
    "tiny": (32, 1, (1, 2), 8),
    "prod": (64, 2, (1, 2, 2, 4, 4), 32),
}
GRIDS = {"tiny": [(2, 16, 16, 16), (1, 32, 32, 32)], "prod": [(1, 64, 64, 64), (1, 128, 128, 128)]}
IN_CHANNELS = (16, 32)
DTYPES = ("fp32", "bf16", "fp16")


def record(in_channels, model, dtype):
    from cwdm_hip.unet_runtime import UNetPlan
    mc, nrb, mult, groups = MODELS[model]
    plan = UNetPlan(in_channels, mc, 8, nrb, mult, groups, dtype)
    rec = {"packed_bytes": plan.packed_bytes, "packed_bwd_bytes": plan.packed_bwd_bytes,
           "num_segments": plan.num_segments, "grids": {}}
    for g in GRIDS[model]:
        rec["grids"]["x".join(str(v) for v in g)] = {
            "workspace_bytes": plan.workspace_bytes(*g), "train_workspace_bytes": plan.train_workspace_bytes(*g),
            "grad_workspace_bytes": plan.grad_workspace_bytes(*g), "flops": plan.flops(*g),
            "backward_flops": plan.backward_flops(*g)}
    return rec


def main():
    out = {}
    for model in MODELS:
        for cin in IN_CHANNELS:
            for dt in DTYPES:
                out[f"{model}/in{cin}/{dt}"] = record(cin, model, dt)
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
