"""Host-side AddressSanitizer + UBSan over the attention plans' host logic (no
GPU): tests/asan/plan_attn_asan.cpp, a stand-alone program, compiled on its own
with -Xarch_host -fsanitize=address,undefined and linked against the object
files of the sanitized library build test_asan_cpu already keeps under
fast-cwdm_amd/build/asan/<source hash>/ (built through its asan_binary() when
missing).  The program runs directly; nothing is preloaded."""
import glob
import os
import subprocess

from conftest import ROOT
from test_asan_cpu import asan_binary

SAN = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host",
       "-fno-omit-frame-pointer"]
HIPCC = "/opt/rocm/bin/hipcc"


def attn_binary():
    out = os.path.dirname(asan_binary())
    drv = os.path.join(ROOT, "tests", "asan", "plan_attn_asan.cpp")
    exe = os.path.join(out, "plan_attn_asan")
    objs = sorted(glob.glob(os.path.join(out, "*.hip.o")) + glob.glob(os.path.join(out, "*.cpp.o")))
    assert any(o.endswith("attention.hip.o") for o in objs) and any(o.endswith("unet_plan.cpp.o") for o in objs), objs
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(drv):
        obj = os.path.join(out, "attn_driver.o")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", *SAN,
                        "-I" + os.path.join(ROOT, "include"), "-x", "hip", "-c", drv, "-o", obj], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        subprocess.run([HIPCC, "--offload-arch=gfx950", *SAN, *objs, obj, "-o", exe], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
    return exe


def test_attention_plan_host_logic_under_asan_ubsan():
    exe = attn_binary()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_attn_asan: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
