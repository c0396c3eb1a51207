"""Generates tests/golden/g12_mip_losses.npz: the REFERENCE's own lossfun_outer / lossfun_distortion (mipnerf360/helper.py:135-148,
imported under the stubs of _ref_loader.py) with their autograd gradients, in fp64 and in fp32, on the inputs of
tests/mip_loss_cases.py: both families, every shape up to 385 intervals, nine rays each.  Build-container only.

Stored per family and quantity as ONE flat array "<family>/<name>", the cases concatenated in the order of FIXTURE_SHAPES (an
archive member per case and tensor costs more in headers than the small cases hold; mip_loss_cases.fixture_case cuts a case out
again): the inputs t, w, t_env, w_env, up, up_dist (fp32) and the five outputs loss, g_w, g_w_env, dist, g_dist as "<name>64"
(fp64) and "<name>32_ulps" (int32): the fp32 result's distance in units of the last place from the fp64 result rounded to fp32 -
bit pattern minus bit pattern, lossless, and mostly 0 or +-1, which keeps the file under 0.5 MB.  Data only.

    python tests/golden/make_mip_losses.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _ref_loader as ref  # noqa: E402
import mip_loss_cases as M  # noqa: E402


def g12_mip_losses():
    H = ref.load("models.mipnerf360.helper")
    out = {}
    for family in M.FAMILIES:
        parts = {}
        for (N, Ne) in M.FIXTURE_SHAPES:
            inp = M.inputs(family, N, Ne)
            for k in M.INPUTS:
                parts.setdefault(k, []).append(inp[k].numpy().reshape(-1))
            for dtype in (torch.float64, torch.float32):
                res = M.evaluate(inp, dtype, outer=H.lossfun_outer, distortion=H.lossfun_distortion)
                for k in M.OUTPUTS:
                    v = res[k].numpy().reshape(-1)
                    assert res[k].dtype == dtype
                    if dtype == torch.float64:
                        parts.setdefault(k + "64", []).append(v)
                    else:
                        parts.setdefault(k + "32_ulps", []).append(v.view(np.int32) - parts[k + "64"][-1].astype(np.float32).view(np.int32))
        for k, v in parts.items():
            out[family + "/" + k] = np.concatenate(v)
    path = os.path.join(HERE, "g12_mip_losses.npz")
    np.savez_compressed(path, **out)
    print("g12_mip_losses %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))


if __name__ == "__main__":
    if not ref.reference_available():
        sys.exit("reference tree not found at %s" % ref.REFERENCE_ROOT)
    g12_mip_losses()
